"""The kernels of the RANGES result format on the host: bifromq_amd/csrc/bmq_format_kernels.h compiled by g++ against the wave64 emulator
(tools/emu/format_emu.cpp) and compared with a restatement of the contract of include/bmq.h (bmq_match_wait_ranges).  Then: can this tier
notice a wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a temporary directory (none is ever built into a library or run
on a GPU), each compiled into the harness: every one must make it fail -- an output row, a count, a coverage floor, or an abort -- and the
unmodified copy must pass.  A mutant that survives is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "format_emu.cpp")
ROUNDS = 6
TIMEOUT_S = 600
SEEDS = ("12345", "777")

KERN = "bmq_format_kernels.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("C1", KERN, "    if (t > f.n_topics) return;\n", "    if (t >= f.n_topics) return;\n", "the count of entry n is never written (and with n = 0 neither are the sums)"),
    ("C2", KERN, "if (c & RANGE_INDIRECT) ns += c & ~RANGE_INDIRECT;", "ns += c & ~RANGE_INDIRECT;", "the ids of direct ranges are counted as side ids"),
    ("C3", KERN, "        f.sums[2] = 0;\n", "", "the count of overlapping rows goes on from the batch before"),
    ("C4", KERN, "f.sums[3] = (f.ctr->status & (ST_RERUN | ST_RANGE)) ? 2ull : 0ull;", "f.sums[3] = (f.ctr->status & (ST_RERUN | ST_RANGE)) ? 0ull : 0ull;",
     "an incomplete batch is not reported"),
    ("C5", KERN, "    if (t < f.n_topics && !(f.ctr->status & (ST_RERUN | ST_RANGE))) {\n", "    if (t < f.n_topics && !(f.ctr->status & (ST_RERUN))) {\n",
     "a batch of 2^32 ids and more is counted as if it were complete"),
    ("C6", KERN, "    if (t < f.n_topics && !(f.ctr->status & (ST_RERUN | ST_RANGE))) {\n", "    if (t < f.n_topics && !f.ctr->status) {\n",
     "any status bit empties the result: also those that leave the ranges valid (the caller's id buffer, a MIXED rerun)"),
    ("E1", KERN, "const bool fits = n_r <= f.range_cap && n_s <= f.side_cap;", "const bool fits = n_r <= f.range_cap;", "too small a side buffer goes unnoticed"),
    ("E2", KERN, "const bool fits = n_r <= f.range_cap && n_s <= f.side_cap;", "const bool fits = n_r < f.range_cap && n_s <= f.side_cap;", "an exact fit of the ranges is refused"),
    ("E3", KERN, "const bool fits = n_r <= f.range_cap && n_s <= f.side_cap;", "const bool fits = n_r <= f.range_cap && n_s < f.side_cap;", "an exact fit of the side ids is refused"),
    ("E4", KERN, "    if (t >= f.n_topics || !fits) return;\n", "    if (t >= f.n_topics) return;\n", "rows are written into buffers that are too small"),
    ("E5", KERN, "            sp += len;\n", "", "every list of a row lands on the first words of the row's side slice"),
    ("E6", KERN, "f.ix.route_pos[r.begin + k];", "f.ix.route_pos[r.begin + k + 1];", "a list is copied from one word further on"),
    ("E7", KERN, "const bool order = nr <= FMT_SORT_MAX;", "const bool order = nr < FMT_SORT_MAX;", "rows of exactly 32 ranges are copied as matched"),
    ("E8", KERN, "constexpr uint32_t FMT_SORT_MAX = 32;", "constexpr uint32_t FMT_SORT_MAX = 33;", "rows of 33 ranges are ordered (the harness knows 32 from include/bmq.h, not from the kernel)"),
    ("E9", KERN, "if ((q.count & ~RANGE_INDIRECT) != 0 && fmt_first_id(f, q) <= key) break;", "if (fmt_first_id(f, q) <= key) break;",
     "the begin word of an empty range stops the insertion"),
    ("E10", KERN, "if ((q.count & ~RANGE_INDIRECT) != 0 && fmt_first_id(f, q) <= key) break;", "if ((q.count & ~RANGE_INDIRECT) != 0 && fmt_first_id(f, q) >= key) break;",
     "rows come out descending"),
    ("E11", KERN, "        last = fmt_last_id(f, q);\n", "        last = fmt_first_id(f, q);\n", "an overlap is seen only where first ids repeat"),
    ("E12", KERN, "        if ((q.count & ~RANGE_INDIRECT) == 0) continue;\n", "", "empty ranges take part in the overlap scan with their begin word"),
    ("E13", KERN, "f.out_side[r.begin + c - 1] : r.begin + c - 1;", "f.out_side[r.begin + c - 1] : r.begin + c;", "a direct range ends one id late: ranges that touch count as overlapping"),
    ("E14", KERN, "f.out_side[r.begin + c - 1] : r.begin + c - 1;", "f.out_side[r.begin + c] : r.begin + c - 1;", "a list ends with the word behind it"),
    ("E15", KERN, "    if (bad) atomicAdd(f.sums + 2, 1ull);\n", "    if (bad) f.sums[2] = 1ull;\n", "the count of overlapping rows is 0 or 1"),
    ("E16", KERN, "        if (!fits) f.sums[3] |= 1ull;\n", "", "buffers that are too small are not reported"),
    ("E17", KERN, "        if (have && fmt_first_id(f, q) <= last) bad = true;\n", "        if (have && fmt_first_id(f, q) < last) bad = true;\n",
     "a range that begins with the last id of the one before it is not an overlap"),
    ("E18", KERN, "            r.begin = sp;\n", "            r.begin = sp - f.side_ptr[t];\n", "a list's place is counted inside the row's side slice"),
    ("E19", KERN, "return (r.count & RANGE_INDIRECT) ? f.out_side[r.begin] : r.begin; }", "return r.begin; }", "lists are ordered by their place in the side array"),
]


def _compile(csrc, exe):
    return subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe],
                          capture_output=True, text=True)


def _build_and_run(work, name, mutant, seeds):
    """-> (name, caught or passed as expected, report)"""
    csrc = os.path.join(work, name, "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.hipfb", "*.bc"))
    if mutant is not None:
        _, fname, old, new, _ = mutant
        path = os.path.join(csrc, fname)
        with open(path) as f:
            src = f.read()
        if src.count(old) != 1:
            return name, False, "update the mutant table: %r occurs %d times in %s" % (old, src.count(old), fname)
        with open(path, "w") as f:
            f.write(src.replace(old, new))
    exe = os.path.join(work, name, "format_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    for seed in seeds:
        try:
            r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
        tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
        if mutant is None:
            if r.returncode != 0 or not r.stdout.startswith("format emu ok:"):
                return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
            continue
        if r.returncode == 0:
            return name, False, "SURVIVED: format_emu %d %s says ok" % (ROUNDS, seed)
        msg = r.stderr
        told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", "coverage:"))
        if not told:
            return name, False, "seed %s: exit %d without a row, count or coverage message: %s" % (seed, r.returncode, tail)
        return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]
    return name, True, "passes at seeds " + ", ".join(seeds)


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_format_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/format_emu.cpp: batches that end at, before and behind a workgroup, rows at, below and above the ordering limit in every input
    order, empty ranges, several lists, interleaved and touching sets, short buffers, incomplete batches; the harness fails if its cases miss
    one of them."""
    exe = str(tmp_path / "format_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("format emu ok:"), r.stdout


def test_every_mutant_of_the_format_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 12
    jobs = [("unmodified", None, SEEDS)] + [(m[0], m, SEEDS[:1]) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
