"""The kernels that answer a retain match on a CHURNED index -- dead ids inside the bulk-loaded id space, an overlay trie beside it -- on the host:
bifromq_amd/csrc/bmq_retain_kernels.h (retain_walk_body of k_retain_overlay / k_retain_walk_deep, k_retain_sums, k_retain_rowptr_dyn,
k_retain_expand_dyn, k_limit_select / _compact / _count_live / _copy_live) compiled by g++ against the wave64 emulator (tools/emu/retain_dyn_emu.cpp)
and compared with a plain loop over ids and with a brute force over the live topic strings, at both LDS geometries.  Then: can this tier notice a
wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a temporary directory (none is ever built into a library or run on a GPU),
each compiled into the harness that reaches its line (retain_dyn_emu, or rwalk_emu for the DYN sites of bmq_rwalk_kernel.h): every one must make it
fail -- a row, a listing, a live count, a coverage floor, or an abort of the emulator -- and the unmodified copy must pass.  A mutant that survives
is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
EMU = os.path.join(ROOT, "tools", "emu")
CASES = 40         # random cases of one run (the directed ones and the floors do not depend on it)
MUTANT_CASES = 6
TIMEOUT_S = 900
# the second geometry: lists of 8 entries, so that small cases cross every list border (OV_OUT takes a whole wave's matches: 64 is its minimum)
SMALL = ("-DBMQ_R_FRONT=8", "-DBMQ_R_OUT=8", "-DBMQ_OV_OUT=64")

# harness -> (sources beside the harness file, arguments of a mutant run, what its ok output holds, words of a verdict)
HARNESS = {
    "retain_dyn_emu": (("bmq_retain.cpp", "bmq_codec.cpp"), [str(MUTANT_CASES), "12345"], "retain dyn emu ok:", (" row ", "listing", "coverage:", "wave_emu")),
    "rwalk_emu": (("bmq_retain.cpp",), ["24", "12345"], "ok: G 4", ("route_cnt", "coverage:", "wave_emu")),
}
RK, RW = "bmq_retain_kernels.h", "bmq_rwalk_kernel.h"
# (name, harness, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    # k_retain_expand_dyn
    ("E1", "retain_dyn_emu", RK, "            if (((hi - 1) >> 6) != (lo >> 6)) w1 = dead_bits[(lo >> 6) + 1];\n", "", "the second bitmap word of a short range is not read"),
    ("E2", "retain_dyn_emu", RK, "                if (wb == we && (eb & 63u)) edge &= ~0ull >> (64u - (eb & 63u));\n", "", "a streamed range inside one word is not clipped at its end"),
    ("E3", "retain_dyn_emu", RK, "for (; w < we; w++) put_word", "for (; w + 1 < we; w++) put_word", "the remainder of the four-word loop drops its last word"),
    ("E4", "retain_dyn_emu", RK, "((eb & 63u) ? ~0ull >> (64u - (eb & 63u)) : ~0ull)); // the last word", "(~0ull)); // the last word", "the last word of a streamed range is not masked"),
    ("E5", "retain_dyn_emu", RK, "if (lane == 0) prev_last = carry_last;", "prev_last = 0;", "the out-of-order check forgets the last id of the 64 ranges before"),
    ("E6", "retain_dyn_emu", RK, "if (__any(bad) && nr > 1 && lane == 0)", "if (__any(bad) && nr > 2 && lane == 0)", "a row of two ids out of order is not listed"),
    # match(limit, now)
    ("L1", "retain_dyn_emu", RK, "r.begin >= cursor", "r.begin > cursor", "a range that begins at the cursor (id 0, an adjacent range) is skipped"),
    ("L2", "retain_dyn_emu", RK, "if (live && slot < lim)", "if (live)", "ids behind the quota are written into the next filter's slots"),
    ("L3", "retain_dyn_emu", RK, "expire_at[id] > now", "expire_at[id] >= now", "a message that expires at `now` counts as live in k_limit_select"),
    ("L4", "retain_dyn_emu", RK, "list < (ov.pairs ? 2u : 1u)", "list < 1u", "the overlay's list is not read"),
    ("L5", "retain_dyn_emu", RK, "k < e && t < c; k++)", "k < e; k++)", "k_limit_copy_live copies behind the row's quota"),
    # retain_walk_body
    ("O1", "retain_dyn_emu", RK, "                        if (skip_sys && (dyn.onodes[c].str_len & ON_SYS)) continue; // a first-level wildcard never matches a '$' level\n", "",
     "a first-level wildcard follows the '$' children of the overlay"),
    ("O2", "retain_dyn_emu", RK, "rk += ovb[k] < x ? 1u : 0u;", "rk += ovb[k] <= x ? 1u : 0u;", "the rank sort of the overlay buffer is off by one"),
    ("O3", "retain_dyn_emu", RK, "return (id != NONE && !id_dead(dyn.dead_bits, id)) ? id : NONE;", "return id;", "removed overlay topics are matched"),
    ("O4", "retain_dyn_emu", RK, "if (wp <= R_OUT) { // everything is in LDS", "if (wp <= R_OUT + 1u) { // everything is in LDS", "R_OUT + 1 ranges are copied out of an LDS list of R_OUT"),
    ("O5", "retain_dyn_emu", RK, "dead_before(dyn.dead_bits, dyn.dead_rank, g + c) -", "dead_before(dyn.dead_bits, dyn.dead_rank, g + c - 1u) -", "the live count of a range ignores its last id"),
    # the DYN instantiation of k_retain_walk
    ("W1", "rwalk_emu", RW, "dead_before(dyn.dead_bits, dyn.dead_rank, g + gc) -", "dead_before(dyn.dead_bits, dyn.dead_rank, g + gc - 1u) -", "the live count of a range ignores its last id"),
    ("W2", "rwalk_emu", RW, "                    if (DYN && dyn.use_dead && g < dyn.base_n) alive = !id_dead(dyn.dead_bits, g);\n", "", "a removed topic found by a bulk chunk counts as live"),
    ("W3", "rwalk_emu", RW, "l2 = gc2 - (dead_before(dyn.dead_bits, dyn.dead_rank, g + gc2) - dead_before(dyn.dead_bits, dyn.dead_rank, g));", "l2 = gc2;",
     "the range behind the '$' run of the filter '#' is counted whole"),
]


def _build(csrc, harness, exe, defs=()):
    cmd = ["g++", "-O1", "-std=c++17", *defs, "-I", csrc, "-I", EMU, os.path.join(EMU, harness + ".cpp"), *[os.path.join(csrc, s) for s in HARNESS[harness][0]], "-o", exe, "-pthread"]
    return subprocess.run(cmd, capture_output=True, text=True)


def _build_and_run(work, name, harness, mutant):
    """-> (name, caught or passed as expected, report)"""
    csrc = os.path.join(work, name, "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.hipfb", "*.bc"))
    if mutant is not None:
        _, _, fname, old, new, _ = mutant
        path = os.path.join(csrc, fname)
        with open(path) as f:
            src = f.read()
        if src.count(old) != 1:
            return name, False, "update the mutant table: %r occurs %d times in %s" % (old, src.count(old), fname)
        with open(path, "w") as f:
            f.write(src.replace(old, new))
    exe = os.path.join(work, name, harness)
    b = _build(csrc, harness, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    _, args, ok_text, words = HARNESS[harness]
    try:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "no verdict within %d s" % TIMEOUT_S
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or ok_text not in r.stdout:
            return name, False, "the unmodified source fails: %s" % tail
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: %s %s says ok" % (harness, " ".join(args))
    told = r.returncode < 0 or any(w in r.stderr for w in words)
    if not told:
        return name, False, "exit %d without a row, listing, count or coverage message: %s" % (r.returncode, tail)
    return name, True, "caught: " + (r.stderr.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
@pytest.mark.parametrize("defs", [(), SMALL], ids=["lists-256-256-128", "lists-8-8-64"])
def test_the_kernels_of_a_churned_retain_index_under_the_wave_emulator(tmp_path, defs, seed):
    """tools/emu/retain_dyn_emu.cpp: range lengths 1 .. 400 at every word offset against nine dead patterns and base_n inside and on a bitmap word, rows of
    64 / 65 / 129 ranges, disorder at a 64-range chunk border, limits around LIM_FAST over two lists with expiry at equality, 16 385 and 32 769 rows;
    overlay rows at OV_OUT / R_OUT, '$' levels, dead overlay topics, deep filters of 17 .. 300 levels over both tries; the chain of a batch from the
    walks to the CSR.  The harness fails if its cases miss one of those paths; the `ok` line lists them."""
    exe = str(tmp_path / "retain_dyn_emu")
    b = _build(CSRC, "retain_dyn_emu", exe, defs)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(CASES), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("retain dyn emu ok:"), r.stdout[:2000]
    counts = [int(f.rsplit(": ", 1)[1]) for f in r.stdout.strip().rstrip(";").split("; ")[1:]]
    assert len(counts) > 100 and min(counts) > 0, r.stdout


def test_every_mutant_of_the_churned_retain_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 19
    jobs = [("unmodified-" + h, h, None) for h in HARNESS] + [(m[0], m[1], m) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[5] for m in MUTANTS}
    report = "\n".join("%-26s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
