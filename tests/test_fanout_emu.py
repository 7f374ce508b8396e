"""k_fo_hist and k_fo_scatter -- the counting sort of the fan-out grouping's fast path, code that exists only as gfx950 kernels -- on the host:
bifromq_amd/csrc/bmq_fanout_kernels.h compiled by g++ against the wave64 emulator (tools/emu/fanout_emu.cpp) and compared with a stable sort of
the pairs by key.  Then: can this tier notice a wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a temporary directory (none
is ever built into a library or run on a GPU), each compiled into the harness: every one must make it fail -- an output row, a count (of pairs
without a group slot, of a histogram word, of a wave's cross-lane operations), a coverage floor, or an abort of the emulator -- and the
unmodified copy must pass.  A mutant that survives is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "fanout_emu.cpp")
ROUNDS = 6
TIMEOUT_S = 600

KERN = "bmq_fanout_kernels.h"
# (name, file or None for a compiler flag, exact source substring -- it must occur exactly once -- or the flag, replacement, what the mutant does)
MUTANTS = [
    ("W1", KERN, "if (em <= p) lo = mid + 1;", "if (em < p) lo = mid + 1;", "window search: the first pair of a row lands in the row before"),
    ("W2", KERN, "wbase += 64; //", "wbase += 63; //", "the row window moves on by 63 rows: right rows, more loads"),
    ("W3", KERN, "if (!placed && e_last > p) {", "if (!placed && e_last >= p) {", "a pair at the window's end is placed inside the window"),
    ("W4", KERN, "if (f.row_ptr[mid] <= p0) lo = mid;", "if (f.row_ptr[mid] < p0) lo = mid;",
     "the tile's first row is searched with '<': the window starts in front of the empty rows"),
    ("P1", KERN, "            carry += __shfl(inc, 63);\n", "            (void)__shfl(inc, 63);\n", "the multi-chunk prefix loses its carry"),
    ("P2", KERN, "const uint32_t l = carry + inc - c;", "const uint32_t l = carry + inc;", "inclusive in place of exclusive prefix inside the tile"),
    ("R1", KERN, "same &= ((key >> b) & 1u) ? mb : ~mb;", "same &= ((key >> b) & 1u) ? mb : mb;", "same-key mask: the complement of the ballot is dropped"),
    ("R2", KERN, "loff[key] = base_off + cnt;", "loff[key] = base_off + rank;", "the key's running offset moves on by the leader's rank (0)"),
    ("R3", None, "-DFANOUT_EMU_KEY_BITS_BIAS=1", None, "the control hands over one key bit too few: keys that differ in the top bit rank together"),
    ("H1", KERN, "    if (tile == 0 && lane == 0) f.hist[(size_t)f.n_bins * f.n_tiles] = 0;", "    if (false) f.hist[(size_t)f.n_bins * f.n_tiles] = 0;",
     "the end mark of the histogram is not written"),
    ("H2", KERN, "f.hist[(size_t)b * f.n_tiles + tile] = cnt[b];", "f.hist[(size_t)tile * f.n_bins + b] = cnt[b];",
     "the histogram is written tile-major while k_fo_scatter reads it key-major"),
    ("H3", KERN, "            if (g == FO_DEAD_ID) {\n", "            if (false) {\n", "deleted routes count as routes without a group slot"),
    ("H4", KERN, "if (id < f.id_end && id < st.id_cap) {", "if (id < st.id_cap) {", "ids never handed out are looked up in the cache"),
    ("H5", KERN, "key = g == st.gt_cap ? f.n_bins - 2 :", "key = g == st.gt_cap ? f.n_bins - 1 :", "shared subscriptions are filed under the dead ids"),
    ("H6", KERN, "    for (uint32_t b = lane; b < f.n_bins; b += 64) cnt[b] = 0;\n", "", "the wave's LDS counters start with what the wave before left"),
]


def _build_and_run(work, name, mutant, seeds):
    """-> (name, caught or passed as expected, report)"""
    csrc = os.path.join(work, name, "csrc")
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so", "*.hipfb", "*.bc"))
    flags = []
    if mutant is not None:
        _, fname, old, new, _ = mutant
        if fname is None:
            flags = [old]
        else:
            path = os.path.join(csrc, fname)
            with open(path) as f:
                src = f.read()
            if src.count(old) != 1:
                return name, False, "update the mutant table: %r occurs %d times in %s" % (old, src.count(old), fname)
            with open(path, "w") as f:
                f.write(src.replace(old, new))
    exe = os.path.join(work, name, "fanout_emu")
    b = subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    for seed in seeds:
        try:
            r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
        tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
        if mutant is None:
            if r.returncode != 0 or not r.stdout.startswith("fanout emu ok:"):
                return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
            continue
        if r.returncode == 0:
            return name, False, "SURVIVED: fanout_emu %d %s says ok" % (ROUNDS, seed)
        msg = r.stderr
        told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", "coverage:", "wave_emu"))
        if not told:
            return name, False, "seed %s: exit %d without a row, count or coverage message: %s" % (seed, r.returncode, tail)
        return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]
    return name, True, "passes"


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_fast_path_of_the_fanout_grouping_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/fanout_emu.cpp: the row shapes and key patterns of tests/fanout_cases.py and random ones, 2 to 1026 bins, tiles of 64, 128, 192 and 1024
    pairs; the harness fails if its cases miss one of the kernels' rarely taken paths."""
    exe = str(tmp_path / "fanout_emu")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("fanout emu ok:"), r.stdout


def test_every_mutant_of_the_fast_path_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 10
    jobs = [("unmodified", None, ["12345"])] + [(m[0], m, ["12345"]) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
