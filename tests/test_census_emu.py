"""k_b_census and k_r_census -- the per-tenant census kernels, code that exists only as gfx950 kernels -- on the host:
bifromq_amd/csrc/bmq_census_kernels.h compiled by g++ against the wave64 emulator (tools/emu/census_emu.cpp) and compared with a per-key loop
over indexes the product's host builder made.  Then: can this tier notice a wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a
temporary directory (none is ever built into a library or run on a GPU), each compiled into the harness: every one must make it fail -- a count
(of a table word, of a launch's flushes), a coverage floor, or an abort of the emulator -- and the unmodified copy must pass.  A mutant that
survives is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "census_emu.cpp")
ROUNDS = 2
TIMEOUT_S = 600

KERN, CORE, RCORE = "bmq_census_kernels.h", "bmq_build_core.h", "bmq_retain_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("E1", KERN, "    census_flush<4>(table, run, lane);\n", "", "k_b_census: the carried sums are not flushed at the end"),
    ("E2", KERN, "    census_flush<1>(table, run, lane);\n", "", "k_r_census: the carried count is not flushed at the end"),
    ("B1", KERN, "uint32_t b = mine ? len : 0u;", "uint32_t b = len;", "the byte sum is taken over all lanes, not over the lanes of the slot"),
    ("F1", KERN, "__ballot(mine && flag == 2u)", "__ballot(mine && flag == 1u)", "the ballot of the unordered shares asks for flag 1"),
    ("F2", KERN, "__ballot(mine && flag == 3u)", "__ballot(mine && flag >= 2u)", "the ballot of the ordered shares takes the unordered ones too"),
    ("K1", CORE, "    if ((b.flags & 2u) && key_compare(k, len, b.end, b.end_len) >= 0) return false;\n", "", "the boundary's end compare is dropped"),
    ("K2", CORE, "if ((b.flags & 1u) && key_compare(k, len, b.start, b.start_len) < 0) return false;",
     "if ((b.flags & 1u) && key_compare(k, len, b.start, b.start_len) <= 0) return false;", "a key equal to the start key is left out"),
    ("R1", KERN, "            run.c[0] = run.c[1] = run.c[2] = 0;\n", "", "a new run starts with the counts of the one before"),
    ("R2", KERN, "if (s != run.slot) { //", "if (true) { //", "the wave flushes after every turn: right counts, twenty times the atomics"),
    ("S1", KERN, "* turns * 64ull; // the wave's stretch of ids", "* 64ull; // the wave's stretch of ids", "the stretches of the waves overlap"),
    ("L1", KERN, "s_key[wave][1][p] = b.end[p];", "s_key[wave][0][p] = b.end[p];", "the end key is staged over the start key"),
    ("D1", RCORE, "if (id >= m.id_cap || id_dead(m.dead_bits, id)) return NONE;", "if (id >= m.id_cap) return NONE;", "k_r_census counts removed topics"),
    ("M1", KERN, "        const bool mine = slot == s;\n", "        const bool mine = slot == s || slot == NONE;\n", "lanes with nothing to count join every slot"),
]


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
    exe = os.path.join(work, name, "census_emu")
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], capture_output=True, text=True)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    for seed in seeds:
        try:
            r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
        tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
        if mutant is None:
            if r.returncode != 0 or not r.stdout.startswith("census emu ok:"):
                return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
            continue
        if r.returncode == 0:
            return name, False, "SURVIVED: census_emu %d %s says ok" % (ROUNDS, seed)
        msg = r.stderr
        told = r.returncode < 0 or any(w in msg for w in (" count ", "coverage:", "wave_emu"))
        if not told:
            return name, False, "seed %s: exit %d without a count or coverage message: %s" % (seed, r.returncode, tail)
        return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]
    return name, True, "passes"


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_census_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/census_emu.cpp: tenants as runs of 1, 63, 64, 65 and 200 keys, 70 tenants interleaved, one tenant, random ones; deletes; the
    boundary table; grids of one and two workgroups beside the product's; the harness fails if its cases miss one of the kernels' paths."""
    exe = str(tmp_path / "census_emu")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("census emu ok:"), r.stdout


def test_every_mutant_of_the_census_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 6
    jobs = [("unmodified", None, ["12345"])] + [(m[0], m, ["12345"]) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
