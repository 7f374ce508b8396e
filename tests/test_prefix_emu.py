"""k_b_prefix_census -- the per-prefix census kernel, code that exists only as a gfx950 kernel -- and the control around it on the host:
bifromq_amd/csrc/bmq_prefix_kernels.h compiled by g++ against the wave64 emulator (tools/emu/prefix_emu.cpp), launched from DistIndex::prefix_census
over indexes the product's host builder made, and compared with a per-key loop.  Then: can this tier notice a wrong kernel?  Single-line
mutants of a copy of bifromq_amd/csrc in a temporary directory (none is ever built into a library or run on a GPU), each compiled into the
harness: every one must make it fail -- a count, a coverage floor, or an abort of the emulator -- and the unmodified copy must pass.  A mutant
that survives is a blind spot of the harness, not of this test.

One mutant one might expect is left out because it cannot change an answer: `a prefix longer than the key counts as a match` (dropping
`if (pl > kl) return false;` from prefix_is_of).  The walk only ever tests the floor F <= key and prefixes P of F; a P longer than the key
with P[0, len(key)) == key would be above the key, and so would F.  P1 below breaks the same compare in a way that shows."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "prefix_emu.cpp")
ROUNDS = 2
TIMEOUT_S = 600

KERN, CORE, CENSUS, INDEX = "bmq_prefix_kernels.h", "bmq_prefix_core.h", "bmq_census_kernels.h", "bmq_dist_index.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("F1", CORE, "return lo == 0 ? NONE : lo - 1;", "return lo < T.n ? lo : NONE;", "the floor search returns the first prefix above the key"),
    ("F2", CORE, "k, kl) <= 0) lo = mid + 1;", "k, kl) < 0) lo = mid + 1;", "a key equal to a prefix is left out"),
    ("W1", CORE, "        s = T.parent[s];\n", "        s = NONE;\n", "the chain walk stops at the floor"),
    ("P1", CORE, "    return key_compare(p, m, k, m) == 0;\n", "    return true;\n", "an entry that is no longer than the key counts as a prefix of it"),
    ("D1", CORE, "if (len == 0) return NONE; // a dead reference", "if (len == 0) return flag = 1u, T.n ? 0u : NONE; // a dead reference",
     "dead references are counted"),
    ("C1", INDEX, "            for (uint32_t w = 0; w < 4; w++) t[4 * (size_t)parent[s] + w] += t[4 * (size_t)s + w];\n", "", "the sums are not carried to the parents"),
    ("C2", INDEX, "t[4 * (size_t)parent[s] + w] += t[4 * (size_t)s + w];", "t[4 * (size_t)parent[s] + w] += 2 * t[4 * (size_t)s + w];", "the sums are carried twice"),
    ("E1", KERN, "    census_flush<4>(table, run, lane); // the sums the wave still carries\n", "", "the final flush is dropped"),
    ("B1", CENSUS, "uint32_t b = mine ? len : 0u;", "uint32_t b = len;", "the byte sum is taken over all lanes, not over the lanes of the slot"),
    ("R1", INDEX, "out[4 * (size_t)i + w] = t[4 * (size_t)slot_of[i] + w];", "out[4 * (size_t)i + w] = rep[slot_of[i]] == i ? t[4 * (size_t)slot_of[i] + w] : 0;",
     "repeated inputs get zeros"),
    ("S1", KERN, "* turns * 64ull; // the wave's stretch of ids", "* 64ull; // the wave's stretch of ids", "the stretches of the waves overlap"),
    ("A1", INDEX, "                parent[s] = stack.back();\n", "                parent[s] = stack.front();\n", "the parent is the shortest prefix, not the longest"),
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
    exe = os.path.join(work, name, "prefix_emu")
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
            if r.returncode != 0 or not r.stdout.startswith("prefix emu ok:"):
                return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
            continue
        if r.returncode == 0:
            return name, False, "SURVIVED: prefix_emu %d %s says ok" % (ROUNDS, seed)
        msg = r.stderr
        told = r.returncode < 0 or any(w in msg for w in (" count ", "coverage:", "wave_emu"))
        if not told:
            return name, False, "seed %s: exit %d without a count or coverage message: %s" % (seed, r.returncode, tail)
        return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]
    return name, True, "passes"


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_prefix_census_kernel_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/prefix_emu.cpp: filters as runs of 1, 63, 64, 65 and 200 receivers, tenants and filters interleaved, one tenant, random ones;
    deletes; seven kinds of prefix sets; grids of one and two workgroups beside the product's; the harness fails if its cases miss a path."""
    exe = str(tmp_path / "prefix_emu")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("prefix emu ok:"), r.stdout


def test_every_mutant_of_the_prefix_census_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 9
    jobs = [("unmodified", None, ["12345"])] + [(m[0], m, ["12345"]) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
