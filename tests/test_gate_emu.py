"""The kernels of the submit-time fan-out gate over a match CSR on the host: bifromq_amd/csrc/bmq_gate_kernels.h compiled by g++ against the
wave64 emulator (tools/emu/gate_emu.cpp) and compared with the rule written plainly there -- the loop of DeliverExecutorGroup.submit over a
row's live routes in key order.  Then: can this tier notice a wrong kernel or a wrong rule?  Single-line mutants of a copy of
bifromq_amd/csrc in a temporary directory (none is ever built into a library or run on a GPU), each compiled into the harness: every one
must make it fail -- a row, a count, a flag, a meter, a coverage floor, or an abort -- and the unmodified copy must pass.  A mutant that
survives is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "gate_emu.cpp")
ROUNDS = 6
TIMEOUT_S = 600

KERN, CORE, CAPS_KERN, CAPS_CORE = "bmq_gate_kernels.h", "bmq_gate_core.h", "bmq_caps_kernels.h", "bmq_caps_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("P1", CORE, "if (A >= pf) o.flags |= GATE_P_COUNT;", "if (A > pf) o.flags |= GATE_P_COUNT;", "> for >= in the count comparison: PersistentFanoutThrottled is never reported"),
    ("P2", CORE, "if (A * (unsigned long long)s >= pb) o.flags", "if (A * (unsigned long long)s > pb) o.flags", "> for >= in the bytes comparison: bytes exactly at the limit go unreported"),
    ("P3", CORE, "const unsigned long long lim = pb / s + (pb % s != 0 ? 1ull : 0ull);", "const unsigned long long lim = pb / s;", "floor for ceil: the route that crosses the bytes limit is turned away"),
    ("P4", CORE, "if (A * (unsigned long long)s >= pb) o.flags", "if ((uint32_t)(A * (unsigned long long)s) >= pb) o.flags", "the bytes compare in 32 bits"),
    ("B1", CORE, "    if (n == 1) { // routes.size() == 1", "    if (n == 1 && nP == 7) { // routes.size() == 1", "no bypass for a pack of one route"),
    ("B2", CORE, "        o.record = nP;\n", "        o.record = 1;\n", "a single transient route or group leaves a meter record"),
    ("Z1", CORE, "    o.record = 1;\n", "    o.record = o.meter != 0 ? 1u : 0u;\n", "no meter record for a sum of zero bytes"),
    ("N1", CORE, "    } else if (nP > 0) {\n", "    } else {\n", "a row without persistent routes reports persistent events"),
    ("N2", CORE, "        if (pf > 0 && pb > 0) o.flags |= GATE_NO_P_BANDWIDTH;\n", "        if (pf > 0) o.flags |= GATE_NO_P_BANDWIDTH;\n", "a byte limit of 0 is reported as missing bandwidth"),
    ("G1", CORE, "    if (nG > gf) o.flags |= GATE_GROUP;\n", "    if (nG >= gf) o.flags |= GATE_GROUP;\n", "groups exactly at their limit count as throttled"),
    ("I1", CORE, "    if (n < inline_threshold) o.flags |= GATE_INLINE;\n", "    if (n <= inline_threshold) o.flags |= GATE_INLINE;\n", "<= for < at the inline threshold"),
    ("S1", CORE, "b.c.keep[p] = rank + 1 <= b.row_keep[", "b.c.keep[p] = rank + 1 < b.row_keep[", "< for <= at the kept count: the last admitted member is turned away"),
    ("L1", CORE, "    b.c.keep[i] = !over && b.row_keep[3 * (size_t)r + gate_slot_of(c)] > 0 ? 1u : 0u;", "    b.c.keep[i] = !over ? 1u : 0u;", "a class that is dropped whole survives"),
    ("O1", CORE, "    m |= (xp ? CAPS_OVER_P : 0u) | (xg ? CAPS_OVER_G : 0u);\n", "    m |= (xp ? CAPS_OVER_P : 0u);\n", "a group class of which some members stay is never ranked"),
    ("W1", CORE, "c.out_ids[c.keep_scan[i] - 1] = c.ids[i];", "c.out_ids[c.keep_scan[i]] = c.ids[i];", "every survivor lands one place late"),
    ("W2", CORE, "at < c.total ? c.keep_scan[at] - c.keep[at] :", "at < c.total ? c.keep_scan[at] :", "the row offsets are the inclusive scan"),
    ("R1", CAPS_CORE, "order_compare(ix.kpool, ix.kref[b.ids[k]], ix.kref[b.ids[p]]) < 0;", "b.ids[k] < b.ids[p];", "the rank is taken by id, not by key"),
    ("D1", CAPS_CORE, "    const unsigned long long r = id < id_end && id < ix.id_cap ? ix.kref[id] : 0ull;\n", "    const unsigned long long r = id < ix.id_cap ? ix.kref[id] : 0ull;\n",
     "an id the index never handed out is looked up"),
    ("T1", KERN, "        const bool in = i < total;\n", "        const bool in = i + 1 < total;\n", "the last pair of the batch is never classified: a dropped tail lane"),
    ("T2", CAPS_KERN, "caps_ballot(k < hi && caps_below_one(ix, b, k, p))", "caps_ballot(k + 1 < hi && caps_below_one(ix, b, k, p))", "the last pair of a row is never compared: a dropped tail lane"),
    ("T3", KERN, "        const bool in = r < n_rows;\n", "        const bool in = r + 1 < n_rows;\n", "the last row of the batch is never answered"),
    ("X1", KERN, "            const bool mine = pending && r == lr;\n", "            const bool mine = pending;\n", "a wave's live pairs are all counted for its first row"),
    ("M1", KERN, "            const bool mine = pending && t == lt;\n", "            const bool mine = pending;\n", "the meter of a wave's rows all goes to the first lane's table entry"),
    ("M2", KERN, "gate_sum_wave(mine ? meter : 0ull)", "gate_sum_wave(meter)", "an entry's sum takes the bytes of the wave's other entries too"),
    ("M3", KERN, "    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);\n", "    for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d);\n", "the meter is summed over half a wave"),
    ("M4", KERN, "atomicAdd(b.meter_records + lt, (uint32_t)__popcll(mm));", "atomicAdd(b.meter_records + lt, 1u);", "one record per wave and entry instead of one per row"),
    ("X2", KERN, "        if (rank) b.c.work[at + caps_lanes_below(m)] = (uint32_t)i;\n", "        if (rank) b.c.work[at] = (uint32_t)i;\n", "the pairs of a wave share one place of the work list"),
]


def _compile(csrc, exe):
    return subprocess.run(["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, "-o", exe], capture_output=True, text=True)


def _build_and_run(work, name, mutant, seed):
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
    exe = os.path.join(work, name, "gate_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    try:
        r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or not r.stdout.startswith("gate emu ok:"):
            return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: gate_emu %d %s says ok" % (ROUNDS, seed)
    msg = r.stderr
    told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", " flag ", " meter ", "coverage:", "wave_emu", "guard row"))
    if not told:
        return name, False, "seed %s: exit %d without a row, count, flag, meter or coverage message: %s" % (seed, r.returncode, tail)
    return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_gate_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/gate_emu.cpp: single-route rows of every class, both persistent bits, rows without bandwidth, classes that end at waves, ranked
    and whole-dropped classes, meter sums above 2^32, several table entries per wave; the harness fails if its cases miss one of them."""
    exe = str(tmp_path / "gate_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("gate emu ok:"), r.stdout


def test_every_mutant_of_the_gate_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 12
    jobs = [("unmodified", None, "12345")] + [(m[0], m, "12345") for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
