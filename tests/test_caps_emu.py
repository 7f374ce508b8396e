"""The kernels of the fan-out caps over a match CSR on the host: bifromq_amd/csrc/bmq_caps_kernels.h compiled by g++ against the wave64
emulator (tools/emu/caps_emu.cpp) and compared with the contract written plainly there -- per row, a class's members sorted by key bytes, the
first `cap` kept, the others reported.  Then: can this tier notice a wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a
temporary directory (none is ever built into a library or run on a GPU), each compiled into the harness: every one must make it fail -- an
id, an offset, a count, an event, a coverage floor, or an abort -- and the unmodified copy must pass.  A mutant that survives is a blind spot
of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "caps_emu.cpp")
ROUNDS = 6
TIMEOUT_S = 600

KERN, CORE = "bmq_caps_kernels.h", "bmq_caps_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("C1", CORE, "    if (rank + 1 <= cap) {\n", "    if (rank + 1 < cap) {\n", "< for <= at the cap: the member of key rank cap - 1 is turned away"),
    ("C2", CORE, "return n > (pf < gf ? pf : gf); }", "return n >= (pf < gf ? pf : gf); }", "a row exactly as long as its smaller cap is classified"),
    ("R1", CORE, "order_compare(ix.kpool, ix.kref[b.ids[k]], ix.kref[b.ids[p]]) < 0;", "b.ids[k] < b.ids[p];", "the rank is taken by id, not by key"),
    ("G1", CORE, "    return k != p && b.cls[k] == b.cls[p] && ", "    return k != p && ", "the rank counts the keys of every class of the row"),
    ("E1", CORE, "    return b.ev_scan[s] - b.ev_cnt[s];\n", "    return b.ev_scan[s] - b.ev_cnt[s] + 1;\n", "the event base is off by one"),
    ("E2", CORE, "    const uint32_t s = 2 * r + (c - CAPS_PERSISTENT);\n", "    const uint32_t s = 2 * r;\n", "the group events of a row begin where its persistent events do"),
    ("E3", CORE, "caps_event_base(b, r, c) + (rank - cap);", "caps_event_base(b, r, c) + rank;", "an event's place counts the survivors too"),
    ("T1", KERN, "caps_ballot(k < hi && caps_below_one(ix, b, k, p))", "caps_ballot(k + 1 < hi && caps_below_one(ix, b, k, p))", "the last pair of a row is never compared: a dropped tail lane"),
    ("T2", KERN, "i < n; i += (unsigned long long)gridDim.x * CAPS_BLOCK) caps_write_one", "i + 1 < n; i += (unsigned long long)gridDim.x * CAPS_BLOCK) caps_write_one",
     "the last index of the write pass is never written"),
    ("T3", KERN, "    if (item >= n_work) return; // (the whole wave)\n", "    if (item + 1 >= n_work) return; // (the whole wave)\n", "the last pair of the work list is never ranked"),
    ("W1", CORE, "b.out_ids[b.keep_scan[i] - 1] = b.ids[i];", "b.out_ids[b.keep_scan[i]] = b.ids[i];", "every survivor lands one place late"),
    ("W2", CORE, "at < b.total ? b.keep_scan[at] - b.keep[at] :", "at < b.total ? b.keep_scan[at] :", "the row offsets are the inclusive scan"),
    ("K1", CORE, "        kp = b.row_cnt[2 * i] < pf ? b.row_cnt[2 * i] : pf;\n", "        kp = b.row_cnt[2 * i];\n", "the persistent count is the members', not the survivors'"),
    ("D1", CORE, "    b.keep[i] = c != CAPS_DEAD && !over ? 1u : 0u;\n", "    b.keep[i] = !over ? 1u : 0u;\n", "dead ids survive in classified rows"),
    ("D2", CORE, "    const unsigned long long r = id < id_end && id < ix.id_cap ? ix.kref[id] : 0ull;\n", "    const unsigned long long r = id < ix.id_cap ? ix.kref[id] : 0ull;\n",
     "an id the index never handed out is looked up"),
    ("P1", CORE, "    return broker == 1 && p > recv ? CAPS_PERSISTENT : CAPS_TRANSIENT;\n", "    return broker >= 1 && p > recv ? CAPS_PERSISTENT : CAPS_TRANSIENT;\n",
     "sub-broker 11 counts as persistent"),
    ("X1", KERN, "            const bool mine = pending && r == lr;\n", "            const bool mine = pending;\n", "a wave's capped pairs are all counted for its first row"),
    ("X2", KERN, "        if (rank) b.work[at + caps_lanes_below(m)] = (uint32_t)i;\n", "        if (rank) b.work[at] = (uint32_t)i;\n", "the pairs of a wave share one place of the work list"),
    ("O1", CORE, "        m |= (xp ? CAPS_OVER_P : 0u) | (xg ? CAPS_OVER_G : 0u);\n", "        m |= (xp ? CAPS_OVER_P : 0u);\n", "a group class over its cap is never ranked"),
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
    exe = os.path.join(work, name, "caps_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    try:
        r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or not r.stdout.startswith("caps emu ok:"):
            return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: caps_emu %d %s says ok" % (ROUNDS, seed)
    msg = r.stderr
    told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", "coverage:", "wave_emu", "guard row"))
    if not told:
        return name, False, "seed %s: exit %d without an id, offset, count, event or coverage message: %s" % (seed, r.returncode, tail)
    return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_caps_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/caps_emu.cpp: ids out of key order, classes that end at waves, rows longer than a workgroup, dead ids, rows at their cap, a short
    event buffer; the harness fails if its cases miss one of them."""
    exe = str(tmp_path / "caps_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("caps emu ok:"), r.stdout


def test_every_mutant_of_the_caps_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 12
    jobs = [("unmodified", None, "12345")] + [(m[0], m, "12345") for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
