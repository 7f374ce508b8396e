"""The kernels of the delivery plan on the host: bifromq_amd/csrc/bmq_delivery_kernels.h compiled by g++ against the wave64 emulator
(tools/emu/delivery_emu.cpp) and compared with a stable merge by key bytes.  Then: can this tier notice a wrong kernel?  Single-line mutants of
a copy of bifromq_amd/csrc in a temporary directory (none is ever built into a library or run on a GPU), each compiled into the harness: every
one must make it fail -- an output row, a count, a coverage floor, or an abort -- and the unmodified copy must pass.  A mutant that survives is
a blind spot of the harness, not of this test.

One decision a reader might look for is not in the table because it is not in the kernels: the sender takes no part in the rank search.  A
route is normal or shared, never both, so a pair and a member row never agree in (topic, route); rows that do are neighbours in one list
already, in sender order.  What a row carries of its sender is its side index (mutant A1)."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "delivery_emu.cpp")
ROUNDS = 6
TIMEOUT_S = 600

KERN, CORE = "bmq_delivery_kernels.h", "bmq_delivery_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("V1", CORE, "|| !dl_same_deliverer(P.sd_bytes, a, ix.kpool, c)) g = DL_NONE;", "|| false) g = DL_NONE;",
     "the probe's byte verify is dropped: a hash that agrees merges two keys"),
    ("M1", CORE, "if (slot < st.gt_cap) P.slot_group[slot] = g;", "if (slot < st.gt_cap) P.slot_group[slot] = 0;", "every slot of the batch names group 0"),
    ("M2", CORE, "            if (cur != h) continue;\n", "            if (cur != h) break;\n", "the probe stops at the first slot that holds another hash"),
    ("M3", CORE, "if (sd >= P.n_sd) { // rows without a member", "if (sd > P.n_sd) { // rows without a member", "the unresolved rows are looked up as a share-deliverer number"),
    ("N1", CORE, "else if (g == DL_NONE) g = P.n_norm + P.new_scan[j] - 1;", "else if (g == DL_NONE) g = P.new_scan[j] - 1;",
     "a group reached through members only is filed under group 0 and its neighbours"),
    ("N2", CORE, "if (g == DL_UNRESOLVED) g = P.n_norm + P.n_new;", "if (g == DL_UNRESOLVED) g = P.n_norm;", "the unresolved group is filed under the first member-only group"),
    ("K1", CORE, "P.cnt[g] = (hi - lo) + (j == DL_NONE ? 0u : P.r_off[j + 1] - P.r_off[j]);", "P.cnt[g] = (hi - lo);", "the member rows are left out of a group's size"),
    ("B1", CORE, "        if (off[mid] <= i) lo = mid;\n", "        if (off[mid] < i) lo = mid;\n",
     "the group of a row: a lower bound where the upper bound belongs -- the first row of a group lands in the group before"),
    ("B2", CORE, "        if (dl_key(P.g_topic[p], P.g_route[p]) < key) lo = mid + 1;\n", "        if (dl_key(P.g_topic[p], P.g_route[p]) > key) lo = mid + 1;\n",
     "the rank among the member rows is searched the wrong way round"),
    ("S1", CORE, "    dst += g ? P.cnt_scan[g - 1] : 0u;\n", "    dst += g ? P.cnt_scan[g] : 0u;\n", "the group's base is taken from its own scan element: the base of the NEXT group"),
    ("S2", CORE, "P.out_group_off[i] = i ? P.cnt_scan[i - 1] : 0u;", "P.out_group_off[i] = P.cnt_scan[i];", "the offsets are the inclusive scan: group ends in place of starts"),
    ("A1", CORE, "        aux = r;\n", "        aux = r - P.r_off[j];\n", "a member row's side index counts inside its share group: the sender and member of another row"),
    ("T1", KERN, "    if (i < n) dl_merge_one(P, i, hint);", "    if (i + 1 < n) dl_merge_one(P, i, hint);", "the last row of the batch is never written"),
    ("W1", CORE, "hint.kind == 1 && p < hint.hi ? hint.k", "hint.kind == 1 && p <= hint.hi ? hint.k",
     "the wave's hint reaches one pair too far: the first pair of the next group is filed under the hint's group"),
    ("W2", CORE, "hint.kind == 2 && r < hint.hi ? hint.k", "hint.kind == 2 && r <= hint.hi ? hint.k", "... and the same for the first member row of the next share group"),
    ("T2", CORE, "    if (i <= P.n_groups) P.out_group_off[i]", "    if (i < P.n_groups) P.out_group_off[i]", "the end offset is never written"),
    ("T3", CORE, "return i < P.s0 ? i : i + (P.s1 - P.s0);", "return i <= P.s0 ? i : i + (P.s1 - P.s0);",
     "the first pair behind the shared slice is taken from the slice"),
    ("T4", KERN, "    if (j < P.n_sgroups) dl_map_one(ix, st, P, j);", "    if (j + 1 < P.n_sgroups) dl_map_one(ix, st, P, j);", "the last share group is never mapped"),
    ("D1", CORE, "lo = P.s1, hi = P.total;", "lo = P.s0, hi = P.total;", "the dead group's pairs begin with the shared slice"),
    ("D2", CORE, "else if (P.has_dead && g + 1 == P.n_groups) lo", "else if (P.has_dead) lo", "every group behind the normal ones owns the dead pairs"),
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
    exe = os.path.join(work, name, "delivery_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    try:
        r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or not r.stdout.startswith("delivery emu ok:"):
            return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: delivery_emu %d %s says ok" % (ROUNDS, seed)
    msg = r.stderr
    told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", "coverage:", "wave_emu"))
    if not told:
        return name, False, "seed %s: exit %d without a row, count or coverage message: %s" % (seed, r.returncode, tail)
    return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_delivery_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/delivery_emu.cpp: keys in the batch, absent from it and unknown, planted hashes, lists that end at waves and workgroups, both
    special groups; the harness fails if its cases miss one of them."""
    exe = str(tmp_path / "delivery_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("delivery emu ok:"), r.stdout


def test_every_mutant_of_the_delivery_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 12
    jobs = [("unmodified", None, "12345")] + [(m[0], m, "12345") for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
