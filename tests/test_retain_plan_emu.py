"""The kernels of the retain plan on the host: bifromq_amd/csrc/bmq_rplan_kernels.h compiled by g++ against the wave64 emulator
(tools/emu/rplan_emu.cpp), on indexes the product's own host builder and apply path make, compared with the rule written plainly there.
Then: can this tier notice a wrong kernel?  Single-line mutants of a copy of bifromq_amd/csrc in a temporary directory (none is ever built
into a library or run on a GPU), each compiled into the harness: every one must make it fail -- an op, a count, a delta, a key, a guard, a
coverage floor, or an abort -- and the unmodified copy must pass.  A mutant that survives is a blind spot of the harness, not of this test.
The sanitizer checker of the same functions on host threads (tools/retain_plan_check.cpp) is built and run here too."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "rplan_emu.cpp")
ROUNDS = 3
TIMEOUT_S = 600

KERN, CORE = "bmq_rplan_kernels.h", "bmq_rplan_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("D1", CORE, "if (id != NONE && !id_dead(m.dead_bits, id)) {", "if (id != NONE) {", "a dead bulk-loaded id counts as present"),
    ("D2", CORE, "if (tid != NONE && tid < m.id_cap && !id_dead(m.dead_bits, tid)) b.found[i] = tid;", "if (tid != NONE && tid < m.id_cap) b.found[i] = tid;",
     "a dead overlay id counts as present"),
    ("D3", CORE, "if (tid != NONE && tid < m.id_cap && !id_dead(m.dead_bits, tid)) b.found[i] = tid;",
     "if (tid == NONE || (tid < m.id_cap && !id_dead(m.dead_bits, tid))) b.found[i] = tid == NONE ? node : tid;", "an overlay node without a topic (topic_id == NONE) counts as present"),
    ("W1", CORE, "    const uint32_t w = b.last[rep];\n", "    const uint32_t w = rep;\n", "the op that claimed the slot wins instead of the last one"),
    ("W2", CORE, "atom_max(&b.last[rep], i);", "b.last[rep] = i;", "the op that ran last wins instead of the last one of the batch"),
    ("T1", CORE, "    if (ti != tj && (b.tenant_off[tj + 1] - b.tenant_off[tj] != tl || !bytes_equal(b.tenants, b.tenant_off[ti], b.tenants, b.tenant_off[tj], tl))) return false;\n", "",
     "topics are compared without their tenants"),
    ("H1", CORE, "if (rep == i || rp_same(b, i, rep)) {", "if (rep == i || rp_hash(b, i) == rp_hash(b, rep)) {", "keys are compared by hash only"),
    ("L1", KERN, "    if (i < b.n) rp_find_one(m, b, (uint32_t)i, have_index != 0);", "    if (i + 1 < b.n) rp_find_one(m, b, (uint32_t)i, have_index != 0);",
     "the last op is never looked up: a dropped tail lane"),
    ("L2", KERN, "    if (i < b.n) action = rp_classify_one(b, (uint32_t)i, dt, dv);", "    if (i + 1 < b.n) action = rp_classify_one(b, (uint32_t)i, dt, dv);", "the last op is never classified"),
    ("L3", KERN, "    if (i < b.n) rp_key_write_one(b, (uint32_t)i, offs, out);", "    if (i + 1 < b.n) rp_key_write_one(b, (uint32_t)i, offs, out);", "the last op's key is never written"),
    ("K1", CORE, "    if (i == w) {\n", "    if (i <= w) {\n", "superseded ops are classified and given keys like winners"),
    ("K2", CORE, "        if (action != RP_NONE) {\n", "        if (true) {\n", "a NONE is given a key"),
    ("E1", CORE, "            if (action == RP_ADD) dv = 1;", "            if (action == RP_ADD || action == RP_UPDATE) dv = 1;",
     "an UPDATE counts as a new topic"),
    ("E2", CORE, "            const uint32_t ti = rp_tenant(b, i);\n            const unsigned long long pb", "            const uint32_t ti = rp_tenant(b, rep);\n            const unsigned long long pb",
     "the delta is filed under the tenant index of the group's representative, not the winner's"),
    ("V1", CORE, "            uint32_t levels = 1;\n", "            uint32_t levels = 0;\n", "the key's level count is one short"),
    ("C1", CORE, "            if (e == 0) e = i + 1u;\n", "            e = i + 1u;\n", "a lane whose CAS was lost goes on as if the slot were its own"),
    ("C2", CORE, "const bool clear = b.clear[w] != 0, present", "const bool clear = b.clear[i] != 0, present", "every op reports its own clear flag, not the winner's"),
    ("X1", KERN, "        const bool mine = pending && dt == lt;\n", "        const bool mine = pending;\n", "the deltas of a wave all go to its first winner's table entry"),
    ("X2", KERN, "const uint32_t sum = (uint32_t)__popcll(up) - (uint32_t)__popcll(down);", "const uint32_t sum = (uint32_t)__popcll(up);", "the removes of a wave are not subtracted"),
    ("N1", KERN, "for (uint32_t a = RP_NONE; a <= RP_REMOVE; a++) {", "for (uint32_t a = RP_NONE; a < RP_REMOVE; a++) {", "the REMOVE winners are not counted"),
]


def _compile(csrc, exe):
    return subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), HARNESS, os.path.join(csrc, "bmq_retain.cpp"),
                           os.path.join(csrc, "bmq_codec.cpp"), "-o", exe], capture_output=True, text=True)


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
    exe = os.path.join(work, name, "rplan_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    try:
        r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or not r.stdout.startswith("rplan emu ok:"):
            return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: rplan_emu %d %s says ok" % (ROUNDS, seed)
    msg = r.stderr
    told = r.returncode < 0 or any(w in msg for w in (": op ", ": count: ", ": delta ", "guard bytes", "coverage:", "wave_emu"))
    if not told:
        return name, False, "seed %s: exit %d without an op, count, delta, guard or coverage message: %s" % (seed, r.returncode, tail)
    return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_plan_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/rplan_emu.cpp: every index state, every duplicate pattern, colliding hashes, lost CAS claims, the group table at its minimum
    size; the harness fails if its cases miss one of them."""
    exe = str(tmp_path / "rplan_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("rplan emu ok:"), r.stdout


def test_every_mutant_of_the_plan_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 12
    jobs = [("unmodified", None, "12345")] + [(m[0], m, "12345") for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report


def test_the_plan_functions_on_host_threads_under_sanitizers():
    """tools/retain_plan_check.cpp (a program of its own, nothing preloaded): the per-item functions of the plan against the rule written plainly,
    under ASan/UBSan, and under TSan with 8 host threads -- the CAS table of the grouping, also at its minimum size."""
    subprocess.run(["make", "-C", CSRC, "rpcheck"], check=True, capture_output=True, timeout=900)
    exe = os.path.join(ROOT, "tools", "retain_plan_check")
    for seed in ("1", "2"):
        r = subprocess.run([exe, "3", seed, "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "retain_plan_check ok" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe + "_tsan", "2", "3", "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "retain_plan_check ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
