"""Can the CPU tier notice a wrong k_walk?  Single-line mutants of bifromq_amd/csrc (a copy in a temporary directory: none is ever built into a library or
run on a GPU), each compiled into tools/emu/walk_emu.cpp and run under the wave emulator: every one must make the harness fail -- a row that differs
from the rule, a count of discovered nodes that differs from the node model, a coverage floor missed, or an abort of the emulator -- and the unmodified
copy must pass.  The table is the definition of "the harness sees tail records, visit counts and child filter words": a mutant that survives is a blind
spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
ROUNDS = 8  # (the harness' coverage floors hold from 8 rounds on)
TIMEOUT_S = 900

WALK = "bmq_walk_kernel.h"
BUILD = "bmq_build_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    # tail records
    ("S1", WALK, "ok = ok && rem > 1u && (r1 == TOK_PLUS || r1 == tnext2);", "ok = ok && (r1 == TOK_PLUS || r1 == tnext2);",
     "second record level compared without `rem > 1u`: reads the next topic's token"),
    ("S2", WALK, "ok = ok && rem > 2u && (r2 == TOK_PLUS", "ok = ok && rem > 1u && (r2 == TOK_PLUS",
     "third record level guarded by `rem > 1u`: rows for a topic that ends early"),
    ("S3", WALK, "(r2 == TOK_PLUS || r2 == tokens[tp + 3])", "(r2 == tokens[tp + 3])", "a '+' at the record's third level matches nothing"),
    ("S4", WALK, "(r3 == TOK_PLUS || r3 == tokens[tp + 4])", "(r3 == tokens[tp + 4])", "a '+' at the record's fourth level matches nothing"),
    ("S5", WALK, "(plus_here ? 2u : 1u) + n_tail);", "(plus_here ? 2u : 1u));", "the levels a record resolves are not counted as discovered nodes"),
    ("S6", BUILD, "        tail_invalidate(ix, child, sa);\n", "", "locate leaves the records beside the nodes of a changed path alone: stale records answer"),
    ("T0", WALK, "bool ok = (r0 == TOK_PLUS || r0 == tnext);", "bool ok = (r0 == tnext);", "a '+' at the record's first level matches nothing"),
    ("T1", WALK, "q_own_count = (reach && !is_hash && rem == k) ? cnt : 0u;", "q_own_count = (reach && !is_hash) ? cnt : 0u;",
     "a record's own routes emitted for topics that go on below the leaf"),
    # visit counts
    ("V1", WALK, "(plus_here ? 2u : 1u) + n_tail);", "1u + n_tail);", "the '+' child resolved beside its parent is not counted"),
    ("V2", WALK, "            if (part != 0 && actp) cnt_visit[ln] += 1u; // (the lane's own topic; the drain's atomics come later)\n", "",
     "the root's '+' child and its '+' child, resolved at the wave's start, are not counted"),
    # child filter words (controls: the harness caught these before the directed family came)
    ("C1", WALK, "? FILTER_NONE : own_begin) >> (fh >> 27))", "? FILTER_NONE : own_begin) >> ((fh >> 27) ^ 1u))", "wrong own-bit index in the drain's node decision"),
    ("C2", WALK, "const uint32_t ph = tnext2 * FILTER_MUL;", "const uint32_t ph = tnext * FILTER_MUL;", "tnext in place of tnext2 in the '+'-sibling decision"),
    ("C3", WALK, "(f_hash >> ((fh >> 22) & 31u))", "(f_hash >> (fh >> 27))", "the boot decision's hash word shifted by the own index"),
    ("C4", WALK, "(((hash_count | f_off) != 0 ? FILTER_NONE : hash_begin)", "((f_off != 0 ? FILTER_NONE : hash_begin)", "hash_count ignored in the drain decision"),
    ("C5", BUILD, "atom_or(&ps.hash_begin, b_hash);", "(void)b_hash;", "locate does not OR the child's bit into the hash word"),
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
    exe = os.path.join(work, name, "walk_emu")
    cmd = ["g++", "-O1", "-std=c++17", "-I", csrc, "-I", os.path.join(ROOT, "tools", "emu"), os.path.join(ROOT, "tools", "emu", "walk_emu.cpp"),
           os.path.join(csrc, "bmq_codec.cpp"), "-o", exe, "-pthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    for seed in seeds:
        try:
            r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
        tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
        if mutant is None:
            if r.returncode != 0 or not r.stdout.startswith("walk emu ok:"):
                return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
            continue
        if r.returncode == 0:
            return name, False, "SURVIVED: walk_emu %d %s says ok" % (ROUNDS, seed)
        msg = r.stderr
        told = r.returncode < 0 or any(w in msg for w in (" row ", "visits:", "coverage:", "wave_emu", "Sanitizer", "runtime error"))
        if not told:
            return name, False, "seed %s: exit %d without a row, visit or coverage message: %s" % (seed, r.returncode, tail)
        return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[-1][:300]
    return name, True, "passes"


def test_every_mutant_of_k_walk_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS)
    # (the unmodified source runs all its rounds, twice: a job per seed, first in the queue)
    jobs = [("unmodified/%s" % s, None, [s]) for s in ("12345", "777")] + [(m[0], m, ["12345"]) for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0].replace("/", "_"), j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-16s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
