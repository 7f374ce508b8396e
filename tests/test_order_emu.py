"""The kernels of the key-ordered window on the host: bifromq_amd/csrc/bmq_order_kernels.h compiled by g++ against the wave64 emulator
(tools/emu/order_emu.cpp) and compared with a brute force over std::sort and memcmp.  Then: can this tier notice a wrong kernel?  Single-line
mutants of a copy of bifromq_amd/csrc in a temporary directory (none is ever built into a library or run on a GPU), each compiled into the
harness: every one must make it fail -- a row, a count, a coverage floor, or an abort -- and the unmodified copy must pass.  A mutant that
survives is a blind spot of the harness, not of this test."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")
HARNESS = os.path.join(ROOT, "tools", "emu", "order_emu.cpp")
ROUNDS = 2
TIMEOUT_S = 600

KERN, CORE = "bmq_order_kernels.h", "bmq_order_core.h"
# (name, file, exact source substring -- it must occur exactly once --, replacement, what the mutant does)
MUTANTS = [
    ("F1", CORE, "return (c.flags & 2u) ? d > 0 : d >= 0;", "return d >= 0;", "an exclusive cursor lets its own key pass"),
    ("F2", CORE, "    if (len == 0) return false;\n", "    if (len == 0) return true;\n", "dead ids are candidates"),
    ("F3", CORE, "if ((c.flags & 1u) == 0) return true;", "if ((c.flags & 1u) == 0) return false;", "without a cursor nothing passes"),
    ("F4", CORE, "if ((c.flags & 5u) != 5u) return;", "if ((c.flags & 5u) != 4u) return;", "a cursor given by id is never resolved through the key store"),
    ("C1", CORE, "return __builtin_bswap32(x[w]) < __builtin_bswap32(y[w]) ? -1 : 1;", "return x[w] < y[w] ? -1 : 1;",
     "the first word that differs is compared as a little-endian number: its LAST byte decides"),
    ("C2", CORE, "const uint32_t c = (uint32_t)(m - i < 16 ? m - i : 16);", "const uint32_t c = 16;",
     "the chunks are not cut at the shorter key: what follows it in the pool decides against a key it is a prefix of"),
    ("C3", CORE, "    return an < bn ? -1 : (an > bn ? 1 : 0);\n}\n// The bin of route", "    return 0;\n}\n// The bin of route", "a proper prefix compares equal to its extension"),
    ("B1", CORE, "if (order_compare(ix.kpool, ix.kref[piv[mid]], r) < 0) lo = mid + 1;", "if (order_compare(ix.kpool, ix.kref[piv[mid]], r) <= 0) lo = mid + 1;",
     "an upper bound where the lower bound belongs: a pivot lands in the bin behind itself"),
    ("B2", CORE, "return 2 * lo + (lo < P && piv[lo] == id ? 1u : 0u);", "return 2 * lo;", "a pivot shares the bin of the keys below it: the bin that is split again holds a pivot"),
    ("R1", CORE, "ix.kref[ids[(size_t)j * stride]]) < 0;", "ix.kref[ids[(size_t)j * stride]]) > 0;", "the ranks run from the largest key down"),
    ("R2", CORE, "ix.kref[ids[(size_t)k * stride]], ix.kref[ids[(size_t)j * stride]]) < 0;", "ix.kref[ids[(size_t)k * stride]], ix.kref[ids[j]]) < 0;",
     "a pivot is ranked as the key of another row of the list"),
    ("R4", KERN, "for (uint32_t k0 = 0; k0 < n; k0 += 64) {", "for (uint32_t k0 = 0; k0 + 64 <= n; k0 += 64) {", "the keys behind the last full step of 64 are never counted"),
    ("R5", KERN, "rank += (uint32_t)__popcll(o_ballot(k < n && order_below_one(ix, ids, stride, k, j)));", "rank += (uint32_t)__popcll(o_ballot(order_below_one(ix, ids, stride, k, j)));",
     "lanes behind the list's end compare whatever follows it"),
    ("L1", KERN, "if (lane == 0 && rank < lf.keep) out[lf.out_off + rank] = src[j];", "if (lane == 0 && rank <= lf.keep) out[lf.out_off + rank] = src[j];",
     "a bucket writes one row more than it keeps"),
    ("L2", KERN, "const uint32_t* src = (lf.list ? list1 : list0) + lf.off;", "const uint32_t* src = (lf.list ? list1 : list0);", "a bucket's ids are read from the head of the list"),
    ("L3", KERN, "const uint32_t j = blockIdx.x % ORDER_BUCKET_MAX, lane = threadIdx.x;\n    if (j >= lf.n) return;", "const uint32_t j = blockIdx.x % ORDER_BUCKET_MAX, lane = threadIdx.x;\n    if (j > lf.n) return;",
     "the key slot behind a bucket's last key is ranked and written too"),
    ("K1", KERN, "if (in) cand[at + o_below(m)] = (uint32_t)i;", "if (in) cand[at + lane] = (uint32_t)i;", "the candidates are not compacted: holes, and rows behind the count"),
    ("K2", KERN, "        at = __shfl(at, 0);\n", "        at = __shfl(at, 1);\n", "the wave's place in the candidate list is read from a lane that did not take it"),
    ("K3", KERN, "for (uint32_t p = lane; p < c.len; p += 64) s_key[wave][p] = c.key[p];", "for (uint32_t p = lane; p < c.len; p += 128) s_key[wave][p] = c.key[p];",
     "half of a cursor longer than a wave is never staged"),
    ("K4", KERN, "base < n_ids; base += (unsigned long long)gridDim.x * ORD_BLOCK)", "base < n_ids; base += (unsigned long long)gridDim.x * 64u)",
     "the flag pass strides by a wave where it owns a workgroup: ids are flagged more than once"),
    ("H1", KERN, "atomicAdd(&s_hist[wave][bin], 1u);", "atomicAdd(&s_hist[0][bin], 1u);", "every wave counts into the first wave's slice of the histogram"),
    ("H2", KERN, "        if (v) atomicAdd(hist + b, v);\n", "        if (v) hist[b] = v;\n", "a wave's counts replace the counts of the waves before it"),
    ("S1", KERN, "const bool mine = pending && bin == lb;", "const bool mine = pending;", "every kept lane of a wave is filed under the leader's bin"),
    ("S2", KERN, "dst[to + at + o_below(m)] = id;", "dst[to + at] = id;", "the lanes of a bin all write the first place their wave took"),
    ("S3", KERN, "if (lane == leader) at = atomicAdd(cursor + lb, (uint32_t)__popcll(m));", "if (lane == leader) at = atomicAdd(cursor + lb, 1u);",
     "a wave takes one place for all its ids of a bin"),
    ("S4", KERN, "const uint32_t to = i < n ? base[bin] : ORDER_DROP;", "const uint32_t to = base[bin];", "the lanes behind the list's end scatter an id of their own"),
    ("P1", KERN, "if (lane == 0) piv[rank] = list[(size_t)j * stride];", "if (lane == 0) piv[rank] = list[j];",
     "the pivots written are the head of the list, not the rows that were ranked"),
    ("T1", KERN, "const uint32_t rank = o_rank_wave(ix, src, lf.n, 1u, j, lane);", "const uint32_t rank = o_rank_wave(ix, src, lf.keep, 1u, j, lane);",
     "a bucket's keys are ranked among its first keep rows only"),
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
    exe = os.path.join(work, name, "order_emu")
    b = _compile(csrc, exe)
    if b.returncode != 0:
        return name, False, "does not compile: " + b.stderr[-1500:]
    try:
        r = subprocess.run([exe, str(ROUNDS), seed], capture_output=True, text=True, timeout=TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return name, False, "seed %s: no verdict within %d s" % (seed, TIMEOUT_S)
    tail = (r.stdout[-600:] + r.stderr[-1200:]).strip()
    if mutant is None:
        if r.returncode != 0 or not r.stdout.startswith("order emu ok:"):
            return name, False, "seed %s: the unmodified source fails: %s" % (seed, tail)
        return name, True, "passes"
    if r.returncode == 0:
        return name, False, "SURVIVED: order_emu %d %s says ok" % (ROUNDS, seed)
    msg = r.stderr
    told = r.returncode < 0 or any(w in msg for w in (" row ", " count ", " bin ", " rank ", "coverage:", "wave_emu"))
    if not told:
        return name, False, "seed %s: exit %d without a row, count or coverage message: %s" % (seed, r.returncode, tail)
    return name, True, "caught: " + (msg.strip().splitlines() or ["(signal %d)" % -r.returncode])[0][:300]


@pytest.mark.parametrize("seed", [12345, 777])
def test_the_order_kernels_under_the_wave_emulator(tmp_path, seed):
    """tools/emu/order_emu.cpp: every kind of cursor, passes that stride, dropped bins, waves with several bins, full and cut buckets; the
    harness fails if its cases miss one of them."""
    exe = str(tmp_path / "order_emu")
    b = _compile(CSRC, exe)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, str(ROUNDS), str(seed)], capture_output=True, text=True, timeout=TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("order emu ok:"), r.stdout


def test_every_mutant_of_the_order_kernels_is_caught_and_the_unmodified_source_passes(tmp_path):
    assert len({m[0] for m in MUTANTS}) == len(MUTANTS) >= 15
    jobs = [("unmodified", None, "12345")] + [(m[0], m, "12345") for m in MUTANTS]
    with ThreadPoolExecutor(max_workers=U.host_threads()) as pool:
        results = list(pool.map(lambda j: _build_and_run(str(tmp_path), j[0], j[1], j[2]), jobs))
    what = {m[0]: m[4] for m in MUTANTS}
    report = "\n".join("%-12s %-5s %s%s" % (n, "ok" if ok else "FAIL", rep, " [%s]" % what[n] if n in what else "") for n, ok, rep in results)
    print(report)
    assert all(ok for _, ok, _ in results), "\n" + report
