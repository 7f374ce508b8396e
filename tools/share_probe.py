#!/usr/bin/env python3
"""Times the shared-subscription resolve (bmq_share_resolve_dev) on the device and prints ONE JSON line.

  leg "c3":    the C3 index of bench.py (1000 tenants x 10k routes; bmq_gen.cpp makes 0.5 % of the routes $share / $oshare groups), every
               group route with a seeded table of 1-200 members; one 1 M-publish batch: match -> bmq_fanout_group_dev -> its
               shared-subscription slice, still in HBM -> bmq_share_resolve_dev with one sender per topic.
  leg "heavy": synthetic, 1 M (pair, sender) items over ordered groups of 200 members each.

Per step of the resolve: HIP-event times (bmq_set_kernel_timing -> bmq_share_info.ms_*), medians over --reps calls after --warmup calls;
per call: wall time of the C-ABI call (it returns after a stream synchronise), and that of bmq_fanout_group_dev on the same batch for
scale.  rows/s and scores/s are over the resolve KERNEL's time.  Needs a gfx950 device: there is no fallback.

  python tools/share_probe.py [--topics 1000000] [--heavy-items 1000000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd import _lib  # noqa: E402

NONE = 0xFFFFFFFF


class Hbm:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        if self.hip.hipMalloc(C.byref(p), a.nbytes + 64) != 0:
            raise MemoryError("hipMalloc(%d)" % a.nbytes)
        if a.nbytes and self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy to the device")
        self.bufs.append(p)
        return p.value

    def zeros(self, n, dtype=np.uint32):
        return self.put(np.zeros(max(int(n), 1), dtype=dtype))

    def get(self, p, n, dtype=np.uint32):
        out = np.zeros(int(n), dtype=dtype)
        if n and self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy from the device")
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


def member_tables(rng, route_ids, lo, hi, chunk=4000):
    """seeded member lists of lo..hi members per group route -> yields ({route id: [urls]}, member counts)"""
    for at in range(0, len(route_ids), chunk):
        ids = route_ids[at:at + chunk]
        counts = rng.integers(lo, hi + 1, size=len(ids))
        out = {}
        for rid, n in zip(ids.tolist(), counts.tolist()):
            brokers = rng.integers(0, 4, size=n).tolist()
            dkeys = rng.integers(0, 64, size=n).tolist()
            out[rid] = ["%d\0inbox-%d-%d\0deliverer%02d" % (b, rid, m, d) for m, (b, d) in enumerate(zip(brokers, dkeys))]
        yield out, counts


def timed_resolve(eng, args, reps, warmup):
    """-> (n_rows, n_groups, special, {step: median ms}, median wall ms)"""
    steps = {k: [] for k in ("count_scan", "rows", "resolve_kernel", "sort", "groups")}
    wall = []
    for i in range(warmup + reps):
        a = list(args)
        a[7] = 0x9E3779B97F4A7C15 * (i + 1)  # a fresh nonce per batch
        t0 = time.perf_counter()
        nr, ng, sp = eng.share_resolve_device(*a)
        dt = (time.perf_counter() - t0) * 1e3
        if i < warmup:
            continue
        wall.append(dt)
        inf = eng.share_info()
        for k, v in zip(steps, (inf.ms_count, inf.ms_rows, inf.ms_resolve, inf.ms_sort, inf.ms_group)):
            steps[k].append(float(v))
    return nr, ng, sp, {k: float(np.median(v)) for k, v in steps.items()}, float(np.median(wall))


def leg_c3(n_topics, reps, warmup):
    seed = 0xB1F20003
    w = B.Workload(seed, 1000, 10_000, 1)
    eng = B.Engine(device=0, kernel_timing=True)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    ends = ko[1:].astype(np.int64)
    rlen = kb[ends - 2].astype(np.int64) * 256 + kb[ends - 1]
    flag = kb[ends - 3 - rlen]
    group_ids = np.nonzero((flag == 2) | (flag == 3))[0].astype(np.uint32)  # ids = ranks of the sorted keys
    for rid in group_ids[:: max(1, len(group_ids) // 16)].tolist():  # ... which the generator yields in order: checked, not assumed
        if eng.route_key(rid) != kb[ko[rid]:ko[rid + 1]].tobytes():
            raise SystemExit("route id %d is not the rank of its key" % rid)
    rng = np.random.default_rng(20261016)
    members_of = np.zeros(w.n_keys, dtype=np.uint32)
    t0 = time.perf_counter()
    for tabs, counts in member_tables(rng, group_ids, 1, 200):
        eng.share_members_apply(tabs)
        members_of[np.fromiter(tabs.keys(), dtype=np.uint32)] = counts
    t_apply = time.perf_counter() - t0
    inf = eng.share_info()
    mem = Hbm()
    tdata, toff = w.tenants_packed()
    data, off, tt = w.topics(seed + 1000, n_topics, grouped=True)
    cap = 32 * n_topics  # (a C3 batch of 1 M publishes matches 18 M routes)
    d = [mem.put(x) for x in (tdata, toff, tt, data, off)]
    d_row, d_ids, d_tot = mem.zeros(n_topics + 1), mem.zeros(cap), mem.zeros(1, np.uint64)
    eng.match_batch_device(d[0], d[1], w.n_tenants, d[2], d[3], d[4], n_topics, d_row, d_ids, cap, d_tot)
    total = eng.finish()
    gcap = 1 << 16
    d_ot, d_or, d_goff, d_grep = mem.zeros(total), mem.zeros(total), mem.zeros(gcap + 1), mem.zeros(gcap)
    fo_ms = []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        ng, sp = eng.fanout_group_device(d_row, d_ids, n_topics, total, d_ot, d_or, d_goff, d_grep, gcap)
        if i:
            fo_ms.append((time.perf_counter() - t0) * 1e3)
    if not sp & 1:
        raise SystemExit("the batch matched no shared-subscription route")
    goff, grep = mem.get(d_goff, ng + 1), mem.get(d_grep, ng)
    g = int(np.nonzero(grep == 0xFFFFFFFE)[0][0])
    lo, hi = int(goff[g]), int(goff[g + 1])
    n_pairs = hi - lo
    sender_off = np.arange(n_topics + 1, dtype=np.uint32)  # one publisher per topic
    sender_hash = rng.integers(-(1 << 31), 1 << 31, size=n_topics).astype(np.int32)
    d_so, d_sh = mem.put(sender_off), mem.put(sender_hash)
    d_out = [mem.zeros(n_pairs) for _ in range(3)] + [mem.zeros(gcap + 1)]
    a = (d_ot + 4 * lo, d_or + 4 * lo, n_pairs, d_so, d_sh, n_topics, n_topics, 0, d_out[0], d_out[1], d_out[2], n_pairs, d_out[3], gcap)
    nr, nsg, ssp, steps, wall = timed_resolve(eng, a, reps, warmup)
    routes = mem.get(d_or + 4 * lo, n_pairs)
    o_pair, o_sender = mem.get(d_out[0], nr), mem.get(d_out[1], nr)
    scores = int(members_of[routes[o_pair[o_sender != NONE]]].sum())
    k_ms = steps["resolve_kernel"]
    out = {"index_routes": int(w.n_keys), "group_routes": int(len(group_ids)), "members": int(inf.n_members), "share_deliverers": int(inf.n_deliverers),
           "table_device_bytes": int(inf.device_bytes), "members_apply_s": t_apply, "publishes": n_topics, "matched_pairs": int(total),
           "shared_pairs": n_pairs, "rows": int(nr), "ordered_rows": int((o_sender != NONE).sum()), "groups": int(nsg), "special": int(ssp), "scores": scores,
           "ms_steps": steps, "ms_call_wall": wall, "ms_fanout_group_dev_wall": float(np.median(fo_ms)),
           "rows_per_s": nr / (k_ms * 1e-3) if k_ms else None, "scores_per_s": scores / (k_ms * 1e-3) if k_ms else None}
    mem.free()
    eng.close()
    return out


def leg_heavy(n_items, reps, warmup, n_groups=1000, n_members=200):
    keys = sorted(B.route_key_from_mqtt("heavy", "$oshare/g%d/f/%d" % (i % 16, i)) for i in range(n_groups))
    eng = B.Engine(device=0, kernel_timing=True).rebuild(keys)
    rng = np.random.default_rng(7)
    for tabs, _ in member_tables(rng, np.arange(n_groups, dtype=np.uint32), n_members, n_members):
        eng.share_members_apply(tabs)
    inf = eng.share_info()
    mem = Hbm()
    pt = np.arange(n_items, dtype=np.uint32)
    pr = rng.integers(0, n_groups, size=n_items).astype(np.uint32)
    so = np.arange(n_items + 1, dtype=np.uint32)
    sh = rng.integers(-(1 << 31), 1 << 31, size=n_items).astype(np.int32)
    gcap = 4096
    d = [mem.put(x) for x in (pt, pr, so, sh)]
    o = [mem.zeros(n_items) for _ in range(3)] + [mem.zeros(gcap + 1)]
    a = (d[0], d[1], n_items, d[2], d[3], n_items, n_items, 0, o[0], o[1], o[2], n_items, o[3], gcap)
    nr, ng, sp, steps, wall = timed_resolve(eng, a, reps, warmup)
    k_ms = steps["resolve_kernel"]
    scores = int(nr) * n_members
    out = {"groups_in_index": n_groups, "members_per_group": n_members, "table_device_bytes": int(inf.device_bytes), "items": n_items, "rows": int(nr),
           "groups": int(ng), "scores": scores, "ms_steps": steps, "ms_call_wall": wall, "rows_per_s": nr / (k_ms * 1e-3) if k_ms else None,
           "scores_per_s": scores / (k_ms * 1e-3) if k_ms else None}
    mem.free()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--heavy-items", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    out = {"probe": "share_resolve", "library": _lib.lib().bmq_version().decode(), "reps": args.reps, "warmup": args.warmup,
           "timing": "ms_steps: HIP events on the engine stream, median of reps; *_wall: host clock around the C-ABI call, which returns after a stream synchronise",
           "c3": leg_c3(args.topics, args.reps, args.warmup), "heavy": leg_heavy(args.heavy_items, args.reps, args.warmup)}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
