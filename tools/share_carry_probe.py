#!/usr/bin/env python3
"""What bmq_config.share_carry costs and what it replaces, and what bmq_routes_find costs; writes profiles/share_carry.json.

On the C3 index of bench.py (1000 tenants x 10 k routes; bmq_gen.cpp makes 0.5 % of the routes $share / $oshare groups), every group route
with a seeded member table of 1-200 members (as tools/share_probe.py loads them), in one run:

  1. share_carry = 0: wall time of bmq_compact_swap, and of giving every table again with bmq_share_members_apply -- what a caller needs today
     after every swap and the carry replaces (the C-ABI calls alone, over pre-packed URLs; the ids come from bmq_routes_find first).
  2. share_carry = 1: wall time of bmq_compact_swap, the three HIP-event parts of the carry (bmq_share_carry_info), and how much longer the
     swap holds the engine lock than (1)'s swap (the swap holds it from entry to return: the difference of the medians).
  3. bmq_routes_find of 100 000 keys sampled from the index: wall time.  The kernels' own times come from a run of their own,
     `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/share_carry_probe.py --kernel-only` (k_b_find_keys of the same 100 000 keys, and
     k_b_locate of a 100 000-op apply beside it for scale only; tracing slows the host, so no wall time of that run is reported);
     --kernel-stats CSV folds the two rows of its *kernel_stats.csv into the JSON.

Every timed quantity: --warmup rounds first, then the median, min and max of --reps >= 7 rounds (a round = one whole generation change:
bmq_compact_begin, bmq_compact_poll to the end, bmq_compact_swap).  The probe exits with an error if the carried tables differ from the
re-applied ones, per key: the URLs in order (every member of every table, and each table's member count) and the ordered flag (the rows of one resolve over every group route, which differ with the flag).
Needs a gfx950 device: there is no fallback.

  python tools/share_carry_probe.py [--tenants 1000] [--routes 10000] [--device 0] [--reps 7] [--warmup 1] [--kernel-only] [--kernel-stats CSV] [--out FILE]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd import _lib  # noqa: E402
from bifromq_amd.engine import _ptr, pack  # noqa: E402

SEED = 0xB1F20003
N_FIND = 100_000
NONE = 0xFFFFFFFF


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def load(tenants, routes, share_carry, device=0):
    w = B.Workload(SEED, tenants, routes, 1)
    eng = B.Engine(device=device, kernel_timing=True, share_carry=share_carry)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    return w, eng, kb, ko


def group_keys(kb, ko):
    ends = ko[1:].astype(np.int64)
    rlen = kb[ends - 2].astype(np.int64) * 256 + kb[ends - 1]
    flag = kb[ends - 3 - rlen]
    idx = np.nonzero((flag == 2) | (flag == 3))[0]
    return [kb[ko[i]:ko[i + 1]].tobytes() for i in idx.tolist()], flag[idx]


class Tables:
    """seeded member lists per group KEY (1-200 members), packed once in chunks of 4000 tables; only the ids change with the generation"""

    def __init__(self, keys, chunk=4000):
        rng = np.random.default_rng(20261016)
        self.keys, self.packed_keys = keys, pack(keys)
        self.counts = rng.integers(1, 201, size=len(keys))
        self.urls, self.chunks = [], []
        for at in range(0, len(keys), chunk):
            part = []
            for j in range(at, min(len(keys), at + chunk)):
                n = int(self.counts[j])
                brokers, dkeys = rng.integers(0, 4, size=n).tolist(), rng.integers(0, 64, size=n).tolist()
                part.append(["%d\0inbox-%d-%d\0deliverer%02d" % (b, j, m, d) for m, (b, d) in enumerate(zip(brokers, dkeys))])
            self.urls += part
            moff = np.zeros(len(part) + 1, dtype=np.uint32)
            moff[1:] = np.cumsum([len(p) for p in part])
            data, off = pack([u.encode() for p in part for u in p])
            self.chunks.append((at, len(part), moff, data, off))

    def apply(self, eng):
        """-> (ms of bmq_routes_find for the ids, ms of the bmq_share_members_apply calls)"""
        t0 = time.perf_counter()
        ids = eng.find_routes(packed=self.packed_keys)
        t1 = time.perf_counter()
        if (ids == NONE).any():
            raise SystemExit("a group key has no id")
        for at, n, moff, data, off in self.chunks:
            part = np.ascontiguousarray(ids[at:at + n])
            eng._check(_lib.lib().bmq_share_members_apply(eng.h, _ptr(part), n, _ptr(moff), _ptr(data), _ptr(off)))
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def generation_change(eng):
    """-> ms of the swap alone"""
    eng.compact_begin()
    while eng.compact_poll(65536) < 1000:
        pass
    t0 = time.perf_counter()
    eng.compact_swap()
    return (time.perf_counter() - t0) * 1e3


def compare(a, b, tabs, flags):
    """the carried tables of b against the re-applied ones of a, per key"""
    ia, ib = a.find_routes(packed=tabs.packed_keys), b.find_routes(packed=tabs.packed_keys)
    sa, sb = a.share_info(), b.share_info()
    if (sa.n_tables, sa.n_members) != (sb.n_tables, sb.n_members) or sa.n_tables != len(tabs.keys):
        raise SystemExit("tables / members differ: re-applied %d / %d, carried %d / %d" % (sa.n_tables, sa.n_members, sb.n_tables, sb.n_members))
    rng = np.random.default_rng(5)
    for j, urls in enumerate(tabs.urls):
        n = len(urls)
        for m in range(n):
            ua, ub = a.share_member(int(ia[j]), m), b.share_member(int(ib[j]), m)
            if not ua == ub == urls[m].encode():
                raise SystemExit("member %d of table %d differs" % (m, j))
        for eng, ids in ((a, ia), (b, ib)):
            try:
                eng.share_member(int(ids[j]), n)
            except B.BmqError:
                continue
            raise SystemExit("table %d has more members than it was given" % j)
    # the ordered flag: one pair per group route, two senders per topic -- an ordered route gives a row per sender, an unordered one a single row
    n = len(tabs.keys)
    so = np.arange(0, 2 * n + 1, 2, dtype=np.uint32)
    sh = rng.integers(-(1 << 31), 1 << 31, size=2 * n).astype(np.int32)
    ra = a.share_resolve(np.arange(n, dtype=np.uint32), ia, so, sh, nonce=77, group_cap=4096)
    rb = b.share_resolve(np.arange(n, dtype=np.uint32), ib, so, sh, nonce=77, group_cap=4096)
    rows = lambda r: sorted(zip(r[0].tolist(), r[1].tolist(), r[2].tolist()))
    if rows(ra) != rows(rb) or len(ra[0]) != int(n + (flags == 3).sum()):
        raise SystemExit("the resolve rows of the carried tables differ from those of the re-applied ones")
    return {"tables": int(sb.n_tables), "members": int(sb.n_members), "members_compared": "every member of every table, in order, and each table's member count",
            "resolve_rows_compared": len(ra[0])}


def find_and_locate(eng, w, kb, ko, reps, warmup):
    rng = np.random.default_rng(9)
    pick = rng.integers(0, w.n_keys, size=N_FIND)
    packed = pack([kb[ko[i]:ko[i + 1]].tobytes() for i in pick.tolist()])
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        ids = eng.find_routes(packed=packed)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    if (ids == NONE).any():
        raise SystemExit("a sampled key was not found")
    # for scale: one apply of as many ops (puts of keys that are there: nothing changes, k_b_locate walks the same paths)
    ops = np.zeros(N_FIND, dtype=np.uint8)
    ams = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        eng._check(_lib.lib().bmq_routes_apply(eng.h, _ptr(packed[0]), _ptr(packed[1]), _ptr(ops), N_FIND))
        if i >= warmup:
            ams.append((time.perf_counter() - t0) * 1e3)
    return {"keys": N_FIND, "ms_routes_find_wall": spread(ms), "keys_per_s": N_FIND / (float(np.median(ms)) * 1e-3),
            "ms_routes_apply_wall_same_keys_as_puts": spread(ams)}


def kernel_rows(path):
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or ""
            for k in ("k_b_find_keys", "k_b_locate", "k_sh_rekey"):
                if k in name:
                    total_ns, n = float(r["TotalDurationNs"]), int(float(r["Calls"]))
                    out[k] = {"calls": n, "total_ns": total_ns, "mean_us": total_ns / max(1, n) / 1e3, "min_ns": float(r["MinNs"]), "max_ns": float(r["MaxNs"])}
    if "k_b_find_keys" not in out or "k_b_locate" not in out:
        raise SystemExit("no k_b_find_keys / k_b_locate rows in %s" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--device", type=int, default=0, help="-1: a host-only engine (a dry run of the probe itself: its numbers mean nothing)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", action="store_true", help="bmq_routes_find and the apply of 100 000 keys only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run: its k_b_find_keys / k_b_locate rows go into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "share_carry.json"))
    args = ap.parse_args()
    if args.device < 0 and os.path.abspath(args.out) == os.path.abspath(ap.get_default("out")):
        raise SystemExit("--device -1 is a dry run of the probe: give it an --out of its own, not the committed profile")
    if args.reps < 7:
        raise SystemExit("--reps must be at least 7")
    out = {"probe": "tools/share_carry_probe.py", "device": "MI355X (gfx950), one GPU, one run" if args.device >= 0 else "host-only engine: a dry run of the probe", "library": _lib.lib().bmq_version().decode(),
           "workload": "C3: %d tenants x %d routes, a member table of 1-200 members on every group route" % (args.tenants, args.routes),
           "timing": "host clock around C-ABI calls that return after a stream synchronise; ms_gather / ms_find / ms_rekey: HIP events; %d warm-up round(s), "
                     "then median / min / max of %d rounds" % (args.warmup, args.reps)}
    w, a, kb, ko = load(args.tenants, args.routes, 0, args.device)
    if args.kernel_only:
        out["routes_find"] = find_and_locate(a, w, kb, ko, args.reps, args.warmup)
        print(json.dumps(out))
        a.close()
        return
    keys, flags = group_keys(kb, ko)
    tabs = Tables(keys)
    out["index_routes"], out["group_routes"], out["members"] = int(w.n_keys), len(keys), int(tabs.counts.sum())
    first = tabs.apply(a)
    swap0, again, lookups = [], [], []
    for i in range(args.warmup + args.reps):
        ms = generation_change(a)
        if a.share_info().n_tables != 0:
            raise SystemExit("share_carry = 0 kept tables")
        f, r = tabs.apply(a)
        if i >= args.warmup:
            swap0.append(ms), again.append(r), lookups.append(f)
    out["share_carry_0"] = {"ms_compact_swap_wall": spread(swap0), "ms_share_members_apply_all_tables_wall": spread(again),
                            "ms_routes_find_group_keys_wall": spread(lookups), "ms_first_apply_wall": first[1]}
    out["routes_find"] = find_and_locate(a, w, kb, ko, args.reps, args.warmup)
    _, b, _, _ = load(args.tenants, args.routes, 1, args.device)
    tabs.apply(b)
    swap1, parts = [], {"ms_gather": [], "ms_find": [], "ms_rekey": []}
    for i in range(args.warmup + args.reps):
        ms = generation_change(b)
        ci = b.share_carry_info()
        if ci.status != 1 or ci.n_carried != len(keys) or ci.n_dropped != 0:
            raise SystemExit("the carry reports status %d, %d carried, %d dropped" % (ci.status, ci.n_carried, ci.n_dropped))
        if i >= args.warmup:
            swap1.append(ms)
            for k in parts:
                parts[k].append(float(getattr(ci, k)))
    out["share_carry_1"] = dict({"ms_compact_swap_wall": spread(swap1)}, **{k: spread(v) for k, v in parts.items()})
    out["share_carry_1"]["ms_swap_lock_hold_growth"] = float(np.median(swap1) - np.median(swap0))
    out["carried_equals_reapplied"] = compare(a, b, tabs, flags)
    a.close()
    b.close()
    if args.kernel_stats:
        out["kernels_rocprofv3"] = kernel_rows(args.kernel_stats)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
