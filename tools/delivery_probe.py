#!/usr/bin/env python3
"""What the delivery plan (bmq_delivery_plan_dev / bmq_delivery_wait) costs beside the chain it completes; writes profiles/delivery_plan.json.

On the C3 index of bench.py (1000 tenants x 10 k routes; bmq_gen.cpp makes 0.5 % of the routes $share / $oshare groups), every group route
with a seeded member table of 1-200 members (as tools/share_probe.py loads them), one 1 M-publish batch with one publisher per topic, in ONE
process, device-resident, kernel timing on:

  (a) bmq_fanout_group_dev + bmq_share_resolve_dev back to back on the batch's CSR -- the chain without the merge, which has no device form
      without this step (the slice of the shared group is known from the first repetition: (a) pays no read of the group table);
  (b) bmq_delivery_plan_dev on the same CSR.

(a) and (b) alternate; --warmup rounds first, then the median, min and max of --reps >= 20 rounds each: wall time of the C-ABI calls (they
return after a stream synchronise) and, for (b), the HIP-event times of its four steps (bmq_delivery_info.ms_*).  Then the host-visible pair:
bmq_match_submit_fmt + bmq_match_wait_grouped against bmq_match_submit_fmt(BMQ_FMT_DELIVERY) + bmq_delivery_wait on the same batch, submit
to return of the wait, alternated the same way (GROUPED returns 8 bytes per pair, DELIVERY 12 bytes per row + the side arrays).
The probe exits with an error if the plan's rows are not those of (a): the same (topic, route) multiset, the share rows' (sender, member) equal
per (topic, route, sender).  Needs a gfx950 device: there is no fallback.

  python tools/delivery_probe.py [--topics 1000000] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd import _lib  # noqa: E402
from tools.share_probe import Hbm, member_tables  # noqa: E402

SEED = 0xB1F20003
WRITE_CEILING_TBS = 5.14  # profiles/r06/extras/write_ceiling.txt: grid-stride 16-byte stores, the plain store loop of this chip


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "delivery_plan.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    n_topics = args.topics
    w = B.Workload(SEED, args.tenants, args.routes, 1)
    eng = B.Engine(device=0, kernel_timing=True)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    ends = ko[1:].astype(np.int64)
    rlen = kb[ends - 2].astype(np.int64) * 256 + kb[ends - 1]
    flag = kb[ends - 3 - rlen]
    group_ids = np.nonzero((flag == 2) | (flag == 3))[0].astype(np.uint32)  # ids = ranks of the sorted keys (tools/share_probe.py checks it)
    rng = np.random.default_rng(20261016)
    for tabs, _ in member_tables(rng, group_ids, 1, 200):
        eng.share_members_apply(tabs)
    sinf = eng.share_info()
    mem = Hbm()
    tdata, toff = w.tenants_packed()
    data, off, tt = w.topics(SEED + 1000, n_topics, grouped=True)
    cap = 32 * n_topics
    d = [mem.put(x) for x in (tdata, toff, tt, data, off)]
    d_row, d_ids, d_tot = mem.zeros(n_topics + 1), mem.zeros(cap), mem.zeros(1, np.uint64)
    eng.match_batch_device(d[0], d[1], w.n_tenants, d[2], d[3], d[4], n_topics, d_row, d_ids, cap, d_tot)
    total = eng.finish()
    sender_off = np.arange(n_topics + 1, dtype=np.uint32)  # one publisher per topic
    sender_hash = rng.integers(-(1 << 31), 1 << 31, size=n_topics).astype(np.int32)
    d_so, d_sh = mem.put(sender_off), mem.put(sender_hash)
    gcap = 1 << 16
    # ---- (a): the two calls; the slice from a first grouping
    d_ot, d_or, d_goff, d_grep = mem.zeros(total), mem.zeros(total), mem.zeros(gcap + 1), mem.zeros(gcap)
    ng, sp = eng.fanout_group_device(d_row, d_ids, n_topics, total, d_ot, d_or, d_goff, d_grep, gcap)
    if not sp & 1:
        raise SystemExit("the batch matched no shared-subscription route")
    goff, grep = mem.get(d_goff, ng + 1), mem.get(d_grep, ng)
    g = int(np.nonzero(grep == 0xFFFFFFFE)[0][0])
    lo, hi = int(goff[g]), int(goff[g + 1])
    n_shared = hi - lo
    rcap = 2 * n_shared + 64
    d_rp, d_rs, d_rm, d_rgo = mem.zeros(rcap), mem.zeros(rcap), mem.zeros(rcap), mem.zeros(gcap + 1)
    # ---- (b): the plan's outputs
    row_cap = total + rcap
    d_pt, d_pr, d_pa, d_ps, d_pm, d_pgo = mem.zeros(row_cap), mem.zeros(row_cap), mem.zeros(row_cap), mem.zeros(rcap), mem.zeros(rcap), mem.zeros(gcap + 1)

    def chain(nonce):
        t0 = time.perf_counter()
        eng.fanout_group_device(d_row, d_ids, n_topics, total, d_ot, d_or, d_goff, d_grep, gcap)
        r = eng.share_resolve_device(d_ot + 4 * lo, d_or + 4 * lo, n_shared, d_so, d_sh, n_topics, n_topics, nonce, d_rp, d_rs, d_rm, rcap, d_rgo, gcap)
        return (time.perf_counter() - t0) * 1e3, r

    def plan(nonce):
        t0 = time.perf_counter()
        info = eng.delivery_plan_device(d_row, d_ids, n_topics, total, d_so, d_sh, n_topics, nonce, d_pt, d_pr, d_pa, row_cap, d_ps, d_pm, rcap, d_pgo, gcap)
        return (time.perf_counter() - t0) * 1e3, info

    ms_a, ms_b, steps = [], [], {k: [] for k in ("ms_group", "ms_resolve", "ms_map", "ms_merge")}
    for i in range(args.warmup + args.reps):
        nonce = 0x9E3779B97F4A7C15 * (i + 1)
        ta, ra = chain(nonce)
        tb, info = plan(nonce)
        if i >= args.warmup:
            ms_a.append(ta), ms_b.append(tb)
            for k in steps:
                steps[k].append(float(getattr(info, k)))
    # ---- the plan of the last round against the chain of the last round
    nr = ra[0]
    pt, pr, pa = mem.get(d_pt, info.n_rows), mem.get(d_pr, info.n_rows), mem.get(d_pa, info.n_rows)
    ps, pm = mem.get(d_ps, info.n_share_rows), mem.get(d_pm, info.n_share_rows)
    ot, orr = mem.get(d_ot, total), mem.get(d_or, total)
    rp, rs, rm = mem.get(d_rp, nr), mem.get(d_rs, nr), mem.get(d_rm, nr)
    if info.n_share_rows != nr or info.n_rows != total - n_shared + nr:
        raise SystemExit("the plan has %d rows / %d share rows, the chain %d / %d" % (info.n_rows, info.n_share_rows, total - n_shared + nr, nr))
    normal = np.ones(total, dtype=bool)
    normal[lo:hi] = False
    key = lambda t, r: (t.astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    if not np.array_equal(np.sort(key(pt[pa == 0xFFFFFFFF], pr[pa == 0xFFFFFFFF])), np.sort(key(ot[normal], orr[normal]))):
        raise SystemExit("the plan's normal rows are not the chain's pairs")
    sel = pa != 0xFFFFFFFF
    got = sorted(zip(pt[sel].tolist(), pr[sel].tolist(), ps[pa[sel]].tolist(), pm[pa[sel]].tolist()))
    want = sorted(zip(ot[lo + rp].tolist(), orr[lo + rp].tolist(), rs.tolist(), rm.tolist()))
    if got != want:
        raise SystemExit("the plan's member rows are not the chain's")
    pgo = mem.get(d_pgo, info.n_groups + 1)
    if pgo[0] != 0 or pgo[-1] != info.n_rows or (np.diff(pgo.astype(np.int64)) <= 0).any():
        raise SystemExit("the plan's group offsets do not partition the rows")
    # ---- host-visible: GROUPED against DELIVERY through tickets
    a = (tdata, toff, w.n_tenants, tt, data, off, n_topics)
    h_t, h_r, h_a = (np.zeros(row_cap, dtype=np.uint32) for _ in range(3))
    h_ss, h_sm = (np.zeros(rcap, dtype=np.uint32) for _ in range(2))
    h_go, h_gr = np.zeros(gcap + 1, dtype=np.uint32), np.zeros(gcap, dtype=np.uint32)
    ms_g, ms_d = [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        k = eng.match_submit_fmt(*a, eng.FMT_GROUPED)
        eng.match_wait_grouped(k, h_t[:total], h_r[:total], h_go, h_gr)
        t1 = time.perf_counter()
        k = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
        eng.match_wait_delivery(k, sender_off, sender_hash, i + 1, h_t, h_r, h_a, h_ss, h_sm, h_go)
        t2 = time.perf_counter()
        if i >= args.warmup:
            ms_g.append((t1 - t0) * 1e3), ms_d.append((t2 - t1) * 1e3)
    fi = eng.fanout_info()
    diff = float(np.median(ms_b) - np.median(ms_a))
    moved = info.n_rows * 12 + info.n_share_rows * 8  # the rows the merge writes; it reads as much again from the two lists
    out = {"probe": "tools/delivery_probe.py", "device": "MI355X (gfx950), one GPU, one run", "library": _lib.lib().bmq_version().decode(),
           "workload": "C3: %d tenants x %d routes, a member table of 1-200 members on every group route; one batch of %d publishes, one publisher each" %
                       (args.tenants, args.routes, n_topics),
           "timing": "host clock around C-ABI calls that return after a stream synchronise; ms_group / ms_resolve / ms_map / ms_merge: HIP events; (a) and (b) "
                     "alternate in one process, %d warm-up round(s), then median / min / max of %d rounds" % (args.warmup, args.reps),
           "index_routes": int(w.n_keys), "group_routes": int(len(group_ids)), "members": int(sinf.n_members), "share_deliverers": int(sinf.n_deliverers),
           "publishes": n_topics, "matched_pairs": int(total), "shared_pairs": n_shared, "rows": int(info.n_rows), "share_rows": int(info.n_share_rows),
           "groups": int(info.n_groups), "merged_groups": int(info.n_merged_groups), "share_only_groups": int(info.n_share_only_groups), "special": int(info.special),
           "grouping_path": {"fast_calls": int(fi.n_fast_calls), "generic_calls": int(fi.n_generic_calls)},
           "a_fanout_group_dev_plus_share_resolve_dev_ms_wall": spread(ms_a), "b_delivery_plan_dev_ms_wall": spread(ms_b), "b_minus_a_ms": diff,
           "b_steps_ms": {k: spread(v) for k, v in steps.items()},
           "one_pass_over_the_rows": {"bytes_written": int(moved), "store_rate_TBs": WRITE_CEILING_TBS, "ms": moved / (WRITE_CEILING_TBS * 1e12) * 1e3},
           "host_visible": {"submit_plus_wait_grouped_ms_wall": spread(ms_g), "submit_plus_wait_delivery_ms_wall": spread(ms_d),
                            "bytes_returned_grouped": int(total) * 8 + (int(ng) * 2 + 1) * 4,
                            "bytes_returned_delivery": int(info.n_rows) * 12 + int(info.n_share_rows) * 8 + (int(info.n_groups) + 1) * 4},
           "plan_equals_chain": "normal rows: the same (topic, route) multiset; member rows: the same (topic, route, sender, member) multiset; offsets partition the rows"}
    mem.free()
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
