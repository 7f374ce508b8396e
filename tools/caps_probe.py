#!/usr/bin/env python3
"""What the fan-out caps of MatchedRoutes cost on a whole match batch, beside the host path the engine had before; writes
profiles/routes_cap.json.

On the C3 index of bench.py (1000 tenants x 10 k routes), every group route with a seeded member table (as tools/delivery_probe.py loads
them), one 1 M-publish batch ordered by tenant, one publisher per topic, in ONE process, kernel timing on, under the caps (pf 10, gf 100),
(INT_MAX, 100) and -- so that a cap binds on this workload -- (1, 1) for every tenant:

  (a) the parent's way: bmq_match_submit_fmt(IDS) + bmq_match_wait (the CSR comes to the host), one bmq_routes_cap per tenant that has a
      row longer than a cap (the route cache's rule: "one call per tenant that has such rows"), the capped rows put together, then
      bmq_delivery_plan on them (the capped CSR goes back up, the plan comes down);
  (b) bmq_routes_cap_batch on the host CSR of (a), alone (the CSR goes up, the capped one comes down);
  (c) bmq_match_submit_fmt(DELIVERY) + bmq_delivery_wait_capped: neither CSR leaves the GPU, the plan comes down.

(a) and (c) are timed from the submit to the return of the plan; the three alternate; --warmup rounds first, then the median, min and max of
--reps >= 20 rounds each (host clock: every call returns after a stream synchronise), and for (b) / (c) the HIP-event times of the three passes
(bmq_caps_info.ms_*).  The yardstick is (a).  The probe exits with an error unless the capped CSR of (b) is the one (a) put together and the
plans of (a) and (c) have the same sizes.  Needs a gfx950 device: there is no fallback.

  python tools/caps_probe.py [--topics 1000000] [--reps 20] [--warmup 3] [--out FILE]"""
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
from bifromq_amd.engine import _ptr  # noqa: E402
from tools.share_probe import member_tables  # noqa: E402

SEED = 0xB1F20003
INT_MAX = 2**31 - 1


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "routes_cap.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L = _lib.lib()
    n_topics = args.topics
    w = B.Workload(SEED, args.tenants, args.routes, 1)
    eng = B.Engine(device=0, kernel_timing=True)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    ends = ko[1:].astype(np.int64)
    rlen = kb[ends - 2].astype(np.int64) * 256 + kb[ends - 1]
    flag = kb[ends - 3 - rlen]
    group_ids = np.nonzero((flag == 2) | (flag == 3))[0].astype(np.uint32)
    rng = np.random.default_rng(20261016)
    for tabs, _ in member_tables(rng, group_ids, 1, 200):
        eng.share_members_apply(tabs)
    tdata, toff = w.tenants_packed()
    data, off, tt = w.topics(SEED + 1000, n_topics, grouped=True)
    tt = np.ascontiguousarray(tt, dtype=np.uint32)
    if (np.diff(tt.astype(np.int64)) < 0).any():
        raise SystemExit("the batch is not ordered by tenant")
    a = (tdata, toff, w.n_tenants, tt, data, off, n_topics)
    sender_off = np.arange(n_topics + 1, dtype=np.uint32)
    sender_hash = rng.integers(-(1 << 31), 1 << 31, size=n_topics).astype(np.int32)
    row, ids = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(32 * n_topics, dtype=np.uint32)
    total = eng.match_wait(eng.match_submit_fmt(*a, eng.FMT_IDS), row, ids)
    first = np.searchsorted(tt, np.arange(w.n_tenants + 1)).astype(np.int64)  # the rows of tenant t: first[t] .. first[t + 1]
    row_cap, share_cap, gcap, ev_cap = total + (1 << 20), 1 << 20, 1 << 16, 1 << 22
    h_t, h_r, h_a = (np.zeros(row_cap, dtype=np.uint32) for _ in range(3))
    h_ss, h_sm = (np.zeros(share_cap, dtype=np.uint32) for _ in range(2))
    h_go = np.zeros(gcap + 1, dtype=np.uint32)
    c_row, c_ids, c_cc = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(total, dtype=np.uint32), np.zeros(2 * n_topics, dtype=np.uint32)
    b_row, b_ids = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(total, dtype=np.uint32)
    s_row, s_ids = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(total, dtype=np.uint32)
    ev = np.zeros(4 * ev_cap, dtype=np.int32)
    nev, dinfo = C.c_uint32(), _lib.DeliveryInfo()

    def parent_way(pf, gf, nonce):
        """-> (ms, calls of bmq_routes_cap, ids kept, events)"""
        t0 = time.perf_counter()
        tot = eng.match_wait(eng.match_submit_fmt(*a, eng.FMT_IDS), row, ids)
        lens = np.diff(row.astype(np.int64))
        at, calls, n_events = 0, 0, 0
        c_row[0] = 0
        for t in np.nonzero(first[:-1] < first[1:])[0].tolist():
            lo, hi = int(first[t]), int(first[t + 1])
            p0, p1 = int(row[lo]), int(row[hi])
            if lens[lo:hi].max() > min(pf, gf):  # (the route cache's rule: a tenant without an over-long row is not sent)
                s_row[:hi - lo + 1] = row[lo:hi + 1] - row[lo]
                rc = L.bmq_routes_cap(eng.h, _ptr(s_row), _ptr(ids[p0:]), hi - lo, pf, gf, _ptr(c_row[lo:]), _ptr(s_ids), None, _ptr(ev), ev_cap, C.byref(nev))
                if rc:
                    raise SystemExit("bmq_routes_cap: %d" % rc)
                kept = int(c_row[hi])
                c_ids[at:at + kept] = s_ids[:kept]
                c_row[lo:hi + 1] += at
                calls += 1
                n_events += nev.value
            else:
                kept = p1 - p0
                c_ids[at:at + kept] = ids[p0:p1]
                c_row[lo:hi + 1] = row[lo:hi + 1] - p0 + at
            at += kept
        rc = L.bmq_delivery_plan(eng.h, _ptr(c_row), _ptr(c_ids), n_topics, _ptr(sender_off), _ptr(sender_hash), nonce, _ptr(h_t), _ptr(h_r), _ptr(h_a), row_cap, _ptr(h_ss),
                                 _ptr(h_sm), share_cap, _ptr(h_go), gcap, C.byref(dinfo))
        if rc:
            raise SystemExit("bmq_delivery_plan: %d" % rc)
        return (time.perf_counter() - t0) * 1e3, calls, at, n_events, tot

    def batch_call(pf_t, gf_t):
        info = _lib.CapsInfo()
        t0 = time.perf_counter()
        rc = L.bmq_routes_cap_batch(eng.h, _ptr(row), _ptr(ids), n_topics, _ptr(tt), _ptr(pf_t), _ptr(gf_t), w.n_tenants, _ptr(b_row), _ptr(b_ids), total, _ptr(c_cc),
                                    _ptr(ev), ev_cap, C.byref(nev), C.byref(info))
        if rc:
            raise SystemExit("bmq_routes_cap_batch: %d" % rc)
        return (time.perf_counter() - t0) * 1e3, info

    def capped_wait(pf_t, gf_t, nonce):
        info, tot, cinfo = _lib.DeliveryInfo(), C.c_uint64(), _lib.CapsInfo()
        t0 = time.perf_counter()
        k = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
        rc = L.bmq_delivery_wait_capped(eng.h, k, _ptr(pf_t), _ptr(gf_t), w.n_tenants, _ptr(sender_off), _ptr(sender_hash), nonce, _ptr(h_t), _ptr(h_r), _ptr(h_a), row_cap,
                                        _ptr(h_ss), _ptr(h_sm), share_cap, _ptr(h_go), gcap, C.byref(info), C.byref(tot), _ptr(ev), ev_cap, C.byref(nev), C.byref(cinfo))
        if rc:
            raise SystemExit("bmq_delivery_wait_capped: %d" % rc)
        return (time.perf_counter() - t0) * 1e3, info, cinfo

    results = {}
    for pf, gf in ((10, 100), (INT_MAX, 100), (1, 1)):  # (the generator's rows hold few persistent and group routes: only the last pair binds, and gives the rank pass work)
        pf_t, gf_t = np.full(w.n_tenants, pf, dtype=np.int32), np.full(w.n_tenants, gf, dtype=np.int32)
        ms = {"a": [], "b": [], "c": []}
        steps = {"b": {k: [] for k in ("ms_classify", "ms_rank", "ms_write")}, "c": {k: [] for k in ("ms_classify", "ms_rank", "ms_write")}}
        for i in range(args.warmup + args.reps):
            nonce = (0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF
            ta, calls, kept_a, ev_a, tot_a = parent_way(pf, gf, nonce)
            rows_a = (dinfo.n_rows, dinfo.n_share_rows, dinfo.n_groups)
            tb, binfo = batch_call(pf_t, gf_t)
            tc, cdinfo, cinfo = capped_wait(pf_t, gf_t, nonce)
            print("caps (%d, %d) round %d: a %.1f ms, b %.1f ms, c %.1f ms" % (pf, gf, i, ta, tb, tc), file=sys.stderr, flush=True)
            if i >= args.warmup:
                ms["a"].append(ta), ms["b"].append(tb), ms["c"].append(tc)
                for k in steps["b"]:
                    steps["b"][k].append(float(getattr(binfo, k))), steps["c"][k].append(float(getattr(cinfo, k)))
        if tot_a != total or not np.array_equal(b_row, c_row) or not np.array_equal(b_ids[:binfo.n_kept], c_ids[:kept_a]) or binfo.n_events != ev_a:
            raise SystemExit("the capped CSR of bmq_routes_cap_batch is not the one the per-tenant calls give")
        if (cdinfo.n_rows, cdinfo.n_share_rows, cdinfo.n_groups) != rows_a or cinfo.n_kept != kept_a or cinfo.n_events != ev_a:
            raise SystemExit("the plan of bmq_delivery_wait_capped has other sizes than the plan of the capped host CSR")
        ma, mc = float(np.median(ms["a"])), float(np.median(ms["c"]))
        results["pf_%s_gf_%d" % ("max" if pf == INT_MAX else str(pf), gf)] = {
            "caps": [pf, gf], "ids_in": int(total), "ids_kept": int(kept_a), "events": int(ev_a), "rows_classified": int(cinfo.n_rows_classified),
            "n_rows_ranked": int(cinfo.n_rows_ranked), "n_rows_fallback": int(cinfo.n_rows_fallback), "routes_cap_calls_of_a": calls,
            "plan_rows": int(cdinfo.n_rows), "plan_groups": int(cdinfo.n_groups),
            "a_submit_wait_routes_cap_per_tenant_delivery_plan_ms_wall": spread(ms["a"]), "b_routes_cap_batch_ms_wall": spread(ms["b"]),
            "c_submit_delivery_wait_capped_ms_wall": spread(ms["c"]), "c_over_a": mc / ma, "c_beats_a": bool(mc < ma),
            "b_passes_ms": {k: spread(v) for k, v in steps["b"].items()}, "c_passes_ms": {k: spread(v) for k, v in steps["c"].items()}}
    out = {"probe": "tools/caps_probe.py", "device": "MI355X (gfx950), one GPU, one run", "library": L.bmq_version().decode(),
           "workload": "C3: %d tenants x %d routes, a member table of 1-200 members on every group route; one batch of %d publishes ordered by tenant, one publisher "
                       "each; the same caps for every tenant" % (args.tenants, args.routes, n_topics),
           "timing": "host clock, (a) and (c) from the submit to the return of the plan, (b) around the call; every call returns after a stream synchronise; ms_classify / "
                     "ms_rank / ms_write: HIP events; (a), (b), (c) alternate in one process, %d warm-up round(s), then median / min / max of %d rounds" % (args.warmup, args.reps),
           "index_routes": int(w.n_keys), "publishes": n_topics, "matched_pairs": int(total), "yardstick": "(a), the host path of the parent commit", "caps": results}
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
