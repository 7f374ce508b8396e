#!/usr/bin/env python3
"""What the submit-time fan-out gate of DeliverExecutorGroup.submit adds to the capped delivery wait of a whole match batch, beside what
an adapter would pay to walk the CSR on the host; writes profiles/routes_gate.json.

On the C3 index of bench.py (1000 tenants x 10 k routes), every group route with a seeded member table (as tools/caps_probe.py loads them),
one 1 M-publish batch ordered by tenant, one publisher per topic, packs of 256 bytes, in ONE process, kernel timing on, under the default
table (INT_MAX, 100, Long.MAX_VALUE, both bandwidths) and -- so that the gate binds on this workload -- (1, 1, one pack's size, transient
bandwidth off for every third tenant):

  (c) bmq_match_submit_fmt(DELIVERY) + bmq_delivery_wait_capped: the parent's wait, caps between match and plan;
  (g) bmq_match_submit_fmt(DELIVERY) + bmq_delivery_wait_gated: caps, gate and plan, none of the CSRs leaving the GPU;
  (h) the host alternative, as a LOWER bound: bmq_match_submit_fmt(IDS) + bmq_match_wait (the CSR comes to the host) and a NumPy walk of
      the reference's rule over it -- the class of every id from a table made beforehand (not timed), the three class counts per row, the
      flags and the meter per tenant.  It chooses no survivors, applies no caps and makes no plan, all of which an adapter would still owe.

(c) and (g) are timed from the submit to the return of the plan; the three alternate; --warmup rounds first, then the median, min and max of
--reps >= 20 rounds each (host clock: every call returns after a stream synchronise), and for (g) the HIP-event times of the gate's three
passes (bmq_gate_info.ms_*) beside those of the caps in the same wait.  The probe exits with an error unless the flags and the meters of (g)
are those of (h)'s walk over the capped CSR.  Needs a gfx950 device: there is no fallback.

  python tools/gate_probe.py [--topics 1000000] [--reps 20] [--warmup 3] [--out FILE]"""
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
LONG_MAX = 2**63 - 1
PACK = 256
INLINE_THRESHOLD = 1000
INLINE, P_COUNT, P_BYTES, NO_P_BANDWIDTH, NO_T_BANDWIDTH, GROUP = 1, 2, 4, 8, 16, 32


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def classes_of_keys(kb, ko):
    """0 transient, 1 persistent, 2 group per route id (= key rank), the rule of caps_class_of in NumPy: the receiverUrls of the generator
    begin with the decimal subBrokerId and a NUL"""
    ends = ko[1:].astype(np.int64)
    rlen = kb[ends - 2].astype(np.int64) * 256 + kb[ends - 1]
    recv = ends - 2 - rlen
    flag = kb[recv - 1]
    cls = np.where(flag != 1, 2, 0).astype(np.uint8)
    value, on = np.zeros(len(ends), dtype=np.int64), np.ones(len(ends), dtype=bool)
    any_digit = np.zeros(len(ends), dtype=bool)
    for k in range(10):  # (a digit prefix of at most ten characters)
        ch = kb[np.minimum(recv + k, len(kb) - 1)].astype(np.int64)
        on &= (recv + k < ends - 2) & (ch >= 48) & (ch <= 57)
        value = np.where(on, value * 10 + ch - 48, value)
        any_digit |= on
    cls[(flag == 1) & any_digit & (value == 1)] = 1
    return cls


def host_walk(row, ids, total, cls_of_id, tt, pack, pf, gf, pb, bw, n_tenants):
    """the reference's rule over a host CSR -> (flags per row, meter bytes, meter records per tenant); no survivors are chosen"""
    n = len(row) - 1
    lens = np.diff(row.astype(np.int64))
    r_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    cls = cls_of_id[ids[:total]]
    nP = np.bincount(r_of[cls == 1], minlength=n)
    nT = np.bincount(r_of[cls == 0], minlength=n)
    nG = np.bincount(r_of[cls == 2], minlength=n)
    s = pack.astype(np.int64)
    t = tt.astype(np.int64)
    rpf, rgf, rpb, rbw = pf[t].astype(np.int64), gf[t].astype(np.int64), pb[t], bw[t]
    many = lens > 1
    lim = np.where(rpb == 0, 0, np.where(s == 0, INT_MAX, -(-rpb // np.maximum(s, 1))))
    A = np.minimum(rpf, lim)
    has_p, has_t = (rbw & 2) != 0, (rbw & 1) != 0
    kp = np.where(has_p, np.minimum(nP, A), 0)
    over = many & has_p & (nP > A)
    fl = np.where(lens == 1, INLINE, 0) | np.where(many & (lens < INLINE_THRESHOLD), INLINE, 0)
    fl |= np.where(over & (A >= rpf), P_COUNT, 0) | np.where(over & (A.astype(np.float64) * s >= rpb.astype(np.float64)), P_BYTES, 0)
    nobw = many & ~has_p & (nP > 0)
    fl |= np.where(nobw & (rpf > 0) & (rpb > 0), NO_P_BANDWIDTH, 0) | np.where(nobw & (rpf == 0), P_COUNT, 0) | np.where(nobw & (rpb == 0), P_BYTES, 0)
    fl |= np.where(many & ~has_t & (nT > 0), NO_T_BANDWIDTH, 0) | np.where(many & (nG > rgf), GROUP, 0)
    metered = np.where(many, kp * s, np.where((lens == 1) & (nP == 1), s, 0))
    rec = many | ((lens == 1) & (nP == 1))
    return fl.astype(np.uint32), np.bincount(t, weights=metered, minlength=n_tenants).astype(np.uint64), np.bincount(t[rec], minlength=n_tenants).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "routes_gate.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    L = _lib.lib()
    n_topics, n_ten = args.topics, args.tenants
    w = B.Workload(SEED, n_ten, args.routes, 1)
    eng = B.Engine(device=0, kernel_timing=True)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    cls_of_id = classes_of_keys(kb, ko)
    group_ids = np.nonzero(cls_of_id == 2)[0].astype(np.uint32)
    rng = np.random.default_rng(20261016)
    for tabs, _ in member_tables(rng, group_ids, 1, 200):
        eng.share_members_apply(tabs)
    tdata, toff = w.tenants_packed()
    data, off, tt = w.topics(SEED + 1000, n_topics, grouped=True)
    tt = np.ascontiguousarray(tt, dtype=np.uint32)
    a = (tdata, toff, w.n_tenants, tt, data, off, n_topics)
    sender_off = np.arange(n_topics + 1, dtype=np.uint32)
    sender_hash = rng.integers(-(1 << 31), 1 << 31, size=n_topics).astype(np.int32)
    pack = np.full(n_topics, PACK, dtype=np.uint32)
    row, ids = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(32 * n_topics, dtype=np.uint32)
    total = eng.match_wait(eng.match_submit_fmt(*a, eng.FMT_IDS), row, ids)
    row_cap, share_cap, gcap, ev_cap = total + (1 << 20), 1 << 20, 1 << 16, 1 << 22
    h_t, h_r, h_a = (np.zeros(row_cap, dtype=np.uint32) for _ in range(3))
    h_ss, h_sm = (np.zeros(share_cap, dtype=np.uint32) for _ in range(2))
    h_go = np.zeros(gcap + 1, dtype=np.uint32)
    ev = np.zeros(4 * ev_cap, dtype=np.int32)
    fl, mb, mr = np.zeros(n_topics, dtype=np.uint32), np.zeros(n_ten, dtype=np.uint64), np.zeros(n_ten, dtype=np.uint32)
    c_row, c_ids = np.zeros(n_topics + 1, dtype=np.uint32), np.zeros(total, dtype=np.uint32)
    nev = C.c_uint32()

    def capped_wait(T, nonce):
        info, tot, cinfo = _lib.DeliveryInfo(), C.c_uint64(), _lib.CapsInfo()
        t0 = time.perf_counter()
        k = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
        rc = L.bmq_delivery_wait_capped(eng.h, k, _ptr(T[0]), _ptr(T[1]), n_ten, _ptr(sender_off), _ptr(sender_hash), nonce, _ptr(h_t), _ptr(h_r), _ptr(h_a), row_cap, _ptr(h_ss),
                                        _ptr(h_sm), share_cap, _ptr(h_go), gcap, C.byref(info), C.byref(tot), _ptr(ev), ev_cap, C.byref(nev), C.byref(cinfo))
        if rc:
            raise SystemExit("bmq_delivery_wait_capped: %d" % rc)
        return (time.perf_counter() - t0) * 1e3, info, cinfo

    def gated_wait(T, nonce):
        info, tot, cinfo, ginfo = _lib.DeliveryInfo(), C.c_uint64(), _lib.CapsInfo(), _lib.GateInfo()
        t0 = time.perf_counter()
        k = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
        rc = L.bmq_delivery_wait_gated(eng.h, k, _ptr(T[0]), _ptr(T[1]), _ptr(T[2]), _ptr(T[3]), n_ten, _ptr(pack), INLINE_THRESHOLD, _ptr(sender_off), _ptr(sender_hash), nonce,
                                       _ptr(h_t), _ptr(h_r), _ptr(h_a), row_cap, _ptr(h_ss), _ptr(h_sm), share_cap, _ptr(h_go), gcap, C.byref(info), C.byref(tot), _ptr(ev),
                                       ev_cap, C.byref(nev), C.byref(cinfo), _ptr(fl), _ptr(mb), _ptr(mr), C.byref(ginfo))
        if rc:
            raise SystemExit("bmq_delivery_wait_gated: %d" % rc)
        return (time.perf_counter() - t0) * 1e3, info, cinfo, ginfo

    def host_way(T):
        t0 = time.perf_counter()
        tot = eng.match_wait(eng.match_submit_fmt(*a, eng.FMT_IDS), row, ids)
        out = host_walk(row, ids, tot, cls_of_id, tt, pack, *T, n_ten)
        return (time.perf_counter() - t0) * 1e3, out

    third = (np.arange(n_ten) % 3 == 2)
    tables = {
        "default": (np.full(n_ten, INT_MAX, dtype=np.int32), np.full(n_ten, 100, dtype=np.int32), np.full(n_ten, LONG_MAX, dtype=np.int64), np.full(n_ten, 3, dtype=np.uint8)),
        "binding": (np.full(n_ten, 1, dtype=np.int32), np.full(n_ten, 1, dtype=np.int32), np.full(n_ten, PACK, dtype=np.int64), np.where(third, 2, 3).astype(np.uint8)),
    }
    results = {}
    passes = ("ms_classify", "ms_rank", "ms_write")
    for name, T in tables.items():
        ms = {"c": [], "g": [], "h": []}
        steps = {"gate": {k: [] for k in passes}, "caps": {k: [] for k in passes}}
        for i in range(args.warmup + args.reps):
            nonce = (0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF
            tc, cdinfo, ccinfo = capped_wait(T, nonce)
            tg, gdinfo, gcinfo, ginfo = gated_wait(T, nonce)
            th, _ = host_way(T)
            print("table %s round %d: capped %.1f ms, gated %.1f ms, host walk %.1f ms" % (name, i, tc, tg, th), file=sys.stderr, flush=True)
            if i >= args.warmup:
                ms["c"].append(tc), ms["g"].append(tg), ms["h"].append(th)
                for k in passes:
                    steps["gate"][k].append(float(getattr(ginfo, k))), steps["caps"][k].append(float(getattr(gcinfo, k)))
        # the gate's flags and meters against the walk of the CAPPED CSR (the gate runs behind the caps)
        cinfo = _lib.CapsInfo()
        rc = L.bmq_routes_cap_batch(eng.h, _ptr(row), _ptr(ids), n_topics, _ptr(tt), _ptr(T[0]), _ptr(T[1]), n_ten, _ptr(c_row), _ptr(c_ids), total, None, None, 0, C.byref(nev),
                                    C.byref(cinfo))
        if rc:
            raise SystemExit("bmq_routes_cap_batch: %d" % rc)
        w_fl, w_mb, w_mr = host_walk(c_row, c_ids, int(cinfo.n_kept), cls_of_id, tt, pack, *T, n_ten)
        if not (np.array_equal(w_fl, fl) and np.array_equal(w_mb, mb) and np.array_equal(w_mr, mr)):
            raise SystemExit("table %s: the flags or meters of bmq_delivery_wait_gated are not those of the host walk over the capped CSR" % name)
        mc, mg, mh = float(np.median(ms["c"])), float(np.median(ms["g"])), float(np.median(ms["h"]))
        results[name] = {
            "table": [int(T[0][0]), int(T[1][0]), int(T[2][0]), "bandwidth 3, every third tenant 2" if name == "binding" else 3], "ids_in": int(total),
            "ids_after_caps": int(gcinfo.n_kept), "ids_after_gate": int(ginfo.n_kept), "rows_single": int(ginfo.n_rows_single), "rows_gated": int(ginfo.n_rows_gated),
            "rows_flagged": int(ginfo.n_rows_flagged), "rows_ranked": int(ginfo.n_rows_ranked), "rows_fallback": int(ginfo.n_rows_fallback),
            "meter_bytes_total": int(mb.sum()), "meter_records_total": int(mr.sum()), "plan_rows_capped": int(cdinfo.n_rows), "plan_rows_gated": int(gdinfo.n_rows),
            "c_submit_delivery_wait_capped_ms_wall": spread(ms["c"]), "g_submit_delivery_wait_gated_ms_wall": spread(ms["g"]),
            "h_submit_wait_numpy_walk_ms_wall_lower_bound": spread(ms["h"]), "g_minus_c_ms": mg - mc, "g_over_c": mg / mc, "h_over_g": mh / mg,
            "gate_passes_ms": {k: spread(v) for k, v in steps["gate"].items()}, "caps_passes_ms_in_the_same_wait": {k: spread(v) for k, v in steps["caps"].items()}}
    out = {"probe": "tools/gate_probe.py", "device": "MI355X (gfx950), one GPU, one run", "library": L.bmq_version().decode(),
           "workload": "C3: %d tenants x %d routes, a member table of 1-200 members on every group route; one batch of %d publishes ordered by tenant, one publisher "
                       "each, packs of %d bytes, inline threshold %d" % (n_ten, args.routes, n_topics, PACK, INLINE_THRESHOLD),
           "timing": "host clock, (c) and (g) from the submit to the return of the plan, (h) from the submit to the end of the walk; every call returns after a stream "
                     "synchronise; ms_classify / ms_rank / ms_write: HIP events; (c), (g), (h) alternate in one process, %d warm-up round(s), then median / min / max of %d "
                     "rounds" % (args.warmup, args.reps),
           "index_routes": int(w.n_keys), "publishes": n_topics, "matched_pairs": int(total), "yardstick": "(c), the capped wait of the parent commit, in the same run",
           "tables": results}
    eng.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
