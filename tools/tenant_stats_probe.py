#!/usr/bin/env python3
"""Times the per-tenant census calls and the removal by id on the device and writes ONE JSON line (default: profiles/tenant_stats.json).

Dist, the C3 index of bench.py (1000 tenants x 10k routes = 10 M keys), in one run:

  census        bmq_routes_tenant_stats over the full boundary (one pass of k_b_census), host clock around the call;
  count_in      ONE bmq_routes_count_in over the full boundary: the single pass over the same references the parent commit has (the census
                reads those plus each key's header, tail and a directory line);
  tenant_loop   the loop the census replaces: one bmq_routes_count_in per tenant prefix [prefix, upperBound(prefix)), 1000 calls.
The census must beat the loop; its ratio to the single pass is reported.  The loop's per-tenant (routes, key bytes) must equal the census.

Retain, the C4 index of bench.py (1 M retained topics, 1 tenant) churned as its churn leg leaves it (50 k bulk-loaded ids dead, 50 k overlay
topics live):

  tenant_counts bmq_retain_tenant_counts;
  remove_ids    bmq_retain_remove_ids of the ids bmq_retain_expired returns at a `now` that expires about 100 k topics, against
                bmq_retain_apply_batch removing the same topics by string (what a caller does today) on a second engine in the same state.

Times are host-clock times around C-ABI calls that return after a stream synchronise.  The per-kernel time of k_b_census comes from a run of
its own under `rocprofv3 --kernel-trace --stats -- python tools/tenant_stats_probe.py --kernel-only` (tracing slows the host: no wall time of
that run is reported); --kernel-stats CSV folds that file's k_b_census row into the JSON.  Needs a gfx950 device: there is no fallback.

  python tools/tenant_stats_probe.py [--tenants 1000] [--routes 10000] [--no-retain] [--kernel-stats CSV] [--out FILE]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd.engine import pack  # noqa: E402


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    return r, (time.perf_counter() - t0) * 1e3


def upper_bound(p):
    p = p.rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": len(ms)}


def dist_probe(n_tenants, routes, kernel_only):
    w = B.Workload(0xB1F20003, n_tenants, routes, 1)
    kb, ko = w.keys_packed()
    a = B.Engine(device=0)
    _, ms_load = timed(a.rebuild_raw, kb.ctypes.data, ko.ctypes.data, w.n_keys)
    out = {"index_routes": int(w.n_keys), "tenants": n_tenants, "ms_initial_rebuild": ms_load}
    cap = n_tenants + 16
    census = a.routes_tenant_stats(cap=cap, tenants_cap=64 * cap)  # warm-up: code object, the table
    ms = [timed(a.routes_tenant_stats, cap=cap, tenants_cap=64 * cap)[1] for _ in range(9)]
    out["census"] = dict(spread(ms), tenants_out=len(census))
    if kernel_only:
        a.close()
        return out
    total = a.count_in()
    ms1 = [timed(a.count_in)[1] for _ in range(9)]
    out["count_in"] = dict(spread(ms1), routes=total[0], key_bytes=total[1])
    if (sum(r[1] + r[2] + r[3] for r in census), sum(r[4] for r in census)) != total:
        raise SystemExit("the census does not add up to count_in: %r" % (total,))
    loops = []
    for _ in range(2):
        t0 = time.perf_counter()
        per = []
        for r in census:
            p = b"\0" + len(r[0]).to_bytes(2, "big") + r[0]
            per.append(a.count_in(start=p, end=upper_bound(p)))
        loops.append((time.perf_counter() - t0) * 1e3)
    if per != [(r[1] + r[2] + r[3], r[4]) for r in census]:
        raise SystemExit("the per-tenant loop of count_in differs from the census")
    out["tenant_loop"] = {"calls": len(census), "ms": [round(x, 3) for x in loops], "ms_per_call": min(loops) / max(1, len(census))}
    out["census_vs_loop"] = min(loops) / out["census"]["median_ms"]
    out["census_vs_single_pass"] = out["census"]["median_ms"] / out["count_in"]["median_ms"]
    if out["census"]["median_ms"] >= min(loops):
        raise SystemExit("the census (%.3f ms) does not beat the loop of count_in per tenant (%.3f ms)" % (out["census"]["median_ms"], min(loops)))
    a.close()
    return out


def churned_c4(n_topics=1_000_000, n_ops=100_000):
    """bench.py's C4 index after its churn leg: n_ops / 2 bulk-loaded topics removed, n_ops / 2 new ones added"""
    seed = 0xB1F20004
    w = B.Workload(seed, 1, 1, 0)
    data, off, tt = w.retain(seed, n_topics, filters=False)
    rng_t = np.random.default_rng(0xB1F2)
    base_ms = 1_700_000_000_000
    ts = ((base_ms + rng_t.integers(0, 100_000, n_topics)).astype(np.uint64) << np.uint64(16))
    ex = rng_t.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), n_topics)
    eng = B.Engine(device=0)
    eng.retain_rebuild(w.tenants(), tt, packed_topics=(data, off), timestamps=ts, expiry=ex)
    rng = np.random.default_rng(99)
    raw = data.tobytes()
    old = sorted({raw[off[i]:off[i + 1]] for i in rng.choice(n_topics, n_ops // 2, replace=False)})
    new = [b"churn/n%d/x%d" % (j % 977, j) for j in range(n_ops - len(old))]
    codes = np.array([1] * len(old) + [0] * len(new), dtype=np.uint8)
    nts = np.concatenate([np.zeros(len(old), dtype=np.uint64), ((base_ms + rng.integers(0, 100_000, len(new))).astype(np.uint64) << np.uint64(16))])
    nex = np.concatenate([np.zeros(len(old), dtype=np.uint32), rng.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), len(new))])
    eng.retain_apply_batch(w.tenants(), None, None, packed_topics=pack(old + new), op_codes=codes, timestamps=nts, expiry=nex)
    return eng, w, base_ms


def retain_probe():
    a, w, base_ms = churned_c4()
    b, _, _ = churned_c4()  # the same state twice: one engine removes by id, the other by string
    out = {"retained_topics": int(a.retain_info().n_topics), "loaded_removed": int(a.retain_info().loaded_removed), "added_ids": int(a.retain_info().added_ids)}
    counts = a.retain_tenant_counts()
    ms = [timed(a.retain_tenant_counts)[1] for _ in range(9)]
    out["tenant_counts"] = dict(spread(ms), tenants_out=len(counts))
    if sum(n for _, n in counts) != a.retain_info().n_topics:
        raise SystemExit("the tenant counts do not add up to n_topics")
    # a `now` that expires about 100 k topics: the 30 s class is a quarter of the index, its stamps spread over 100 s
    now = base_ms + 30_000 + 40_000
    ids, ms_scan = timed(a.retain_expired, None, now)
    out["expired"] = {"now_ms": now, "ids": len(ids), "scan_ms": ms_scan}
    topics = a.retain_topics(ids)
    (keys, ms_keys) = timed(a.retain_message_keys, ids)
    out["message_keys"] = {"ms": ms_keys, "bytes": sum(map(len, keys))}
    gen = a.retain_info().generation
    ida = np.asarray(ids, dtype=np.uint32)
    removed, ms_ids = timed(a.retain_remove_ids, ida, gen)
    data, off = pack([p for _, p in topics])
    codes = np.ones(len(ids), dtype=np.uint8)
    _, ms_str = timed(b.retain_apply_batch, w.tenants(), None, None, packed_topics=(data, off), op_codes=codes)
    # both engines must be in the same state now (the ids of topics added in ONE batch are handed out in whatever order the lanes arrive,
    # so the engines are compared by their counters and by what is left to expire, not id for id)
    def state(e):
        i = e.retain_info()
        return (int(i.n_topics), int(i.loaded_removed), int(i.id_bound)), e.retain_tenant_counts(), len(e.retain_expired(None, now))
    want = ((out["retained_topics"] - len(ids), None, None), [(counts[0][0], out["retained_topics"] - len(ids))], 0)
    sa, sb = state(a), state(b)
    if removed != len(ids) or sa != sb or sa[0][0] != want[0][0] or sa[1:] != want[1:]:
        raise SystemExit("removal by id and by string leave different indexes: %d ids, %d removed; by id %r, by string %r" % (len(ids), removed, sa, sb))
    # steady state, as the 0.82 ms of the churn leg was taken: the same topics retained again (they get their ids back, stamped to expire),
    # removed again -- by id on one engine, by string on the other; the first calls above carry growth of the overlay's tables and buffers
    ts = np.full(len(ids), (base_ms + 1000) << 16, dtype=np.uint64)
    ex = np.full(len(ids), 30, dtype=np.uint32)
    warm_ids, warm_str = [], []
    for _ in range(3):
        for e in (a, b):
            e.retain_apply_batch(w.tenants(), None, None, packed_topics=(data, off), op_codes=np.zeros(len(ids), dtype=np.uint8), timestamps=ts, expiry=ex)
        again = a.retain_expired(None, now)
        if again != ids:
            raise SystemExit("the topics retained again did not get their ids back")
        r, ms_a = timed(a.retain_remove_ids, ida, gen)
        _, ms_b = timed(b.retain_apply_batch, w.tenants(), None, None, packed_topics=(data, off), op_codes=codes)
        warm_ids.append(ms_a), warm_str.append(ms_b)
        if r != len(ids) or state(a) != state(b) or state(a) != sa:
            raise SystemExit("steady state: removal by id and by string leave different indexes: %r %r" % (state(a), state(b)))
    out["remove_ids"] = {"ids": len(ids), "first_call_ms": ms_ids, "apply_batch_by_string_first_call_ms": ms_str, "steady_ms": [round(x, 3) for x in warm_ids],
                         "apply_batch_by_string_steady_ms": [round(x, 3) for x in warm_str], "topics_left": sa[0][0],
                         "note": "first calls: the string path's batch makes the overlay's tables grow (its worst-case bound counts every level of every op); "
                                 "steady: the same topics retained again and removed again, three times"}
    a.close(), b.close()
    return out


def kernel_row(path):
    """the k_b_census row of a rocprofv3 *kernel_stats.csv"""
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_b_census" in (r.get("Name") or ""):
                return {k: (float(v) if k != "Name" and v not in ("", None) else v) for k, v in r.items()}
    raise SystemExit("no k_b_census row in %s" % path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10000)
    ap.add_argument("--no-retain", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="the census passes only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run: its k_b_census row goes into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tenant_stats.json"))
    args = ap.parse_args()
    out = {"probe": "tools/tenant_stats_probe.py", "device": "MI355X (gfx950), one GPU, one run",
           "timing": "host clock around C-ABI calls that return after a stream synchronise; k_b_census: rocprofv3 --kernel-trace --stats of a --kernel-only run"}
    out["dist"] = dist_probe(args.tenants, args.routes, args.kernel_only)
    if args.kernel_only:
        print(json.dumps(out))
        return
    if not args.no_retain:
        out["retain"] = retain_probe()
    if args.kernel_stats:
        k = kernel_row(args.kernel_stats)
        k["launches_counted"] = "every launch of the --kernel-only run: the warm-up and the timed census passes, all over the whole index"
        out["k_b_census"] = k
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
