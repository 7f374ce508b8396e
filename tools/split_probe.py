#!/usr/bin/env python3
"""Times a split of the route index by KV boundary on the device and writes ONE JSON line (default: profiles/range_split.json).

The C3 index of bench.py (1000 tenants x 10k routes = 10 M keys), cut at the key prefix of the median tenant (in key order):

  count_in     bmq_routes_count_in over the whole index (one pass of k_b_boundary), both halves;
  import       bmq_routes_import of the upper half into a fresh engine: the new sibling range;
  bounded      bmq_compact_begin_in(end = cut) / _poll / _swap on the serving engine, with a match batch between the polls: begin, polls,
               swap, total wall, and the slowest match batch while it runs beside the median batch before it started;
  rescan       in the same run, what a caller must do WITHOUT these calls: bmq_route_keys of every id to the host, cut the (sorted) key
               list, bmq_rebuild of each half.  The cut is a binary search here and the JVM's KV scan, its JNI copies and its filter are
               left out: all of that only widens the gap.

Times are host-clock times around C-ABI calls that return after a stream synchronise.  The per-kernel time of k_b_boundary comes from a
run of its own under `rocprofv3 --kernel-trace --stats -- python tools/split_probe.py --kernel-only` (tracing slows the host: no wall time
of that run is reported); --kernel-stats CSV folds that file's k_b_boundary row into the JSON, next to the bytes the passes read.
Needs a gfx950 device: there is no fallback.

  python tools/split_probe.py [--tenants 1000] [--routes 10000] [--kernel-stats CSV] [--out FILE]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd import _lib  # noqa: E402


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    return r, (time.perf_counter() - t0) * 1e3


def all_keys_to_host(eng, n_ids):
    """bmq_route_keys of every id -> (bytes, offsets) as numpy arrays (no Python object per key)"""
    ids = np.arange(n_ids, dtype=np.uint32)
    off = np.zeros(n_ids + 1, dtype=np.uint64)
    cap = 64 * n_ids
    L = _lib.lib()
    while True:
        out = np.empty(cap + 16, dtype=np.uint8)
        rc = L.bmq_route_keys(eng.h, ids.ctypes.data, n_ids, out.ctypes.data, cap, off.ctypes.data)
        if rc == -3:
            cap = int(off[n_ids])
            continue
        eng._check(rc)
        return out, off


def cut_rank(kb, off, n, s):
    """first rank whose key is >= s: the keys are in KV order"""
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if kb[int(off[mid]):int(off[mid + 1])].tobytes() < s:
            lo = mid + 1
        else:
            hi = mid
    return lo


def rebuild_half(kb, off, lo, hi):
    """a fresh engine from the keys of ranks [lo, hi) -> (engine, ms of the offset arithmetic + bmq_rebuild)"""
    t0 = time.perf_counter()
    o = (off[lo:hi + 1] - off[lo]).astype(np.uint32)
    data = kb[int(off[lo]):int(off[hi]) + 16]
    eng = B.Engine(device=0)
    eng.rebuild_raw(data.ctypes.data, o.ctypes.data, hi - lo)
    return eng, (time.perf_counter() - t0) * 1e3


def probe(n_tenants, routes, n_topics, chunk, kernel_only):
    seed = 0xB1F20003
    w = B.Workload(seed, n_tenants, routes, 1)
    kb, ko = w.keys_packed()
    first = w.tenant_first()
    k0 = int(ko[int(first[n_tenants // 2])])
    tlen = int(kb[k0 + 1]) * 256 + int(kb[k0 + 2])
    cut = kb[k0:k0 + 3 + tlen].tobytes()  # 00 | u16be(len) | tenant of the median tenant
    a = B.Engine(device=0)
    _, ms_load = timed(a.rebuild_raw, kb.ctypes.data, ko.ctypes.data, w.n_keys)
    n_ids = int(a.info().next_route_id)
    out = {"index_routes": int(w.n_keys), "tenants": n_tenants, "cut_key_hex": cut.hex(), "ms_initial_rebuild": ms_load}
    # ---- count_in ----
    a.count_in(end=cut)  # warm-up: code object, scratch copy of the references
    ms = []
    for _ in range(7):
        (lower, ms1) = timed(a.count_in, end=cut)
        (upper, ms2) = timed(a.count_in, start=cut)
        ms += [ms1, ms2]
    if lower[0] + upper[0] != w.n_keys:
        raise SystemExit("count_in: the halves do not add up")
    live_bytes = int(ko[-1])
    out["count_in"] = {"routes_below": lower[0], "routes_from": upper[0], "key_bytes_below": lower[1], "key_bytes_from": upper[1],
                       "ms_call_wall_median": float(np.median(ms)), "ms_call_wall_min": float(min(ms)),
                       "pass_bytes": {"references_copied": 8 * n_ids, "references_read": 8 * n_ids, "key_first_words": 8 * w.n_keys,
                                      "key_lines_upper_bound": min(live_bytes, 64 * w.n_keys),
                                      "note": "per pass: a device copy of kref (8 B/id read + written), then k_b_boundary reads 8 B/id of references and at "
                                              "least the first 8-byte word of every live key (64-byte lines: at most the whole key pool)"}}
    if kernel_only:
        a.close()
        return out
    # ---- the sibling: import of the upper half into a fresh engine ----
    b = B.Engine(device=0)
    (res, ms_import) = timed(b.import_routes, a, start=cut)
    if res != (upper[0], 0):
        raise SystemExit("import: %r, count_in said %r" % (res, upper))
    out["import"] = {"imported": res[0], "ms_call_wall": ms_import, "keys_per_s": res[0] / (ms_import * 1e-3)}
    # ---- the range that shrinks: bounded generation change, a match batch between the polls ----
    tn = w.tenants()
    data, off, tt = w.topics(seed + 1000, n_topics, grouped=True)
    batch = lambda: timed(a.match_batch, tn, tt, packed_topics=(data, off))[1]  # noqa: E731
    for _ in range(3):
        batch()
    quiet = [batch() for _ in range(9)]
    t_all = time.perf_counter()
    _, ms_begin = timed(a.compact_begin, end=cut)
    polls, during, done = [], [], 0
    while done < 1000:
        done, ms1 = timed(a.compact_poll, chunk)
        polls.append(ms1)
        during.append(batch())
    (cr, ms_swap) = timed(a.compact_swap)
    ms_total = (time.perf_counter() - t_all) * 1e3
    if cr != (lower[0], 0) or a.count_in() != lower:
        raise SystemExit("bounded generation change: carried %r, count_in said %r" % (cr, lower))
    out["bounded"] = {"carried": cr[0], "poll_ids": chunk, "polls": len(polls), "ms_begin": ms_begin, "ms_polls_total": float(sum(polls)),
                      "ms_poll_median": float(np.median(polls)), "ms_poll_max": float(max(polls)), "ms_swap": ms_swap,
                      "ms_total_wall_with_match_batches": ms_total, "ms_total_without_match_batches": ms_begin + float(sum(polls)) + ms_swap,
                      "match_batch_topics": n_topics, "ms_match_batch_median_before": float(np.median(quiet)),
                      "ms_match_batch_max_before": float(max(quiet)), "ms_match_batch_median_during": float(np.median(during)),
                      "ms_match_batch_slowest_during": float(max(during))}
    a.close()
    b.close()
    # ---- what a caller does without the three calls: keys to the host, cut, rebuild of each half (same run, same device) ----
    c = B.Engine(device=0)
    c.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    ((hb, hoff), ms_keys) = timed(all_keys_to_host, c, n_ids)
    (r, ms_cut) = timed(cut_rank, hb, hoff, n_ids, cut)
    if r != lower[0]:
        raise SystemExit("rescan: the cut falls at rank %d, count_in said %d" % (r, lower[0]))
    lo_eng, ms_lo = rebuild_half(hb, hoff, 0, r)
    hi_eng, ms_hi = rebuild_half(hb, hoff, r, n_ids)
    ms_rescan = ms_keys + ms_cut + ms_lo + ms_hi
    out["rescan"] = {"ms_route_keys_to_host": ms_keys, "ms_cut": ms_cut, "ms_rebuild_lower": ms_lo, "ms_rebuild_upper": ms_hi, "ms_total": ms_rescan,
                     "left_out": "the JVM's KV scan and its JNI copies; the cut is one binary search over sorted keys, not a compare per key"}
    ms_split = ms_import + out["bounded"]["ms_total_without_match_batches"]
    out["ratios"] = {"rescan_over_split": ms_rescan / ms_split, "rebuild_upper_over_import": ms_hi / ms_import,
                     "rebuild_lower_over_bounded": ms_lo / out["bounded"]["ms_total_without_match_batches"]}
    for e in (c, lo_eng, hi_eng):
        e.close()
    return out


def kernel_row(path):
    """the k_b_boundary row of a rocprofv3 *kernel_stats.csv"""
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_b_boundary" in (r.get("Name") or ""):
                return {"calls": int(r["Calls"]), "ns_total": int(float(r["TotalDurationNs"])), "ns_average": float(r["AverageNs"]),
                        "ns_min": int(float(r["MinNs"])), "ns_max": int(float(r["MaxNs"]))}
    raise SystemExit("no k_b_boundary row in %s" % path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--topics", type=int, default=20_000, help="topics of the match batch between two polls")
    ap.add_argument("--poll-ids", type=int, default=65536)
    ap.add_argument("--kernel-only", action="store_true", help="the count_in passes only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run: its k_b_boundary row goes into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "range_split.json"))
    args = ap.parse_args()
    out = {"probe": "range_split", "library": _lib.lib().bmq_version().decode(),
           "timing": "host clock around C-ABI calls that return after a stream synchronise; k_b_boundary: rocprofv3 --kernel-trace --stats of a --kernel-only run"}
    out.update(probe(args.tenants, args.routes, args.topics, args.poll_ids, args.kernel_only))
    if args.kernel_stats:
        k = kernel_row(args.kernel_stats)
        pb = out["count_in"]["pass_bytes"]
        k["launches_counted"] = "every launch of the --kernel-only run: warm-up and timed count_in passes, all over the whole index"
        k["gb_per_s_references_plus_first_words"] = (pb["references_read"] + pb["key_first_words"]) / k["ns_average"]
        out["k_b_boundary"] = k
    line = json.dumps(out)
    if not args.kernel_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
