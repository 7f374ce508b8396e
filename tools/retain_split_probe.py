#!/usr/bin/env python3
"""Times a split of the retained-topic index by KV boundary on the device and writes ONE JSON line (default: profiles/retain_split.json).

The C4 index of bench.py (1 M retained topics, 1 tenant, with stamps), cut at the median retainMessageKey:

  count_in   bmq_retain_count_in(end = cut) over the whole index (one pass of k_r_boundary, key bytes included): median of 9;
  import     bmq_retain_import of the upper half into a fresh engine: the new sibling range (a bulk load);
  bounded    bmq_retain_compact_begin_in(end = cut) / _build / _swap on the serving engine: the range that shrinks;
  host       in the same run, what a caller does today: bmq_retain_live_ids + bmq_retain_topics to the host, the cut (bmq_retain_message_keys
             and a compare per key), two bmq_retain_rebuild calls.  The JVM's KV scan and its JNI copies are left out; the host route
             rebuilds without stamps (it would need a bmq_retain_topic_info per id, or the KV values, for them).

The probe exits with an error if the two routes leave different topic sets.  Times are host-clock times around C-ABI calls that return after
a stream synchronise.  The time of k_r_boundary alone comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/retain_split_probe.py --kernel-only` (tracing slows the host: no wall time of that run is
reported); --kernel-stats CSV folds that file's k_r_boundary row into the JSON.  Needs a gfx950 device: there is no fallback.

  python tools/retain_split_probe.py [--topics 1000000] [--kernel-only] [--kernel-stats CSV] [--out FILE]"""
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

SEED = 0xB1F20004
BASE_MS = 1_700_000_000_000


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    r = f(*a, **kw)
    return r, (time.perf_counter() - t0) * 1e3


def load_c4(n):
    w = B.Workload(SEED, 1, 1, 0)
    data, off, tt = w.retain(SEED, n, filters=False)
    rng = np.random.default_rng(0xB1F2)
    ts = ((BASE_MS + rng.integers(0, 100_000, n)).astype(np.uint64) << np.uint64(16))
    ex = rng.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), n)
    eng = B.Engine(device=0)
    _, ms = timed(eng.retain_rebuild, w.tenants(), tt, packed_topics=(data, off), timestamps=ts, expiry=ex)
    return eng, w, ms


def raw_ids(eng):
    n = C.c_uint32()
    cap = int(eng.retain_info().n_topics) + 16
    out = np.zeros(cap, dtype=np.uint32)
    eng._check(_lib.lib().bmq_retain_live_ids(eng.h, None, 0, ptr(out), cap, C.byref(n)))
    return out[:n.value]


def raw_strings(eng, call, ids, with_tenant_len):
    """bmq_retain_topics / bmq_retain_message_keys of ids -> (bytes, offsets[, tenant lengths]) as numpy arrays (no Python object per topic)"""
    n = len(ids)
    off, tl = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
    cap = 64 * n
    while True:
        out = np.empty(cap + 16, dtype=np.uint8)
        rc = call(eng.h, ptr(ids), n, ptr(out), cap, ptr(off), ptr(tl)) if with_tenant_len else call(eng.h, ptr(ids), n, ptr(out), cap, ptr(off))
        if rc == -3:
            cap = int(off[n]) + 16
            continue
        eng._check(rc)
        return out, off.astype(np.int64), tl.astype(np.int64)


def topic_set(eng):
    ids = raw_ids(eng)
    out, off, _ = raw_strings(eng, _lib.lib().bmq_retain_topics, ids, True)
    raw = out.tobytes()
    return {raw[off[i]:off[i + 1]] for i in range(len(ids))}


def rebuild_half(w, out, off, tl, sel):
    """a fresh engine from the topics sel (indices into the host copy) -> (engine, ms of the gather + bmq_retain_rebuild)"""
    t0 = time.perf_counter()
    starts, lens = (off[:-1] + tl[:len(off) - 1])[sel], (off[1:] - off[:-1] - tl[:len(off) - 1])[sel]
    o = np.zeros(len(sel) + 1, dtype=np.int64)
    o[1:] = np.cumsum(lens)
    data = np.concatenate([out[np.repeat(starts - o[:-1], lens) + np.arange(o[-1])], np.zeros(16, dtype=np.uint8)])
    eng = B.Engine(device=0)
    eng.retain_rebuild(w.tenants(), np.zeros(len(sel), dtype=np.uint32), packed_topics=(data, o.astype(np.uint32)))
    return eng, (time.perf_counter() - t0) * 1e3


def probe(n, kernel_only):
    a, w, ms_load = load_c4(n)
    ids = raw_ids(a)
    kb, koff, _ = raw_strings(a, _lib.lib().bmq_retain_keys_by_id, ids, False)   # (also builds the key store: not part of any timed call below)
    raw = kb.tobytes()
    cut = sorted(raw[koff[i]:koff[i + 1]] for i in range(len(ids)))[len(ids) // 2]
    out = {"index_topics": int(a.retain_info().n_topics), "cut_key_hex": cut.hex(), "ms_initial_rebuild": ms_load, "key_bytes_all": int(koff[-1])}
    a.retain_count_in(end=cut)  # warm-up: the code object
    ms, lower = [], None
    for _ in range(9):
        lower, ms1 = timed(a.retain_count_in, end=cut)
        ms.append(ms1)
    upper = a.retain_count_in(start=cut)
    (ids_lower, ms_ids) = timed(a.retain_ids_in, end=cut)
    if lower[0] + upper[0] != out["index_topics"] or lower[1] + upper[1] != int(koff[-1]) or len(ids_lower) != lower[0]:
        raise SystemExit("count_in: the halves do not add up")
    out["count_in"] = {"topics_below": lower[0], "topics_from": upper[0], "key_bytes_below": lower[1], "key_bytes_from": upper[1],
                       "ms_call_wall_median": float(np.median(ms)), "ms_call_wall_min": float(min(ms)), "ms_ids_in_call_wall": ms_ids}
    if kernel_only:
        a.close()
        return out
    # ---- the sibling: import of the upper half into a fresh engine ----
    b = B.Engine(device=0)
    (res, ms_import) = timed(b.retain_import, a, start=cut)
    if res != (upper[0], 0) or b.retain_info().loaded_topics != upper[0]:
        raise SystemExit("import: %r, count_in said %r" % (res, upper))
    out["import"] = {"imported": res[0], "ms_call_wall": ms_import, "topics_per_s": res[0] / (ms_import * 1e-3)}
    # ---- the range that shrinks: bounded generation change ----
    _, ms_begin = timed(a.retain_compact_begin, end=cut)
    _, ms_build = timed(a.retain_compact_build)
    (cr, ms_swap) = timed(a.retain_compact_swap)
    if cr != (lower[0], 0) or a.retain_count_in()[0] != lower[0]:
        raise SystemExit("bounded generation change: carried %r, count_in said %r" % (cr, lower))
    out["bounded"] = {"carried": cr[0], "ms_begin": ms_begin, "ms_build_no_engine_lock": ms_build, "ms_swap": ms_swap, "ms_total": ms_begin + ms_build + ms_swap}
    split_sets = (topic_set(a), topic_set(b))
    a.close()
    b.close()
    # ---- what a caller does today: ids and topics to the host, the cut, a rebuild of each half (same run, same device) ----
    c, _, _ = load_c4(n)
    t0 = time.perf_counter()
    cids = raw_ids(c)
    tb, toff, tl = raw_strings(c, _lib.lib().bmq_retain_topics, cids, True)
    ms_topics = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hb, hoff, _ = raw_strings(c, _lib.lib().bmq_retain_message_keys, cids, False)
    ms_keys = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    hraw = hb.tobytes()
    below = np.fromiter((hraw[hoff[i]:hoff[i + 1]] < cut for i in range(len(cids))), dtype=bool, count=len(cids))
    ms_cut = (time.perf_counter() - t0) * 1e3
    lo_eng, ms_lo = rebuild_half(w, tb, toff, tl, np.nonzero(below)[0])
    hi_eng, ms_hi = rebuild_half(w, tb, toff, tl, np.nonzero(~below)[0])
    host_sets = (topic_set(lo_eng), topic_set(hi_eng))
    if split_sets != host_sets:
        raise SystemExit("the two routes leave different topic sets: %d / %d topics against %d / %d" % tuple(len(s) for s in split_sets + host_sets))
    ms_host = ms_topics + ms_keys + ms_cut + ms_lo + ms_hi
    out["host"] = {"ms_live_ids_and_topics_to_host": ms_topics, "ms_message_keys_on_host": ms_keys, "ms_compare_per_key_python": ms_cut, "ms_rebuild_lower": ms_lo,
                   "ms_rebuild_upper": ms_hi, "ms_total": ms_host, "ms_total_without_the_python_compare": ms_host - ms_cut,
                   "left_out": "the JVM's KV scan and its JNI copies; the stamps of the topics (the host route rebuilds without them)"}
    ms_split = ms_import + out["bounded"]["ms_total"]
    out["ratios"] = {"host_over_split": ms_host / ms_split, "host_without_python_compare_over_split": (ms_host - ms_cut) / ms_split,
                     "rebuild_upper_over_import": ms_hi / ms_import, "rebuild_lower_over_bounded": ms_lo / out["bounded"]["ms_total"]}
    out["topic_sets_equal"] = True
    for e in (c, lo_eng, hi_eng):
        e.close()
    return out


def kernel_row(path):
    """the k_r_boundary row of a rocprofv3 *kernel_stats.csv"""
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_r_boundary" in (r.get("Name") or ""):
                return {"calls": int(r["Calls"]), "ns_total": int(float(r["TotalDurationNs"])), "ns_average": float(r["AverageNs"]),
                        "ns_min": int(float(r["MinNs"])), "ns_max": int(float(r["MaxNs"]))}
    raise SystemExit("no k_r_boundary row in %s" % path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--kernel-only", action="store_true", help="the count_in / ids_in passes only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run: its k_r_boundary row goes into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "retain_split.json"))
    args = ap.parse_args()
    out = {"probe": "retain_split", "library": _lib.lib().bmq_version().decode(),
           "timing": "host clock around C-ABI calls that return after a stream synchronise; k_r_boundary: rocprofv3 --kernel-trace --stats of a --kernel-only run"}
    out.update(probe(args.topics, args.kernel_only))
    if args.kernel_stats:
        k = kernel_row(args.kernel_stats)
        k["launches_counted"] = "every launch of the --kernel-only run: warm-up, 9 timed count_in(end), one count_in(start), one ids_in(end), all over the whole index"
        out["k_r_boundary"] = k
    line = json.dumps(out)
    if not args.kernel_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
