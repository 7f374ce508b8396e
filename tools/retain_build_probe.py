#!/usr/bin/env python3
"""Times the bulk load of the retained-topic index with both builders and writes ONE JSON line (default: profiles/retain_build.json).

Two loads of the same size: the C4 index of bench.py (--topics retained topics of ONE tenant, with stamps) and the same number of topics spread
over 1 000 tenants.  Per load, on two engines of one process -- bmq_config.retain_builder = 0 (the host builder: the parent's code path, the
baseline) and = 1 (the executor builder: the k_rb_* kernels) -- alternated call by call after a warm-up:

  rebuild    bmq_retain_rebuild_ex of the packed items: median of --reps;
  compact    bmq_retain_compact of the loaded index (snapshot of the live topics + the load): median of --reps;
  ms_total / ms_sort   what bmq_retain_build_info reports of the last builder-1 load (host clock around the build, ending in a synchronise;
             of which the ordering of the items).

Times are host-clock times around C-ABI calls that return after a stream synchronise.  The probe exits with an error if the two engines do not
hold the same topics under the same ids, or if the builder-1 engine fell back.  Kernel times come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/retain_build_probe.py --kernel-only` (one builder-1 load per shape; tracing slows the host: no
wall time of that run is reported); --kernel-stats CSV folds that file's k_rb_* rows and the sort kernels into the JSON.  Needs a gfx950 device:
there is no fallback.

  python tools/retain_build_probe.py [--topics 1000000] [--reps 7] [--kernel-only] [--kernel-stats CSV] [--out FILE]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402

SEED = 0xB1F20004
BASE_MS = 1_700_000_000_000


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    f(*a, **kw)
    return (time.perf_counter() - t0) * 1e3


def make_load(n_tenants, n):
    w = B.Workload(SEED, n_tenants, 1, 0)
    data, off, tt = w.retain(SEED, n, filters=False)
    rng = np.random.default_rng(0xB1F2)
    ts = ((BASE_MS + rng.integers(0, 100_000, n)).astype(np.uint64) << np.uint64(16))
    ex = rng.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), n)
    return w.tenants(), tt, (data, off), ts, ex


def rebuild(eng, load):
    tenants, tt, packed, ts, ex = load
    eng.retain_rebuild(tenants, tt, packed_topics=packed, timestamps=ts, expiry=ex)


def info_dict(eng):
    bi = eng.retain_build_info()
    return {f: (round(float(getattr(bi, f)), 3) if f.startswith("ms_") else int(getattr(bi, f))) for f, _ in bi._fields_}


def same_ids(a, b, n_sample=4096):
    ia, ib = a.retain_info(), b.retain_info()
    if (int(ia.n_topics), int(ia.id_bound)) != (int(ib.n_topics), int(ib.id_bound)):
        return False
    n = int(ia.id_bound)
    ids = np.unique(np.concatenate([np.arange(min(n, 64)), np.arange(max(0, n - 64), n), np.random.default_rng(1).integers(0, max(n, 1), n_sample)])).astype(np.uint32) if n else []
    return a.retain_topics(ids) == b.retain_topics(ids) and all(a.retain_topic_info(int(i)) == b.retain_topic_info(int(i)) for i in ids[:256])


def measure(name, load, reps):
    e0, e1 = B.Engine(device=0, retain_builder=0), B.Engine(device=0, retain_builder=1)
    try:
        rebuild(e0, load), rebuild(e1, load)                       # warm-up: allocations, code objects
        if not same_ids(e0, e1):
            sys.exit("%s: the two builders disagree on ids" % name)
        t = {"rebuild": ([], []), "compact": ([], [])}
        infos = []
        for _ in range(reps):
            for k, e in enumerate((e0, e1)):
                t["rebuild"][k].append(timed(rebuild, e, load))
                if k:
                    infos.append(info_dict(e))
                t["compact"][k].append(timed(e.retain_compact))
        bi = info_dict(e1)
        if bi["builder"] != 1 or bi["fallback"] or infos[-1]["builder"] != 1:
            sys.exit("%s: the builder-1 engine fell back" % name)
        if not same_ids(e0, e1):
            sys.exit("%s: the two builders disagree on ids after compaction" % name)
        out = {"topics": int(e1.retain_info().n_topics), "tenants": int(e1.retain_info().n_tenants), "reps": reps}
        for what, (h, x) in t.items():
            out[what + "_ms"] = {"builder0_median": round(statistics.median(h), 2), "builder1_median": round(statistics.median(x), 2),
                                 "builder0_all": [round(v, 1) for v in h], "builder1_all": [round(v, 1) for v in x]}
        out["build_info_rebuild"] = infos[-1]
        out["build_info_compact"] = bi
        out["ms_total_median"] = round(statistics.median(i["ms_total"] for i in infos), 2)
        out["ms_sort_median"] = round(statistics.median(i["ms_sort"] for i in infos), 2)
        return out
    finally:
        e0.close(), e1.close()


def kernel_rows(path):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            nm = r.get("Name", "")
            if "k_rb_" in nm or "RbItemLess" in nm or "merge_sort" in nm:
                short = nm.split("(")[0].replace("bmq::", "") if "k_rb_" in nm else ("merge sort: " + ("block_sort" if "block_sort" in nm else "merge"))
                d = rows.setdefault(short, {"calls": 0, "total_us": 0.0})
                d["calls"] += int(r.get("Calls", 0))
                d["total_us"] += float(r.get("TotalDurationNs", 0)) / 1e3
    return {k: {"calls": v["calls"], "total_us": round(v["total_us"], 1)} for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_us"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "retain_build.json"))
    a = ap.parse_args()
    shapes = [("c4_one_tenant", 1), ("thousand_tenants", 1000)]
    if a.kernel_only:
        for name, nt in shapes:
            e = B.Engine(device=0, retain_builder=1)
            rebuild(e, make_load(nt, a.topics))
            print(name, info_dict(e))
            e.close()
        return
    res = {"probe": "retain_build", "topics_per_load": a.topics, "clock": "host clock around calls that end in a stream synchronise; medians of reps, builders alternated in one process"}
    for name, nt in shapes:
        res[name] = measure(name, make_load(nt, a.topics), a.reps)
    if a.kernel_stats:
        res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (one builder-1 load per shape)", "kernels": kernel_rows(a.kernel_stats)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
