#!/usr/bin/env python3
"""What a key-ordered window (bmq_routes_window) and the dist worker's GC sweep over it (bmq_routes_gc_sweep) cost; writes profiles/gc_sweep.json.

On the C3 index of bench.py (1000 tenants x 10 k routes = 10 M keys), clean (ids follow the key order) and after 100 k mutations (50 k deletes
of random keys, 50 k puts of new ones), in ONE process:

  * window of 65 536 from a mid-index cursor;
  * the sweeps (step 1, quota 50 000) -- the cleaner's first -- and (step 10, quota 5 120) -- its largest later one -- from the same cursor;
    --warmup rounds first, then median / min / max of --reps rounds: host clock around the C-ABI call (it returns after the last copy), and the
    window counters per call (candidates behind the cursor, bucketing rounds, buckets ranked);
  * the device memory the first window takes (its scratch; hipMemGetInfo before and after);
  * the yardstick, once, on the churned index: the only way the parent commit offers to read keys in order -- bmq_route_keys of ALL ids to the
    host, then a host sort -- gather and sort timed apart;
  * the batch p99 of a matcher (20 k-topic batches) beside a thread that sweeps in a loop, against its idle p99 from the same run (both take the
    engine lock: a batch submitted during a sweep waits for it);
  * per-kernel times: a child process runs the three calls under `rocprofv3 --kernel-trace --stats` on the clean index and the k_o_* rows of its
    kernel statistics are copied in (--no-kernels skips this).

Needs a gfx950 device: there is no fallback.

  python tools/gc_sweep_probe.py [--reps 10] [--warmup 2] [--out FILE] [--no-kernels]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bifromq_amd as B  # noqa: E402

SEED = 0xB1F20003


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def free_device_bytes():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    if hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise SystemExit("hipMemGetInfo failed")
    return int(free.value)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def key_at(kb, ko, i):
    return kb[int(ko[i]):int(ko[i + 1])].tobytes()


def measure(eng, cursor, reps, warmup):
    """the three calls from `cursor` -> {name: times and counters per call}"""
    out = {}
    calls = (("window_65536", lambda: eng.window(cursor, B.BMQ_WINDOW_MAX)), ("sweep_step1_quota50000", lambda: eng.gc_sweep(cursor, 1, 50000)),
             ("sweep_step10_quota5120", lambda: eng.gc_sweep(cursor, 10, 5120)))
    for name, call in calls:
        ms = []
        for r in range(warmup + reps):
            before = eng.window_info()
            t, res = timed(call)
            after = eng.window_info()
            if r >= warmup:
                ms.append(t)
        per_call = {f: int(getattr(after, f) - getattr(before, f)) for f in ("n_calls", "n_candidates", "n_rounds", "n_bucket_sorts", "n_rebucketed")}
        say(name, "median %.3f ms" % float(np.median(ms)), per_call)
        out[name] = {"ms": spread(ms), "last_call": per_call, "routes_returned": int(len(res[0]))}
    return out


def build(args):
    w = B.Workload(SEED, args.tenants, args.routes, 1)
    eng = B.Engine(device=0)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    return w, eng, kb, ko


def child(args):
    w, eng, kb, ko = build(args)
    cursor = key_at(kb, ko, w.n_keys // 2)
    for _ in range(3):
        eng.window(cursor, B.BMQ_WINDOW_MAX)
        eng.gc_sweep(cursor, 1, 50000)
        eng.gc_sweep(cursor, 10, 5120)
    eng.close()


def kernel_rows(args):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "gc", "--", sys.executable, os.path.abspath(__file__), "--child", "--tenants", str(args.tenants), "--routes",
               str(args.routes)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "k_o_" in row.get("Name", ""):
                    rows.append({"kernel": row["Name"].split("(")[0], "calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                                 "average_us": float(row["AverageNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3})
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mutations", type=int, default=100_000)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gc_sweep.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    kernels = [] if args.no_kernels else kernel_rows(args)  # (before this process opens the device itself)
    say("kernel rows:", len(kernels))
    w, eng, kb, ko = build(args)
    n = w.n_keys
    cursor = key_at(kb, ko, n // 2)
    free0 = free_device_bytes()
    first_ms, (ids, more) = timed(lambda: eng.window(cursor, B.BMQ_WINDOW_MAX))
    scratch = free0 - free_device_bytes()
    if eng.route_keys(ids[:3]) != [key_at(kb, ko, n // 2 + i) for i in range(3)] or not more:
        raise SystemExit("the window does not begin at the cursor")
    res = {"probe": "tools/gc_sweep_probe.py", "device": "MI355X (gfx950), one GPU, one run", "workload": "C3: %d tenants x %d routes" % (args.tenants, args.routes),
           "timing": "host clock around the C-ABI calls, %d warm-up round(s), then median / min / max of %d" % (args.warmup, args.reps), "index_routes": int(n),
           "bucket_max": int(eng.window_info().bucket_max), "first_window_ms": first_ms, "scratch_bytes": int(scratch), "kernels_clean_index": kernels}
    res["clean"] = measure(eng, cursor, args.reps, args.warmup)
    # ---- the matcher beside a loop of sweeps
    tn = w.tenants()
    data, off, tt = w.topics(SEED + 7, 20000)

    def batches(k):
        ms = []
        for _ in range(k):
            t, _r = timed(lambda: eng.match_batch(tn, tt, packed_topics=(data, off)))
            ms.append(t)
        return ms
    batches(20)
    idle = batches(200)
    stop = threading.Event()
    n_sweeps = [0]

    def sweeper():
        while not stop.is_set():
            eng.gc_sweep(cursor, 10, 5120)
            n_sweeps[0] += 1
    th = threading.Thread(target=sweeper)
    th.start()
    busy = batches(200)
    stop.set()
    th.join()
    res["matcher_beside_sweeps"] = {"batch_topics": 20000, "idle_ms": {"p50": float(np.percentile(idle, 50)), "p99": float(np.percentile(idle, 99))},
                                    "beside_sweeps_ms": {"p50": float(np.percentile(busy, 50)), "p99": float(np.percentile(busy, 99))}, "sweeps_meanwhile": n_sweeps[0]}
    say("matcher:", res["matcher_beside_sweeps"])
    # ---- 100 k mutations
    rng = np.random.default_rng(20261020)
    gone = rng.choice(n, size=args.mutations // 2, replace=False)
    ops = [(1, key_at(kb, ko, int(i))) for i in gone] + [(0, B.route_key(tn[i % len(tn)], "gc/probe/%d" % i, 1, "0\0inbox%d\0d" % (i % 5))) for i in range(args.mutations // 2)]
    order = rng.permutation(len(ops))
    for at in range(0, len(ops), 10000):
        eng.apply([ops[int(j)] for j in order[at:at + 10000]])
    res["churned"] = measure(eng, cursor, args.reps, args.warmup)
    res["churned"]["mutations"] = len(ops)
    # ---- the yardstick: every key to the host, then a host sort
    n_ids = int(eng.info().next_route_id)
    t_gather, keys = timed(lambda: [k for at in range(0, n_ids, 1 << 20) for k in eng.route_keys(np.arange(at, min(n_ids, at + (1 << 20)), dtype=np.uint32)) if k])
    say("gathered %d keys in %.0f ms" % (len(keys), t_gather))
    t_sort, keys = timed(lambda: sorted(keys))
    res["host_alternative_churned"] = {"what": "bmq_route_keys of all %d ids in chunks of 2^20 (Python lists of bytes), then sorted()" % n_ids, "gather_ms": t_gather, "sort_ms": t_sort,
                                       "live_keys": len(keys)}
    ids, _ = eng.window(cursor, 1000)
    import bisect
    at = bisect.bisect_left(keys, cursor)
    if eng.route_keys(ids) != keys[at:at + 1000]:
        raise SystemExit("the window on the churned index differs from the host sort")
    eng.close()
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
