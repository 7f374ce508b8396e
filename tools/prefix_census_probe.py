#!/usr/bin/env python3
"""What the per-prefix census (bmq_routes_prefix_census) costs, beside the parent commit's way of answering the same question; writes
profiles/prefix_census.json.

On the C3 index of bench.py (1000 tenants x 10 k routes = 10 M keys) after ONE 100 k-op churn batch as bench.py --churn makes it (50 k deletes of
random keys, 50 k puts under new filters, interleaved), in ONE process:

  * the distinct filter prefixes of the batch (bifromq_amd.hinter.filter_prefix of every op's key) -- what RangeFanoutSplitHinter.record_mutate
    passes; padded with the filter prefixes of further index keys where the batch has fewer than 65 536;
  * prefix_census for n = 1, 1 024 and 65 536 of them: --warmup calls, then median / min / max of --reps calls, host clock around the blocking
    C-ABI call (it returns after the counters came back), and the info counters of the last call;
  * in the SAME run the parent commit's way: 1 024 successive count_in(p, upper_bound(p)) calls over the same 1 024 prefixes, the whole
    loop timed --reps-loop times; the answers of both ways are compared;
  * the device memory the largest call takes (hipMemGetInfo before and after);
  * the state of the box as far as it can be read without changing it: the CPUs this process may use, the load average, the GPU clocks
    rocm-smi shows;
  * the kernel alone: a child process makes five calls of each n under `rocprofv3 --kernel-trace` (a run of its own, before this process
    opens the device) and the durations of its k_b_prefix_census dispatches are copied in, in dispatch order (--no-kernels skips this);
  * k_b_prefix_census's registers, spills and scratch, if --resource-usage FILE names a build log made with
    -Rpass-analysis=kernel-resource-usage.

Needs a gfx950 device: there is no fallback.

  python tools/prefix_census_probe.py [--reps 20] [--warmup 3] [--out FILE] [--resource-usage build.log] [--no-kernels]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bifromq_amd as B  # noqa: E402
from bifromq_amd import hinter as H  # noqa: E402

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


def box_state():
    out = {"cpus_usable": len(os.sched_getaffinity(0)), "cpus_total": os.cpu_count(), "loadavg": list(os.getloadavg()),
           "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)  # (reads only)
        out["gpu_clocks"] = [ln.strip() for ln in r.stdout.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln or "fclk" in ln)]
    except Exception as ex:  # noqa: BLE001
        out["gpu_clocks"] = "not read: %s" % ex
    return out


def resource_usage(path):
    """the remarks of -Rpass-analysis=kernel-resource-usage about k_b_prefix_census in a build log"""
    out, on = {}, False
    for ln in open(path, errors="replace"):
        m = re.search(r"remark: (Function Name: (\S+)|\s+([A-Za-z][^:]*): (\S+))", ln)
        if not m:
            continue
        if m.group(2):
            on = "k_b_prefix_census" in m.group(2)
        elif on:
            out[m.group(3).strip()] = m.group(4)
    return out


CHILD_CALLS = 5


def kernel_rows(args):
    """-> {n: the durations in microseconds of the k_b_prefix_census dispatches of the child's calls with n prefixes}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "pc", "--", sys.executable, os.path.abspath(__file__), "--child", "--tenants",
               str(args.tenants), "--routes", str(args.routes), "--churn", str(args.churn)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=900)
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "k_b_prefix_census" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
        rows.sort()
        us = [r[1] for r in rows]
        if len(us) != 3 * CHILD_CALLS:
            return {"error": "%d dispatches of k_b_prefix_census in the trace, expected %d" % (len(us), 3 * CHILD_CALLS)}
        return {"n_%d" % m: us[i * CHILD_CALLS:(i + 1) * CHILD_CALLS] for i, m in enumerate((1, 1024, B.BMQ_PREFIX_MAX))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--routes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-loop", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--churn", type=int, default=100_000)
    ap.add_argument("--resource-usage", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--device", type=int, default=0, help="-1: a rehearsal of this script on the host executor; its figures say nothing about the GPU")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_census.json"))
    args = ap.parse_args()
    kernels = None if args.no_kernels or args.child or args.device < 0 else kernel_rows(args)  # (before this process opens the device itself)
    w = B.Workload(SEED, args.tenants, args.routes, 1)
    eng = B.Engine(device=args.device)
    kb, ko = w.keys_packed()
    eng.rebuild_raw(kb.ctypes.data, ko.ctypes.data, w.n_keys)
    n = w.n_keys
    mv = memoryview(kb)
    key_at = lambda i: bytes(mv[int(ko[i]):int(ko[i + 1])])  # noqa: E731
    # ---- one churn batch, as bench.py --churn makes it
    rng = np.random.default_rng(1234)
    tn = w.tenants()
    dels = rng.permutation(n)[:args.churn // 2]
    keys_b, ops_b = [key_at(int(i)) for i in dels], [1] * (args.churn // 2)
    for q in range(1, args.churn - args.churn // 2 + 1):
        t = tn[int(rng.integers(0, len(tn)))]
        keys_b.append(B.route_key(t, "churn/l1_%d/+/l3_%d" % (q % 64, q % 4096), 1, "0\0c%d\0d%d" % (q, q % 64)))
        ops_b.append(0)
    order = rng.permutation(len(keys_b))
    ops = [(ops_b[int(i)], keys_b[int(i)]) for i in order]
    t_apply, _ = timed(lambda: eng.apply(ops))
    seen, prefixes = set(), []
    for _, k in ops:  # distinct, in the order of the batch
        p = H.filter_prefix(k)
        if p not in seen:
            seen.add(p)
            prefixes.append(p)
    n_batch = len(prefixes)
    at = 0
    while len(prefixes) < B.BMQ_PREFIX_MAX and at < n:  # (a batch with fewer distinct filters: further filters of the index)
        p = H.filter_prefix(key_at(at))
        at += 97
        if p not in seen:
            seen.add(p)
            prefixes.append(p)
    if args.child:
        for m in (1, 1024, B.BMQ_PREFIX_MAX):
            for _ in range(CHILD_CALLS):
                eng.prefix_census(prefixes[:m])
        eng.close()
        return
    say("index %d keys, batch %d ops in %.1f ms, %d distinct filter prefixes in the batch" % (n, len(ops), t_apply, n_batch))
    res = {"probe": "tools/prefix_census_probe.py", "device": "MI355X (gfx950), one GPU, one run" if args.device >= 0 else "REHEARSAL on the host executor: no figure is a measurement", "workload": "C3: %d tenants x %d routes" % (args.tenants, args.routes),
           "timing": "host clock around the blocking C-ABI call, %d warm-up call(s), then median / min / max of %d" % (args.warmup, args.reps),
           "index_routes": int(eng.info().n_routes), "index_ids": int(eng.info().next_route_id), "churn_ops": len(ops), "distinct_filter_prefixes_of_the_batch": n_batch,
           "box": box_state()}
    free0 = free_device_bytes() if args.device >= 0 else 0
    first_ms, _ = timed(lambda: eng.prefix_census(prefixes[:B.BMQ_PREFIX_MAX]))
    res["first_call_65536_ms"] = first_ms
    res["scratch_bytes"] = free0 - free_device_bytes() if args.device >= 0 else None
    res["prefix_census"] = {}
    answers = {}
    for m in (1, min(1024, len(prefixes)), min(B.BMQ_PREFIX_MAX, len(prefixes))):
        data, off = B.pack(prefixes[:m])
        ms = []
        for r in range(args.warmup + args.reps):
            before = eng.prefix_census_info()
            t, got = timed(lambda: eng.prefix_census(packed=(data, off)))
            after = eng.prefix_census_info()
            if r >= args.warmup:
                ms.append(t)
        last = {f: int(getattr(after, f) - getattr(before, f)) for f in ("n_calls", "n_prefixes", "n_distinct", "n_nested", "n_keys_scanned")}
        last["engine_last_ms"] = float(after.last_ms)
        answers[m] = got
        say("prefix_census n = %d: median %.3f ms" % (m, float(np.median(ms))), last)
        res["prefix_census"]["n_%d" % m] = {"ms": spread(ms), "last_call": last, "prefixes_with_keys": int((got[:, :3].sum(axis=1) > 0).sum())}
    # ---- the parent commit's way: one boundary count per prefix
    bounds = [(p, H.upper_bound(p)) for p in prefixes[:1024]]
    loop_ms, counted = [], None
    for r in range(1 + args.reps_loop):
        t, counted = timed(lambda: [eng.count_in(p, ub) for p, ub in bounds])
        if r >= 1:
            loop_ms.append(t)
    say("1024 count_in calls: median %.1f ms" % float(np.median(loop_ms)))
    if [(int(r[0] + r[1] + r[2]), int(r[3])) for r in answers[min(1024, len(prefixes))]] != counted:
        raise SystemExit("prefix_census and count_in disagree")
    res["count_in_loop_1024"] = {"what": "1024 successive bmq_routes_count_in(p, upper_bound(p)) calls over the same prefixes, the whole loop timed; 1 warm-up loop",
                                 "ms": spread(loop_ms), "ms_per_call": float(np.median(loop_ms)) / 1024}
    res["speedup_1024"] = float(np.median(loop_ms)) / res["prefix_census"]["n_%d" % min(1024, len(prefixes))]["ms"]["median"]
    res["one_call_beats_1024_boundary_calls"] = bool(res["speedup_1024"] > 1.0)
    if kernels is not None:
        res["k_b_prefix_census_us_under_rocprofv3"] = kernels
    if args.resource_usage:
        res["k_b_prefix_census_resources"] = resource_usage(args.resource_usage)
    eng.close()
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
