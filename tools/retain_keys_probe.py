#!/usr/bin/env python3
"""Times RetainStoreCoProc.match(limit, now) WITH its keys, and the key step of the GC recipe, and writes ONE JSON line (default:
profiles/retain_keys.json).

The C4 index of bench.py (1 M retained topics, 1 tenant) with the 100 k filters of its first batch, limit 10, `now` in the middle of the expiry
instants; clean, and after a 100 k-op churn batch (50 k bulk-loaded topics removed, 50 k new ones added).  Per state, in one process:

  A  bmq_retain_match_limited, then bmq_retain_message_keys of the kept ids: both unchanged, the path a caller had before (the key step is host
     code under the engine lock);
  B  bmq_retain_keys_match: the same rows plus the keys, composed by k_r_key_len / k_r_key_write where the kept ids lie.
The key bytes and offsets of A and B must be equal and B must beat A.  Also: bmq_retain_match_limited alone (B minus it = what the keys cost),
the one-time bmq_retain_keys_prepare (the device-resident string store of the generation), and the GC recipe's key step -- bmq_retain_keys_by_id
against bmq_retain_message_keys on the ids bmq_retain_expired returns (about 100 k; DESIGN 3.3 quotes 46 ms for 104 487 ids on the host path).

Times are host-clock times around C-ABI calls that return after a stream synchronise: warm-up first, then the median and the spread of the
repeats.  The key kernels' own time comes from a run under `rocprofv3 --kernel-trace --stats -- python tools/retain_keys_probe.py --kernel-only`
(tracing slows the host: no wall time of that run is reported); --kernel-stats CSV folds the k_r_key_* rows of that file into the JSON as GB/s of
key bytes written.  Needs a gfx950 device: there is no fallback.

  python tools/retain_keys_probe.py [--reps 7] [--kernel-only] [--kernel-stats CSV] [--out FILE]"""
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
from bifromq_amd.engine import pack  # noqa: E402

SEED = 0xB1F20004
BASE_MS = 1_700_000_000_000
N_TOPICS, N_FILTERS, LIMIT, N_OPS = 1_000_000, 100_000, 10, 100_000


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs": len(ms)}


def clock(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def load_c4():
    w = B.Workload(SEED, 1, 1, 0)
    data, off, tt = w.retain(SEED, N_TOPICS, filters=False)
    rng_t = np.random.default_rng(0xB1F2)
    ts = ((BASE_MS + rng_t.integers(0, 100_000, N_TOPICS)).astype(np.uint64) << np.uint64(16))
    ex = rng_t.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), N_TOPICS)
    eng = B.Engine(device=0)
    eng.retain_rebuild(w.tenants(), tt, packed_topics=(data, off), timestamps=ts, expiry=ex)
    return eng, w, (data, off)


def churn(eng, w, topics):
    """bench.py's churn leg: N_OPS / 2 bulk-loaded topics removed, N_OPS / 2 new ones added, one batch"""
    data, off = topics
    rng = np.random.default_rng(99)
    raw = data.tobytes()
    old = sorted({raw[off[i]:off[i + 1]] for i in rng.choice(N_TOPICS, N_OPS // 2, replace=False)})
    new = [b"churn/n%d/x%d" % (j % 977, j) for j in range(N_OPS - len(old))]
    codes = np.array([1] * len(old) + [0] * len(new), dtype=np.uint8)
    nts = np.concatenate([np.zeros(len(old), dtype=np.uint64), ((BASE_MS + rng.integers(0, 100_000, len(new))).astype(np.uint64) << np.uint64(16))])
    nex = np.concatenate([np.zeros(len(old), dtype=np.uint32), rng.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), len(new))])
    eng.retain_apply_batch(w.tenants(), None, None, packed_topics=pack(old + new), op_codes=codes, timestamps=nts, expiry=nex)


class Calls:
    """the three C-ABI calls over buffers allocated once (no Python list is built inside a timed region)"""

    def __init__(self, eng, w, filters):
        self.eng, self.lib = eng, _lib.lib()
        self.tdata, self.toff = w.tenants_packed()
        self.fdata, self.foff, self.ft = filters
        self.n = len(self.foff) - 1
        self.lim = np.full(self.n, LIMIT, dtype=np.uint32)
        cap = self.n * LIMIT + 16
        self.cap, self.kcap = cap, 96 * cap
        self.row, self.cnt = np.zeros(self.n + 1, np.uint32), np.zeros(self.n, np.uint32)
        self.ids = np.zeros(cap, np.uint32)
        self.koff_a, self.koff_b = np.zeros(cap + 1, np.uint64), np.zeros(cap + 1, np.uint64)
        self.keys_a, self.keys_b = np.zeros(self.kcap, np.uint8), np.zeros(self.kcap, np.uint8)
        self.need, self.kneed = C.c_uint64(), C.c_uint64()

    def check(self, rc, what):
        if rc != 0:
            raise SystemExit("%s failed: %d %s" % (what, rc, self.lib.bmq_last_error(self.eng.h)))

    def limited(self, now):
        self.check(self.lib.bmq_retain_match_limited(self.eng.h, ptr(self.tdata), ptr(self.toff), 1, ptr(self.ft), ptr(self.fdata), ptr(self.foff), self.n, ptr(self.lim), now,
                                                     ptr(self.row), ptr(self.ids), self.cap, C.byref(self.need), ptr(self.cnt)), "bmq_retain_match_limited")
        return int(self.need.value)

    def message_keys(self, ids, n, koff, keys):
        self.check(self.lib.bmq_retain_message_keys(self.eng.h, ptr(ids), n, ptr(keys), self.kcap, ptr(koff)), "bmq_retain_message_keys")
        return int(koff[n])

    def keys_by_id(self, ids, n, koff, keys):
        self.check(self.lib.bmq_retain_keys_by_id(self.eng.h, ptr(ids), n, ptr(keys), self.kcap, ptr(koff)), "bmq_retain_keys_by_id")
        return int(koff[n])

    def match_keys(self, now):
        self.check(self.lib.bmq_retain_keys_match(self.eng.h, ptr(self.tdata), ptr(self.toff), 1, ptr(self.ft), ptr(self.fdata), ptr(self.foff), self.n, ptr(self.lim), now,
                                                  ptr(self.row), ptr(self.ids), self.cap, C.byref(self.need), ptr(self.cnt), ptr(self.koff_b), ptr(self.keys_b), self.kcap,
                                                  C.byref(self.kneed)), "bmq_retain_keys_match")
        return int(self.need.value), int(self.kneed.value)


def leg(c, now, gc_now, reps, kernel_only):
    out = {}
    kept, kbytes = c.match_keys(now)                                       # warm-up: code objects, the scratch buffers, the store if there is none
    if kernel_only:
        for _ in range(reps):
            c.match_keys(now)
        return {"kept_ids": kept, "key_bytes": kbytes, "match_keys_calls": reps + 1}
    ids_b, row_b = c.ids[:kept].copy(), c.row.copy()
    a_ms, lim_ms, keys_ms, b_ms = [], [], [], []
    for r in range(reps + 1):
        (k, t_lim) = clock(lambda: c.limited(now))
        (kb, t_keys) = clock(lambda: c.message_keys(c.ids, k, c.koff_a, c.keys_a))
        (_, t_b) = clock(lambda: c.match_keys(now))
        if r:                                                              # (the first round warms the host path up too)
            a_ms.append(t_lim + t_keys), lim_ms.append(t_lim), keys_ms.append(t_keys), b_ms.append(t_b)
        if k != kept or kb != kbytes or not np.array_equal(c.ids[:kept], ids_b) or not np.array_equal(c.row, row_b):
            raise SystemExit("bmq_retain_keys_match and bmq_retain_match_limited disagree on rows / ids")
        if not np.array_equal(c.koff_a[:kept + 1], c.koff_b[:kept + 1]) or not np.array_equal(c.keys_a[:kbytes], c.keys_b[:kbytes]):
            raise SystemExit("the key bytes of bmq_retain_keys_match differ from bmq_retain_message_keys")
    out["kept_ids"], out["key_bytes"] = kept, kbytes
    out["A_match_limited_then_message_keys"] = dict(spread(a_ms), match_limited=spread(lim_ms), message_keys=spread(keys_ms))
    out["B_match_keys"] = spread(b_ms)
    out["B_minus_match_limited_ms"] = out["B_match_keys"]["median_ms"] - float(np.median(lim_ms))
    out["A_over_B"] = out["A_match_limited_then_message_keys"]["median_ms"] / out["B_match_keys"]["median_ms"]
    out["host_keys_over_device_keys"] = float(np.median(keys_ms)) / max(1e-9, out["B_minus_match_limited_ms"])
    if out["B_match_keys"]["median_ms"] >= out["A_match_limited_then_message_keys"]["median_ms"]:
        raise SystemExit("bmq_retain_keys_match (%.3f ms) does not beat match_limited + message_keys (%.3f ms)" %
                         (out["B_match_keys"]["median_ms"], out["A_match_limited_then_message_keys"]["median_ms"]))
    # the GC recipe's key step on the ids the scan returns
    ids = np.asarray(c.eng.retain_expired(None, gc_now), dtype=np.uint32)
    n = len(ids)
    koff_a, koff_b = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    host_ms, dev_ms = [], []
    for r in range(reps + 1):
        (hb, t_h) = clock(lambda: c.message_keys(ids, n, koff_a, c.keys_a))
        (db, t_d) = clock(lambda: c.keys_by_id(ids, n, koff_b, c.keys_b))
        if r:
            host_ms.append(t_h), dev_ms.append(t_d)
        if hb != db or not np.array_equal(koff_a, koff_b) or not np.array_equal(c.keys_a[:hb], c.keys_b[:db]):
            raise SystemExit("bmq_retain_keys_by_id differs from bmq_retain_message_keys on the expired ids")
    out["gc_recipe"] = {"now_ms": gc_now, "ids": n, "key_bytes": hb, "message_keys": spread(host_ms), "keys_by_id": spread(dev_ms),
                        "host_over_device": float(np.median(host_ms)) / float(np.median(dev_ms)), "host_us_per_key": 1e3 * float(np.median(host_ms)) / max(1, n)}
    return out


def kernel_rows(path, key_bytes_per_call, calls):
    """the k_r_key_* rows of a rocprofv3 *kernel_stats.csv of a --kernel-only run"""
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or ""
            for k in ("k_r_key_len", "k_r_key_write"):
                if k in name:
                    total_ns, n = float(r["TotalDurationNs"]), int(float(r["Calls"]))
                    out[k] = {"calls": n, "total_ns": total_ns, "mean_us": total_ns / max(1, n) / 1e3,
                              "gb_per_s_of_key_bytes": key_bytes_per_call * calls / max(1.0, total_ns)}
    if len(out) != 2:
        raise SystemExit("no k_r_key_len / k_r_key_write rows in %s" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true", help="bmq_retain_keys_match on the clean index only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run with the same --reps: its k_r_key_* rows go into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "retain_keys.json"))
    args = ap.parse_args()
    out = {"probe": "tools/retain_keys_probe.py", "device": "MI355X (gfx950), one GPU, one run",
           "workload": "C4: %d retained topics, %d filters, limit %d; clean and after a %d-op churn batch" % (N_TOPICS, N_FILTERS, LIMIT, N_OPS),
           "timing": "host clock around C-ABI calls that return after a stream synchronise; one warm-up round, then the median / min / max of --reps rounds"}
    eng, w, topics = load_c4()
    filters = w.retain(SEED + 1, N_FILTERS, filters=True)
    now, gc_now = BASE_MS + 95_000, BASE_MS + 30_000 + 40_000
    (size, ms) = clock(eng.retain_keys_prepare)
    (_, ms2) = clock(eng.retain_keys_prepare)
    out["keys_prepare"] = {"first_call_ms": ms, "store_bytes": size, "second_call_ms": ms2}
    c = Calls(eng, w, filters)
    out["clean"] = leg(c, now, gc_now, args.reps, args.kernel_only)
    if args.kernel_only:
        print(json.dumps(out))
        eng.close()
        return
    churn(eng, w, topics)
    info = eng.retain_info()
    out["churned"] = dict(leg(c, now, gc_now, args.reps, False), loaded_removed=int(info.loaded_removed), added_ids=int(info.added_ids))
    eng.close()
    if args.kernel_stats:
        out["key_kernels"] = dict(kernel_rows(args.kernel_stats, out["clean"]["key_bytes"], args.reps + 1),
                                  launches_counted="every bmq_retain_keys_match of the --kernel-only run (clean index): the warm-up and the repeats")
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
