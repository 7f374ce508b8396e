#!/usr/bin/env python3
"""Times the two holds of the engine lock of the non-blocking generation change of the retained-topic index -- bmq_retain_compact_begin and
bmq_retain_compact_swap -- with both builders and writes ONE JSON line (default: profiles/retain_generation.json).

The index is the C4 index of bench.py (--topics retained topics of ONE tenant, with stamps) after one apply of --ops ops (half removals of
loaded topics, half adds of new ones): the shape of the bench's extra.c4.compaction.  Two engines of one process -- bmq_config.retain_builder
= 0 (the host builder: the parent commit's code path, unchanged -- the yardstick) and = 3 (the snapshot stays in executor memory, the executor
builder builds beside the matcher, the swap exchanges pointers) -- alternated round by round; before every round the engine gets the ops (or
the ops that undo them), so that every round starts from the same shape.  One warm-up round per engine (builder 1's pays for the key store of
the bmq_retain_rebuild generation under the lock: reported as first_round), then the median of --reps rounds of

  begin_ms / build_ms / swap_ms / locked_copy_bytes   from bmq_retain_compact_info (host clock around each call's own work; swap_ms up to the
                                                      start of the replay);
  build_ms_without_a_matcher_beside                   build_ms of two more rounds (one per direction of the ops) with no matching beside the build;
  batch_ms_idle / batch_ms_while_building             p50 / p99 of the calling thread's --filters-filter bmq_retain_match_batch while another
                                                      thread runs _build, against the same batches with nothing beside them.

The probe exits with an error if the two engines do not hold the same topics afterwards or if the builder-1 engine fell back.  Times are
host-clock times; nothing here is asserted.  Needs a gfx950 device (--device -1: host-only engines, no matching -- to try the script).

  python tools/retain_generation_probe.py [--topics 1000000] [--ops 100000] [--filters 100000] [--reps 7] [--device 0] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bifromq_amd as B  # noqa: E402
from bifromq_amd.engine import pack  # noqa: E402

SEED = 0xB1F20004
BASE_MS = 1_700_000_000_000


def pct(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"n": int(len(v)), "p50": float(v[len(v) // 2]), "p99": float(v[min(len(v) - 1, int(len(v) * 0.99))])} if len(v) else {"n": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--ops", type=int, default=100_000)
    ap.add_argument("--filters", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "retain_generation.json"))
    args = ap.parse_args()
    w = B.Workload(SEED, 1, 1, 0)
    n = args.topics
    data, off, tt = w.retain(SEED, n, filters=False)
    rng = np.random.default_rng(0xB1F2)
    ts = ((BASE_MS + rng.integers(0, 100_000, n)).astype(np.uint64) << np.uint64(16))
    ex = rng.choice(np.array([30, 60, 3600, 0x7FFFFFFF], dtype=np.uint32), n)
    tenants = w.tenants()
    fdata, foff, ft = w.retain(SEED + 1, args.filters, filters=True)
    rng = np.random.default_rng(99)
    raw = data.tobytes()
    old = sorted({raw[off[i]:off[i + 1]] for i in rng.choice(n, args.ops // 2, replace=False)})
    new = [b"churn/n%d/x%d" % (j % 977, j) for j in range(args.ops - len(old))]

    def batch(removes, adds):
        topics = list(removes) + list(adds)
        codes = np.array([1] * len(removes) + [0] * len(adds), dtype=np.uint8)
        order = rng.permutation(len(topics))
        return pack([topics[i] for i in order]), codes[order]
    fwd, back = batch(old, new), batch(new, old)
    engines = {rb: B.Engine(device=args.device, retain_builder=3 * rb) for rb in (0, 1)}  # (keyed by the builder that serves the three calls)
    for e in engines.values():
        e.retain_rebuild(tenants, tt, packed_topics=(data, off), timestamps=ts, expiry=ex)

    def match(e):
        t0 = time.perf_counter()
        e.retain_match_batch(tenants, ft, packed_filters=(fdata, foff))
        return (time.perf_counter() - t0) * 1e3

    def one_round(e, k, beside=True):
        packed, codes = fwd if k % 2 == 0 else back
        e.retain_apply_batch(tenants, None, None, packed_topics=packed, op_codes=codes)
        before = e.retain_info()
        beside = beside and args.device >= 0
        idle = [match(e) for _ in range(6)][1:] if beside else []
        e.retain_compact_begin()
        fail = []

        def build():
            try:
                e.retain_compact_build()
            except Exception as exc:  # noqa: BLE001
                fail.append(repr(exc))
        th = threading.Thread(target=build)
        th.start()
        during = []
        while th.is_alive():
            if beside:
                during.append(match(e))
            else:
                th.join()
        th.join()
        if fail:
            raise SystemExit("bmq_retain_compact_build failed: " + fail[0])
        carried, replayed = e.retain_compact_swap()
        ci = e.retain_compact_info()
        return {"begin_ms": float(ci.begin_ms), "build_ms": float(ci.build_ms), "swap_ms": float(ci.swap_ms), "locked_copy_bytes": int(ci.locked_copy_bytes),
                "snapshot_bytes": int(ci.snapshot_bytes), "n_items": int(ci.n_items), "builder": int(ci.builder), "fallback": int(ci.fallback), "carried": int(carried),
                "replayed": int(replayed), "idle": idle, "during": during, "loaded_removed_before": int(before.loaded_removed), "added_ids_before": int(before.added_ids)}

    rounds = {0: [], 1: []}
    first = {rb: one_round(engines[rb], 0) for rb in (0, 1)}
    for k in range(1, args.reps + 1):
        for rb in (0, 1):
            rounds[rb].append(one_round(engines[rb], k))
    alone = {rb: [one_round(engines[rb], args.reps + 1 + j, beside=False) for j in range(2)] for rb in (0, 1)}  # (both directions of the ops, no matcher beside the build)
    if any(r["builder"] != 1 or r["fallback"] for r in rounds[1]) or any(r["builder"] != 0 for r in rounds[0]):
        raise SystemExit("a round was not served by the builder it was meant for")
    ids = list(range(0, int(engines[0].retain_info().id_bound), max(1, n // 5000)))
    if engines[0].retain_info().n_topics != engines[1].retain_info().n_topics or engines[0].retain_topics(ids) != engines[1].retain_topics(ids):
        raise SystemExit("the two engines do not hold the same topics under the same ids")
    out = {"what": "bmq_retain_compact_begin / _build / _swap on the C4 index (%d topics, 1 tenant) after one apply of %d ops; median of %d rounds per builder, alternated in one process"
                   % (n, args.ops, args.reps), "device": args.device, "filters_per_batch": args.filters}
    for rb in (0, 1):
        rs = rounds[rb]
        out["builder_%d" % rb] = {f: statistics.median(r[f] for r in rs) for f in ("begin_ms", "build_ms", "swap_ms", "locked_copy_bytes", "snapshot_bytes", "n_items")}
        out["builder_%d" % rb].update({"rounds": {f: [round(r[f], 3) for r in rs] for f in ("begin_ms", "build_ms", "swap_ms")},
                                       "shape_before_a_round": {"loaded_removed": rs[0]["loaded_removed_before"], "added_ids": rs[0]["added_ids_before"]},
                                       "batch_ms_idle": pct([x for r in rs for x in r["idle"]]), "batch_ms_while_building": pct([x for r in rs for x in r["during"]]),
                                       "build_ms_without_a_matcher_beside": [round(r["build_ms"], 3) for r in alone[rb]],
                                       "first_round": {f: first[rb][f] for f in ("begin_ms", "build_ms", "swap_ms", "locked_copy_bytes")}})
    for e in engines.values():
        e.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
