#!/usr/bin/env python3
"""Times the pre-commit half of RetainStoreCoProc.batchRetain for a batch and writes ONE JSON line (default: profiles/retain_plan.json).

The C4 index of bench.py (1 M retained topics, 1 tenant), clean, and after the 100 k-op churn batch of tools/retain_keys_probe.py.  The batch:
100 000 ops -- 45 000 distinct retained topics, 45 000 distinct topics nobody retains, 10 000 repeats of those (10 % duplicates), shuffled;
20 % of the ops clear.  Per state, in one process, alternating:

  A  bmq_retain_plan: codes, actions, winners, ids, the winners' retainMessageKeys and the per-tenant delta from four kernels and a scan;
  B  the composition a caller had before: bmq_retain_match_batch with the topics as filters, then on the host the last-wins grouping
     with a dict, the classification, and the codec's bmq_retain_message_key per winner.  The grouping, the classification and the per-key
     calls of B run in Python here (a dict per batch, numpy, one ctypes call per key): its parts are reported one by one, so that the
     share of the match call -- the only part of B that is native -- can be read off.

The outputs of A and B must be equal.  Times are host-clock times around calls that end in a stream synchronise: one warm-up round, then
the median / min / max of --reps rounds.  The kernels' own times come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/retain_plan_probe.py --kernel-only` (tracing slows the host: no wall time of that run is
reported); --kernel-stats CSV folds the k_rp_* rows of that file into the JSON.  Needs a gfx950 device: there is no fallback.

  python tools/retain_plan_probe.py [--reps 7] [--kernel-only] [--kernel-stats CSV] [--out FILE]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import bifromq_amd as B  # noqa: E402
from bifromq_amd import _lib  # noqa: E402
from bifromq_amd.engine import pack  # noqa: E402
from retain_keys_probe import N_TOPICS, churn, clock, load_c4, ptr, spread  # noqa: E402

N_OPS, N_DISTINCT, NONE = 100_000, 90_000, 0xFFFFFFFF


def make_batch(topics):
    """-> (list of topic bytes, clear flags)"""
    data, off = topics
    raw = data.tobytes()
    rng = np.random.default_rng(0x9A7)
    have = sorted({raw[off[i]:off[i + 1]] for i in rng.choice(N_TOPICS, N_DISTINCT // 2, replace=False)})
    fresh = [b"plan/n%d/x%d" % (j % 977, j) for j in range(N_DISTINCT - len(have))]
    distinct = have + fresh
    ops = distinct + [distinct[i] for i in rng.integers(0, len(distinct), N_OPS - len(distinct))]
    order = rng.permutation(len(ops))
    ops = [ops[i] for i in order]
    return ops, (rng.random(len(ops)) < 0.2).astype(np.uint8)


class Calls:
    """both legs over buffers allocated once"""

    def __init__(self, eng, w, ops, clear):
        self.eng, self.lib, self.ops, self.clear = eng, _lib.lib(), ops, clear
        self.tenant = w.tenants()[0].encode()
        self.tdata, self.toff = w.tenants_packed()
        self.pdata, self.poff = pack(ops)
        n = self.n = len(ops)
        self.ot = np.zeros(n, np.uint32)
        self.code, self.action = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.winner, self.ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.delta = np.zeros(1, np.int32)
        self.koff = np.zeros(n + 1, np.uint64)
        self.kcap = 128 * n
        self.keys = np.zeros(self.kcap, np.uint8)
        self.info = _lib.RetainPlanInfo()
        self.row, self.mids, self.need = np.zeros(n + 1, np.uint32), np.zeros(n + 16, np.uint32), C.c_uint64()
        self.kbuf = C.create_string_buffer(4096)

    def check(self, rc, what):
        if rc != 0:
            raise SystemExit("%s failed: %d %s" % (what, rc, self.lib.bmq_last_error(self.eng.h)))

    def plan(self):
        self.check(self.lib.bmq_retain_plan(self.eng.h, ptr(self.tdata), ptr(self.toff), 1, None, ptr(self.pdata), ptr(self.poff), ptr(self.clear), self.n, ptr(self.code),
                                            ptr(self.action), ptr(self.winner), ptr(self.ids), ptr(self.delta), ptr(self.koff), ptr(self.keys), self.kcap, C.byref(self.info)),
                   "bmq_retain_plan")

    def match(self):
        self.check(self.lib.bmq_retain_match_batch(self.eng.h, ptr(self.tdata), ptr(self.toff), 1, ptr(self.ot), ptr(self.pdata), ptr(self.poff), self.n, ptr(self.row),
                                                   ptr(self.mids), self.n + 16, C.byref(self.need)), "bmq_retain_match_batch")

    def classify(self):
        """the host's share of leg B in front of the keys: last wins per topic, then code / action / id / delta per op"""
        last = {}
        for i, t in enumerate(self.ops):
            last[t] = i
        winner = np.fromiter((last[t] for t in self.ops), dtype=np.uint32, count=self.n)
        row = self.row
        hit = row[1:] > row[:-1]
        ids = np.where(hit, self.mids[np.minimum(row[:-1], self.n + 15)], np.uint32(NONE)).astype(np.uint32)
        wclear = self.clear[winner] != 0
        is_w = winner == np.arange(self.n, dtype=np.uint32)
        action = np.where(wclear, np.where(hit, 3, 0), np.where(hit, 2, 1)).astype(np.uint8)
        action[~is_w] = 4
        return winner, ids, wclear.astype(np.uint8), action, int((action == 1).sum()) - int((action == 3).sum())

    def host_keys(self, action):
        out, off = [], [0]
        t, tl, buf, fn = self.tenant, len(self.tenant), self.kbuf, self.lib.bmq_retain_message_key
        for i in np.nonzero((action >= 1) & (action <= 3))[0].tolist():
            p = self.ops[i]
            out.append((i, buf[:fn(t, tl, p, len(p), buf, 4096)]))
        return out


def leg(c, reps, kernel_only):
    c.plan()                                                               # warm-up: code objects, scratch
    if kernel_only:
        for _ in range(reps):
            c.plan()
        return {"plan_calls": reps + 1, "key_bytes": int(c.info.key_bytes)}
    a_ms, b_ms, m_ms, cl_ms, k_ms = [], [], [], [], []
    for r in range(reps + 1):
        (_, t_a) = clock(c.plan)
        (_, t_m) = clock(c.match)
        ((winner, ids, code, action, delta), t_c) = clock(c.classify)
        (keys, t_k) = clock(lambda: c.host_keys(action))
        if r:
            a_ms.append(t_a), b_ms.append(t_m + t_c + t_k), m_ms.append(t_m), cl_ms.append(t_c), k_ms.append(t_k)
        if not (np.array_equal(winner, c.winner) and np.array_equal(ids, c.ids) and np.array_equal(code, c.code) and np.array_equal(action, c.action) and delta == int(c.delta[0])):
            raise SystemExit("bmq_retain_plan and the host composition disagree on codes / actions / winners / ids / delta")
        raw, koff = c.keys, c.koff
        if sum(len(k) for _, k in keys) != int(koff[c.n]) or any(raw[int(koff[i]):int(koff[i + 1])].tobytes() != k for i, k in keys):
            raise SystemExit("the keys of bmq_retain_plan differ from the codec's")
    i = c.info
    out = {"ops": c.n, "groups": int(i.n_groups), "add": int(i.n_add), "update": int(i.n_update), "remove": int(i.n_remove), "none": int(i.n_none), "key_bytes": int(i.key_bytes),
           "present_share_of_groups": (int(i.n_update) + int(i.n_remove) + int(((c.action == 0) & (c.ids != NONE)).sum())) / max(1, int(i.n_groups)),
           "A_retain_plan": spread(a_ms),
           "B_match_batch_then_host": dict(spread(b_ms), match_batch=spread(m_ms), host_grouping_and_classification=spread(cl_ms), host_codec_per_winner=spread(k_ms)),
           "outputs_equal": True}
    out["B_over_A"] = out["B_match_batch_then_host"]["median_ms"] / out["A_retain_plan"]["median_ms"]
    out["match_batch_alone_over_A"] = float(np.median(m_ms)) / out["A_retain_plan"]["median_ms"]
    return out


def kernel_rows(path):
    """the k_rp_* rows (and the scan's) of a rocprofv3 *kernel_stats.csv of a --kernel-only run"""
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or ""
            for k in ("k_rp_find", "k_rp_group", "k_rp_classify", "k_rp_key_write"):
                if k in name:
                    total_ns, n = float(r["TotalDurationNs"]), int(float(r["Calls"]))
                    out[k] = {"calls": n, "total_ns": total_ns, "mean_us": total_ns / max(1, n) / 1e3}
    if len(out) != 4:
        raise SystemExit("no k_rp_* rows in %s" % path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true", help="bmq_retain_plan on the clean index only (the run to put under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *kernel_stats.csv of a --kernel-only run: its k_rp_* rows go into the JSON")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "retain_plan.json"))
    args = ap.parse_args()
    out = {"probe": "tools/retain_plan_probe.py", "device": "MI355X (gfx950), one GPU, one run",
           "workload": "C4: %d retained topics, 1 tenant; a batch of %d ops: %d distinct topics, half of them retained, 10 %% repeats, 20 %% clears; clean and after a 100 k-op churn batch" %
                       (N_TOPICS, N_OPS, N_DISTINCT),
           "timing": "host clock around calls that end in a stream synchronise; one warm-up round, then the median / min / max of --reps rounds; legs alternate in one process",
           "leg_B_note": "the grouping, the classification and the per-key codec calls of leg B run in Python (dict, numpy, one ctypes call per key); only its match call is native"}
    eng, w, topics = load_c4()
    ops, clear = make_batch(topics)
    c = Calls(eng, w, ops, clear)
    out["clean"] = leg(c, args.reps, args.kernel_only)
    if args.kernel_only:
        print(json.dumps(out))
        eng.close()
        return
    churn(eng, w, topics)
    info = eng.retain_info()
    out["churned"] = dict(leg(c, args.reps, False), loaded_removed=int(info.loaded_removed), added_ids=int(info.added_ids))
    eng.close()
    out["kernels"] = kernel_rows(args.kernel_stats) if args.kernel_stats else "not measured"
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
