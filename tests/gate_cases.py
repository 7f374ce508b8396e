"""Cases and the reference of the submit-time fan-out gate over a match CSR (bmq_routes_gate_batch / bmq_routes_gate_dev /
bmq_delivery_wait_gated), shared by the CPU tier (tests/test_routes_gate.py, a host-only engine) and the GPU tier
(tests/test_routes_gate_gpu.py).

The reference is DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-231) restated as the loop it is: the three throttled
flags, the else branch, the break.  `routes` is a concurrent hash set there, so the loop is run under several orders of a row's routes:
what it counts, reports and meters must be the same under all of them (the order-freeness the engine's rule rests on); WHICH routes it
sends is then fixed by the engine's own choice, the members of a class with the smallest keys."""
import random

import numpy as np

from tests import caps_cases as K
from tests import util as U
from tests.caps_cases import class_of, group, persistent, transient  # noqa: F401  (the classes and the key makers are the caps')

INT_MAX = 2**31 - 1
LONG_MAX = 2**63 - 1
RANK_MAX = K.RANK_MAX
INLINE, P_COUNT, P_BYTES, NO_P_BANDWIDTH, NO_T_BANDWIDTH, GROUP = 1, 2, 4, 8, 16, 32
DEFAULT = (INT_MAX, 100, LONG_MAX, 3)  # MaxPersistentFanout, MaxGroupFanout, MaxPersistentFanoutBytes, both bandwidths
SHUFFLES = 4


def submit(routes, msg_pack_size, entry, inline_fan_out_threshold):
    """routes: [(id, class)] in iteration order -> (ids sent in that order, flags, (persistent, transient, group) sent, metered bytes or None)"""
    max_p_fanout_count, max_g_fanout_count, max_p_fanout_bytes, bw = entry
    sent, flags, meter = [], 0, None
    if len(routes) == 1:
        rid, cls = routes[0]
        sent.append(rid)
        flags = INLINE  # send(..., true)
        if cls == 1:
            meter = msg_pack_size
    elif len(routes) > 1:
        if len(routes) < inline_fan_out_threshold:
            flags |= INLINE
        has_transient_fanout_bandwidth, has_persistent_fanout_bandwidth = bool(bw & 1), bool(bw & 2)
        is_transient_fanout_throttled = is_persistent_fanout_throttled = is_group_fanout_throttled = False
        persistent_fanout_count = persistent_fanout_bytes = group_fanout_count = 0
        for rid, cls in routes:
            if cls == 1:
                if persistent_fanout_count < max_p_fanout_count and persistent_fanout_bytes < max_p_fanout_bytes:
                    if has_persistent_fanout_bandwidth:
                        persistent_fanout_count += 1
                        persistent_fanout_bytes += msg_pack_size
                        sent.append(rid)
                    elif not is_persistent_fanout_throttled:
                        is_persistent_fanout_throttled = True
                        flags |= NO_P_BANDWIDTH
                elif not is_persistent_fanout_throttled:
                    is_persistent_fanout_throttled = True
                    if persistent_fanout_count >= max_p_fanout_count:
                        flags |= P_COUNT
                    if persistent_fanout_bytes >= max_p_fanout_bytes:
                        flags |= P_BYTES
            elif cls == 0:
                if has_transient_fanout_bandwidth:
                    sent.append(rid)
                elif not is_transient_fanout_throttled:
                    is_transient_fanout_throttled = True
                    flags |= NO_T_BANDWIDTH
            else:
                if group_fanout_count < max_g_fanout_count:
                    group_fanout_count += 1
                    sent.append(rid)
                elif not is_group_fanout_throttled:
                    is_group_fanout_throttled = True
                    flags |= GROUP
            if is_persistent_fanout_throttled and is_transient_fanout_throttled and is_group_fanout_throttled:
                break
        meter = persistent_fanout_bytes
    return sent, flags, meter


def table_of(table):
    return [tuple(table)] if not hasattr(table[0], "__len__") else [tuple(t) for t in table]


def expected(keys_by_id, rows, pack_bytes, table, row_gate=None, inline_threshold=0, dead=()):
    """keys_by_id[i]: the key of route id i (ids outside it, and those in `dead`, have no route)
    -> (rows, flags, kept counts (p, t, g), meter bytes per entry, meter records per entry)"""
    table = table_of(table)
    out_rows, flags, counts, mb, mr = [], [], [], [0] * len(table), [0] * len(table)
    rng = random.Random(7)
    for r, row in enumerate(rows):
        t = int(row_gate[r]) if row_gate is not None else 0
        live = [(i, class_of(keys_by_id[i])) for i in row if i < len(keys_by_id) and i not in dead]
        by_key = sorted(live, key=lambda m: keys_by_id[m[0]])
        orders = [by_key, by_key[::-1], live] + [rng.sample(live, len(live)) for _ in range(SHUFFLES)]
        seen = set()
        for order in orders:
            sent, fl, meter = submit(order, int(pack_bytes[r]), table[t], inline_threshold)
            cls = dict(live)
            seen.add((fl, meter, tuple(sum(1 for i in sent if cls[i] == c) for c in (1, 0, 2))))
        assert len(seen) == 1, "row %d: what submit() counts, reports or meters depends on the order of its routes: %r" % (r, seen)
        fl, meter, kept = seen.pop()
        sent = set(submit(by_key, int(pack_bytes[r]), table[t], inline_threshold)[0])  # in key order the loop sends the smallest keys of a class
        out_rows.append([i for i in row if i in sent])
        flags.append(fl)
        counts.append(kept)
        if meter is not None:
            mb[t] += meter
            mr[t] += 1
    return out_rows, flags, counts, mb, mr


def plain(result):
    """what Engine.routes_gate_batch returns -> (rows, flags, kept counts, meter bytes, meter records, info) in lists and tuples"""
    o_row, o_ids, fl, cc, mb, mr, info = result
    return U.csr_rows(o_row, o_ids), [int(x) for x in fl], [tuple(int(x) for x in c) for c in cc], [int(x) for x in mb], [int(x) for x in mr], info


def batch(eng, rows, pack_bytes, table, row_gate=None, inline_threshold=0, **kw):
    rp, ids = U.csr_of_rows(rows)
    return plain(eng.routes_gate_batch(rp, ids, pack_bytes, table, row_gate, inline_threshold, **kw))


def info_counts(info):
    return (info.n_in, info.n_kept, info.n_rows_single, info.n_rows_gated, info.n_rows_flagged, info.n_rows_ranked, info.n_rows_fallback)


def assert_batch_equals_reference(eng, keys_by_id, rows, pack_bytes, table, row_gate=None, inline_threshold=0, dead=(), got=None):
    want = expected(keys_by_id, rows, pack_bytes, table, row_gate, inline_threshold, dead)
    got = got or batch(eng, rows, pack_bytes, table, row_gate, inline_threshold)
    for k, name in enumerate(("rows", "flags", "kept counts", "meter bytes", "meter records")):
        assert got[k] == want[k], name
    info = got[5]
    live = [sum(1 for i in row if i < len(keys_by_id) and i not in dead) for row in rows]
    assert (info.n_in, info.n_kept) == (sum(len(r) for r in rows), sum(len(r) for r in want[0]))
    assert (info.n_rows_single, info.n_rows_gated) == (sum(1 for n in live if n == 1), sum(1 for n in live if n > 1))
    assert info.n_rows_flagged == sum(1 for f in want[1] if f & ~INLINE)
    ranked = sum(1 for row, c in zip(rows, want[2]) if _some_stay(keys_by_id, row, c, dead))
    assert info.n_rows_ranked + info.n_rows_fallback == ranked
    return got


def _some_stay(keys_by_id, row, kept, dead):
    n = [0, 0, 0]
    for i in row:
        if i < len(keys_by_id) and i not in dead:
            n[(1, 0, 2).index(class_of(keys_by_id[i]))] += 1
    return 0 < kept[0] < n[0] or 0 < kept[2] < n[2]


def random_case(seed, n_rows=40, **kw):
    """the caps' three-tenant keys and rows, with a pack size and a table entry per row -> (keys, rows, row_gate, pack_bytes)"""
    keys, rows, row_gate = K.random_case(seed, n_rows=n_rows, **kw)
    rng = random.Random(seed + 1000)
    return keys, rows, row_gate, [rng.choice([0, 1, 10, 10, 1000, 2**31, 2**32 - 1]) for _ in rows]


TABLES = (
    [(3, 2, 30, 3), (0, 0, 0, 3), (INT_MAX, 4, LONG_MAX, 3)],
    [(1, 1, 1, 3), (10, 100, 25, 1), (5, INT_MAX, 2**33, 2)],
    [(2, 7, 10**12, 0), DEFAULT, (0, 3, LONG_MAX, 2)],
)
