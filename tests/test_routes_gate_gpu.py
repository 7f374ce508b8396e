"""The submit-time fan-out gate over a match CSR on the device: the gfx950 kernels of bifromq_amd/csrc/bmq_gate_kernels.h behind
bmq_routes_gate_dev / bmq_routes_gate_batch / bmq_delivery_wait_gated against the loop of DeliverExecutorGroup.submit restated in
tests/gate_cases.py and against a host-only engine (the same per-item functions under the other executor).  Shapes: the smallest at which
the kernels can still go wrong -- classes that end at, one before and one behind a wave (64), a class of several workgroups, a row of 1025
pairs, a class at the bound of the counting rank (CAPS_RANK_MAX) and one over it, many short rows of nine tenants mixed inside every wave
of the rows pass, and a table with a different entry for every row of a wave."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import caps_cases as K
from tests import delivery_cases as D
from tests import gate_cases as G
from tests import share_ref as R
from tests import util as U
from tests.test_share_resolve import build_case
from tests.test_share_resolve_gpu import Hbm

assert hasattr(B.Engine, "routes_gate_batch") and hasattr(B.Engine, "routes_gate_device") and hasattr(B.Engine, "match_wait_delivery_gated")

pytestmark = pytest.mark.gpu


def device_batch(eng, mem, want, rows, pack_bytes, table, row_gate=None, inline_threshold=0, slack=8):
    """bmq_routes_gate_dev over plain device buffers: a call with a too-small id buffer first (BMQ_E_NOSPACE, it reports the count and leaves
    flags and meters valid), then one that fits -> what tests/gate_cases.py::batch returns"""
    row, ids = U.csr_of_rows(rows)
    pf, gf, pb, bw = B.Engine._gate_table(table)
    n, total, n_gate = len(rows), int(row[-1]), len(pf)
    d_rg = None if row_gate is None else mem.put(np.asarray(row_gate, dtype=np.uint32))
    a = (mem.put(row), mem.put(ids), n, total, mem.put(np.asarray(pack_bytes, dtype=np.uint32)), d_rg, mem.put(pf), mem.put(gf), mem.put(pb), mem.put(bw), n_gate, inline_threshold)
    n_kept = sum(len(r) for r in want[0])

    def outs():
        return mem.zeros(n + 1), mem.zeros(n_kept + slack), mem.zeros(n), mem.zeros(3 * n), mem.put(np.zeros(n_gate, dtype=np.uint64)), mem.zeros(n_gate)

    def read(o, info, with_rows=True):
        o_row = mem.get(o[0], n + 1)
        return G.plain((o_row, mem.get(o[1], int(o_row[-1]) if with_rows else 0), mem.get(o[2], n), mem.get(o[3], 3 * n).reshape(-1, 3),
                        mem.get(o[4], n_gate, dtype=np.uint64), mem.get(o[5], n_gate), info))

    if n_kept > 1:
        o = outs()
        with pytest.raises(B.BmqError) as ex:
            eng.routes_gate_device(*a, o[0], o[1], 1, o[2], o[3], o[4], o[5])
        assert ex.value.code == -3 and ex.value.info.n_kept == n_kept
        short = read(o, ex.value.info, with_rows=False)
        assert short[1:5] == tuple(want[1:5])
    o = outs()
    info = eng.routes_gate_device(*a, o[0], o[1], n_kept + slack, o[2], o[3], o[4], o[5])
    return read(o, info)


def check_all_ways(keys, rows, pack_bytes, table, row_gate=None, inline_threshold=0):
    """device buffers == host buffers == a host-only engine == the reference's loop"""
    eng, host = B.Engine(device=0).rebuild(keys), B.Engine(device=-1).rebuild(keys)
    mem = Hbm()
    want = G.expected(keys, rows, pack_bytes, table, row_gate, inline_threshold)
    dev = device_batch(eng, mem, want, rows, pack_bytes, table, row_gate, inline_threshold)
    G.assert_batch_equals_reference(eng, keys, rows, pack_bytes, table, row_gate, inline_threshold, got=dev)
    staged = G.assert_batch_equals_reference(eng, keys, rows, pack_bytes, table, row_gate, inline_threshold)
    on_host = G.batch(host, rows, pack_bytes, table, row_gate, inline_threshold)
    assert dev[:5] == staged[:5] == on_host[:5] == want
    assert G.info_counts(dev[5]) == G.info_counts(staged[5]) == G.info_counts(on_host[5])
    mem.free()
    host.close()
    eng.close()
    return dev


def test_gpu_class_sizes_around_a_wave_under_a_three_entry_table():
    sizes = [1, 63, 64, 65, 200, 513]
    keys, rows = K.sizes_case(sizes)
    pack = [10, 2**31, 7, 0, 1000, 2**32 - 1]
    for table, row_gate in (([(0, 1, G.LONG_MAX, 3), (62, 64, G.LONG_MAX, 3), (199, 512, G.LONG_MAX, 1)], [0, 1, 1, 1, 2, 2]),
                            ([(63, 63, 64 * 7, 3), (64, 65, 63 * 7 + 1, 3), (G.INT_MAX, 1, 100 * 1000, 2)], [0, 0, 1, 1, 2, 0]),
                            ([(1, 0, 1, 3)], None)):
        got = check_all_ways(keys, rows, pack, table, row_gate, inline_threshold=130)
        assert got[5].n_rows_ranked >= 3 and got[5].n_rows_fallback == 0 and got[5].n_rows_flagged >= 4
    assert max(got[3]) > 2**32  # (1 route kept in each of six rows, two of them with packs of 2^31 bytes and more)


def test_gpu_a_row_of_1025_pairs():
    keys, rows = K.sizes_case([500], n_transient=25)
    assert len(rows[0]) == 1025
    got = check_all_ways(keys, rows, [3], (499, 3, 3 * 499, 3))
    assert got[2] == [(499, 25, 3)] and got[1] == [G.P_COUNT | G.P_BYTES | G.GROUP] and got[3] == [3 * 499]


def test_gpu_a_class_at_the_bound_of_the_counting_rank_and_one_over():
    keys, rows = K.sizes_case([K.RANK_MAX + 1], n_transient=1)
    drop = next(i for i in rows[0] if K.class_of(keys[i]) == 1)
    at_bound = [i for i in rows[0] if i != drop]
    got = check_all_ways(keys, [rows[0], at_bound, at_bound], [1, 1, 1], [(7, G.INT_MAX, G.LONG_MAX, 3), (G.INT_MAX, 9, G.LONG_MAX, 3)], [0, 0, 1])
    # row 0: 4097 persistent members, 7 stay -> the host; row 1: 4096 -> counted on the device; row 2: 4097 groups, 9 stay -> the host
    assert (got[5].n_rows_fallback, got[5].n_rows_ranked) == (2, 1)
    assert got[2] == [(7, 1, K.RANK_MAX + 1), (7, 1, K.RANK_MAX + 1), (K.RANK_MAX, 1, 9)]


def test_gpu_1400_short_rows_of_nine_tenants_of_which_three_are_ranked():
    keys = sorted([K.group("big/%d" % j, i) for j in range(3) for i in range(20)] + [K.persistent("p", i) for i in range(40)] + [K.transient("t", i) for i in range(40)])
    big = [[i for i, k in enumerate(keys) if b"big" in k and K.O.parse_route_key(k)[2].endswith("/%d" % j)] for j in range(3)]
    small = [i for i, k in enumerate(keys) if b"big" not in k]
    rows = [sorted(set(small[(7 * t + k) % len(small)] for k in range(t % 9))) for t in range(1400)]
    for j, t in enumerate((0, 701, 1399)):
        rows[t] = sorted(set(rows[t]) | set(big[j]))
    row_gate = [(5 * t + t // 64) % 9 for t in range(1400)]  # every wave of the rows pass holds all nine entries, in no order
    pack = [(1 + t % 5) * 2**29 for t in range(1400)]
    table = [(10, 4, G.LONG_MAX, 3)] * 3 + [(2, 4, 2**31, 3)] * 3 + [(10, 4, G.LONG_MAX, 1), (10, 4, G.LONG_MAX, 2), (0, 4, 0, 0)]
    got = check_all_ways(keys, rows, pack, table, row_gate, inline_threshold=4)
    assert got[5].n_rows_fallback == 0 and got[5].n_rows_ranked >= 3 and got[5].n_rows_single > 100 and min(got[4][:6]) > 100 and max(got[3]) > 2**36


def test_gpu_a_different_table_entry_for_every_row_of_a_wave():
    keys, rows0 = K.sizes_case([3], n_transient=2)
    n = 150
    rows = [rows0[0][r % 3:] for r in range(n)]
    row_gate = [(37 * r) % n for r in range(n)]  # 150 entries, a permutation: the 64 rows of a wave name 64 entries
    table = [(t % 4, t % 3, (t % 5) * 10, t % 4) for t in range(n)]
    got = check_all_ways(keys, rows, [10 + r for r in range(n)], table, row_gate, inline_threshold=8)
    assert sum(got[4]) == n and max(got[4]) == 1


@pytest.mark.parametrize("seed", [4, 5])
def test_gpu_random_three_tenant_batches(seed):
    keys, rows, row_gate, pack = G.random_case(seed, n_rows=90)
    check_all_ways(keys, rows, pack, G.TABLES[seed % 3], row_gate, inline_threshold=6)


def test_gpu_ids_out_of_key_order_dead_ids_and_refused_input():
    eng, by_id, row = K.out_of_order_case(lambda: B.Engine(device=0))
    host, _, _ = K.out_of_order_case(lambda: B.Engine(device=-1))
    dead = [row[2], row[-1]]
    for e in (eng, host):
        e.apply([(1, by_id[i]) for i in dead])
    never = len(by_id) + 9
    rows = [row, row + [never], row[:1] + [row[2], never]]  # the last row: one live route beside a dead id and an id never handed out
    mem = Hbm()
    for table, row_gate in (([(4, 3, G.LONG_MAX, 3), (0, 0, 0, 0)], [0, 0, 1]), ([(1, 1, 5, 3)], None)):
        want = G.expected(by_id, rows, [5, 6, 7], table, row_gate, 0, set(dead))
        dev = device_batch(eng, mem, want, rows, [5, 6, 7], table, row_gate)
        assert dev[:5] == want == G.batch(host, rows, [5, 6, 7], table, row_gate)[:5] == G.batch(eng, rows, [5, 6, 7], table, row_gate)[:5]
        kept_p = [i for i in dev[0][0] if K.class_of(by_id[i]) == 1]
        live_p = [i for i in row if K.class_of(by_id[i]) == 1 and i not in dead]
        assert kept_p == sorted(sorted(live_p, key=lambda i: by_id[i])[:table[0][0]]) and kept_p != live_p[:table[0][0]]  # not the smallest ids
        assert not set(dev[0][0]) & set(dead) and dev[0][2] == row[:1] and dev[1][2] == G.INLINE
    # refused: a negative limit, a bandwidth above 3, an index outside the table -- nothing is written
    row_a, ids_a = U.csr_of_rows(rows)
    d = [mem.put(row_a), mem.put(ids_a), mem.put(np.array([5, 6, 7], dtype=np.uint32)), mem.zeros(4), mem.zeros(len(ids_a)), mem.zeros(3), mem.zeros(9),
         mem.put(np.zeros(1, dtype=np.uint64)), mem.zeros(1)]
    for pf, gf, pb, bw, rg in (([-1], [1], [1], [3], [0, 0, 0]), ([1], [1], [-1], [3], [0, 0, 0]), ([1], [1], [1], [4], [0, 0, 0]), ([0], [0], [0], [0], [0, 1, 0])):
        with pytest.raises(B.BmqError) as ex:
            eng.routes_gate_device(d[0], d[1], 3, len(ids_a), d[2], mem.put(np.array(rg, dtype=np.uint32)), mem.put(np.array(pf, dtype=np.int32)),
                                   mem.put(np.array(gf, dtype=np.int32)), mem.put(np.array(pb, dtype=np.int64)), mem.put(np.array(bw, dtype=np.uint8)), 1, 0,
                                   d[3], d[4], len(ids_a), d[5], d[6], d[7], d[8])
        assert ex.value.code == -1
    assert all((mem.get(p, k) == 0).all() for p, k in ((d[3], 4), (d[4], len(ids_a)), (d[5], 3), (d[6], 9), (d[7], 2), (d[8], 1)))
    mem.free()
    host.close()
    eng.close()


def test_gpu_info_times():
    keys, rows = K.sizes_case([70, 65])
    eng = B.Engine(device=0).rebuild(keys)
    eng.set_kernel_timing(True)
    info = G.batch(eng, rows, [1, 1], (3, 3, G.LONG_MAX, 3))[5]
    assert info.ms_classify > 0 and info.ms_rank > 0 and info.ms_write > 0
    eng.set_kernel_timing(False)
    info = G.batch(eng, rows, [1, 1], (3, 3, G.LONG_MAX, 3))[5]
    assert (info.ms_classify, info.ms_rank, info.ms_write) == (0, 0, 0)
    eng.close()


def packed(strings):
    data = np.frombuffer(b"".join(strings) + b"\0" * 16, dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint32)
    return data, off


def test_gpu_gated_delivery_wait():
    from tests.test_fanout import _workload
    tenants, keys0, topics, tt = _workload(31, shared=0.4, brokers=(0, 1), dkeys=5)
    eng, keys, flags, tables, rows, senders = build_case(31, device=0, shared=0.4, counts=[1, 2, 5, 63, 65, 200], brokers=(0, 1), dkeys=5)
    assert keys == keys0
    tdata, toff = packed([t.encode() for t in tenants])
    pdata, poff = packed([t.encode() for t in topics])
    n = len(topics)
    so, sh = R.sender_arrays(senders)
    a = (tdata, toff, len(tenants), tt, pdata, poff, n)
    row, ids = np.zeros(n + 1, dtype=np.uint32), np.zeros(1 << 16, dtype=np.uint32)
    total = eng.match_wait(eng.match_submit_fmt(*a, eng.FMT_IDS), row, ids)
    pack = np.array([100 + 13 * (i % 7) for i in range(n)], dtype=np.uint32)
    table = [(6, 3, 250, 3), (4, 2, G.LONG_MAX, 2)]  # one entry per tenant of the batch: the bytes limit binds in one, the other has no transient bandwidth
    caps = [(t[0], t[1]) for t in table]
    thr = 5
    # the composed path, through host arrays: caps, then the gate, then the plan
    c_row, c_ids, _cc, c_ev, c_info = eng.routes_cap_batch(row, ids[:total], caps, tt)
    g_row, g_ids, g_fl, g_cc, g_mb, g_mr, g_info = eng.routes_gate_batch(c_row, c_ids, pack, table, tt, thr)
    assert g_info.n_kept < c_info.n_kept < total and g_info.n_rows_flagged > 5 and g_info.n_rows_ranked > 0
    assert {G.P_BYTES, G.NO_T_BANDWIDTH} <= {b for f in g_fl for b in (1, 2, 4, 8, 16, 32) if f & b} and g_mb.min() > 0
    ref = D.plan_dict(eng, eng.delivery_plan(g_row, g_ids, so, sh, 21))
    capped = D.plan_dict(eng, eng.delivery_plan(c_row, c_ids, so, sh, 21))

    def outs(rows_cap=1 << 16, share_cap=1 << 14, group_cap=1 << 10):
        return [np.zeros(rows_cap, dtype=np.uint32) for _ in range(3)] + [np.zeros(share_cap, dtype=np.uint32) for _ in range(2)] + [np.zeros(group_cap + 1, dtype=np.uint32)]

    def cut(o, info):
        return o[0][:info.n_rows], o[1][:info.n_rows], o[2][:info.n_rows], o[3][:info.n_share_rows], o[4][:info.n_share_rows], o[5][:info.n_groups + 1], info
    # a ticket of another format: BMQ_E_STATE, and it stays in flight
    t_ids = eng.match_submit_fmt(*a, eng.FMT_IDS)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_gated(t_ids, table, pack, thr, so, sh, 21, *outs())
    assert ex.value.code == -7
    assert eng.match_wait(t_ids, row, ids) == total
    # a table that is not the batch's tenants, or an undefined bandwidth bit: BMQ_E_INVAL, and the ticket stays in flight
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    for bad in (table + [G.DEFAULT], [table[0], (4, 2, 1, 4)]):
        with pytest.raises(B.BmqError) as ex:
            eng.match_wait_delivery_gated(t, bad, pack, thr, so, sh, 21, *outs())
        assert ex.value.code == -1
    o = outs()
    tot, info, ev, cinfo, fl, mb, mr, ginfo = eng.match_wait_delivery_gated(t, table, pack, thr, so, sh, 21, *o, events_cap=len(c_ev) + 5)
    got = D.plan_dict(eng, cut(o, info))
    assert tot == total and cinfo.n_in == total and cinfo.n_kept == len(c_ids) == ginfo.n_in and ginfo.n_kept == len(g_ids)
    assert got == ref and got != capped  # the gap this closes: the plan without the routes submit() would have throttled
    assert ev.tolist() == c_ev.tolist() and cinfo.n_events == c_info.n_events
    assert fl.tolist() == g_fl.tolist() and mb.tolist() == g_mb.tolist() and mr.tolist() == g_mr.tolist()
    assert G.info_counts(ginfo) == G.info_counts(g_info) and ginfo.n_rows_fallback == 0
    # and the capped wait of the same batch still gives the capped plan
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    o = outs()
    tot, info, _ev, _ci = eng.match_wait_delivery_capped(t, caps, so, sh, 21, *o)
    assert D.plan_dict(eng, cut(o, info)) == capped
    # too-small plan buffers: NOSPACE with the counts; events, flags and meters all the same; the ticket is released
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_gated(t, table, pack, thr, so, sh, 21, *outs(4, 4, 4), events_cap=len(c_ev))
    assert ex.value.code == -3 and ex.value.events.tolist() == c_ev.tolist()
    assert ex.value.flags.tolist() == g_fl.tolist() and ex.value.meter_bytes.tolist() == g_mb.tolist() and ex.value.meter_records.tolist() == g_mr.tolist()
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_gated(t, table, pack, thr, so, sh, 21, *outs())
    assert ex.value.code == -7
    # a stage that cannot bind is a stage that is skipped: three tickets of the batch, waited for plainly, capped and gated
    tickets = [eng.match_submit_fmt(*a, eng.FMT_DELIVERY) for _ in range(3)]
    o = outs()
    tot, info = eng.match_wait_delivery(tickets[0], so, sh, 21, *o)
    plain = D.plan_dict(eng, cut(o, info))
    assert tot == total
    o = outs()
    tot, info, ev, cinfo = eng.match_wait_delivery_capped(tickets[1], [(G.INT_MAX, G.INT_MAX)] * len(tenants), so, sh, 21, *o)
    assert D.plan_dict(eng, cut(o, info)) == plain and tot == total
    assert cinfo.n_kept == total and cinfo.n_events == 0 and len(ev) == 0
    o = outs()
    tot, info, ev, cinfo, fl, mb, mr, ginfo = eng.match_wait_delivery_gated(tickets[2], [(G.INT_MAX, G.INT_MAX, G.LONG_MAX, 3)] * len(tenants), pack, 0, so, sh, 21, *o)
    assert D.plan_dict(eng, cut(o, info)) == plain and tot == total
    assert cinfo.n_kept == total and ginfo.n_kept == total and cinfo.n_events == 0 and len(ev) == 0
    assert fl.tolist() == [G.INLINE if row[i + 1] - row[i] == 1 else 0 for i in range(n)]
    eng.close()
