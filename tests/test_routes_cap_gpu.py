"""The fan-out caps over a match CSR on the device: the gfx950 kernels of bifromq_amd/csrc/bmq_caps_kernels.h behind bmq_routes_cap_dev /
bmq_routes_cap_batch / bmq_delivery_wait_capped against bmq_routes_cap (one call per row: tests/caps_cases.py) and against a host-only engine
(the same per-item functions under the other executor).  Shapes: the smallest at which the kernels can still go wrong -- classes that end
at, one before and one behind a wave (64), a class of several workgroups, a row of a tile of the grouping's fast path plus one (1025), a class
at the bound of the counting rank (CAPS_RANK_MAX) and one over it, a batch of many rows of which few are ranked."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import caps_cases as K
from tests import delivery_cases as D
from tests import share_ref as R
from tests import util as U
from tests.test_share_resolve import build_case
from tests.test_share_resolve_gpu import Hbm

assert hasattr(B.Engine, "routes_cap_batch") and hasattr(B.Engine, "routes_cap_device") and hasattr(B.Engine, "match_wait_delivery_capped")

pytestmark = pytest.mark.gpu

FREE = (0xFFFFFFFF, 0xFFFFFFFF)


def device_batch(eng, mem, rows, caps, row_caps=None, events_cap=None, slack=8):
    """bmq_routes_cap_dev over plain device buffers: a call with a too-small id buffer first (it reports the count), then one that fits
    -> what tests/caps_cases.py::batch returns"""
    row, ids = U.csr_of_rows(rows)
    table = np.asarray(caps, dtype=np.int32).reshape(-1, 2)
    n, total = len(rows), int(row[-1])
    events_cap = total if events_cap is None else events_cap
    d_row, d_ids = mem.put(row), mem.put(ids)
    d_rc = None if row_caps is None else mem.put(np.asarray(row_caps, dtype=np.uint32))
    d_pf, d_gf = mem.put(np.ascontiguousarray(table[:, 0])), mem.put(np.ascontiguousarray(table[:, 1]))
    a = (d_row, d_ids, n, total, d_rc, d_pf, d_gf, len(table))
    d_orow, d_cc, d_ev = mem.zeros(n + 1), mem.zeros(2 * n), mem.zeros(4 * events_cap + slack)
    want = K.expected(eng, rows, caps, row_caps)
    n_kept = sum(len(r) for r in want[0])
    if n_kept > 1:
        with pytest.raises(B.BmqError) as ex:
            eng.routes_cap_device(*a, d_orow, mem.zeros(1), 1, d_cc, d_ev, events_cap)
        assert ex.value.code == -3 and ex.value.info.n_kept == n_kept
    d_oids = mem.zeros(n_kept + slack)
    n_events, info = eng.routes_cap_device(*a, d_orow, d_oids, n_kept + slack, d_cc, d_ev, events_cap)
    o_row = mem.get(d_orow, n + 1)
    ev = mem.get(d_ev, 4 * min(n_events, events_cap), dtype=np.int32).reshape(-1, 4)
    return K.plain((o_row, mem.get(d_oids, int(o_row[-1])), mem.get(d_cc, 2 * n).reshape(-1, 2), ev, info)), want


def check_all_ways(keys, rows, caps, row_caps=None, prepare=None):
    """device buffers == host buffers == a host-only engine == one bmq_routes_cap per row"""
    eng, host = B.Engine(device=0).rebuild(keys), B.Engine(device=-1).rebuild(keys)
    if prepare:
        prepare(eng), prepare(host)
    mem = Hbm()
    dev, want = device_batch(eng, mem, rows, caps, row_caps)
    K.assert_batch_equals_per_row(eng, rows, caps, row_caps, got=dev)
    staged = K.assert_batch_equals_per_row(eng, rows, caps, row_caps)
    on_host = K.batch(host, rows, caps, row_caps)
    assert dev[:3] == staged[:3] == on_host[:3] == want
    counts = lambda i: (i.n_in, i.n_kept, i.n_rows_classified, i.n_rows_ranked, i.n_rows_fallback, i.n_events)
    assert counts(dev[3]) == counts(staged[3]) == counts(on_host[3])
    mem.free()
    host.close()
    eng.close()
    return dev


def test_gpu_class_sizes_around_a_wave_under_a_three_tenant_table():
    sizes = [1, 63, 64, 65, 200, 513]
    keys, rows = K.sizes_case(sizes)
    for caps, row_caps in (([(0, 1), (62, 64), (199, 512)], [0, 1, 1, 1, 2, 2]), ([(63, 63), (64, 65), (K.INT_MAX, 1)], [0, 0, 1, 1, 2, 0]), ([(1, 0)], None)):
        got = check_all_ways(keys, rows, caps, row_caps)
        assert got[3].n_rows_ranked >= 3 and got[3].n_rows_fallback == 0


def test_gpu_a_row_of_1025_pairs():
    keys, rows = K.sizes_case([500], n_transient=25)
    assert len(rows[0]) == 1025
    got = check_all_ways(keys, rows, (499, 3))
    assert got[1] == [(499, 3)] and len(got[2]) == 1 + 497


def test_gpu_a_class_at_the_bound_of_the_counting_rank_and_one_over():
    keys, rows = K.sizes_case([K.RANK_MAX + 1], n_transient=1)
    drop = next(i for i in rows[0] if K.class_of(keys[i]) == 1)
    at_bound = [i for i in rows[0] if i != drop]
    got = check_all_ways(keys, [rows[0], at_bound, at_bound], [(7, K.INT_MAX), (K.INT_MAX, 9)], [0, 0, 1])
    # row 0: 4097 persistent members over a cap of 7 -> the host; row 1: 4096 -> counted on the device; row 2: 4097 groups over 9 -> the host
    assert (got[3].n_rows_fallback, got[3].n_rows_ranked, got[3].n_rows_classified) == (2, 1, 3)
    assert got[1] == [(7, K.RANK_MAX + 1), (7, K.RANK_MAX + 1), (K.RANK_MAX, 9)]


def test_gpu_many_rows_of_which_three_are_ranked():
    keys = sorted([K.group("big/%d" % j, i) for j in range(3) for i in range(20)] + [K.persistent("p", i) for i in range(40)] + [K.transient("t", i) for i in range(40)])
    big = [[i for i, k in enumerate(keys) if b"big" in k and K.O.parse_route_key(k)[2].endswith("/%d" % j)] for j in range(3)]
    small = [i for i, k in enumerate(keys) if b"big" not in k]
    rows = [sorted(small[(7 * t + k) % len(small)] for k in range(t % 9)) for t in range(1400)]
    rows = [sorted(set(r)) for r in rows]
    for j, t in enumerate((0, 701, 1399)):
        rows[t] = sorted(set(rows[t]) | set(big[j]))
    got = check_all_ways(keys, rows, (10, 4))
    assert got[3].n_rows_ranked == 3 and got[3].n_events == 3 * 16 and 3 < got[3].n_rows_classified < 1400


@pytest.mark.parametrize("seed", [4, 5])
def test_gpu_random_multi_tenant_batches(seed):
    keys, rows, row_caps = K.random_case(seed, n_rows=90)
    check_all_ways(keys, rows, [(3, 2), (0, 0), (K.INT_MAX, 4)], row_caps)


def test_gpu_ids_out_of_key_order_and_dead_ids():
    eng, by_id, row = K.out_of_order_case(lambda: B.Engine(device=0))
    host, _, _ = K.out_of_order_case(lambda: B.Engine(device=-1))
    dead = [row[2], row[-1]]
    for e in (eng, host):
        e.apply([(1, by_id[i]) for i in dead])
    never = len(by_id) + 9
    rows = [row, row + [never], row[:3] + [never]]
    mem = Hbm()
    for caps, row_caps in (([(4, 3), (100, 100)], [0, 0, 1]), ([(1, 1)], None)):
        dev, want = device_batch(eng, mem, rows, caps, row_caps)
        assert dev[:3] == want == K.batch(host, rows, caps, row_caps)[:3] == K.batch(eng, rows, caps, row_caps)[:3]
        kept_p = [i for i in dev[0][0] if K.class_of(by_id[i]) == 1]
        assert kept_p == sorted(sorted((i for i in row if K.class_of(by_id[i]) == 1 and i not in dead), key=lambda i: by_id[i])[:caps[0][0]])
        assert kept_p != [i for i in row if K.class_of(by_id[i]) == 1 and i not in dead][:caps[0][0]]  # not the smallest ids
        assert not set(dev[0][0]) & set(dead)
        if row_caps:  # row 2 under (100, 100) is copied through, its dead id and the id never handed out with it
            assert dev[0][2] == rows[2] and dev[1][2] == FREE
    mem.free()
    host.close()
    eng.close()


def test_gpu_short_event_buffer_and_refused_input():
    keys, rows = K.sizes_case([9, 70])
    eng = B.Engine(device=0).rebuild(keys)
    mem = Hbm()
    for cap in (0, 5, 140):
        dev, want = device_batch(eng, mem, rows, (2, 3), events_cap=cap)
        assert dev[0] == want[0] and dev[2] == want[2][:cap] and dev[3].n_events == len(want[2]) == 7 + 6 + 68 + 67
    row, ids = U.csr_of_rows(rows)
    d = [mem.put(row), mem.put(ids), mem.zeros(len(rows) + 1), mem.zeros(len(ids))]
    for pf, gf, rc in (([-1], [1], [0, 0]), ([1], [1], [0, 1])):
        with pytest.raises(B.BmqError) as ex:
            eng.routes_cap_device(d[0], d[1], len(rows), len(ids), mem.put(np.array(rc, dtype=np.uint32)), mem.put(np.array(pf, dtype=np.int32)),
                                  mem.put(np.array(gf, dtype=np.int32)), 1, d[2], d[3], len(ids), None, None, 0)
        assert ex.value.code == -1
    assert (mem.get(d[2], len(rows) + 1) == 0).all() and (mem.get(d[3], len(ids)) == 0).all()  # refused before anything was written
    mem.free()
    eng.close()


def test_gpu_info_times():
    keys, rows = K.sizes_case([70, 65])
    eng = B.Engine(device=0).rebuild(keys)
    eng.set_kernel_timing(True)
    info = K.batch(eng, rows, (3, 3))[3]
    assert info.ms_classify > 0 and info.ms_rank > 0 and info.ms_write > 0
    eng.set_kernel_timing(False)
    assert K.batch(eng, rows, (3, 3))[3].ms_rank == 0
    eng.close()


def packed(strings):
    data = np.frombuffer(b"".join(strings) + b"\0" * 16, dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint32)
    return data, off


def test_gpu_capped_delivery_wait():
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
    caps = [(2, 1), (1, 2)]  # one entry per tenant of the batch
    c_row, c_ids, _cc, c_ev, c_info = eng.routes_cap_batch(row, ids[:total], caps, tt)
    assert c_info.n_events > 10 and {int(e[0]) for e in c_ev} == {0, 1}  # rows with more groups than gf, and more persistent routes than pf
    ref = D.plan_dict(eng, eng.delivery_plan(c_row, c_ids, so, sh, 21))
    uncapped = D.plan_dict(eng, eng.delivery_plan(row, ids[:total], so, sh, 21))

    def outs(rows_cap=1 << 16, share_cap=1 << 14, group_cap=1 << 10):
        return [np.zeros(rows_cap, dtype=np.uint32) for _ in range(3)] + [np.zeros(share_cap, dtype=np.uint32) for _ in range(2)] + [np.zeros(group_cap + 1, dtype=np.uint32)]

    def cut(o, info):
        return o[0][:info.n_rows], o[1][:info.n_rows], o[2][:info.n_rows], o[3][:info.n_share_rows], o[4][:info.n_share_rows], o[5][:info.n_groups + 1], info
    # a ticket of another format: BMQ_E_STATE, and it stays in flight
    t_ids = eng.match_submit_fmt(*a, eng.FMT_IDS)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_capped(t_ids, caps, so, sh, 21, *outs())
    assert ex.value.code == -7
    assert eng.match_wait(t_ids, row, ids) == total
    # a caps table that is not the batch's tenants: BMQ_E_INVAL, and the ticket stays in flight
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_capped(t, caps + [(1, 1)], so, sh, 21, *outs())
    assert ex.value.code == -1
    o = outs()
    tot, info, ev, cinfo = eng.match_wait_delivery_capped(t, caps, so, sh, 21, *o, events_cap=len(c_ev) + 5)
    got = D.plan_dict(eng, cut(o, info))
    assert tot == total and cinfo.n_in == total and cinfo.n_kept == len(c_ids) < total  # *out_total stays the uncapped id count
    assert got == ref and got != uncapped  # the gap this closes: the plan of the batch, without the routes the reference throttles
    assert ev.tolist() == c_ev.tolist() and cinfo.n_events == c_info.n_events
    assert (cinfo.n_rows_classified, cinfo.n_rows_ranked, cinfo.n_rows_fallback) == (c_info.n_rows_classified, c_info.n_rows_ranked, 0)
    # and the uncapped wait of the same batch still gives the uncapped plan
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    o = outs()
    tot, info = eng.match_wait_delivery(t, so, sh, 21, *o)
    assert D.plan_dict(eng, cut(o, info)) == uncapped
    # too-small plan buffers: NOSPACE with the three counts, the events all the same, the ticket is released
    t = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_capped(t, caps, so, sh, 21, *outs(4, 4, 4), events_cap=len(c_ev))
    assert ex.value.code == -3 and ex.value.events.tolist() == c_ev.tolist()
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_capped(t, caps, so, sh, 21, *outs())
    assert ex.value.code == -7
    eng.close()
