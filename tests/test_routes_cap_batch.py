"""The fan-out caps of MatchedRoutes over a whole match CSR (bmq_routes_cap_batch) on a host-only engine: the per-item functions of
bifromq_amd/csrc/bmq_caps_core.h under HostExec.  The contract is bit-agreement with the function the engine had before -- one
bmq_routes_cap call per row under that row's caps (tests/caps_cases.py: expected) -- and, through it, with the restated MatchedRoutes of the
oracle.  A host-only engine cannot match, so the rows are made by hand (ascending ids, as a match returns them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from oracle import oracle as O
from tests import caps_cases as K
from tests import util as U

assert hasattr(B.Engine, "routes_cap_batch") and hasattr(B.Engine, "routes_cap_device") and hasattr(B.Engine, "match_wait_delivery_capped")

FREE = (0xFFFFFFFF, 0xFFFFFFFF)


def host_engine():
    return B.Engine(device=-1)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_multi_tenant_batches_equal_the_per_row_function(seed):
    keys, rows, row_caps = K.random_case(seed)
    eng = host_engine().rebuild(keys)
    for caps in ([(3, 2), (0, 0), (K.INT_MAX, 4)], [(1, 1), (10, 100), (5, K.INT_MAX)], [(2, 7), (K.INT_MAX, K.INT_MAX), (0, 3)]):
        got = K.assert_batch_equals_per_row(eng, rows, caps, row_caps)
        assert got[3].n_rows_ranked > 0 and got[3].n_rows_fallback == 0
    # no row_caps: every row under entry 0
    K.assert_batch_equals_per_row(eng, rows, [(3, 2), (0, 0)])
    K.assert_batch_equals_per_row(eng, rows, (4, 1))
    eng.close()


def test_the_digit_prefix_rule_is_the_old_one():
    keys = sorted(K.odd_receivers("a") + [K.transient("a", 1), K.group("a", 1)])
    eng = host_engine().rebuild(keys)
    row = list(range(len(keys)))
    rows, counts, ev, info = K.assert_batch_equals_per_row(eng, [row], (0, 0))
    assert sorted(rows[0]) == [i for i, k in enumerate(keys) if K.class_of(k) == 0] and len(rows[0]) == 5  # "", "11", "2", "x1" and the plain transient
    assert sorted(e[2] for e in ev if e[0] == 0) == [i for i, k in enumerate(keys) if K.class_of(k) == 1] and len(ev) == 3
    eng.close()


def _oracle_rows(keys, tenant, topics):
    rows = []
    for topic in topics:
        row = []
        for i, k in enumerate(keys):
            flag, kt, flt, _r = O.parse_route_key(k)
            plain = flt if flag == 1 else flt.split("/", 2)[2]
            if kt == tenant and O.semantic_match(topic, plain):
                row.append(i)
        rows.append(row)
    return rows


def _assert_equals_matched_routes(eng, keys, tenant, topics, rows, caps, got):
    for r, topic in enumerate(topics):
        want = O.matched_routes_load(tenant, topic, keys, *caps)
        assert {keys[i] for i in got[0][r]} == want.routes() and got[0][r] == sorted(got[0][r])
        # the oracle reports in key order with the types interleaved; per type that is the batch call's order
        mine = [(typ, keys[rid], mx) for typ, rr, rid, mx in got[2] if rr == r]
        assert mine == [e for e in want.events if e[0] == 0] + [e for e in want.events if e[0] == 1]
        if got[1][r] != FREE:
            assert got[1][r] == (want.persistent, len(want.groups))


def test_hand_made_topics_equal_the_restated_matched_routes():
    tenant = "tenantA"
    n = lambda tf, b, r, d: B.route_key_from_mqtt(tenant, tf, O.receiver_url(b, r, d))
    keys = [n("alarms/+/critical", 1, "receiverA", "delivererA"), n("alarms/+/critical", 1, "receiverB", "delivererB"),  # TenantRouteMatcherTest.java:272-303
            B.route_key_from_mqtt(tenant, "$share/groupA/jobs/+/progress"), B.route_key_from_mqtt(tenant, "$share/groupB/jobs/+/progress")]  # :305-342
    keys += [n("alarms/+/critical", 1, "recv%02d" % i, "d%d" % i) for i in range(10)] + [B.route_key_from_mqtt(tenant, "$share/g%02d/alarms/#" % i) for i in range(12)]
    keys += [n("alarms/#", 0, "transient%d" % i, "d") for i in range(5)] + [B.route_key_from_mqtt(tenant, "$oshare/o%d/+/+/critical" % i) for i in range(3)]
    keys = sorted(set(keys))
    topics = ["alarms/device1/critical", "jobs/job1/progress", "alarms/x", "nobody/home"]
    rows = _oracle_rows(keys, tenant, topics)
    assert [len(r) for r in rows] == [32, 2, 17, 0]
    eng = host_engine().rebuild(keys)
    for caps in ((1, 10), (10, 1), (3, 2), (1, 1), (0, 0), (15, 100), (100, 4), (100, 100)):
        got = K.assert_batch_equals_per_row(eng, rows, caps)
        _assert_equals_matched_routes(eng, keys, tenant, topics, rows, caps, got)
    # the reference's own two throttle cases: the second persistent route is turned away; of the two groups the one whose KEY is smaller stays
    got = K.batch(eng, rows, (1, 1))
    jobs = [keys[i] for i in got[0][1]]
    assert jobs == [min(k for k in keys if b"jobs" in k)] and [e[:2] + e[3:] for e in got[2] if e[1] == 1] == [(1, 1, 1)]
    eng.close()


def test_survivors_are_the_smallest_keys_not_the_smallest_ids():
    eng, by_id, row = K.out_of_order_case(host_engine)
    for caps in ((4, 3), (1, 1), (7, 100), (100, 6)):
        rows, counts, ev, info = K.assert_batch_equals_per_row(eng, [row], caps)
        for cls, cap in ((1, caps[0]), (2, caps[1])):
            members = [i for i in row if K.class_of(by_id[i]) == cls]
            by_key, by_small_id = sorted(members, key=lambda i: by_id[i])[:cap], members[:cap]
            kept = [i for i in rows[0] if K.class_of(by_id[i]) == cls]
            assert kept == sorted(by_key)
            if cap < len(members):
                assert sorted(by_key) != by_small_id  # the two orders differ here: keeping the smallest ids would be wrong
                assert [e[2] for e in ev if e[0] == cls - 1] == sorted(members, key=lambda i: by_id[i])[cap:]
        assert rows[0] == sorted(rows[0])
    eng.close()


def test_dead_ids_stay_in_free_rows_and_leave_classified_ones():
    keys, rows = K.sizes_case([6, 6])
    eng = host_engine().rebuild(keys)
    dead = [rows[0][1], rows[0][4], rows[1][0], rows[1][7]]
    eng.apply([(1, keys[i]) for i in dead])
    never = int(eng.info().next_route_id) + 5  # an id the index never handed out
    rows = [rows[0] + [never], rows[1] + [never, never + 1]]
    caps, row_caps = [(3, 2), (100, 100)], [0, 1]
    got = K.assert_batch_equals_per_row(eng, rows, caps, row_caps)
    assert not set(got[0][0]) & (set(dead) | {never}) and got[1][0] == (3, 2)
    assert got[0][1] == rows[1] and got[1][1] == FREE  # no longer than its caps: copied through, dead ids and all
    eng.close()


@pytest.mark.parametrize("m", [1, 5, 64])
def test_caps_around_the_class_size(m):
    keys, rows = K.sizes_case([m])
    eng = host_engine().rebuild(keys)
    for cap in sorted({0, 1, max(m - 1, 0), m, m + 1, K.INT_MAX}):
        for caps in ((cap, K.INT_MAX), (K.INT_MAX, cap), (cap, cap)):
            got = K.assert_batch_equals_per_row(eng, rows, caps)
            if got[1][0] != FREE:
                assert got[1][0] == (min(m, caps[0]), min(m, caps[1]))
            assert len(got[2]) == (max(m - caps[0], 0) + max(m - caps[1], 0) if got[1][0] != FREE else 0)
    eng.close()


def test_empty_rows_empty_batches_and_refused_input():
    keys, rows = K.sizes_case([4, 3])
    eng = host_engine().rebuild(keys)
    K.assert_batch_equals_per_row(eng, [[], rows[0], [], [], rows[1], []], [(1, 1), (0, 2)], [0, 0, 1, 1, 1, 0])
    got = K.batch(eng, [], (1, 1))
    assert got[0] == [] and got[2] == [] and (got[3].n_in, got[3].n_kept) == (0, 0)
    got = K.batch(eng, [[], []], (0, 0))
    assert got[0] == [[], []] and got[1] == [FREE, FREE]
    for caps, row_caps in (([(1, 1)], [0, 1]), ([(1, 1), (2, 2)], [2, 0]), ([(-1, 1)], None), ([(1, 1), (3, -5)], [0, 0])):
        with pytest.raises(B.BmqError) as ex:
            K.batch(eng, rows, caps, row_caps)
        assert ex.value.code == -1  # BMQ_E_INVAL
    with pytest.raises(B.BmqError) as ex:  # an empty table names no row
        eng.routes_cap_batch(*U.csr_of_rows(rows), np.zeros((0, 2), dtype=np.int32))
    assert ex.value.code == -1
    # out_cap below the survivors: BMQ_E_NOSPACE, the count is in the info
    want = K.expected(eng, rows, [(1, 1)])
    with pytest.raises(B.BmqError) as ex:
        K.batch(eng, rows, (1, 1), out_cap=2)
    assert ex.value.code == -3 and ex.value.info.n_kept == sum(len(r) for r in want[0]) > 2 and ex.value.n_events == len(want[2])
    eng.close()


def test_events_cap_smaller_than_the_event_count():
    keys, rows = K.sizes_case([9, 7])
    eng = host_engine().rebuild(keys)
    want = K.expected(eng, rows, [(2, 3)])
    assert len(want[2]) == 7 + 6 + 5 + 4
    for cap in (0, 1, 8, 21, 22, 23):
        got = K.batch(eng, rows, (2, 3), events_cap=cap)
        assert got[0] == want[0] and got[2] == want[2][:cap] and got[3].n_events == len(want[2])
    eng.close()


def test_a_class_of_more_than_rank_max_members_is_sorted_on_the_host():
    keys, rows = K.sizes_case([K.RANK_MAX + 1, 20], n_transient=1)
    eng = host_engine().rebuild(keys)
    late = [K.persistent("f/0", 10 ** 5 - 1 - i) for i in range(3)]  # ids out of key order in the large row too
    eng.apply([(0, k) for k in late])
    first = len(keys)
    rows[0] = rows[0] + [first, first + 1, first + 2]
    got = K.assert_batch_equals_per_row(eng, rows, [(7, K.INT_MAX), (5, 5)], [0, 1])
    assert (got[3].n_rows_fallback, got[3].n_rows_ranked, got[3].n_rows_classified) == (1, 1, 2)
    # the same row with its large class exactly at the bound is ranked by counting
    drop = next(i for i in rows[0] if K.class_of(keys[i]) == 1)
    at_bound = [i for i in rows[0][:-3] if i != drop]
    assert len([i for i in at_bound if K.class_of(keys[i]) == 1]) == K.RANK_MAX
    got = K.assert_batch_equals_per_row(eng, [at_bound], (7, K.INT_MAX))
    assert (got[3].n_rows_fallback, got[3].n_rows_ranked) == (0, 1)
    eng.close()


def test_the_device_form_needs_a_device():
    eng = host_engine().rebuild([K.persistent("a", 1)])
    out = np.full(8, 7, dtype=np.uint32)
    with pytest.raises(B.BmqError) as ex:
        eng.routes_cap_device(out.ctypes.data, out.ctypes.data, 1, 1, None, out.ctypes.data, out.ctypes.data, 1, out.ctypes.data, out.ctypes.data, 8, None, None, 0)
    assert ex.value.code == -2
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_capped(0, [(1, 1)], [0, 0], [], 1, *[np.full(4, 7, dtype=np.uint32) for _ in range(6)])
    assert ex.value.code == -2 and (out == 7).all()
    eng.close()


def test_caps_info_mirror_has_the_layout_of_the_header(tmp_path):
    """_lib.CapsInfo restates bmq_caps_info: same size, every field at the same offset"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_caps_info));']
    lines += ['printf("%s %%zu\\n", offsetof(bmq_caps_info, %s));' % (f, f) for f, _ in _lib.CapsInfo._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.CapsInfo)
    for f, _ in _lib.CapsInfo._fields_:
        assert int(got[f]) == getattr(_lib.CapsInfo, f).offset, f
    assert {"n_in", "n_kept", "n_rows_classified", "n_rows_ranked", "n_rows_fallback", "n_events", "generation", "ms_classify", "ms_rank",
            "ms_write"} == {f for f, _ in _lib.CapsInfo._fields_}
    assert {"bmq_routes_cap_batch", "bmq_routes_cap_dev", "bmq_delivery_wait_capped"} <= set(_lib.ABI_SYMBOLS)
