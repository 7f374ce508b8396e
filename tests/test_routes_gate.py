"""The submit-time fan-out gate of DeliverExecutorGroup.submit over a whole match CSR (bmq_routes_gate_batch) on a host-only engine: the
per-item functions of bifromq_amd/csrc/bmq_gate_core.h under HostExec, against the loop of the reference restated in tests/gate_cases.py.
A host-only engine cannot match, so the rows are made by hand (ascending ids, as a match returns them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bifromq_amd as B

assert hasattr(B.Engine, "routes_gate_batch")

from bifromq_amd import _lib  # noqa: E402
from tests import caps_cases as K  # noqa: E402
from tests import gate_cases as G  # noqa: E402
from tests import util as U  # noqa: E402


def host_engine():
    return B.Engine(device=-1)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_three_tenant_batches_equal_the_reference(seed):
    keys, rows, row_gate, pack = G.random_case(seed)
    eng = host_engine().rebuild(keys)
    for table, thr in zip(G.TABLES, (0, 6, 1000)):
        got = G.assert_batch_equals_reference(eng, keys, rows, pack, table, row_gate, thr)
        assert got[5].n_rows_ranked > 0 and got[5].n_rows_fallback == 0 and got[5].n_rows_flagged > 0
    # no row_gate: every row under entry 0
    G.assert_batch_equals_reference(eng, keys, rows, pack, G.TABLES[0][:2])
    G.assert_batch_equals_reference(eng, keys, rows, pack, (4, 1, 2**31, 3), inline_threshold=3)
    # under the default table nothing but the group limit of 100 can bind, and no row here has 100 groups
    got = G.assert_batch_equals_reference(eng, keys, rows, pack, G.DEFAULT)
    assert got[0] == rows and got[5].n_rows_flagged == 0
    eng.close()


def test_survivors_are_the_smallest_keys_not_the_smallest_ids():
    eng, by_id, row = K.out_of_order_case(host_engine)
    for table in ((4, 3, G.LONG_MAX, 3), (1, 1, G.LONG_MAX, 3), (7, 100, 40, 3), (100, 6, G.LONG_MAX, 3)):
        rows, flags, counts, mb, mr, info = G.assert_batch_equals_reference(eng, by_id, [row], [10], table)
        for cls, slot in ((1, 0), (2, 2)):
            members = [i for i in row if K.class_of(by_id[i]) == cls]
            kept = [i for i in rows[0] if K.class_of(by_id[i]) == cls]
            n = counts[0][slot]
            assert kept == sorted(sorted(members, key=lambda i: by_id[i])[:n])
            if n < len(members):
                assert kept != members[:n]  # the two orders differ here: keeping the smallest ids would be wrong
        assert rows[0] == sorted(rows[0]) and mb == [10 * counts[0][0]] and mr == [1]
    eng.close()


def test_dead_ids_bring_a_row_down_to_one_route_and_the_bypass_applies():
    keys, rows = K.sizes_case([2], n_transient=1)  # one row: 2 persistent, 2 groups, 1 transient
    eng = host_engine().rebuild(keys)
    by_cls = {c: [i for i in rows[0] if K.class_of(keys[i]) == c] for c in (0, 1, 2)}
    dead = by_cls[1][1:] + by_cls[2] + by_cls[0]  # one persistent route is left
    eng.apply([(1, keys[i]) for i in dead])
    never = int(eng.info().next_route_id) + 5  # an id the index never handed out
    row = rows[0] + [never]
    closed = (0, 0, 0, 0)  # no limit admits anything, no bandwidth: the single live route is sent all the same
    got = G.assert_batch_equals_reference(eng, keys, [row, [never], []], [77, 5, 5], closed, dead=set(dead))
    assert got[0] == [[by_cls[1][0]], [], []] and got[1] == [G.INLINE, 0, 0] and got[2][0] == (1, 0, 0)
    assert got[3] == [77] and got[4] == [1] and G.info_counts(got[5])[2:5] == (1, 0, 0)
    eng.close()
    # the same row alive: nothing is sent, and the events say why
    eng = host_engine().rebuild(keys)
    got = G.assert_batch_equals_reference(eng, keys, [rows[0]], [77], closed)
    assert got[0] == [[]] and got[1] == [G.P_COUNT | G.P_BYTES | G.NO_T_BANDWIDTH | G.GROUP] and got[3] == [0] and got[4] == [1]
    eng.close()


# (pf, pb, bw), s, persistent routes -> flags of the persistent class, kept; the row also has 2 transient routes and 2 groups under gf = 100
RULE = [
    ((3, 30, 3), 10, 5, G.P_COUNT | G.P_BYTES, 3),   # the third route fills both limits at once
    ((3, 25, 3), 10, 5, G.P_COUNT | G.P_BYTES, 3),   # ceil(25 / 10) == 3 == pf
    ((5, 25, 3), 10, 6, G.P_BYTES, 3),               # bytes only
    ((3, 25, 3), 0, 5, G.P_COUNT, 3),                # s == 0: no bytes limit
    ((3, 0, 3), 10, 5, G.P_BYTES, 0),                # pb == 0
    ((0, 1000, 3), 10, 5, G.P_COUNT, 0),             # pf == 0, with bandwidth
    ((0, 1000, 1), 10, 5, G.P_COUNT, 0),             # pf == 0, without
    ((3, 0, 1), 10, 5, G.P_BYTES, 0),
    ((0, 0, 1), 10, 5, G.P_COUNT | G.P_BYTES, 0),
    ((3, 1000, 1), 10, 5, G.NO_P_BANDWIDTH, 0),
    ((3, G.LONG_MAX, 3), 2**32 - 1, 5, G.P_COUNT, 3),  # pb = 2^63 - 1
    ((4, G.LONG_MAX, 3), 2**31, 3, 0, 3),            # s = 2^31 with 3 kept: the meter exceeds 2^32
    ((3, 3 * 2**31, 3), 2**31, 5, G.P_COUNT | G.P_BYTES, 3),  # the bytes compare needs 64 bits
    ((5, 5, 3), 10, 5, G.P_BYTES, 1),                # ceil(5 / 10) == 1: the first route alone reaches the bytes limit
    ((5, 50, 3), 10, 5, 0, 5),                       # exactly as many as both limits admit: not throttled
]


def test_the_value_table_of_the_row_rule():
    keys, rows = K.sizes_case([6], n_transient=2)
    eng = host_engine().rebuild(keys)
    pers = [i for i in rows[0] if K.class_of(keys[i]) == 1]
    groups = [i for i in rows[0] if K.class_of(keys[i]) == 2][:2]
    trans = [i for i in rows[0] if K.class_of(keys[i]) == 0]
    table = [(pf, 100, pb, bw) for (pf, pb, bw), _s, _n, _f, _k in RULE]
    case_rows = [sorted(pers[:n] + groups + trans) for _t, _s, n, _f, _k in RULE]
    pack = [s for _t, s, _n, _f, _k in RULE]
    got = G.assert_batch_equals_reference(eng, keys, case_rows, pack, table, list(range(len(RULE))), inline_threshold=11)  # every row here has fewer than 11 routes
    for r, ((pf, pb, bw), s, n, fl, kept) in enumerate(RULE):
        t_flag = 0 if bw & 1 else G.NO_T_BANDWIDTH
        assert got[1][r] == G.INLINE | fl | t_flag, (r, got[1][r])
        assert got[2][r] == (kept, 2 if bw & 1 else 0, 2), r
        assert got[3][r] == kept * s and got[4][r] == 1
    assert got[3][11] == 3 * 2**31 > 2**32
    # the inline bit: n < threshold, strictly
    n = len(case_rows[0])
    for thr, inline in ((n, 0), (n + 1, G.INLINE), (0, 0)):
        assert G.batch(eng, case_rows[:1], pack[:1], table[0], inline_threshold=thr)[1][0] & G.INLINE == inline
    eng.close()


def test_refused_input_leaves_the_outputs_untouched():
    keys, rows = K.sizes_case([4, 3])
    eng = host_engine().rebuild(keys)
    row, ids = U.csr_of_rows(rows)
    lib = _lib.lib()
    pack = np.array([5, 5], dtype=np.uint32)

    def call(pf, gf, pb, bw, row_gate):
        out = [np.full(8, 7, dtype=np.uint32), np.full(len(ids), 7, dtype=np.uint32), np.full(2, 7, dtype=np.uint32), np.full(6, 7, dtype=np.uint32),
               np.full(len(pf), 7, dtype=np.uint64), np.full(len(pf), 7, dtype=np.uint32)]
        a = [np.array(pf, dtype=np.int32), np.array(gf, dtype=np.int32), np.array(pb, dtype=np.int64), np.array(bw, dtype=np.uint8)]
        rg = None if row_gate is None else np.array(row_gate, dtype=np.uint32)
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
        info = _lib.GateInfo()
        rc = lib.bmq_routes_gate_batch(eng.h, p(row), p(ids), 2, p(pack), p(rg), p(a[0]), p(a[1]), p(a[2]), p(a[3]), len(pf), 0, p(out[0]), p(out[1]), len(ids),
                                       p(out[2]), p(out[3]), p(out[4]), p(out[5]), C.byref(info))
        return rc, out

    for args in (([-1], [1], [1], [3], None), ([1], [-1], [1], [3], None), ([1], [1], [-1], [3], None), ([1], [1], [1], [4], None), ([1], [1], [1], [3], [0, 1]),
                 ([1, 1], [1, 1], [1, 1], [3, 255], [0, 0]), ([1, 1], [1, 1], [1, 1], [3, 3], [2, 0])):
        rc, out = call(*args)
        assert rc == -1, args  # BMQ_E_INVAL
        assert all((o == 7).all() for o in out), args
    rc, out = call([1], [1], [1], [3], None)
    assert rc == 0 and not (out[0][:3] == 7).any()
    with pytest.raises(B.BmqError) as ex:  # an empty table names no row
        eng.routes_gate_batch(row, ids, pack, [])
    assert ex.value.code == -1
    # out_cap below the survivors: BMQ_E_NOSPACE; the count is in the info, flags and meters are valid
    want = G.expected(keys, rows, pack, (2, 2, G.LONG_MAX, 3))
    with pytest.raises(B.BmqError) as ex:
        G.batch(eng, rows, pack, (2, 2, G.LONG_MAX, 3), out_cap=2)
    assert ex.value.code == -3 and ex.value.info.n_kept == sum(len(r) for r in want[0]) > 2
    assert ex.value.flags.tolist() == want[1] and ex.value.meter_bytes.tolist() == want[3] and ex.value.meter_records.tolist() == want[4]
    eng.close()


def test_empty_rows_and_empty_batches():
    keys, rows = K.sizes_case([4, 3])
    eng = host_engine().rebuild(keys)
    G.assert_batch_equals_reference(eng, keys, [[], rows[0], [], [], rows[1], []], [1, 2, 3, 4, 5, 6], [(1, 1, 100, 3), (0, 2, 100, 2)], [0, 0, 1, 1, 1, 0])
    got = G.batch(eng, [], [], G.DEFAULT)
    assert got[0] == [] and got[3] == [0] and got[4] == [0] and G.info_counts(got[5]) == (0,) * 7
    got = G.batch(eng, [[], []], [9, 9], (0, 0, 0, 0))
    assert got[0] == [[], []] and got[1] == [0, 0] and got[4] == [0]
    eng.close()


def test_gating_the_gated_rows_again_changes_nothing():
    keys, rows, row_gate, pack = G.random_case(5)
    eng = host_engine().rebuild(keys)
    for table in G.TABLES:
        once = G.batch(eng, rows, pack, table, row_gate, 6)
        twice = G.assert_batch_equals_reference(eng, keys, once[0], pack, table, row_gate, 6)
        assert twice[0] == once[0] and twice[2] == once[2]
    eng.close()


def test_a_ranked_class_of_more_than_rank_max_members_is_sorted_on_the_host():
    keys, rows = K.sizes_case([G.RANK_MAX + 1, 20], n_transient=1)
    eng = host_engine().rebuild(keys)
    late = [K.persistent("f/0", 10 ** 5 - 1 - i) for i in range(3)]  # ids out of key order in the large row too
    eng.apply([(0, k) for k in late])
    by_id = keys + late
    rows[0] = rows[0] + [len(keys), len(keys) + 1, len(keys) + 2]
    got = G.assert_batch_equals_reference(eng, by_id, rows, [10, 10], [(7, G.INT_MAX, G.LONG_MAX, 3), (5, 5, G.LONG_MAX, 3)], [0, 1])
    assert (got[5].n_rows_fallback, got[5].n_rows_ranked) == (1, 1)
    # a class of that size that is dropped whole needs no rank, and none on the host
    got = G.assert_batch_equals_reference(eng, by_id, rows[:1], [10], (0, G.INT_MAX, G.LONG_MAX, 3))
    assert (got[5].n_rows_fallback, got[5].n_rows_ranked, got[5].n_rows_flagged) == (0, 0, 1)
    eng.close()


def test_the_device_forms_need_a_device():
    eng = host_engine().rebuild([K.persistent("a", 1)])
    out = np.full(8, 7, dtype=np.uint32)
    p = out.ctypes.data
    with pytest.raises(B.BmqError) as ex:
        eng.routes_gate_device(p, p, 1, 1, p, None, p, p, p, p, 1, 0, p, p, 8, p, None, p, p)
    assert ex.value.code == -2
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery_gated(0, [G.DEFAULT], [1], 0, [0, 0], [], 1, *[np.full(4, 7, dtype=np.uint32) for _ in range(6)])
    assert ex.value.code == -2 and (out == 7).all()
    eng.close()


def test_gate_info_mirror_has_the_layout_of_the_header(tmp_path):
    """_lib.GateInfo restates bmq_gate_info: same size, every field at the same offset; the flag bits are the header's"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_gate_info));']
    lines += ['printf("%s %%zu\\n", offsetof(bmq_gate_info, %s));' % (f, f) for f, _ in _lib.GateInfo._fields_]
    lines += ['printf("bits %u %u %u %u %u %u\\n", BMQ_GATE_INLINE, BMQ_GATE_P_COUNT, BMQ_GATE_P_BYTES, BMQ_GATE_NO_P_BANDWIDTH, BMQ_GATE_NO_T_BANDWIDTH, BMQ_GATE_GROUP);']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(l.split() for l in out[:-1])
    assert int(got["size"]) == C.sizeof(_lib.GateInfo)
    for f, _ in _lib.GateInfo._fields_:
        assert int(got[f]) == getattr(_lib.GateInfo, f).offset, f
    assert {"n_in", "n_kept", "n_rows_single", "n_rows_gated", "n_rows_flagged", "n_rows_ranked", "n_rows_fallback", "generation", "ms_classify", "ms_rank",
            "ms_write"} == {f for f, _ in _lib.GateInfo._fields_}
    assert out[-1].split()[1:] == [str(b) for b in (G.INLINE, G.P_COUNT, G.P_BYTES, G.NO_P_BANDWIDTH, G.NO_T_BANDWIDTH, G.GROUP)]
    E = B.Engine
    assert (E.GATE_INLINE, E.GATE_P_COUNT, E.GATE_P_BYTES, E.GATE_NO_P_BANDWIDTH, E.GATE_NO_T_BANDWIDTH, E.GATE_GROUP) == (1, 2, 4, 8, 16, 32)
    assert {"bmq_routes_gate_batch", "bmq_routes_gate_dev", "bmq_delivery_wait_gated"} <= set(_lib.ABI_SYMBOLS)
