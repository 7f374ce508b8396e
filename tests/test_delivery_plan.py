"""The delivery plan of a match batch (bmq_delivery_plan, bifromq_amd/csrc/bmq_delivery_core.h) against the restatement of
DeliverExecutorGroup.submit in tests/test_share_resolve.py::submit_ref: one group per DelivererKey, members of shared subscriptions filed
beside the normal routes of their key, rows of one topic adjacent.

CPU tier: a host-only engine runs the per-item functions the gfx950 kernels wrap (tests/test_delivery_plan_gpu.py runs the kernels)."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from oracle import oracle as O
from tests import delivery_cases as D
from tests import share_ref as R
from tests import util as U
from tests.test_share_resolve import build_case, submit_ref

assert hasattr(B.Engine, "delivery_plan") and hasattr(B.Engine, "delivery_plan_device") and hasattr(B.Engine, "match_wait_delivery")

NONE = R.NONE
COUNTS = [1, 2, 5, 63, 65, 200]


@pytest.mark.parametrize("seed", [31, 32])
def test_random_parity(seed):
    # (the normal routes use 2 x 5 of the 3 x 9 deliverer keys the members use: some keys are reached through members only)
    eng, keys, flags, tables, rows, senders = build_case(seed, shared=0.4, counts=COUNTS, brokers=(0, 1), dkeys=5)
    exp = submit_ref(keys, flags, rows, senders, tables, 77)
    # the reference itself has keys reached both ways and keys reached through members only
    kinds = [{x[3] is None for x in v} for v in exp.values()]
    assert sum(len(k) == 2 for k in kinds) > 0 and sum(k == {False} for k in kinds) > 0
    plan = D.run_plan(eng, rows, senders, 77)
    got, unres, dead = D.plan_dict(eng, plan)
    assert got == exp and not unres and not dead
    info = plan[-1]
    assert info.n_merged_groups > 0 and info.n_share_only_groups > 0 and info.special == 0
    assert info.generation == eng.info().generation
    # a second plan (cached group slots) with another nonce
    assert D.plan_dict(eng, D.run_plan(eng, rows, senders, 78))[0] == submit_ref(keys, flags, rows, senders, tables, 78)
    eng.close()


def test_hand_built_interleave():
    eng, keys, flags, rows, tables, senders = D.interleave_case()
    exp = submit_ref(keys, flags, rows, senders, tables, 1)
    assert list(exp) == [b"1\0k"]
    plan = D.run_plan(eng, rows, senders, 1)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == exp
    ot, orr, oa, ss, sm, goff, info = plan
    assert (info.n_groups, info.n_merged_groups, info.n_share_only_groups, info.n_rows, info.n_share_rows) == (1, 1, 0, 8, 5)
    # exactly (topic, route, sender) order, normal and member rows interleaved
    assert ot.tolist() == [0, 1, 2, 2, 2, 2, 3, 4]
    o_id = flags.index(3)
    n2 = [i for i in rows[2] if flags[i] == 1][0]
    middle = [(n2, NONE)] + [(o_id, 1 + k) for k in range(3)] if n2 < o_id else [(o_id, 1 + k) for k in range(3)] + [(n2, NONE)]
    assert [(r, NONE if a == NONE else int(ss[a])) for r, a in zip(orr[2:6].tolist(), oa[2:6].tolist())] == middle
    assert [a == NONE for a in oa.tolist()] == [True, False] + [r == n2 for r in orr[2:6].tolist()] + [False, True]
    eng.close()


def test_the_nul_matters():
    eng, keys, flags, rows, tables, senders = D.nul_case()
    exp = submit_ref(keys, flags, rows, senders, tables, 0)
    assert set(exp) == {b"12\0x", b"1\0" + b"2x", b"1\0k"}
    plan = D.run_plan(eng, rows, senders, 0)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == exp
    assert {x[3] for x in got[b"1\0k"]} == {None, b"1\0inboxA\0k", b"1\0inboxB\0k"}  # both members AND the normal route: one group
    assert all(x[3] is None for x in got[b"12\0x"]) and all(x[3] is not None for x in got[b"1\0" + b"2x"])
    info = plan[-1]
    assert (info.n_groups, info.n_merged_groups, info.n_share_only_groups) == (3, 1, 1)
    eng.close()


def test_key_known_to_the_index_but_absent_from_the_batch():
    T = "T"
    keys = [O.route_key_from_mqtt(T, "a", O.receiver_url(1, "i", "k")), O.route_key_from_mqtt(T, "b", O.receiver_url(2, "j", "q")), O.route_key_from_mqtt(T, "$share/g/b")]
    eng, keys, flags, rows = D.index_of(keys, [T], ["a", "b"])
    tables = {flags.index(2): (False, ["1\0m\0k"])}
    eng.share_members_apply({flags.index(2): tables[flags.index(2)][1]})
    senders = [[1], [2]]
    first = D.run_plan(eng, rows, senders, 4)  # the group table now holds the slot of 1 NUL k
    assert D.plan_dict(eng, first)[0] == submit_ref(keys, flags, rows, senders, tables, 4) and first[-1].n_merged_groups == 1
    only_b = [[], rows[1]]
    plan = D.run_plan(eng, only_b, senders, 4)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == submit_ref(keys, flags, only_b, senders, tables, 4)
    assert [x[3] for x in got[b"1\0k"]] == [b"1\0m\0k"] and all(x[3] is None for x in got[b"2\0q"])
    info = plan[-1]
    assert (info.n_groups, info.n_merged_groups, info.n_share_only_groups) == (2, 0, 1)
    eng.close()


def test_specials():
    eng, exp, exp_unres, exp_dead, rows, senders, live_rows = D.specials_case()
    assert exp_unres and len({x[1] for x in exp_dead}) == 3
    plan = D.run_plan(eng, rows, senders, 3)
    got, unres, dead = D.plan_dict(eng, plan)
    assert (got, unres, dead) == (exp, exp_unres, exp_dead)
    assert plan[-1].special == 3
    # ... and a batch with neither
    plan = D.run_plan(eng, live_rows, senders, 3)
    assert D.plan_dict(eng, plan) == (exp, [], []) and plan[-1].special == 0
    eng.close()


def test_degenerate_batches():
    eng, keys, flags, tables, rows, senders = build_case(33, shared=0.4, counts=COUNTS, n_filters=120, n_topics=60)
    # an empty CSR
    ot, orr, oa, ss, sm, goff, info = eng.delivery_plan(np.zeros(4, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(4, dtype=np.uint32), [], 1)
    assert (info.n_rows, info.n_share_rows, info.n_groups, info.special) == (0, 0, 0, 0) and goff.tolist() == [0] and len(ot) == 0
    # no shared pairs: the groups of the fan-out grouping, as dictionaries
    normal = [[i for i in r if flags[i] == 1] for r in rows]
    plan = D.run_plan(eng, normal, senders, 1)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == submit_ref(keys, flags, normal, senders, tables, 1)
    fot, forr, fgoff, frep, fsp = eng.fanout_group(*U.csr_of_rows(normal))
    fan = sorted(sorted(zip(fot[fgoff[g]:fgoff[g + 1]].tolist(), forr[fgoff[g]:fgoff[g + 1]].tolist())) for g in range(len(fgoff) - 1))
    assert sorted([(t, r) for t, r, _, _ in v] for v in got.values()) == fan and fsp == 0
    assert (plan[2] == NONE).all() and plan[-1].n_share_rows == 0 and plan[-1].n_merged_groups == 0
    # shared pairs only
    shared = [[i for i in r if flags[i] != 1] for r in rows]
    plan = D.run_plan(eng, shared, senders, 1)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == submit_ref(keys, flags, shared, senders, tables, 1)
    assert (plan[2] != NONE).all() and plan[-1].n_share_only_groups == plan[-1].n_groups > 0
    # ordered shares only and nobody published: no row at all
    ordered = [[i for i in r if flags[i] == 3] for r in rows]
    assert sum(len(r) for r in ordered) > 0
    plan = D.run_plan(eng, ordered, [[] for _ in rows], 1)
    assert (plan[-1].n_rows, plan[-1].n_groups) == (0, 0) and plan[5].tolist() == [0]
    # a topic with zero senders on an $oshare route: no row for it, the others as ever
    some = [s if t % 2 else [] for t, s in enumerate(senders)]
    plan = D.run_plan(eng, rows, some, 1)
    got, _, _ = D.plan_dict(eng, plan)
    assert got == submit_ref(keys, flags, rows, some, tables, 1)
    silent = {t for t, s in enumerate(some) if not s}
    assert not any(x[0] in silent and flags[x[1]] == 3 for v in got.values() for x in v)
    eng.close()


def test_nospace_reports_all_three_counts():
    eng, keys, flags, tables, rows, senders = build_case(34, shared=0.4, counts=COUNTS, n_filters=120, n_topics=60)
    full = D.run_plan(eng, rows, senders, 9, row_cap=1 << 16, share_cap=1 << 16, group_cap=1 << 10)
    info = full[-1]
    need = (info.n_rows, info.n_share_rows, info.n_groups)
    assert min(need) > 1
    for which in range(3):
        caps = [need[0], need[1], need[2]]
        caps[which] -= 1
        with pytest.raises(B.BmqError) as ex:
            D.run_plan(eng, rows, senders, 9, row_cap=caps[0], share_cap=caps[1], group_cap=caps[2], retry=False)
        assert ex.value.code == -3 and ex.value.needed == need
        again = D.run_plan(eng, rows, senders, 9, row_cap=need[0], share_cap=need[1], group_cap=need[2], retry=False)
        assert D.plan_dict(eng, again) == D.plan_dict(eng, full)
    # the wrapper's own retry
    assert D.plan_dict(eng, D.run_plan(eng, rows, senders, 9, row_cap=1, share_cap=1, group_cap=1)) == D.plan_dict(eng, full)
    eng.close()


def test_across_a_generation_change():
    for carry in (1, 0):
        rnd_case = build_case(35, shared=0.4, counts=COUNTS, n_filters=150, n_topics=80)
        eng0, keys, flags, tables, rows, senders = rnd_case
        eng0.close()
        eng = B.Engine(device=-1, share_carry=carry).rebuild(keys)
        eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
        assert D.plan_dict(eng, D.run_plan(eng, rows, senders, 5))[0] == submit_ref(keys, flags, rows, senders, tables, 5)
        # routes with new deliverer keys, one of them the key of existing members: the refill path
        # (n_refill_calls counts refills of the device's fast path, which a host-only engine does not have: here the generic passes map the new
        # routes, so the two counts are summed; tests/test_delivery_plan_gpu.py asserts on n_refill_calls alone)
        before = eng.fanout_info().n_refill_calls + eng.fanout_info().n_generic_calls
        new_keys = [O.route_key_from_mqtt("tenantA", "x/%d" % i, O.receiver_url(7 if i else 0, "inbox%d" % i, "fresh%d" % (i % 3) if i else "d0")) for i in range(12)]
        eng.apply([(0, k) for k in new_keys])
        first = eng.info().next_route_id - len(new_keys)
        all_keys, all_flags = keys + new_keys, flags + [1] * len(new_keys)
        rows2 = [r + [first + (t % 12)] for t, r in enumerate(rows)]
        assert D.plan_dict(eng, D.run_plan(eng, rows2, senders, 5))[0] == submit_ref(all_keys, all_flags, rows2, senders, tables, 5)
        after = eng.fanout_info()
        assert after.n_refill_calls + after.n_generic_calls > before
        # compact: ids are renumbered (ranks of the sorted keys again)
        eng.compact()
        live = sorted(all_keys)
        new_id = {k: i for i, k in enumerate(live)}
        lflags = [O.parse_route_key(k)[0] for k in live]
        rows3 = [sorted(new_id[all_keys[i]] for i in r) for r in rows2]
        plan = D.run_plan(eng, rows3, senders, 5)
        got, unres, dead = D.plan_dict(eng, plan)
        if carry:
            ltables = {new_id[keys[rid]]: tab for rid, tab in tables.items()}
            assert got == submit_ref(live, lflags, rows3, senders, ltables, 5) and not unres and not dead
        else:  # every shared row lands in the unresolved group
            normal = [[i for i in r if lflags[i] == 1] for r in rows3]
            assert got == submit_ref(live, lflags, normal, senders, {}, 5) and not dead
            first_s = np.concatenate([[0], np.cumsum([len(s) for s in senders])]).tolist()
            exp_unres = sorted([(t, i, NONE, None) for t, r in enumerate(rows3) for i in r if lflags[i] == 2] +
                               [(t, i, NONE, None) for t, r in enumerate(rows3) for i in r if lflags[i] == 3])
            assert unres == exp_unres and plan[-1].special == 1 and plan[-1].n_share_rows == len(exp_unres)
            assert first_s[-1] > 0
        eng.close()


def test_device_forms_need_a_device():
    """bmq_delivery_plan_dev and bmq_delivery_wait on a host-only engine: BMQ_E_NODEVICE, nothing written"""
    eng = B.Engine(device=-1).rebuild([O.route_key_from_mqtt("T", "a", O.receiver_url(1, "i", "k"))])
    out = [np.full(4, 7, dtype=np.uint32) for _ in range(6)]
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery(0, [0, 0], [], 1, *out)
    assert ex.value.code == -2
    with pytest.raises(B.BmqError) as ex:
        eng.delivery_plan_device(*([out[0].ctypes.data] * 2), 1, 0, out[0].ctypes.data, out[0].ctypes.data, 0, 1, *([out[1].ctypes.data] * 3), 4,
                                 *([out[2].ctypes.data] * 2), 4, out[3].ctypes.data, 3)
    assert ex.value.code == -2
    assert all((o == 7).all() for o in out)
    eng.close()


def test_delivery_info_mirror_has_the_layout_of_the_header(tmp_path):
    """_lib.DeliveryInfo restates bmq_delivery_info: same size, every field at the same offset"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_delivery_info));']
    lines += ['printf("%s %%zu\\n", offsetof(bmq_delivery_info, %s));' % (f, f) for f, _ in _lib.DeliveryInfo._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.DeliveryInfo)
    for f, _ in _lib.DeliveryInfo._fields_:
        assert int(got[f]) == getattr(_lib.DeliveryInfo, f).offset, f
    assert {"n_rows", "n_share_rows", "n_groups", "n_merged_groups", "n_share_only_groups", "special", "generation", "ms_group", "ms_resolve", "ms_map",
            "ms_merge"} == {f for f, _ in _lib.DeliveryInfo._fields_}
