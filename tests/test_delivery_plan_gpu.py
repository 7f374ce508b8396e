"""The delivery plan on the device: the gfx950 kernels of bifromq_amd/csrc/bmq_delivery_kernels.h behind bmq_delivery_plan_dev /
bmq_delivery_plan / bmq_delivery_wait against tests/test_share_resolve.py::submit_ref and against a host-only engine (the same
per-item functions under the other executor).  Shapes: the smallest at which the kernels can still go wrong -- lists that end at, one
before and one behind a wave (64) and a tile of the grouping's fast path (FO_TILE = 1024), both grouping paths, a group table that grows."""
import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import delivery_cases as D
from tests import share_ref as R
from tests import util as U
from tests.test_share_resolve import build_case, submit_ref
from tests.test_share_resolve_gpu import Hbm

assert hasattr(B.Engine, "delivery_plan") and hasattr(B.Engine, "delivery_plan_device") and hasattr(B.Engine, "match_wait_delivery")

pytestmark = pytest.mark.gpu

NONE = R.NONE
COUNTS = [1, 2, 5, 63, 65, 200]


def device_plan(eng, mem, rows, senders, nonce, slack=8):
    """bmq_delivery_plan_dev over plain device buffers: a call with too-small buffers first (it reports the three counts), then one that fits"""
    row, ids = U.csr_of_rows(rows)
    so, sh = R.sender_arrays(senders)
    d_row, d_ids, d_so, d_sh = mem.put(row), mem.put(ids), mem.put(so), mem.put(sh)
    a = (d_row, d_ids, len(rows), int(row[-1]), d_so, d_sh, len(sh), nonce)
    tiny = [mem.zeros(1) for _ in range(5)] + [mem.zeros(2)]
    with pytest.raises(B.BmqError) as ex:
        eng.delivery_plan_device(*a, tiny[0], tiny[1], tiny[2], 1, tiny[3], tiny[4], 1, tiny[5], 1)
    assert ex.value.code == -3
    nr, ns, ng = ex.value.needed
    o = [mem.zeros(nr + slack) for _ in range(3)] + [mem.zeros(ns + slack) for _ in range(2)] + [mem.zeros(ng + 1 + slack)]
    info = eng.delivery_plan_device(*a, o[0], o[1], o[2], nr + slack, o[3], o[4], ns + slack, o[5], ng + slack)
    assert (info.n_rows, info.n_share_rows, info.n_groups) == (nr, ns, ng)
    return mem.get(o[0], nr), mem.get(o[1], nr), mem.get(o[2], nr), mem.get(o[3], ns), mem.get(o[4], ns), mem.get(o[5], ng + 1), info


def test_gpu_device_parity():
    eng, keys, flags, tables, rows, senders = build_case(31, device=0, shared=0.4, counts=COUNTS, brokers=(0, 1), dkeys=5)
    host, *_ = build_case(31, device=-1, shared=0.4, counts=COUNTS, brokers=(0, 1), dkeys=5)
    exp = submit_ref(keys, flags, rows, senders, tables, 77)
    mem = Hbm()
    plan = device_plan(eng, mem, rows, senders, 77)
    got, unres, dead = D.plan_dict(eng, plan)
    assert got == exp and not unres and not dead
    assert plan[-1].n_merged_groups > 0 and plan[-1].n_share_only_groups > 0
    assert D.plan_dict(host, D.run_plan(host, rows, senders, 77)) == (got, unres, dead)  # same functions, two executors
    # the host-buffer entry point stages the same arrays: the same plan (through its own retry)
    assert D.plan_dict(eng, D.run_plan(eng, rows, senders, 77, row_cap=3, share_cap=2, group_cap=1)) == (got, unres, dead)
    mem.free()
    host.close()
    eng.close()


def edge_case():
    """deliverer key j has ONE normal route matched by N_j topics and one $share route with a single member under the same key, matched
    by S_j topics that fall before, between and behind the normal ones; key 4: share rows outnumber the normal ones (an $oshare route, three
    senders per topic); the CSR is laid out by hand (rows ascending: what a match returns)"""
    T = "T"
    sizes = [(63, 1, "before"), (64, 64, "between"), (65, 65, "behind"), (1025, 64, "between"), (5, 100, "between")]
    keys = []
    for j in range(len(sizes)):
        keys.append(O.route_key_from_mqtt(T, "n/%d" % j, O.receiver_url(3, "in%d" % j, "key%d" % j)))
        keys.append(O.route_key_from_mqtt(T, "$%sshare/g/s/%d" % ("o" if j == 4 else "", j)))
    keys = sorted(keys)
    flags = [O.parse_route_key(k)[0] for k in keys]
    parsed = [O.parse_route_key(k) for k in keys]
    n_topics = 1400
    rows = [[] for _ in range(n_topics)]
    tables = {}
    for j, (n_norm, n_share, where) in enumerate(sizes):
        nid = [i for i, p in enumerate(parsed) if p[0] == 1 and p[2] == "n/%d" % j][0]
        sid = [i for i, p in enumerate(parsed) if p[0] != 1 and ("/" + p[2]).endswith("/s/%d" % j)][0]
        tables[sid] = (flags[sid] == 3, ["3\0member%d\0key%d" % (j, j)])
        first = 150
        for t in range(first, first + n_norm):
            rows[t].append(nid)
        start = {"before": first - n_share - 3, "between": first + 1, "behind": first + n_norm + 2}[where]
        for t in range(start, start + n_share):
            rows[t].append(sid)
    rows = [sorted(r) for r in rows]
    senders = [[t, -t, t * 7] if 150 <= t < 260 else [t] for t in range(n_topics)]
    return keys, flags, rows, tables, senders


def test_gpu_wave_and_tile_edges():
    keys, flags, rows, tables, senders = edge_case()
    exp = submit_ref(keys, flags, rows, senders, tables, 6)
    assert sorted(len([x for x in v if x[3] is None]) for v in exp.values()) == [5, 63, 64, 65, 1025]
    assert sorted(len([x for x in v if x[3] is not None]) for v in exp.values()) == [1, 64, 64, 65, 300]
    mem = Hbm()
    eng = B.Engine(device=0).rebuild(keys)
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    for _ in range(2):  # the first plan maps the routes (refill), the second runs on the cached slots
        plan = device_plan(eng, mem, rows, senders, 6)
        got, unres, dead = D.plan_dict(eng, plan)
        assert got == exp and not unres and not dead
        assert (plan[-1].n_groups, plan[-1].n_merged_groups, plan[-1].n_share_only_groups) == (5, 5, 0)
    assert eng.fanout_info().n_fast_calls > 0
    mem.free()
    eng.close()


def keys_case(n_keys, n_topics=300):
    """n_keys distinct deliverer keys, one normal route each; $share / $oshare routes whose members live under a handful of those keys
    and under two keys no route has -> (keys, flags, tables, rows(subset of the deliverer keys), senders)"""
    T = "T"
    keys = [O.route_key_from_mqtt(T, "n/%d" % j, O.receiver_url(j % 3, "in%d" % j, "dk%d" % j)) for j in range(n_keys)]
    keys += [O.route_key_from_mqtt(T, "$%sshare/g/s/%d" % ("o" if j % 2 else "", j)) for j in range(6)]
    keys = sorted(keys)
    parsed = [O.parse_route_key(k) for k in keys]
    flags = [p[0] for p in parsed]
    normal = {int(p[2][2:]): i for i, p in enumerate(parsed) if p[0] == 1}
    shared = [i for i, p in enumerate(parsed) if p[0] != 1]
    members = ["%d\0m%d\0dk%d" % (j % 3, j, j) for j in (0, 1, 7, n_keys - 1, n_keys // 2)] + ["9\0x\0nobody", "1\0y\0dk%d" % (n_keys + 5)]
    tables = {sid: (flags[sid] == 3, members[k:] + members[:k]) for k, sid in enumerate(shared)}

    def rows_over(js):
        js = list(js)
        rows = [sorted({normal[js[(t * 7 + k) % len(js)]] for k in range(7)} | {shared[t % len(shared)], shared[(t + 1) % len(shared)]}) for t in range(n_topics)]
        return rows
    senders = [[t * 31 + 1, -t] if t % 3 else [t] for t in range(n_topics)]
    return keys, flags, tables, rows_over, senders


@pytest.mark.parametrize("n_keys", [40, 1100])
def test_gpu_both_grouping_paths(n_keys):
    keys, flags, tables, rows_over, senders = keys_case(n_keys)
    eng = B.Engine(device=0).rebuild(keys)
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    mem = Hbm()
    # a first plan over few keys, a second over all of them: with 1100 keys the group table grows in between, and the map must probe the
    # table and the seed of the moment
    for js in (range(0, n_keys, 11), range(n_keys)):
        rows = rows_over(js)
        plan = device_plan(eng, mem, rows, senders, 12)
        got, unres, dead = D.plan_dict(eng, plan)
        assert got == submit_ref(keys, flags, rows, senders, tables, 12) and not unres and not dead
        assert plan[-1].n_share_only_groups >= 2 and plan[-1].n_merged_groups >= 1
    fi = eng.fanout_info()
    if n_keys == 40:
        assert fi.n_fast_calls > 0
    else:
        assert plan[-1].n_groups > 1026  # (more groups than the fast path's counters hold)
        assert fi.n_generic_calls > 0 and fi.n_table_grows > 0
    mem.free()
    eng.close()


def packed(strings):
    data = np.frombuffer(b"".join(strings) + b"\0" * 16, dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint32)
    return data, off


def test_gpu_ticket():
    from tests.test_fanout import _workload
    tenants, keys0, topics, tt = _workload(31, shared=0.4, brokers=(0, 1), dkeys=5)
    eng, keys, flags, tables, rows, senders = build_case(31, device=0, shared=0.4, counts=COUNTS, brokers=(0, 1), dkeys=5)
    assert keys == keys0
    tdata, toff = packed([t.encode() for t in tenants])
    pdata, poff = packed([t.encode() for t in topics])
    n = len(topics)
    so, sh = R.sender_arrays(senders)
    a = (tdata, toff, len(tenants), tt, pdata, poff, n)
    # the CSR a BMQ_FMT_IDS ticket of the same batch returns
    t_ids = eng.match_submit_fmt(*a, eng.FMT_IDS)
    row, ids = np.zeros(n + 1, dtype=np.uint32), np.zeros(1 << 16, dtype=np.uint32)
    total = eng.match_wait(t_ids, row, ids)
    ref = D.plan_dict(eng, eng.delivery_plan(row, ids[:total], so, sh, 21))
    assert ref[0] == submit_ref(keys, flags, rows, senders, tables, 21)

    def outs(rows_cap=1 << 16, share_cap=1 << 14, group_cap=1 << 10):
        return [np.zeros(rows_cap, dtype=np.uint32) for _ in range(3)] + [np.zeros(share_cap, dtype=np.uint32) for _ in range(2)] + [np.zeros(group_cap + 1, dtype=np.uint32)]

    def cut(o, info):
        return o[0][:info.n_rows], o[1][:info.n_rows], o[2][:info.n_rows], o[3][:info.n_share_rows], o[4][:info.n_share_rows], o[5][:info.n_groups + 1], info
    # two tickets in flight, two right answers (other nonces: other unordered picks)
    t1 = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    t2 = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    o1, o2 = outs(), outs()
    # the wrong wait is BMQ_E_STATE and leaves the ticket in flight -- both ways round
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait(t1, row, ids)
    assert ex.value.code == -7
    t3 = eng.match_submit_fmt(*a, eng.FMT_IDS)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery(t3, so, sh, 21, *outs())
    assert ex.value.code == -7
    assert eng.match_wait(t3, row, ids) == total
    tot2, info2 = eng.match_wait_delivery(t2, so, sh, 22, *o2)
    tot1, info1 = eng.match_wait_delivery(t1, so, sh, 21, *o1)
    assert tot1 == tot2 == total
    assert D.plan_dict(eng, cut(o1, info1)) == ref
    assert D.plan_dict(eng, cut(o2, info2))[0] == submit_ref(keys, flags, rows, senders, tables, 22)
    # too-small buffers: NOSPACE with the three counts, the ticket is released
    t4 = eng.match_submit_fmt(*a, eng.FMT_DELIVERY)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery(t4, so, sh, 21, *outs(4, 4, 4))
    assert ex.value.code == -3 and ex.value.needed == (info1.n_rows, info1.n_share_rows, info1.n_groups)
    with pytest.raises(B.BmqError) as ex:
        eng.match_wait_delivery(t4, so, sh, 21, *outs())
    assert ex.value.code == -7
    eng.close()


def test_gpu_specials():
    eng, exp, exp_unres, exp_dead, rows, senders, live_rows = D.specials_case(device=0)
    mem = Hbm()
    plan = device_plan(eng, mem, rows, senders, 3)
    assert D.plan_dict(eng, plan) == (exp, exp_unres, exp_dead) and plan[-1].special == 3
    plan = device_plan(eng, mem, live_rows, senders, 3)
    assert D.plan_dict(eng, plan) == (exp, [], []) and plan[-1].special == 0
    mem.free()
    eng.close()


@pytest.mark.parametrize("carry", [1, 0])
def test_gpu_across_a_generation_change(carry):
    host, keys, flags, tables, rows, senders = build_case(35, shared=0.4, counts=COUNTS, n_filters=150, n_topics=80)
    host.close()
    eng = B.Engine(device=0, share_carry=carry).rebuild(keys)
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    mem = Hbm()
    assert D.plan_dict(eng, device_plan(eng, mem, rows, senders, 5))[0] == submit_ref(keys, flags, rows, senders, tables, 5)
    # routes with new deliverer keys (and one under the key of existing members): the refill path of the fast grouping
    before = eng.fanout_info().n_refill_calls
    new_keys = [O.route_key_from_mqtt("tenantA", "x/%d" % i, O.receiver_url(7 if i else 0, "inbox%d" % i, "fresh%d" % (i % 3) if i else "d0")) for i in range(12)]
    eng.apply([(0, k) for k in new_keys])
    first = eng.info().next_route_id - len(new_keys)
    all_keys, all_flags = keys + new_keys, flags + [1] * len(new_keys)
    rows2 = [r + [first + (t % 12)] for t, r in enumerate(rows)]
    assert D.plan_dict(eng, device_plan(eng, mem, rows2, senders, 5))[0] == submit_ref(all_keys, all_flags, rows2, senders, tables, 5)
    assert eng.fanout_info().n_refill_calls > before
    eng.compact()
    live = sorted(all_keys)
    new_id = {k: i for i, k in enumerate(live)}
    lflags = [O.parse_route_key(k)[0] for k in live]
    rows3 = [sorted(new_id[all_keys[i]] for i in r) for r in rows2]
    plan = device_plan(eng, mem, rows3, senders, 5)
    got, unres, dead = D.plan_dict(eng, plan)
    if carry:
        ltables = {new_id[keys[rid]]: tab for rid, tab in tables.items()}
        assert got == submit_ref(live, lflags, rows3, senders, ltables, 5) and not unres and not dead
    else:
        normal = [[i for i in r if lflags[i] == 1] for r in rows3]
        assert got == submit_ref(live, lflags, normal, senders, {}, 5) and not dead
        assert unres == sorted((t, i, NONE, None) for t, r in enumerate(rows3) for i in r if lflags[i] != 1) and plan[-1].special == 1
    mem.free()
    eng.close()


def test_gpu_info_times():
    eng, keys, flags, tables, rows, senders = build_case(31, device=0, shared=0.4, counts=COUNTS, brokers=(0, 1), dkeys=5)
    eng.set_kernel_timing(True)
    plan = D.run_plan(eng, rows, senders, 1)
    info = plan[-1]
    assert info.n_share_rows > 0
    assert info.ms_group > 0 and info.ms_resolve > 0 and info.ms_map > 0 and info.ms_merge > 0
    eng.set_kernel_timing(False)
    assert D.run_plan(eng, rows, senders, 1)[-1].ms_merge == 0
    eng.close()
