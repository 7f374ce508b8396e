"""What tests/test_delivery_plan.py (host-only engine) and tests/test_delivery_plan_gpu.py (gfx950 kernels) share (not a conftest): the
reading of a delivery plan (bmq_delivery_plan, include/bmq.h) as the dictionary tests/test_share_resolve.py::submit_ref builds --
{DelivererKey bytes: [(topic, route id, sender index | NONE, member url | None)]} -- and the hand-built cases both tiers run."""
import functools
import random

import numpy as np

import bifromq_amd as B
from oracle import oracle as O
from tests import share_ref as R
from tests import util as U
from tests.test_share_resolve import dk_bytes, submit_ref

NONE = R.NONE


def plan_dict(eng, plan):
    """-> ({DelivererKey: rows}, unresolved rows, dead rows).  Checks on the way: the groups partition the rows, none is empty, the rows of a
    group are in (topic, route, sender) order and ALL name the group's DelivererKey (the first row's, as the header says), no key has two
    groups, the special groups come last and carry what their bit says."""
    ot, orr, oa, ss, sm, goff, info = plan
    n = info.n_rows
    assert len(ot) == len(orr) == len(oa) == n and len(ss) == len(sm) == info.n_share_rows and len(goff) == info.n_groups + 1
    assert goff[0] == 0 and goff[-1] == n and (np.diff(goff.astype(np.int64)) > 0).all()
    aux = oa[oa != NONE]
    assert sorted(aux.tolist()) == list(range(info.n_share_rows))  # every side entry belongs to exactly one row
    url = functools.lru_cache(maxsize=None)(lambda rid, m: eng.share_member(rid, m))
    key = functools.lru_cache(maxsize=None)(lambda rid: eng.route_key(rid))
    n_special = (info.special & 1) + ((info.special >> 1) & 1)
    got, unresolved, dead = {}, [], []
    merged = share_only = 0
    for g in range(info.n_groups):
        rows, keys = [], set()
        lo, hi = int(goff[g]), int(goff[g + 1])
        is_dead = (info.special & 2) and g == info.n_groups - 1
        is_unres = (info.special & 1) and g == info.n_groups - n_special
        for t, rid, a in zip(ot[lo:hi].tolist(), orr[lo:hi].tolist(), oa[lo:hi].tolist()):
            if is_dead:
                assert a == NONE
                rows.append((t, rid, NONE, None))
            elif a == NONE:
                rows.append((t, rid, NONE, None))
                keys.add(dk_bytes(key(rid)))
            elif sm[a] == NONE:
                assert is_unres
                rows.append((t, rid, int(ss[a]), None))
            else:
                assert not is_unres
                u = url(rid, int(sm[a]))
                rows.append((t, rid, int(ss[a]), u))
                keys.add(R.deliverer_key(u))
        assert rows == sorted(rows, key=lambda x: (x[0], x[1], x[2])), g
        if is_dead:
            dead = rows
        elif is_unres:
            unresolved = rows
        else:
            assert len(keys) == 1, (g, keys)  # a group = one DelivererKey
            dk = keys.pop()
            assert dk not in got  # ... and a DelivererKey = one group
            got[dk] = rows
            kinds = {x[3] is None for x in rows}
            merged += len(kinds) == 2
            share_only += kinds == {False}
    assert (info.n_merged_groups, info.n_share_only_groups) == (merged, share_only)
    return got, unresolved, dead


def run_plan(eng, rows, senders, nonce, **kw):
    so, sh = R.sender_arrays(senders)
    return eng.delivery_plan(*U.csr_of_rows(rows), so, sh, nonce, **kw)


def index_of(keys, tenants, topics, device=-1, **kw):
    """engine over sorted keys (ids = ranks), flags, the oracle's rows"""
    keys = sorted(keys)
    eng = B.Engine(device=device, **kw).rebuild(keys)
    flags = [O.parse_route_key(k)[0] for k in keys]
    tt = np.zeros(len(topics), dtype=np.uint32)
    rows = U.semantic_rows(O.KV(keys), tenants, tt, topics)
    return eng, keys, flags, rows


def interleave_case(device=-1):
    """one deliverer key 1 NUL k: normal routes match topics 0, 2, 4; members chosen for topics 1, 2, 3 live under it; topic 2 has three
    senders on an $oshare route"""
    T = "T"
    keys = [O.route_key_from_mqtt(T, "t/%d" % i, O.receiver_url(1, "inbox%d" % i, "k")) for i in (0, 2, 4)]
    keys += [O.route_key_from_mqtt(T, "$share/g/t/1"), O.route_key_from_mqtt(T, "$oshare/g/t/2"), O.route_key_from_mqtt(T, "$share/g/t/3")]
    topics = ["t/%d" % i for i in range(5)]
    eng, keys, flags, rows = index_of(keys, [T], topics, device)
    tables = {}
    for rid, f in enumerate(flags):
        if f in (2, 3):
            tables[rid] = (f == 3, ["1\0m%d_%d\0k" % (rid, j) for j in range(3)])
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    senders = [[5], [], [11, -12, 13], [7], []]
    return eng, keys, flags, rows, tables, senders


def nul_case(device=-1):
    """("1", "2x") and ("12", "x") concatenate alike; members that differ only in receiverId share the group of a normal route of their key"""
    T = "T"
    keys = [O.route_key_from_mqtt(T, "a", O.receiver_url(12, "c", "x")), O.route_key_from_mqtt(T, "a", O.receiver_url(1, "zz", "k")),
            O.route_key_from_mqtt(T, "$oshare/g/a"), O.route_key_from_mqtt(T, "$oshare/h/a")]
    eng, keys, flags, rows = index_of(keys, [T], ["a"] * 6, device)
    g_ids = [i for i, f in enumerate(flags) if f == 3]
    tables = {g_ids[0]: (True, ["1\0c\0" + "2x"]), g_ids[1]: (True, ["1\0inboxA\0k", "1\0inboxB\0k"])}
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    rnd = random.Random(9)
    senders = [[rnd.randint(R.INT_MIN, R.INT_MAX) for _ in range(4)] for _ in range(6)]
    return eng, keys, flags, rows, tables, senders


def specials_case(device=-1, **kw):
    """a shared route without a table, routes deleted after the CSR was taken (a normal one, a shared one WITH a table), an id never handed
    out -> (engine, expected {key: rows}, expected unresolved, expected dead, rows, senders, the rows without any of them: their plan is the first dictionary alone)"""
    T = "T"
    keys = [O.route_key_from_mqtt(T, "a", O.receiver_url(0, "i%d" % i, "d%d" % (i % 2))) for i in range(4)]
    keys += [O.route_key_from_mqtt(T, "$share/g%d/a" % i) for i in range(3)] + [O.route_key_from_mqtt(T, "$oshare/g3/a")]
    eng, keys, flags, rows = index_of(keys, [T], ["a"] * 5, device, **kw)
    shared = [i for i, f in enumerate(flags) if f in (2, 3)]
    normal = [i for i, f in enumerate(flags) if f == 1]
    unordered = [i for i in shared if flags[i] == 2]
    no_table, gone_shared, gone_normal = unordered[0], unordered[1], normal[0]
    tables = {rid: (flags[rid] == 3, ["0\0m%d\0d%d" % (j, j % 3) for j in range(4)]) for rid in shared if rid != no_table}
    eng.share_members_apply({rid: u for rid, (_, u) in tables.items()})
    senders = [[1, 2], [3], [], [4, 5, 6], [7]]
    never = eng.info().next_route_id + 1000
    rows = [r + [never] if t % 2 == 0 else r for t, r in enumerate(rows)]
    eng.apply([(1, keys[gone_shared]), (1, keys[gone_normal])])
    gone = {gone_shared, gone_normal, never}
    live_rows = [[i for i in r if i not in gone and i != no_table] for r in rows]
    exp = submit_ref(keys, flags, live_rows, senders, tables, 3)
    # (an unordered share without a table: one row, the whole pack)
    exp_unres = [(t, no_table, NONE, None) for t, r in enumerate(rows) if no_table in r]
    exp_dead = sorted((t, i, NONE, None) for t, r in enumerate(rows) for i in r if i in gone)
    return eng, exp, exp_unres, exp_dead, rows, senders, live_rows
