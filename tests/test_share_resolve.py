"""Receivers of shared subscriptions (bmq_share_members_apply / bmq_share_resolve, bifromq_amd/csrc/bmq_share_core.h) against the
restatement of DeliverExecutorGroup.send(GroupMatching, ...) in tests/share_ref.py: the rendezvous hash of ordered shares, the documented
pick of unordered ones, the regrouping of the chosen members by DelivererKey, and the life cycle of the member tables.

CPU tier: a host-only engine runs the per-item functions the gfx950 kernels wrap (tests/test_share_resolve_gpu.py runs the kernels)."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from oracle import oracle as O
from tests import share_ref as R
from tests import util as U
from tests.test_fanout import SHARED, _csr, _workload


def test_murmur3_reference_vectors():
    """the published vectors of MurmurHash3_x64_128 pin the restatement"""
    assert R.murmur3_x64_128(b"") == (0, 0)
    assert R.murmur3_x64_128(b"hell") == (0x629942693E10F867, 0x92DB0B82BAEB5347)
    assert R.murmur3_x64_128(b"hello") == (0xCBD8A7B341BD9B02, 0x5B1E906A48AE1D19)
    assert R.murmur3_x64_128(b"The quick brown fox jumps over the lazy dog") == (0xE34BBC7BBC071B6C, 0x7A433CA9C49A9347)


def build_case(seed, device=-1, shared=0.4, counts=R.MEMBER_COUNTS, **kw):
    """an index built like tests/test_fanout.py::_workload, a member table for every group route (member counts cycling through `counts`),
    the oracle's rows and random senders"""
    rnd = random.Random(seed)
    tenants, keys, topics, tt = _workload(seed, shared=shared, **kw)
    eng = B.Engine(device=device).rebuild(keys)  # ids = ranks of the sorted keys
    flags = [O.parse_route_key(k)[0] for k in keys]
    group_ids = [i for i, f in enumerate(flags) if f in (2, 3)]
    tables = {rid: (flags[rid] == 3, R.member_list(rnd, counts[j % len(counts)])) for j, rid in enumerate(group_ids)}
    eng.share_members_apply({rid: urls for rid, (_, urls) in tables.items()})
    rows = U.semantic_rows(O.KV(keys), tenants, tt, topics)
    senders = R.senders_for(rnd, len(topics))
    return eng, keys, flags, tables, rows, senders


def member_url_of(eng):
    return functools.lru_cache(maxsize=None)(lambda rid, m: eng.share_member(rid, m))


def shared_pairs(rows, flags):
    return [(t, rid) for t, r in enumerate(rows) for rid in r if flags[rid] in (2, 3)]


def test_ordered_parity_with_rendezvous_hash():
    eng, keys, flags, tables, rows, senders = build_case(21)
    pairs = shared_pairs(rows, flags)
    assert len(pairs) > 200 and {len(u) for _, u in tables.values()} == set(R.MEMBER_COUNTS)
    lengths = {(4 + len(u.encode())) for _, urls in tables.values() for u in urls}
    assert {15, 16, 17, 31, 32, 33, 48} <= lengths and any(len(u) != len(u.encode()) for _, urls in tables.values() for u in urls)
    so, sh = R.sender_arrays(senders)
    assert set(R.SPECIAL_SENDERS) <= set(sh.tolist())
    res = eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=5)
    assert R.check_rows(member_url_of(eng), pairs, senders, tables, 5, res) > 10
    # every ordered row's member is the rendezvous winner (check_rows compared whole groups; this is the statement itself) ...
    op, os_, om, _, _ = res
    n_ordered = differ = 0
    seen = set()
    for p, s, m in zip(op.tolist(), os_.tolist(), om.tolist()):
        ordered, urls = tables[pairs[p][1]]
        if not ordered:
            continue
        n_ordered += 1
        assert m == R.rendezvous(int(sh[s]), urls)
        # ... and the inputs tell a signed comparison of the scores from an unsigned one
        case = (int(sh[s]), pairs[p][1])
        if len(urls) > 1 and case not in seen:
            seen.add(case)
            differ += m != R.rendezvous(int(sh[s]), urls, signed=False)
    assert n_ordered > 100 and differ > 0
    eng.close()


def test_unordered_pick_is_the_documented_formula():
    eng, keys, flags, tables, rows, senders = build_case(22, counts=[1, 2, 3, 7, 64, 200])
    pairs = [p for p in shared_pairs(rows, flags) if flags[p[1]] == 2]
    assert len(pairs) > 100
    so, sh = R.sender_arrays(senders)
    picks = []
    for nonce in (1, 0xDEADBEEFCAFEF00D):
        res = eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=nonce)
        R.check_rows(member_url_of(eng), pairs, senders, tables, nonce, res)
        by_pair = dict(zip(res[0].tolist(), res[2].tolist()))
        assert (res[1] == R.NONE).all()
        picks.append([by_pair[i] for i in range(len(pairs))])
        assert picks[-1] == [R.pick(nonce, t, rid, len(tables[rid][1])) for t, rid in pairs]
    assert picks[0] != picks[1]
    eng.close()


def test_unordered_pick_is_uniform():
    """one 7-member group, 70 000 topics: each member's count within 5 standard deviations of the binomial expectation"""
    key = O.route_key_from_mqtt("t", "$share/g/a")
    eng = B.Engine(device=-1).rebuild([key])
    eng.share_members_apply({0: ["0\0inbox%d\0d%d" % (i, i) for i in range(7)]})
    n = 70000
    op, os_, om, goff, sp = eng.share_resolve(np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32), [], nonce=20261016)
    assert len(om) == n and sp == 0 and len(goff) == 8
    counts = np.bincount(om, minlength=7)
    bound = 5 * math.sqrt(n * (1 / 7) * (6 / 7))
    assert 462 < bound < 464
    assert (np.abs(counts - n / 7) <= bound).all(), counts
    eng.close()


def test_grouping_by_deliverer_key():
    key = O.route_key_from_mqtt("t", "$oshare/g/a")
    eng = B.Engine(device=-1).rebuild([key])
    # members 0 / 1 differ only in receiverId; ("1", "2x") and ("12", "x") concatenate alike
    urls = ["1\0inboxA\0k", "1\0inboxB\0k", "1\0c\0" + "2x", "12\0c\0x"]
    eng.share_members_apply({0: urls})
    assert eng.share_info().n_deliverers == 3
    n_topics = 40
    rnd = random.Random(4)
    senders = [[rnd.randint(R.INT_MIN, R.INT_MAX) for _ in range(5)] for _ in range(n_topics)]
    pairs = [(t, 0) for t in range(n_topics)] + [(3, 7), (5, 0)]  # (route id 7 was never handed out: unresolved)
    so, sh = R.sender_arrays(senders)
    res = eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=0)
    assert R.check_rows(member_url_of(eng), pairs, senders, {0: (True, urls)}, 0, res) == 3
    op, os_, om, goff, sp = res
    group_of = {}
    for g in range(len(goff) - 1):
        for m in set(om[goff[g]:goff[g + 1]].tolist()):
            assert m not in group_of  # the groups partition the rows by member ...
            group_of[m] = g
    assert set(group_of) == {0, 1, 2, 3, R.NONE}
    assert group_of[0] == group_of[1] and group_of[2] != group_of[3] and group_of[R.NONE] == len(goff) - 2 and sp == 1
    eng.close()


def test_table_lifecycle():
    keys = sorted([O.route_key_from_mqtt("t", "$oshare/g/a"), O.route_key_from_mqtt("t", "$share/g/b"), O.route_key_from_mqtt("t", "c", O.receiver_url(0, "i", "d"))])
    flags = [O.parse_route_key(k)[0] for k in keys]
    o_id, u_id, n_id = flags.index(3), flags.index(2), flags.index(1)
    eng = B.Engine(device=-1).rebuild(keys)
    gen0 = eng.info().generation
    assert eng.share_info().n_tables == 0 and eng.share_info().generation == gen0
    senders = [[7, -7, 1 << 20]]
    so, sh = R.sender_arrays(senders)
    pairs = [(0, o_id), (0, u_id), (0, n_id)]

    def run(tables, **kw):
        res = eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=9, **kw)
        R.check_rows(member_url_of(eng), pairs, senders, tables, 9, res)
        return res

    run({})  # no tables: everything unresolved
    a = ["%d\0in%d\0dk%d" % (i % 2, i, i % 3) for i in range(9)]
    eng.share_members_apply({o_id: a, u_id: a[:4]})
    inf = eng.share_info()
    assert (inf.n_tables, inf.n_members, inf.n_deliverers) == (2, 13, 6)
    assert eng.share_member(o_id, 8) == a[8].encode()
    tables = {o_id: (True, a), u_id: (False, a[:4])}
    run(tables)
    # too-small buffers: BMQ_E_NOSPACE with the needed counts; a second call with those counts succeeds
    pt, pr = np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)
    nr, ng, spc = C.c_uint32(), C.c_uint32(), C.c_uint32()

    def raw(row_cap, group_cap):
        out = [np.zeros(max(row_cap, 1), dtype=np.uint32) for _ in range(3)] + [np.zeros(group_cap + 1, dtype=np.uint32)]
        p = [o.ctypes.data_as(C.c_void_p) for o in (pt, pr, so, sh)] + [o.ctypes.data_as(C.c_void_p) for o in out]
        rc = _lib.lib().bmq_share_resolve(eng.h, p[0], p[1], len(pt), p[2], p[3], 1, 9, p[4], p[5], p[6], row_cap, p[7], group_cap, C.byref(nr), C.byref(ng), C.byref(spc))
        return rc, out
    rc, _ = raw(2, 1)
    assert rc == -3 and nr.value == 5 and ng.value >= 2
    need = (nr.value, ng.value)
    rc, _ = raw(need[0], 1)
    assert rc == -3 and (nr.value, ng.value) == need
    rc, out = raw(*need)
    assert rc == 0 and (nr.value, ng.value) == need
    R.check_rows(member_url_of(eng), pairs, senders, tables, 9, (out[0][:need[0]], out[1][:need[0]], out[2][:need[0]], out[3][:need[1] + 1], spc.value))
    # malformed URL / normal-route id / dead id / too many members: BMQ_E_INVAL and nothing changed
    for bad in ({o_id: ["0\0only-two-parts"]}, {o_id: ["0\0a\0b\0c"]}, {n_id: a}, {99: a}, {u_id: a[:2], o_id: ["x"]}, {o_id: ["0\0i%d\0d" % i for i in range(65536)]}):
        with pytest.raises(B.BmqError) as ex:
            eng.share_members_apply(bad)
        assert ex.value.code == -1
    inf = eng.share_info()
    assert (inf.n_tables, inf.n_members) == (2, 13)
    run(tables)
    # replace a table (other members, other deliverer keys), then remove one
    b = ["5\0z%d\0other%d" % (i, i % 2) for i in range(70)]
    eng.share_members_apply({o_id: b})
    tables[o_id] = (True, b)
    run(tables)
    assert eng.share_info().n_members == 74
    eng.share_members_apply({u_id: []})
    del tables[u_id]
    run(tables)
    assert eng.share_info().n_tables == 1
    with pytest.raises(B.BmqError):
        eng.share_member(u_id, 0)
    # delete the route: its table is unreachable; a route added later gets an id of its own and can get a table
    eng.apply([(1, keys[o_id])])
    run({})
    with pytest.raises(B.BmqError) as ex:
        eng.share_members_apply({o_id: a})
    assert ex.value.code == -1
    new_key = O.route_key_from_mqtt("t", "$oshare/g2/zz")
    eng.apply([(0, new_key)])
    new_id = eng.info().next_route_id - 1
    assert eng.route_key(new_id) == new_key
    eng.share_members_apply({new_id: a})
    pairs.append((0, new_id))
    run({new_id: (True, a)})
    # a new generation of the route index drops every table
    assert eng.share_info().generation == gen0
    eng.compact()
    inf = eng.share_info()
    assert inf.n_tables == 0 and inf.n_members == 0 and inf.generation == eng.info().generation != gen0
    pairs[:] = [(0, i) for i in range(3)]
    run({})
    live = sorted([keys[u_id], keys[n_id], new_key])
    lf = [O.parse_route_key(k)[0] for k in live]
    eng.share_members_apply({lf.index(3): a})
    run({lf.index(3): (True, a)})
    gen1 = eng.share_info().generation
    eng.rebuild(live)
    inf = eng.share_info()
    assert inf.n_tables == 0 and inf.generation == eng.info().generation != gen1
    run({})
    eng.close()


def dk_bytes(route_key_bytes):
    sub, dkey = O.deliverer_key_of(route_key_bytes)
    return str(sub).encode() + b"\0" + dkey.encode()


def submit_ref(keys, flags, rows, senders, tables, nonce):
    """DeliverExecutorGroup.submit for the batch: every topic's normal routes as they are, one member per unordered group route, one per
    (sender, ordered group route) -> {DelivererKey bytes: sorted [(topic, route id, sender index | NONE, member url | None)]}"""
    first = np.concatenate([[0], np.cumsum([len(s) for s in senders])]).tolist()
    out = {}
    for t, r in enumerate(rows):
        for rid in r:
            if flags[rid] == 1:
                out.setdefault(dk_bytes(keys[rid]), []).append((t, rid, R.NONE, None))
            elif flags[rid] == 2:
                url = tables[rid][1][R.pick(nonce, t, rid, len(tables[rid][1]))]
                out.setdefault(R.deliverer_key(url), []).append((t, rid, R.NONE, url.encode()))
            else:
                for k, s in enumerate(senders[t]):
                    url = tables[rid][1][R.rendezvous(s, tables[rid][1])]
                    out.setdefault(R.deliverer_key(url), []).append((t, rid, first[t] + k, url.encode()))
    return {k: sorted(v, key=lambda x: (x[0], x[1], x[2])) for k, v in out.items()}


def merge_deliveries(eng, fan, share, base):
    """the normal groups of Engine.fanout_group and the groups of Engine.share_resolve over its shared slice [base, ...), by DelivererKey"""
    ot, orr, goff, grep, _ = fan
    got = {}
    for g in range(len(goff) - 1):
        if grep[g] >= SHARED:
            continue
        dk = dk_bytes(eng.route_key(int(grep[g])))
        got.setdefault(dk, []).extend((t, rid, R.NONE, None) for t, rid in zip(ot[goff[g]:goff[g + 1]].tolist(), orr[goff[g]:goff[g + 1]].tolist()))
    op, os_, om, sgoff, sp = share
    assert sp == 0
    url = member_url_of(eng)
    for g in range(len(sgoff) - 1):
        for p, s, m in zip(op[sgoff[g]:sgoff[g + 1]].tolist(), os_[sgoff[g]:sgoff[g + 1]].tolist(), om[sgoff[g]:sgoff[g + 1]].tolist()):
            t, rid = int(ot[base + p]), int(orr[base + p])
            u = url(rid, m)
            got.setdefault(R.deliverer_key(u), []).append((t, rid, s, u))
    return {k: sorted(v, key=lambda x: (x[0], x[1], x[2])) for k, v in got.items()}


def test_end_to_end_with_fanout_group():
    eng, keys, flags, tables, rows, senders = build_case(23, counts=[1, 2, 5, 63, 65, 200])
    fan = eng.fanout_group(*_csr(rows))
    ot, orr, goff, grep, special = fan
    assert special == 1 and grep[-1] == SHARED
    lo, hi = int(goff[-2]), int(goff[-1])
    so, sh = R.sender_arrays(senders)
    share = eng.share_resolve(ot[lo:hi], orr[lo:hi], so, sh, nonce=77)
    exp = submit_ref(keys, flags, rows, senders, tables, 77)
    got = merge_deliveries(eng, fan, share, lo)
    assert got == exp
    assert any(any(x[3] is None for x in v) and any(x[3] is not None for x in v) for v in got.values())  # members land beside normal routes
    eng.close()


def test_share_info_mirror_has_the_layout_of_the_header(tmp_path):
    """_lib.ShareInfo restates bmq_share_info: same size, every field at the same offset"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_share_info));']
    lines += ['printf("%s %%zu\\n", offsetof(bmq_share_info, %s));' % (f, f) for f, _ in _lib.ShareInfo._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.ShareInfo)
    for f, _ in _lib.ShareInfo._fields_:
        assert int(got[f]) == getattr(_lib.ShareInfo, f).offset, f
