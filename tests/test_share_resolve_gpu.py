"""Receivers of shared subscriptions on the device: the gfx950 kernels of bifromq_amd/csrc/bmq_share_kernels.h behind bmq_share_resolve /
bmq_share_resolve_dev against tests/share_ref.py and against a host-only engine (the same per-item functions under the other executor).
The cases are those of tests/test_share_resolve.py; the device-resident ones take their pairs from bmq_fanout_group_dev in HBM."""
import ctypes as C
import random

import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import share_ref as R
from tests.test_fanout import SHARED, _csr
from tests.test_share_resolve import build_case, member_url_of, merge_deliveries, shared_pairs, submit_ref

pytestmark = pytest.mark.gpu


class Hbm:
    """plain device buffers for the *_dev entry points"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), a.nbytes + 64) == 0
        if a.nbytes:
            assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        self.bufs.append(p)
        return p.value

    def zeros(self, n):
        return self.put(np.zeros(max(n, 1), dtype=np.uint32))

    def get(self, p, n, dtype=np.uint32):
        out = np.zeros(n, dtype=dtype)
        if n:
            assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)
        self.bufs = []


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def device_resolve(eng, mem, rows, senders, nonce, gcap=1024):
    """match CSR -> bmq_fanout_group_dev -> its 0xFFFFFFFE slice, left in HBM -> bmq_share_resolve_dev (a call with too-small buffers first: it
    reports both counts) -> (the slice's pairs, the rows, the fan-out result, where the slice begins)"""
    row, ids = _csr(rows)
    n, total = len(rows), int(row[-1])
    d_row, d_ids = mem.put(row), mem.put(ids)
    d_ot, d_or, d_goff, d_grep = mem.zeros(total), mem.zeros(total), mem.zeros(gcap + 1), mem.zeros(gcap)
    ng, sp = eng.fanout_group_device(d_row, d_ids, n, total, d_ot, d_or, d_goff, d_grep, gcap)
    fan = (mem.get(d_ot, total), mem.get(d_or, total), mem.get(d_goff, ng + 1), mem.get(d_grep, ng), sp)
    assert sp & 1
    g = fan[3].tolist().index(SHARED)
    lo, hi = int(fan[2][g]), int(fan[2][g + 1])
    so, sh = R.sender_arrays(senders)
    d_so, d_sh = mem.put(so), mem.put(sh)
    row_cap = (hi - lo) * (max(len(x) for x in senders) + 1)
    d_op, d_os, d_om, d_sgoff = mem.zeros(row_cap), mem.zeros(row_cap), mem.zeros(row_cap), mem.zeros(gcap + 1)
    a = (d_ot + 4 * lo, d_or + 4 * lo, hi - lo, d_so, d_sh, n, len(sh), nonce, d_op, d_os, d_om)
    with pytest.raises(B.BmqError) as ex:
        eng.share_resolve_device(*a, 2, d_sgoff, 1)
    assert ex.value.code == -3
    nr, nsg, ssp = eng.share_resolve_device(*a, row_cap, d_sgoff, gcap)
    assert ex.value.needed == (nr, nsg)
    share = (mem.get(d_op, nr), mem.get(d_os, nr), mem.get(d_om, nr), mem.get(d_sgoff, nsg + 1), ssp)
    pairs = list(zip(fan[0][lo:hi].tolist(), fan[1][lo:hi].tolist()))
    return pairs, share, fan, lo


def test_gpu_ordered_and_unordered_equal_reference_and_host_engine():
    eng, keys, flags, tables, rows, senders = build_case(31, device=0)
    host, *_ = build_case(31, device=-1)
    assert {len(u) for _, u in tables.values()} == set(R.MEMBER_COUNTS)
    so, sh = R.sender_arrays(senders)
    mem = Hbm()
    picks = []
    for nonce in (5, 0xDEADBEEFCAFEF00D):
        pairs, res, _, _ = device_resolve(eng, mem, rows, senders, nonce)
        assert sorted(pairs) == sorted(shared_pairs(rows, flags)) and len(pairs) > 200
        assert R.check_rows(member_url_of(eng), pairs, senders, tables, nonce, res) > 10
        assert same(res, host.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=nonce))  # same functions, two executors
        picks.append([m for p, s, m in sorted(zip(res[0].tolist(), res[1].tolist(), res[2].tolist())) if s == R.NONE])
        assert picks[-1] == [R.pick(nonce, t, rid, len(tables[rid][1])) for t, rid in pairs if not tables[rid][0]]
    assert picks[0] != picks[1]
    # the signed comparison matters on this input
    op, os_, om, _, _ = res
    differ = sum(m != R.rendezvous(int(sh[s]), tables[pairs[p][1]][1], signed=False) for p, s, m in zip(op.tolist(), os_.tolist(), om.tolist()) if s != R.NONE)
    assert differ > 0
    # the host-buffer entry point stages the same arrays: the same rows
    assert same(res, eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=nonce, row_cap=3, group_cap=1))
    mem.free()
    host.close()
    eng.close()


@pytest.mark.parametrize("counts", [[1, 2, 3, 5, 8, 9, 17], [2, 9, 16, 17, 33, 40]])
def test_gpu_small_tables_share_a_wave(counts):
    """mean scores per row that make the resolve kernel pack 8 / 4 rows into a wave (8- / 16-lane sub-groups), tables larger than a sub-group included"""
    eng, keys, flags, tables, rows, senders = build_case(32, device=0, counts=counts)
    host, *_ = build_case(32, device=-1, counts=counts)
    so, sh = R.sender_arrays(senders)
    mem = Hbm()
    pairs, res, _, _ = device_resolve(eng, mem, rows, senders, 8)
    assert R.check_rows(member_url_of(eng), pairs, senders, tables, 8, res) > 10
    assert same(res, host.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=8))
    mem.free()
    host.close()
    eng.close()


def test_gpu_grouping_by_deliverer_key():
    key = O.route_key_from_mqtt("t", "$oshare/g/a")
    eng = B.Engine(device=0).rebuild([key])
    urls = ["1\0inboxA\0k", "1\0inboxB\0k", "1\0c\0" + "2x", "12\0c\0x"]
    eng.share_members_apply({0: urls})
    rnd = random.Random(4)
    senders = [[rnd.randint(R.INT_MIN, R.INT_MAX) for _ in range(5)] for _ in range(40)]
    mem = Hbm()
    pairs, res, _, _ = device_resolve(eng, mem, [[0]] * 40, senders, 0)
    assert pairs == [(t, 0) for t in range(40)]
    assert R.check_rows(member_url_of(eng), pairs, senders, {0: (True, urls)}, 0, res) == 3
    op, os_, om, goff, sp = res
    group_of = {}
    for g in range(len(goff) - 1):
        for m in set(om[goff[g]:goff[g + 1]].tolist()):
            assert m not in group_of
            group_of[m] = g
    assert set(group_of) == {0, 1, 2, 3} and group_of[0] == group_of[1] and group_of[2] != group_of[3] and sp == 0
    # a pair whose route id was never handed out joins as the last, unresolved group
    so, sh = R.sender_arrays(senders)
    pairs2 = pairs + [(3, 7)]
    res2 = eng.share_resolve([p[0] for p in pairs2], [p[1] for p in pairs2], so, sh, nonce=0)
    assert R.check_rows(member_url_of(eng), pairs2, senders, {0: (True, urls)}, 0, res2) == 3 and res2[4] == 1 and res2[2][-1] == R.NONE
    mem.free()
    eng.close()


def test_gpu_end_to_end_device_resident():
    """match CSR -> bmq_fanout_group_dev -> its 0xFFFFFFFE slice, still in HBM -> bmq_share_resolve_dev; normal and share groups merged by DelivererKey"""
    eng, keys, flags, tables, rows, senders = build_case(33, device=0, counts=[1, 2, 5, 63, 65, 200])
    host, *_ = build_case(33, device=-1, counts=[1, 2, 5, 63, 65, 200])
    mem = Hbm()
    pairs, share, fan, lo = device_resolve(eng, mem, rows, senders, 77)
    assert merge_deliveries(eng, fan, share, lo) == submit_ref(keys, flags, rows, senders, tables, 77)
    so, sh = R.sender_arrays(senders)
    assert same(share, host.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=77))
    mem.free()
    host.close()
    eng.close()


def test_gpu_large_case_against_host_engine():
    """more than 200 000 (pair, sender) items over tables of up to 200 members: every row against the host-only engine, a seeded sample of
    5 000 rows against the restatement"""
    rnd = random.Random(35)
    n_groups, n_topics, n_pairs = 1500, 40000, 110000
    keys = sorted(O.route_key_from_mqtt("t", "$%sshare/g%d/f/%d" % ("o" if i % 5 else "", i % 7, i)) for i in range(n_groups))
    flags = [O.parse_route_key(k)[0] for k in keys]
    tables = {rid: (flags[rid] == 3, R.member_list(rnd, rnd.choice([1, 2, 3, 5, 8, 20, 64, 65, 130, 200]), brokers=(0, 1, 2, 3), dkeys=40)) for rid in range(n_groups)}
    senders = [[rnd.randint(R.INT_MIN, R.INT_MAX) for _ in range(rnd.randint(1, 4))] for _ in range(n_topics)]
    pt = np.sort(np.array([rnd.randrange(n_topics) for _ in range(n_pairs)], dtype=np.uint32))
    pr = np.array([rnd.randrange(n_groups + 3) for _ in range(n_pairs)], dtype=np.uint32)  # (a few ids beyond the index: unresolved)
    so, sh = R.sender_arrays(senders)
    res = []
    for device in (0, -1):
        eng = B.Engine(device=device).rebuild(keys)
        eng.share_members_apply({rid: urls for rid, (_, urls) in tables.items()})
        if device == 0:
            mem = Hbm()
            d = [mem.put(a) for a in (pt, pr, so, sh)]
            row_cap, gcap = 4 * n_pairs, 1024
            o = [mem.zeros(row_cap) for _ in range(3)] + [mem.zeros(gcap + 1)]
            nr, ng, sp = eng.share_resolve_device(d[0], d[1], n_pairs, d[2], d[3], n_topics, len(sh), 99, o[0], o[1], o[2], row_cap, o[3], gcap)
            res.append((mem.get(o[0], nr), mem.get(o[1], nr), mem.get(o[2], nr), mem.get(o[3], ng + 1), sp))
            mem.free()
        else:
            res.append(eng.share_resolve(pt, pr, so, sh, nonce=99))
        eng.close()
    gpu, host = res
    assert len(gpu[0]) >= 200000 and gpu[4] == 1
    assert same(gpu, host)
    op, os_, om, goff, _ = gpu
    for r in random.Random(36).sample(range(len(op)), 5000):
        t, rid = int(pt[op[r]]), int(pr[op[r]])
        if rid not in tables:
            assert om[r] == R.NONE and os_[r] == R.NONE
        elif tables[rid][0]:
            assert so[t] <= os_[r] < so[t + 1] and om[r] == R.rendezvous(int(sh[os_[r]]), tables[rid][1])
        else:
            assert os_[r] == R.NONE and om[r] == R.pick(99, t, rid, len(tables[rid][1]))
    # rows of one group share one share-deliverer; groups are in (pair, sender) order
    for g in range(len(goff) - 1):
        seg = slice(int(goff[g]), int(goff[g + 1]))
        order = op[seg].astype(np.int64) * (1 << 32) + os_[seg]
        assert (np.diff(order) > 0).all()
