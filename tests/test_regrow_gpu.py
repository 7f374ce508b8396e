"""The id buffer a fresh batch slot starts with is a guess; a batch that needs more tells the size, the buffer grows and the batch is
launched again.  Every entry point that does so, on shapes whose first guess is too small, against the oracle.

Dist: one tenant, 64 normal routes on "#" with 64 receivers, 256 distinct topics -> 64 ids per row, 16384 in all: more than the 6144
a ticket's slot starts with (24 per topic) and the 1024 of the blocking call (4 per topic, at least 1024).
Retain: one tenant, 2048 retained topics, 64 filters "#" -> 131072 ids: more than the 1024 the slot starts with (16 per filter)."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd.engine import _ptr, pack, pinned
from oracle import oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

E_NOSPACE = -3
N_ROUTES, N_TOPICS = 64, 256
N_RETAINED, N_FILTERS = 2048, 64


def first_guess(n_rows, ids_per_row):
    """ids the id buffer of a fresh slot holds: ids_per_row per row -- 4 for bmq_match_batch, 24 for a ticket, 16 for the retain calls
    (stage_input's callers, bifromq_amd/csrc) -- and at least 1024.  A total above it cannot be answered without growing the buffer and
    launching again: every test below asserts that of its own shape, so that a larger first guess fails here instead of quietly leaving
    the regrow path unrun."""
    return max(n_rows * ids_per_row, 1024)


class _Dist:
    def __init__(self):
        self.keys = sorted(B.route_key_from_mqtt("t", "#", O.receiver_url(j % 3, "inbox%d" % j, "d%d" % (j % 5))) for j in range(N_ROUTES))
        self.topics = ["s%d/x/%d" % (i % 7, i) for i in range(N_TOPICS)]
        assert len(set(self.keys)) == N_ROUTES and len(set(self.topics)) == N_TOPICS
        tdata, toff = pack(["t"])
        pdata, poff = pack(self.topics)
        self.tdata, self.toff = pinned(len(tdata) + 32, np.uint8), pinned(len(toff), np.uint32)
        self.pdata, self.poff, self.tt = pinned(len(pdata) + 32, np.uint8), pinned(len(poff), np.uint32), pinned(N_TOPICS, np.uint32)
        self.tdata[:], self.pdata[:], self.tt[:] = 0, 0, 0
        self.tdata[:len(tdata)], self.toff[:], self.pdata[:len(pdata)], self.poff[:] = tdata, toff, pdata, poff
        # the oracle's rows, once: ranks of the matching keys = the ids after a rebuild
        self.rows = [sorted(r) for r in O.KV(self.keys).match_bruteforce("t", self.topics).per_topic()]
        assert all(r == list(range(N_ROUTES)) for r in self.rows)
        self.total = N_ROUTES * N_TOPICS
        self.erow = np.arange(N_TOPICS + 1, dtype=np.uint32) * N_ROUTES

    def batch(self):
        return (_ptr(self.tdata), _ptr(self.toff), 1, _ptr(self.tt), _ptr(self.pdata), _ptr(self.poff), N_TOPICS)

    def engine(self):
        return B.Engine(device=0).rebuild(self.keys)

    def check(self, row, ids):
        assert np.array_equal(row, self.erow)
        assert U.csr_rows(row, ids[:self.total]) == self.rows


@pytest.fixture(scope="module")
def dist():
    return _Dist()


def test_blocking_match_batch(dist):
    eng, L = dist.engine(), B._lib.lib()
    assert dist.total > first_guess(N_TOPICS, 4)
    try:
        for _ in range(2):  # the second call finds the buffer grown
            row, ids, need = np.zeros(N_TOPICS + 1, dtype=np.uint32), np.zeros(dist.total, dtype=np.uint32), C.c_uint64()
            assert L.bmq_match_batch(eng.h, *dist.batch(), _ptr(row), _ptr(ids), dist.total, C.byref(need)) == 0
            assert need.value == dist.total
            dist.check(row, ids)
        # a caller's buffer that is too small stays the caller's problem: the size, no ids
        ids = np.full(100, 0xFFFFFFFF, dtype=np.uint32)
        assert L.bmq_match_batch(eng.h, *dist.batch(), _ptr(row), _ptr(ids), 100, C.byref(need)) == E_NOSPACE
        assert need.value == dist.total and (ids == 0xFFFFFFFF).all()
    finally:
        eng.close()


def test_submit_and_wait(dist):
    eng = dist.engine()
    assert dist.total > first_guess(N_TOPICS, 24)
    try:
        for _ in range(2):
            t = eng.match_submit(dist.tdata, dist.toff, 1, dist.tt, dist.pdata, dist.poff, N_TOPICS)
            row, ids = pinned(N_TOPICS + 1, np.uint32), pinned(dist.total, np.uint32)
            assert eng.match_wait(t, row, ids) == dist.total
            dist.check(row, ids)
    finally:
        eng.close()


def test_submit_grouped_and_wait(dist):
    eng = dist.engine()
    assert dist.total > first_guess(N_TOPICS, 24)
    try:
        for _ in range(2):
            t = eng.match_submit_fmt(dist.tdata, dist.toff, 1, dist.tt, dist.pdata, dist.poff, N_TOPICS, eng.FMT_GROUPED)
            ot, orr = pinned(dist.total, np.uint32), pinned(dist.total, np.uint32)
            goff, grep = pinned(N_ROUTES + 2, np.uint32), pinned(N_ROUTES + 1, np.uint32)
            total, ng, _special = eng.match_wait_grouped(t, ot, orr, goff, grep)
            assert total == dist.total and 0 < ng <= N_ROUTES
            # the pairs of the IDS result, as a multiset
            want = sorted((i, r) for i, rw in enumerate(dist.rows) for r in rw)
            assert sorted(zip(ot[:total].tolist(), orr[:total].tolist())) == want
    finally:
        eng.close()


def test_submit_dev_and_wait_dev(dist):
    eng, L = dist.engine(), B._lib.lib()
    try:
        row, ids, tot = pinned(N_TOPICS + 1, np.uint32), pinned(dist.total, np.uint32), pinned(1, np.uint64)
        for _ in range(2):
            row[:], ids[:], tot[:] = 0, 0xFFFFFFFF, 0
            t, need = C.c_int(), C.c_uint64()
            assert L.bmq_match_submit_dev(eng.h, *dist.batch(), _ptr(row), _ptr(ids), dist.total, _ptr(tot), C.byref(t)) == 0
            assert L.bmq_match_wait_dev(eng.h, t.value, C.byref(need)) == 0
            assert need.value == dist.total == int(tot[0])
            dist.check(row, ids)
        # the caller's buffer is the caller's: too small is NOSPACE with the size, nothing grows, the row pointers are there
        row[:], ids[:] = 0, 0xFFFFFFFF
        assert L.bmq_match_submit_dev(eng.h, *dist.batch(), _ptr(row), _ptr(ids), 100, _ptr(tot), C.byref(t)) == 0
        assert L.bmq_match_wait_dev(eng.h, t.value, C.byref(need)) == E_NOSPACE
        assert need.value == dist.total and np.array_equal(row, dist.erow) and (ids[100:] == 0xFFFFFFFF).all()  # (nothing past the capacity)
        assert L.bmq_match_wait_dev(eng.h, t.value, C.byref(need)) == -7  # released
    finally:
        eng.close()


class _Retain:
    def __init__(self):
        topics = ["r%d/%d" % (i % 11, i) for i in range(N_RETAINED)]
        self.topics = topics
        order = U.retain_order(["t"], [0] * N_RETAINED, topics)  # ids = ranks, independent of the engine
        assert len(order) == N_RETAINED
        lt = O.LevelTrie(1)
        for i, (tn, tp) in enumerate(order):
            lt.add(tn, tp, i)
        self.lt = lt
        self.full = sorted(lt.match("t", "#"))
        assert self.full == list(range(N_RETAINED))
        self.filters = ["#"] * N_FILTERS
        self.total = N_RETAINED * N_FILTERS

    def engine(self):
        return B.Engine(device=0).retain_rebuild(["t"], [0] * N_RETAINED, self.topics)

    def limited(self, limit):
        return [O.retain_store_match(self.lt, "t", "#", limit, 0, lambda i: 1 << 62) for _ in self.filters]


@pytest.fixture(scope="module")
def retain():
    return _Retain()


def test_retain_match_batch(retain):
    eng, L = retain.engine(), B._lib.lib()
    try:
        tdata, toff = pack(["t"])
        fdata, foff = pack(retain.filters)
        ft = np.zeros(N_FILTERS, dtype=np.uint32)
        assert retain.total > first_guess(N_FILTERS, 16)
        for _ in range(2):
            row, ids, need = np.zeros(N_FILTERS + 1, dtype=np.uint32), np.zeros(retain.total, dtype=np.uint32), C.c_uint64()
            assert L.bmq_retain_match_batch(eng.h, _ptr(tdata), _ptr(toff), 1, _ptr(ft), _ptr(fdata), _ptr(foff), N_FILTERS, _ptr(row), _ptr(ids),
                                            retain.total, C.byref(need)) == 0
            assert need.value == retain.total
            assert U.csr_rows(row, ids) == [retain.full] * N_FILTERS
    finally:
        eng.close()


@pytest.mark.parametrize("limit", [3000, 10])  # the complete CSR first (limits above 64) | picked from the matched ranges
def test_retain_match_limited(retain, limit):
    eng = retain.engine()
    try:
        exp = retain.limited(limit)
        assert retain.total > first_guess(N_FILTERS, 16)  # (limit 3000 goes through the complete CSR: the slot's own buffer grows)
        assert len(exp[0]) == min(limit, N_RETAINED)
        for _ in range(2):
            row, ids, counts = eng.retain_match_limited(["t"], [0] * N_FILTERS, retain.filters, [limit] * N_FILTERS, now_ms=0)
            assert counts.tolist() == [N_RETAINED] * N_FILTERS
            assert U.csr_rows(row, ids) == exp
    finally:
        eng.close()
