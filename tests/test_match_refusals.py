"""What the match entry points of the C ABI answer when they cannot run (no GPU needed): the return code and the bmq_last_error text
of every one of them on a null engine and on a host-only engine, the ticket range check in front of the device check, and the empty
retain batch.  The texts are the library's, literally."""
import ctypes as C

import numpy as np
import pytest

from bifromq_amd import _lib
from bifromq_amd.engine import _ptr

OK, E_INVAL, E_NODEVICE = 0, -1, -2
MAX_TICKETS = 3  # BMQ_MAX_TICKETS
NO_MATCH = b"engine is host-only: matching requires a gfx950 device"
HOST_ONLY = b"engine is host-only"


class _Bufs:
    """one tenant "t", two rows "a/b" and "c": valid arguments for every entry point"""

    def __init__(self):
        self.tenants = np.frombuffer(b"t" + b"\0" * 31, dtype=np.uint8).copy()
        self.tenant_off = np.array([0, 1], dtype=np.uint32)
        self.rows = np.frombuffer(b"a/bc" + b"\0" * 28, dtype=np.uint8).copy()
        self.row_off = np.array([0, 3, 4], dtype=np.uint32)
        self.row_tenant = np.zeros(2, dtype=np.uint32)
        self.limit = np.array([5, 5], dtype=np.uint32)
        self.out_row = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        self.out_ids = np.zeros(64, dtype=np.uint32)
        self.out2 = np.zeros(64, dtype=np.uint32)
        self.out3 = np.zeros(64, dtype=np.uint32)
        self.total = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
        self.need = C.c_uint64(77)
        self.ticket = C.c_int(-5)
        self.info = _lib.RangesInfo()
        self.n_groups, self.special = C.c_uint32(), C.c_uint32()

    def batch(self, n=2):
        return (_ptr(self.tenants), _ptr(self.tenant_off), 1, _ptr(self.row_tenant), _ptr(self.rows), _ptr(self.row_off), n)


def _launchers(L, h, b):
    """(name, call) of the eight entry points that launch a batch"""
    out = (_ptr(b.out_row), _ptr(b.out_ids), len(b.out_ids))
    return [
        ("bmq_match_batch", lambda: L.bmq_match_batch(h, *b.batch(), *out, C.byref(b.need))),
        ("bmq_match_batch_dev", lambda: L.bmq_match_batch_dev(h, *b.batch(), *out, _ptr(b.total))),
        ("bmq_match_submit", lambda: L.bmq_match_submit(h, *b.batch(), C.byref(b.ticket))),
        ("bmq_match_submit_fmt", lambda: L.bmq_match_submit_fmt(h, *b.batch(), 1, C.byref(b.ticket))),
        ("bmq_match_submit_dev", lambda: L.bmq_match_submit_dev(h, *b.batch(), *out, _ptr(b.total), C.byref(b.ticket))),
        ("bmq_retain_match_batch", lambda: L.bmq_retain_match_batch(h, *b.batch(), *out, C.byref(b.need))),
        ("bmq_retain_match_batch_dev", lambda: L.bmq_retain_match_batch_dev(h, *b.batch(), *out, _ptr(b.total))),
        ("bmq_retain_match_limited", lambda: L.bmq_retain_match_limited(h, *b.batch(), _ptr(b.limit), 0, *out, C.byref(b.need), _ptr(b.out2))),
    ]


def _waits(L, h, b, ticket):
    """(name, call) of the five waits on `ticket`"""
    return [
        ("bmq_match_wait", lambda: L.bmq_match_wait(h, ticket, _ptr(b.out_row), _ptr(b.out_ids), len(b.out_ids), C.byref(b.need))),
        ("bmq_match_wait_dev", lambda: L.bmq_match_wait_dev(h, ticket, C.byref(b.need))),
        ("bmq_match_wait_counts", lambda: L.bmq_match_wait_counts(h, ticket, _ptr(b.out_row), C.byref(b.need))),
        ("bmq_match_wait_ranges", lambda: L.bmq_match_wait_ranges(h, ticket, _ptr(b.out_row), _ptr(b.out2), _ptr(b.out_ids), 32, _ptr(b.out3), 64,
                                                                  C.byref(b.info))),
        ("bmq_match_wait_grouped", lambda: L.bmq_match_wait_grouped(h, ticket, _ptr(b.out_ids), _ptr(b.out2), 64, _ptr(b.out_row), _ptr(b.out3), 2,
                                                                    C.byref(b.n_groups), C.byref(b.special), C.byref(b.need))),
    ]


@pytest.fixture()
def host_engine():
    L = _lib.lib()
    cfg = _lib.Config()
    cfg.struct_size = C.sizeof(_lib.Config)
    cfg.device = -1
    h = C.c_void_p()
    assert L.bmq_engine_create(C.byref(cfg), C.byref(h)) == OK
    yield L, h
    L.bmq_engine_destroy(h)


def test_every_entry_point_covered():
    """the lists above are the match entry points of the ABI, all of them"""
    b = _Bufs()
    names = {n for n, _ in _launchers(None, None, b)} | {n for n, _ in _waits(None, None, b, 0)} | {"bmq_match_finish"}
    in_abi = {s for s in _lib.ABI_SYMBOLS if s.startswith(("bmq_match_", "bmq_retain_match_")) and s != "bmq_match_all"}
    assert names == in_abi


def test_null_engine_is_invalid():
    L, b = _lib.lib(), _Bufs()
    calls = _launchers(L, None, b) + _waits(L, None, b, 0) + [("bmq_match_finish", lambda: L.bmq_match_finish(None, C.byref(b.need)))]
    for name, call in calls:
        assert call() == E_INVAL, name
        assert L.bmq_last_error(None) == b"null engine"
    assert b.ticket.value == -5 and b.need.value == 77 and b.out_row[0] == 0xFFFFFFFF  # nothing was written


def test_host_only_engine_cannot_match(host_engine):
    L, h = host_engine
    b = _Bufs()
    assert L.bmq_last_error(h) == b""
    for name, call in _launchers(L, h, b):
        assert call() == E_NODEVICE, name
        assert L.bmq_last_error(h) == NO_MATCH, name
        assert L.bmq_match_finish(h, C.byref(b.need)) == E_NODEVICE, name
        assert L.bmq_last_error(h) == HOST_ONLY, name
    assert b.ticket.value == -5
    for t in range(MAX_TICKETS):
        for name, call in _waits(L, h, b, t):
            L.bmq_match_batch(h, *b.batch(), _ptr(b.out_row), _ptr(b.out_ids), 64, C.byref(b.need))  # (leaves the launchers' text behind)
            assert L.bmq_last_error(h) == NO_MATCH
            assert call() == E_NODEVICE, (name, t)
            assert L.bmq_last_error(h) == HOST_ONLY, (name, t)
    # the device check comes first for the launchers: null buffers and an empty dist batch get the same answer
    assert L.bmq_match_batch(h, None, None, 0, None, None, None, 0, None, None, 0, None) == E_NODEVICE
    assert L.bmq_last_error(h) == NO_MATCH
    assert L.bmq_match_batch_dev(h, None, None, 0, None, None, None, 0, None, None, 0, None) == E_NODEVICE
    assert L.bmq_match_submit_fmt(h, None, None, 0, None, None, None, 0, 99, None) == E_NODEVICE
    assert L.bmq_match_submit_dev(h, None, None, 0, None, None, None, 0, None, None, 0, None, None) == E_NODEVICE
    assert L.bmq_retain_match_batch_dev(h, None, None, 0, None, None, None, 0, None, None, 0, None) == E_NODEVICE
    assert L.bmq_retain_match_batch(h, None, None, 0, None, None, None, 2, None, None, 0, None) == E_NODEVICE
    assert L.bmq_retain_match_limited(h, None, None, 0, None, None, None, 2, None, 0, None, None, 0, None, None) == E_NODEVICE
    assert L.bmq_last_error(h) == NO_MATCH
    assert L.bmq_match_finish(h, None) == E_NODEVICE and L.bmq_last_error(h) == HOST_ONLY


def test_ticket_range_is_checked_before_the_device(host_engine):
    L, h = host_engine
    b = _Bufs()
    assert L.bmq_match_batch(h, *b.batch(), _ptr(b.out_row), _ptr(b.out_ids), 64, C.byref(b.need)) == E_NODEVICE
    for t in (-1, MAX_TICKETS, 1 << 20, -(1 << 31)):
        for name, call in _waits(L, h, b, t):
            assert call() == E_INVAL, (name, t)
            assert L.bmq_last_error(h) == NO_MATCH, (name, t)  # (decided in front of everything that writes a text)
        for name, call in _waits(L, None, b, t):
            assert call() == E_INVAL, (name, t)
    # ... and so are the waits' required pointers
    assert L.bmq_match_wait(h, 0, None, _ptr(b.out_ids), 64, C.byref(b.need)) == E_INVAL
    assert L.bmq_match_wait(h, 0, _ptr(b.out_row), _ptr(b.out_ids), 64, None) == E_INVAL
    assert L.bmq_match_wait_counts(h, 0, None, C.byref(b.need)) == E_INVAL
    assert L.bmq_match_wait_ranges(h, 0, None, None, None, 0, None, 0, C.byref(b.info)) == E_INVAL
    assert L.bmq_match_wait_ranges(h, 0, None, _ptr(b.out2), None, 0, None, 0, None) == E_INVAL
    assert L.bmq_match_wait_grouped(h, 0, None, None, 0, None, None, 0, None, None, C.byref(b.need)) == E_INVAL
    assert L.bmq_match_wait_grouped(h, 0, None, None, 0, _ptr(b.out_row), None, 0, None, None, None) == E_INVAL
    assert L.bmq_match_wait_grouped(h, 0, None, None, 0, _ptr(b.out_row), None, 2, None, None, C.byref(b.need)) == E_INVAL
    assert L.bmq_last_error(h) == NO_MATCH
    # optional pointers left out: the device check answers
    assert L.bmq_match_wait_dev(h, 0, None) == E_NODEVICE and L.bmq_last_error(h) == HOST_ONLY
    assert L.bmq_match_wait_counts(h, 0, _ptr(b.out_row), None) == E_NODEVICE
    assert L.bmq_match_wait_ranges(h, 0, None, _ptr(b.out2), None, 0, None, 0, C.byref(b.info)) == E_NODEVICE
    assert L.bmq_match_wait_grouped(h, 0, None, None, 0, _ptr(b.out_row), None, 0, None, None, C.byref(b.need)) == E_NODEVICE


def test_empty_retain_batch_on_a_host_only_engine(host_engine):
    L, h = host_engine
    for limited in (False, True):
        b = _Bufs()
        before = L.bmq_last_error(h)
        if limited:
            rc = L.bmq_retain_match_limited(h, *b.batch(0), _ptr(b.limit), 0, _ptr(b.out_row), _ptr(b.out_ids), 64, C.byref(b.need), _ptr(b.out2))
        else:
            rc = L.bmq_retain_match_batch(h, *b.batch(0), _ptr(b.out_row), _ptr(b.out_ids), 64, C.byref(b.need))
        assert rc == E_NODEVICE
        assert b.out_row[0] == 0 and b.need.value == 0  # the empty CSR is written all the same
        assert L.bmq_last_error(h) == before  # (the early return leaves the text alone)
        # no output pointers: not the early return, the usual refusal
        if limited:
            rc = L.bmq_retain_match_limited(h, *b.batch(0), _ptr(b.limit), 0, None, None, 0, None, None)
        else:
            rc = L.bmq_retain_match_batch(h, *b.batch(0), None, None, 0, None)
        assert rc == E_NODEVICE and L.bmq_last_error(h) == NO_MATCH
    assert L.bmq_retain_match_batch(None, None, None, 0, None, None, None, 0, None, None, 0, None) == E_INVAL
    assert L.bmq_retain_match_limited(None, None, None, 0, None, None, None, 0, None, 0, None, None, 0, None, None) == E_INVAL
