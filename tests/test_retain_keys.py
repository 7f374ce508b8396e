"""retainMessageKey composed by the per-item key functions (bmq_retain_keys_prepare / bmq_retain_keys_by_id) over the host executor
(device = -1: the functions the key kernels run, on host threads, over a string store in host memory).  The unchanged host path
bmq_retain_message_keys and the codec's retain_message_key are the references; host engines do not match, so bmq_retain_keys_match is
compared on the device (tests/test_retain_keys_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from bifromq_amd.engine import retain_message_key
from tests import retain_gc_ref as G

NEVER = 0xFFFFFFFF
TENANT = "ten-é"
SPECIAL = [b"/", b"a/", b"/a", b"a//b", b"$sys/x", "é/x".encode(), "x/你好/y".encode(), "\U0001F604".encode(), "s/\U0001F604é/你".encode(),
           b"cut/\xe4\xbd", b"\xf0\x9f\x98/z", b"\xc3", b"lone/\xa0\xa0/x", b"t" * 255, b"/".join(b"l%d" % i for i in range(40))]


def check_all_ids(eng, m):
    """every id of the generation, a few behind it and 0xFFFFFFFF: the device-side composer == the host path; live ids == the codec"""
    bound = int(eng.retain_info().id_bound)
    ids = list(range(bound + 4)) + [NEVER]
    got = eng.retain_keys_by_id(ids)
    assert got == eng.retain_message_keys(ids)
    live = sorted(m.ids.values())
    by_id = dict(zip(live, eng.retain_topics(live)))
    for i in ids:
        assert got[i if i != NEVER else -1] == (retain_message_key(*by_id[i]) if i in by_id else b""), i
    return got


def test_every_id_of_the_churned_model():
    eng = B.Engine(device=-1)
    try:
        m = G.populated(eng)
        base, bound = int(eng.retain_info().loaded_topics), int(eng.retain_info().id_bound)
        live = set(m.ids.values())
        kinds = {(i < base, i in live) for i in range(bound)}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}   # bulk-loaded / overlay ids, retained / removed
        got = check_all_ids(eng, m)
        # a topic removed and retained again: the same id, and its key is back
        for t, p in (("t0", "s/1"), ("ov", "q/3")):
            i = m.known[(t, p)]
            assert got[i] == retain_message_key(t, p)
            m.apply([(1, t, p)])
            assert eng.retain_keys_by_id([i]) == [b""]
            assert m.apply([(0, t, p)]).tolist() == [i]
            assert eng.retain_keys_by_id([i]) == [retain_message_key(t, p)]
        for name, ids in G.removal_cases(m):
            m.remove_ids(ids)
            eng.retain_remove_ids(ids, eng.retain_info().generation)
            assert all(k == b"" for k in eng.retain_keys_by_id(ids)), name
        check_all_ids(eng, m)
    finally:
        eng.close()


@pytest.mark.parametrize("where", ["bulk", "overlay"])
def test_special_topics(where):
    eng = B.Engine(device=-1)
    try:
        if where == "bulk":
            eng.retain_rebuild([TENANT, ""], [0] * len(SPECIAL) + [1], SPECIAL + [b"a/b"])
        else:
            eng.retain_rebuild(["other"], [0], ["a/b"])
        # an add of a retained topic reports its id (a bulk-loaded rank in the first case, a fresh overlay id in the second)
        ids = eng.retain_apply_batch([TENANT, ""], [0] * len(SPECIAL) + [1], [(0, p) for p in SPECIAL + [b"a/b"]]).tolist()
        base = int(eng.retain_info().loaded_topics)
        assert len(set(ids)) == len(ids) and all((i < base) == (where == "bulk") for i in ids)
        want = [retain_message_key(TENANT, p) for p in SPECIAL] + [retain_message_key("", "a/b")]
        assert eng.retain_keys_by_id(ids) == want == eng.retain_message_keys(ids)
        assert eng.retain_keys_by_id(ids[::-1] + ids) == want[::-1] + want                 # any order, repeats
        k = want[SPECIAL.index(b"a//b")]
        t = TENANT.encode()
        assert k == b"\0" + len(t).to_bytes(2, "big") + t + b"\0\3" + k[5 + len(t):8 + len(t)] + b"a\0\0b"
        assert want[-1][:5] == b"\0\0\0\0\2"                                                # the empty tenant id
    finally:
        eng.close()


def raw_keys_by_id(eng, ids, cap):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    off = np.full(len(ids) + 1, 0xDEAD, dtype=np.uint64)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    rc = _lib.lib().bmq_retain_keys_by_id(eng.h, ids.ctypes.data_as(C.c_void_p) if len(ids) else None, len(ids), out.ctypes.data_as(C.c_void_p) if cap else None, cap,
                                          off.ctypes.data_as(C.c_void_p))
    return rc, off, out


def test_buffer_protocol():
    eng = B.Engine(device=-1)
    try:
        rc, off, _ = raw_keys_by_id(eng, [0, 1], 64)                       # no index: empty keys, as bmq_retain_message_keys answers
        assert rc == 0 and off.tolist() == [0, 0, 0]
        m = G.populated(eng)
        ids = sorted(m.ids.values())[::7] + [NEVER, 3]
        want = eng.retain_message_keys(ids)
        need = sum(map(len, want))
        for cap in (0, need - 1):
            rc, off, _ = raw_keys_by_id(eng, ids, cap)
            assert rc == -3 and int(off[len(ids)]) == need                 # BMQ_E_NOSPACE, the offsets are written
            assert np.diff(off.astype(np.int64)).tolist() == [len(k) for k in want]
        rc, off, out = raw_keys_by_id(eng, ids, need)
        assert rc == 0 and out.tobytes() == b"".join(want)
        rc, off, _ = raw_keys_by_id(eng, [], 16)
        assert rc == 0 and off.tolist() == [0]
        assert eng.retain_keys_by_id([]) == []
        assert _lib.lib().bmq_retain_keys_by_id(eng.h, None, 2, None, 0, off.ctypes.data_as(C.c_void_p)) == -1
    finally:
        eng.close()


def test_generations():
    eng = B.Engine(device=-1)
    try:
        with pytest.raises(B.BmqError) as ei:
            eng.retain_keys_prepare()                                      # no index is loaded: refused, and nothing changes
        assert ei.value.code == -7
        info = eng.retain_info()
        assert (info.generation, info.epoch, info.n_topics) == (0, 0, 0) and eng.retain_keys_by_id([0]) == [b""]
        m = G.populated(eng)
        info = eng.retain_info()
        size = eng.retain_keys_prepare()
        assert size > sum(len(p) for t, p in G.bulk_items()) and eng.retain_keys_prepare() == size
        assert (eng.retain_info().generation, eng.retain_info().epoch) == (info.generation, info.epoch)
        check_all_ids(eng, m)                                              # before the compaction
        eng.retain_compact_begin()
        check_all_ids(eng, m)
        m.apply([(0, "t0", "mid/compaction"), (1, "t1", "s/5")])
        eng.retain_compact_build()
        check_all_ids(eng, m)                                              # between begin and swap: still the old generation's ids
        old = {k: eng.retain_keys_by_id([i])[0] for k, i in m.ids.items()}
        eng.retain_compact_swap()
        assert eng.retain_info().generation == info.generation + 1
        live = eng.retain_live_ids()
        after = eng.retain_info()
        assert len(live) == len(m.ids) and after.loaded_removed == 1 and after.added_ids == 1   # new ids: ranks again, then the replayed log
        topics = eng.retain_topics(live)
        every = list(range(int(after.id_bound) + 2))
        keys = eng.retain_keys_by_id(every)                                # (the store is rebuilt on this first use)
        assert keys == eng.retain_message_keys(every) and [i for i in every if keys[i]] == live
        assert {k: keys[i] for k, i in zip(topics, live)} == old
        assert eng.retain_keys_prepare() != size                           # another load, another store
        # a rebuild of a different load
        eng.retain_rebuild(["zz"], [0, 0, 0], ["only/one", "two", "x/y/z"])
        assert eng.retain_keys_by_id([0, 1, 2, 3]) == [retain_message_key("zz", p) for p in ("only/one", "two", "x/y/z")] + [b""]
        small = eng.retain_keys_prepare()
        assert 0 < small < size and eng.retain_keys_prepare() == small
        eng.retain_rebuild([], [], [])                                     # an empty load has an (empty) store too
        assert eng.retain_keys_prepare() == eng.retain_keys_prepare() and eng.retain_keys_by_id([0]) == [b""]
        assert eng.retain_apply_batch(["n"], [0], [(0, "fresh")]).tolist() == [0]
        assert eng.retain_keys_by_id([0, 1]) == [retain_message_key("n", "fresh"), b""]
    finally:
        eng.close()
