"""retainMessageKey composed on the device (k_r_key_len / k_r_key_write behind bmq_retain_keys_by_id and bmq_retain_keys_match): against the
host executor, against the unchanged host path bmq_retain_message_keys, against bmq_retain_match_limited for rows, ids and counts, and
against the codec for every key; the shapes at which a lane-per-key kernel with byte-granular destinations can go wrong."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from bifromq_amd.engine import pack, retain_message_key
from tests import retain_gc_ref as G
from tests.test_retain_gc_ids_gpu import FILTERS

pytestmark = pytest.mark.gpu

NEVER = 0xFFFFFFFF
HLC_1S = 1000 << 16  # an HLC timestamp whose physical part is 1000 ms


def all_ids(eng):
    return list(range(int(eng.retain_info().id_bound) + 4)) + [NEVER]


def check_match_keys(eng, tn, ft, fl, limits, now_ms):
    """retain_match_keys == retain_match_limited for rows, ids and counts; key_off consistent; every key the codec's"""
    row, ids, counts = eng.retain_match_limited(tn, ft, fl, limits, now_ms=now_ms)
    krow, kids, kcounts, koff, keys = eng.retain_match_keys(tn, ft, fl, limits, now_ms=now_ms)
    assert krow.tolist() == row.tolist() and kids.tolist() == ids.tolist() and kcounts.tolist() == counts.tolist()
    assert len(koff) == len(ids) + 1 and int(koff[0]) == 0 and int(koff[-1]) == len(keys)
    topics = eng.retain_topics(ids)
    for j, i in enumerate(ids.tolist()):
        k = keys[int(koff[j]):int(koff[j + 1])]
        assert k and k == retain_message_key(*topics[j]), (j, i, topics[j])
    return row, ids, keys


def test_device_equals_host_for_every_id():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        m, h = G.populated(dev), G.populated(host)
        name, ids = G.removal_cases(m)[0]                                  # ranks: the same topics in both engines
        want = m.remove_ids(ids)                                           # (the churn removed some of them already)
        assert 0 < want == h.remove_ids(ids)
        assert dev.retain_remove_ids(ids, dev.retain_info().generation) == host.retain_remove_ids(ids, host.retain_info().generation) == want
        gone = [(1, "ov", "q/%d" % i) for i in range(10, 20)]              # overlay topics go by string: their ids differ between the engines
        m.apply(gone), h.apply(gone)
        assert dev.retain_info().id_bound == host.retain_info().id_bound
        dk, hk = dev.retain_keys_by_id(all_ids(dev)), host.retain_keys_by_id(all_ids(host))
        assert dk == dev.retain_message_keys(all_ids(dev))                # bytes and offsets, id for id, dead and out-of-range ids included
        base = int(dev.retain_info().loaded_topics)
        assert dk[:base] == hk[:base] and dk[-5:] == hk[-5:]               # ranks are the same ids in both engines; overlay ids are compared by topic
        assert sorted(dk) == sorted(hk)
        assert {k: dk[i] for k, i in m.ids.items()} == {k: hk[i] for k, i in h.ids.items()} == {k: retain_message_key(*k) for k in m.ids}
        assert sum(1 for k in dk if k) == len(m.ids) and dk[-5:] == [b""] * 5
    finally:
        dev.close(), host.close()


def test_match_keys_against_match_limited_on_both_limit_paths():
    dev = B.Engine(device=0)
    try:
        m = G.populated(dev)
        # every third retained topic gets a stamp that has expired at now_ms = 5000 (ids stay as they are: an add of a retained topic)
        some = sorted(m.ids)[::3]
        tn = sorted({t for t, _ in some})
        out = dev.retain_apply_batch(tn, [tn.index(t) for t, _ in some], [(0, p, HLC_1S, 1) for _, p in some])
        assert out.tolist() == [m.ids[k] for k in some]
        tn = sorted({t for t, _ in m.known})
        ft = [i for i in range(len(tn)) for _ in FILTERS]
        fl = FILTERS * len(tn)
        expired = {m.ids[k] for k in some}
        for lim in (0, 1, 3, 10, 64):
            row, ids, _ = check_match_keys(dev, tn, ft, fl, [lim] * len(fl), 5000)
            assert not set(ids.tolist()) & expired and int(np.diff(row.astype(np.int64)).max()) == lim
        mixed = [(65, 1000, 10, 0, 64, 1)[j % 6] for j in range(len(fl))]
        row, ids, _ = check_match_keys(dev, tn, ft, fl, mixed, 5000)
        assert not set(ids.tolist()) & expired and int(np.diff(row.astype(np.int64)).max()) >= 65
        row0, ids0, _ = check_match_keys(dev, tn, ft, fl, mixed, 0)
        assert set(ids0.tolist()) & expired and len(ids0) > len(ids)      # at now = 0 nothing has expired
    finally:
        dev.close()


def test_shapes_at_which_the_key_kernels_can_go_wrong():
    long_t = "T" * 200
    wave = [("w", "n/%02d" % i) for i in range(65)]
    xs = [("xs", "x" * k) for k in range(1, 49)]
    ends = [("", "a/b"), ("", "c"), (long_t, "a/b"), (long_t, "$d/é")]
    dev = B.Engine(device=0)
    try:
        m = G.Model(dev).load(wave + xs + ends)
        m.apply([(0, "", "ov/1"), (0, long_t, "ov/你/2"), (0, "xs", "x" * 49 + "/" + "x" * 50)])
        # nothing is kept: no filter matches / every limit is 0
        for fl, lim in ((["none/+", "zz"], [10, 10]), (["#", "n/+"], [0, 0]), (["none/#"], [1000])):
            row, ids, counts, koff, keys = dev.retain_match_keys(["w"], [0] * len(fl), fl, lim)
            assert row.tolist() == [0] * (len(fl) + 1) and len(ids) == 0 and koff.tolist() == [0] and keys == b""
        # exactly 1, 63, 64 kept ids (the select path) and 65 (the expand-then-copy path): the edge of a wave
        for lim in (1, 63, 64, 65):
            row, ids, keys = check_match_keys(dev, ["w"], [0], ["n/+"], [lim], 0)
            assert len(ids) == lim and len(keys) == lim * len(retain_message_key("w", "n/00"))
        # key lengths 1 .. 48 back to back: destination offsets take every residue mod 16, lengths cross every copy width
        for lim in (64, 1000):
            row, ids, keys = check_match_keys(dev, ["xs"], [0], ["#"], [lim], 0)
            assert len(ids) == 49 and len(keys) == sum(len(retain_message_key("xs", p)) for (t, p) in m.ids if t == "xs")
        # tenant ids of 0 and of 200 bytes, bulk-loaded and added later
        for t in ("", long_t):
            for lim in (10, 100):
                row, ids, keys = check_match_keys(dev, [t], [0, 0], ["#", "ov/#"], [lim, lim], 0)
                assert len(ids) >= 3
        ids = all_ids(dev)
        assert dev.retain_keys_by_id(ids) == dev.retain_message_keys(ids)
    finally:
        dev.close()


def raw_match_keys(eng, tn, ft, fl, limits, cap, kcap):
    tdata, toff = pack(tn)
    pdata, poff = pack(fl)
    n = len(fl)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ft, lim = np.ascontiguousarray(ft, dtype=np.uint32), np.ascontiguousarray(limits, dtype=np.uint32)
    row, counts, ids, koff, keys = np.zeros(n + 1, np.uint32), np.zeros(n, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap + 1, np.uint64), np.zeros(max(kcap, 1), np.uint8)
    need, kneed = C.c_uint64(), C.c_uint64()
    rc = _lib.lib().bmq_retain_keys_match(eng.h, p(tdata), p(toff), len(tn), p(ft), p(pdata), p(poff), n, p(lim), 0, p(row), p(ids), cap, C.byref(need), p(counts), p(koff), p(keys),
                                          kcap, C.byref(kneed))
    return rc, int(need.value), int(kneed.value), row, ids, koff, keys


def test_key_buffer_growth_on_the_16k_topic_load():
    tn = ["gc-%02d" % t for t in range(20)]
    items = [(tn[i % 20], "d/%d/%d" % (i % 97, i)) for i in range(16000)]
    dev = B.Engine(device=0)
    try:
        dev.retain_rebuild(tn, [tn.index(t) for t, _ in items], [p for _, p in items])
        add = [("gc-%02d" % (i % 25), "late/%d" % i) for i in range(4000)]
        tn2 = sorted({t for t, _ in add})
        dev.retain_apply_batch(tn2, [tn2.index(t) for t, _ in add], [(0, p) for _, p in add])
        rc, need, kneed, *_ = raw_match_keys(dev, tn2, [0], ["d/1/1"], [1], 4, 64)           # a first, small call: the device key buffer is small
        assert rc == 0 and need <= 1
        ft = list(range(len(tn2)))
        rc, need, kneed, row, _, _, _ = raw_match_keys(dev, tn2, ft, ["#"] * len(tn2), [1000] * len(tn2), 20000, 64)
        assert rc == -3 and need == 20000 and kneed > 20000 * 12 and int(row[-1]) == need    # the ids fit, the keys do not: sizes reported
        rc, need2, kneed2, row, ids, koff, keys = raw_match_keys(dev, tn2, ft, ["#"] * len(tn2), [1000] * len(tn2), need, kneed)
        assert rc == 0 and (need2, kneed2) == (need, kneed) and int(koff[need]) == kneed
        want = dev.retain_keys_by_id(ids)
        assert keys.tobytes() == b"".join(want) and np.diff(koff.astype(np.int64)).tolist() == [len(k) for k in want]
        assert want == dev.retain_message_keys(ids) and all(want)
        rc, need3, kneed3, *_ = raw_match_keys(dev, tn2, ft, ["#"] * len(tn2), [1000] * len(tn2), 100, kneed)   # too few ids: both sizes all the same
        assert rc == -3 and (need3, kneed3) == (need, kneed)
    finally:
        dev.close()


def test_keys_follow_mutations_in_stream_order_and_generations():
    dev = B.Engine(device=0)
    try:
        m = G.populated(dev)
        gen = dev.retain_info().generation
        by_string = [("t0", "s/5"), ("ov", "q/7"), ("t1", "new/4/z")]
        ids_a = [m.ids[k] for k in by_string]
        ids_b = [i for i in sorted(m.ids.values())[40:300:9] if i not in ids_a]
        assert all(dev.retain_keys_by_id(ids_a + ids_b))
        m.apply([(1, t, p) for t, p in by_string])                         # removal by string, then by id: the key kernels queue behind both
        assert dev.retain_remove_ids(ids_b, gen) == m.remove_ids(ids_b) == len(ids_b)
        assert dev.retain_keys_by_id(ids_a + ids_b) == [b""] * (len(ids_a) + len(ids_b))
        assert m.apply([(0, t, p) for t, p in by_string]).tolist() == ids_a
        assert dev.retain_keys_by_id(ids_a) == [retain_message_key(*k) for k in by_string]
        # across a compaction: the old generation's keys until the swap, the new one's after it
        dev.retain_compact_begin()
        old = {k: dev.retain_keys_by_id([i])[0] for k, i in m.ids.items()}
        assert old == {k: retain_message_key(*k) for k in m.ids}
        dev.retain_compact_build()
        m.apply([(0, "t2", "after/build")])
        old[("t2", "after/build")] = retain_message_key("t2", "after/build")
        dev.retain_compact_swap()
        assert dev.retain_info().generation == gen + 1
        live = dev.retain_live_ids()
        assert len(live) == len(old) and live[-1] >= int(dev.retain_info().loaded_topics)
        every = all_ids(dev)
        keys = dev.retain_keys_by_id(every)
        assert keys == dev.retain_message_keys(every)
        assert {k: keys[i] for k, i in zip(dev.retain_topics(live), live)} == old
        tn = sorted({t for t, _ in old})
        check_match_keys(dev, tn, list(range(len(tn))), ["#"] * len(tn), [1000] * len(tn), 0)
    finally:
        dev.close()
