"""The retain census and the id-based half of RetainStoreCoProc.gc on the device (k_r_census, k_r_remove_ids): the cases of
tests/test_retain_gc_ids.py with the rows of filters against oracle.LevelTrie, one pass of the whole GC recipe, and a removal queued behind a
submitted match batch."""
import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import retain_gc_ref as G

pytestmark = pytest.mark.gpu

FILTERS = ["#", "+/#", "s/+/x", "s/1", "q/3", "$sys/#", "new/+/z", "k/#", "e/+", "a/b/7"]


def _rows(m):
    """rows of '#', '+/#' and literal filters for every tenant against the LevelTrie that saw the same adds and removes"""
    tn = sorted({t for t, _ in m.known})
    ft = [i for i in range(len(tn)) for _ in FILTERS]
    fl = FILTERS * len(tn)
    row, ids = m.eng.retain_match_batch(tn, ft, fl)
    for j, (ti, f) in enumerate(zip(ft, fl)):
        assert ids[row[j]:row[j + 1]].tolist() == sorted(m.lt.match(tn[ti], f)), (tn[ti], f)
    return tn, ft, fl


def test_tenant_counts_and_remove_ids_cases_on_the_device():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        m, h = G.populated(dev), G.populated(host)
        m.check()
        assert dev.retain_tenant_counts() == host.retain_tenant_counts()
        _rows(m)
        gen = dev.retain_info().generation
        for name, ids in G.removal_cases(m):
            want = m.remove_ids(ids)
            assert dev.retain_remove_ids(ids, gen) == want == host.retain_remove_ids(ids, h.eng.retain_info().generation), name
            m.check()
            tn, ft, fl = _rows(m)
            row, kept, _ = dev.retain_match_limited(tn, ft, fl, [10] * len(fl), now_ms=0)
            assert not set(kept.tolist()) & set(ids), name               # match(limit, now) no longer returns them
            assert all(k == b"" for k in dev.retain_message_keys(ids)), name
        back = [k for k, i in m.known.items() if k not in m.ids][:40]
        out = m.apply([(0, t, p) for t, p in back])
        assert out.tolist() == [m.known[k] for k in back]                # re-adding gives the old id
        m.check()
        _rows(m)
        info = dev.retain_info()
        for ids, g, code in (([1], info.generation + 1, -7), ([1, int(info.id_bound)], info.generation, -1)):
            with pytest.raises(B.BmqError) as ei:
                dev.retain_remove_ids(ids, g)
            assert ei.value.code == code
        assert dev.retain_info().epoch == info.epoch
    finally:
        dev.close(), host.close()


def test_removals_between_compact_begin_and_swap_on_the_device():
    dev = B.Engine(device=0)
    try:
        m = G.populated(dev)
        gen = dev.retain_info().generation
        dev.retain_compact_begin()
        ids = sorted(m.ids.values())[10:400:3]
        assert dev.retain_remove_ids(ids + ids[:5], gen) == m.remove_ids(ids) == len(ids)
        dev.retain_compact_build()
        carried, replayed = dev.retain_compact_swap()
        assert replayed == len(ids) and dev.retain_info().n_topics == len(m.ids)
        assert sorted(dev.retain_topics(dev.retain_live_ids())) == sorted(m.ids)
        assert dev.retain_tenant_counts() == m.counts()
    finally:
        dev.close()


def test_one_pass_of_the_gc_recipe_on_20k_topics():
    """retain_expired -> retain_message_keys -> (KV deletes) -> retain_remove_ids -> retain_expired returns nothing"""
    rng = np.random.default_rng(7)
    tn = ["gc-%02d" % t for t in range(20)]
    items = [(tn[i % 20], "d/%d/%d" % (i % 97, i)) for i in range(16000)]
    ts = (rng.integers(1, 1000, len(items)).astype(np.uint64) * 1000) << np.uint64(16)   # HLC: milliseconds << 16
    ex = rng.integers(1, 2000, len(items)).astype(np.uint32)
    dev = B.Engine(device=0)
    try:
        dev.retain_rebuild(tn, [tn.index(t) for t, _ in items], [p for _, p in items], timestamps=ts, expiry=ex)
        add = [("gc-%02d" % (i % 25), "late/%d" % i) for i in range(4000)]             # five tenants that live in the overlay only
        tn2 = sorted({t for t, _ in add})
        ats = (rng.integers(1, 1000, len(add)).astype(np.uint64) * 1000) << np.uint64(16)
        aex = rng.integers(1, 2000, len(add)).astype(np.uint32)
        from bifromq_amd.engine import pack
        dev.retain_apply_batch(tn2, [tn2.index(t) for t, _ in add], None, packed_topics=pack([p for _, p in add]), op_codes=np.zeros(len(add), dtype=np.uint8),
                               timestamps=ats, expiry=aex)
        live = dev.retain_live_ids()
        topics = dict(zip(live, dev.retain_topics(live)))
        at = {i: dev.retain_topic_info(i)[2] for i in live[::50]}
        now = int(np.median([O.retain_expire_at(int(t), int(e)) for t, e in zip(ts.tolist(), ex.tolist())]))
        assert all((at[i] <= now) == (O.retain_expire_at(*dev.retain_topic_info(i)[:2]) <= now) for i in at)
        gen = dev.retain_info().generation
        expired = dev.retain_expired(None, now)
        assert 0.35 * len(live) < len(expired) < 0.65 * len(live)
        keys = dev.retain_message_keys(expired)
        assert keys == [O.retain_message_key(*topics[i]) for i in expired]
        assert dev.retain_remove_ids(expired, gen) == len(expired)
        assert dev.retain_expired(None, now) == []
        left = sorted(set(live) - set(expired))
        assert dev.retain_live_ids() == left and dev.retain_info().n_topics == len(left)
        acc = {}
        for i in left:
            acc[topics[i][0].encode()] = acc.get(topics[i][0].encode(), 0) + 1
        assert dev.retain_tenant_counts() == sorted(acc.items())
        lt = O.LevelTrie(1)
        for i in left:
            lt.add(topics[i][0], topics[i][1], i)
        names = sorted({t for t, _ in topics.values()})
        fl = ["#", "d/+/#", "late/+"]
        ft = [i for i in range(len(names)) for _ in fl]
        row, ids = dev.retain_match_batch(names, ft, fl * len(names))
        for j, ti in enumerate(ft):
            assert ids[row[j]:row[j + 1]].tolist() == sorted(lt.match(names[ti], fl[j % len(fl)])), (names[ti], fl[j % len(fl)])
    finally:
        dev.close()


def test_a_removal_queued_behind_a_submitted_match_batch_leaves_its_rows_as_they_were():
    """bmq_retain_match_batch_dev launches and returns; the removal's kernels go onto the engine stream behind it; bmq_match_finish then
    delivers the rows of the index as it was at the launch.  Device buffers come straight from the HIP runtime the library is linked against."""
    import ctypes as C
    from bifromq_amd.engine import pack
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    bufs = []

    def to_dev(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes + 64) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        bufs.append(p)
        return p

    dev = B.Engine(device=0)
    try:
        m = G.populated(dev)
        tn = ["t0", "t1", "ov"]
        ft = [0, 0, 1, 2, 2]
        fs = ["#", "s/+/x", "#", "#", "q/#"]
        want = [sorted(m.lt.match(tn[t], f)) for t, f in zip(ft, fs)]
        row, got = dev.retain_match_batch(tn, ft, fs)                    # (the engine's scratch has its size now)
        assert [got[row[j]:row[j + 1]].tolist() for j in range(len(ft))] == want
        tdata, toff = pack(tn)
        fdata, foff = pack(fs)
        cap = 4096
        d = [to_dev(np.ascontiguousarray(x)) for x in (np.concatenate([tdata, np.zeros(16, np.uint8)]), toff.astype(np.uint32), np.array(ft, dtype=np.uint32),
                                                        np.concatenate([fdata, np.zeros(16, np.uint8)]), foff.astype(np.uint32))]
        d_row, d_ids, d_tot = to_dev(np.zeros(len(ft) + 1, dtype=np.uint32)), to_dev(np.zeros(cap, dtype=np.uint32)), to_dev(np.zeros(1, dtype=np.uint64))
        gen = dev.retain_info().generation
        ids = sorted(set(sum(want, [])))[::2]
        dev.retain_match_batch_device(d[0].value, d[1].value, len(tn), d[2].value, d[3].value, d[4].value, len(ft), d_row.value, d_ids.value, cap, d_tot.value)
        assert dev.retain_remove_ids(ids, gen) == m.remove_ids(ids) == len(ids)   # queued behind the batch in flight
        total = dev.finish()
        assert total == sum(map(len, want))
        h_row, h_ids = np.zeros(len(ft) + 1, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        assert hip.hipMemcpy(h_row.ctypes.data_as(C.c_void_p), d_row, h_row.nbytes, 2) == 0 and hip.hipMemcpy(h_ids.ctypes.data_as(C.c_void_p), d_ids, h_ids.nbytes, 2) == 0
        assert [h_ids[h_row[j]:h_row[j + 1]].tolist() for j in range(len(ft))] == want       # the rows as they were at the launch
        row, got = dev.retain_match_batch(tn, ft, fs)
        assert [got[row[j]:row[j + 1]].tolist() for j in range(len(ft))] == [sorted(m.lt.match(tn[t], f)) for t, f in zip(ft, fs)]
        assert not set(got.tolist()) & set(ids)
        m.check()
    finally:
        dev.close()
        for p in bufs:
            hip.hipFree(p)


def test_topics_are_found_by_string_after_the_overlay_table_grew_on_the_device():
    """30 k adds below shared levels in one batch leave thousands of never-published nodes on the device; the re-filled edge table must
    not hold them (they carry the labels of the nodes that won, and hide the topics behind those)"""
    dev = B.Engine(device=0)
    try:
        G.growth_case(dev)
    finally:
        dev.close()
