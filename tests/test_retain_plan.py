"""bmq_retain_plan / bmq_retain_plan_commit over the host executor (device = -1: the per-item functions of bmq_rplan_core.h that the plan
kernels run, on host threads): every output against the rule of tests/retain_plan_ref.py, every key against the codec's retain_message_key.
Host engines do not match, so the "a fixed retain_match_batch answers the same before and after a plan" half of the read-only check runs on
the device (tests/test_retain_plan_gpu.py); here the index's counters, its live ids and their keys stand for it."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from bifromq_amd.engine import retain_message_key
from tests import retain_plan_cases as K
from tests import retain_plan_ref as R


@pytest.fixture(scope="module")
def index():
    eng = B.Engine(device=-1)
    present, known = K.build_index(eng)
    yield eng, present, known
    eng.close()


def info_tuple(eng):
    i = eng.retain_info()
    return tuple(getattr(i, f) for f, _ in i._fields_)


def test_index_states_and_duplicates(index):
    eng, present, known = index
    K.assert_states(eng, present, known)
    seen_actions, seen_codes = set(), set()
    for clear in (0, 1):
        got, want = K.run_and_check(eng, present, *K.state_batch(clear), where="states clear=%d" % clear)
        seen_actions |= set(want["action"])
        seen_codes |= set(want["code"])
        assert R.SUPERSEDED not in want["action"]                       # every key once: every op is its own winner
    tenants, ot, ops = K.duplicate_batch()
    got, want = K.run_and_check(eng, present, tenants, ot, ops, where="duplicates")
    a, w = want["action"], want["winner"]
    assert (a[0], a[1], a[2], a[3]) == (R.SUPERSEDED, R.REMOVE, R.SUPERSEDED, R.NONE)
    assert (a[4], a[5], a[6], a[7]) == (R.SUPERSEDED, R.UPDATE, R.SUPERSEDED, R.ADD)
    assert (a[8], a[9], a[10]) == (R.UPDATE, R.REMOVE, R.ADD)           # one topic, three tenants, three groups
    assert (a[12], a[13], w[12]) == (R.SUPERSEDED, R.REMOVE, 13) and (want["delta"][4], a[15]) == (-1, R.ADD)
    assert w[64:128] == [127] * 64 and a[127] == R.UPDATE and want["code"][64:128] == [R.RETAINED] * 64
    assert [w[64 * k + 5] for k in (2, 3, 4)] == [261] * 3 and a[261] == R.UPDATE
    seen_actions |= set(a)
    seen_codes |= set(want["code"])
    assert seen_actions == {R.NONE, R.ADD, R.UPDATE, R.REMOVE, R.SUPERSEDED} and seen_codes == {R.RETAINED, R.CLEARED}
    for i, k in enumerate(got.keys):                                    # the keys are the codec's, and only winners that write have one
        t = tenants[ot[i]]
        assert k == (retain_message_key(t, ops[i][0]) if a[i] in (R.ADD, R.UPDATE, R.REMOVE) else b"")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_batch_sizes(index, n):
    eng, present, known = index
    before = info_tuple(eng)
    tenants, ot, ops = K.random_batch(present, known, n, seed=n)
    got, want = K.run_and_check(eng, present, tenants, ot, ops, where="n=%d" % n)
    if n >= 257:
        assert want["action"].count(R.SUPERSEDED) > n // 8 and len(set(want["action"])) == 5
    assert got.info.generation == before[-1] and got.info.epoch == before[-2]
    assert info_tuple(eng) == before
    if n:                                                               # op_tenant NULL: every op belongs to tenant 0
        one = [tenants[ot[0]]]
        K.run_and_check(eng, present, one, None, ops, where="n=%d, tenant 0" % n)


def test_read_only(index):
    eng, present, known = index
    before = info_tuple(eng)
    live = eng.retain_live_ids()
    keys = eng.retain_keys_by_id(live)
    counts = eng.retain_tenant_counts()
    for clear in (0, 1):
        K.run_and_check(eng, present, *K.state_batch(clear), where="read-only")
    K.run_and_check(eng, present, *K.random_batch(present, known, 3000, seed=11), where="read-only")
    assert info_tuple(eng) == before                                    # epoch, id_bound, added_ids, overlay_nodes: nothing was created
    assert eng.retain_live_ids() == live == sorted(present.values())
    assert eng.retain_keys_by_id(live) == keys and eng.retain_tenant_counts() == counts


def raw_plan(eng, tenants, ot, ops, keys_cap, fill=0xAB):
    td, to = B.pack(tenants)
    pd, po = B.pack([p for p, _ in ops])
    n = len(ops)
    cl = np.array([c for _, c in ops], dtype=np.uint8)
    otn = np.array(ot, dtype=np.uint32)
    code, act = np.full(n, fill, dtype=np.uint8), np.full(n, fill, dtype=np.uint8)
    win, ids = np.full(n, fill, dtype=np.uint32), np.full(n, fill, dtype=np.uint32)
    delta = np.full(len(tenants), fill, dtype=np.int32)
    koff = np.full(n + 1, fill, dtype=np.uint64)
    keys = np.full(max(keys_cap, 1), fill, dtype=np.uint8)
    info = _lib.RetainPlanInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().bmq_retain_plan(eng.h, p(td), p(to), len(tenants), p(otn), p(pd), p(po), p(cl), n, p(code), p(act), p(win), p(ids), p(delta), p(koff),
                                    p(keys) if keys_cap else None, keys_cap, C.byref(info))
    return rc, (code, act, win, ids, delta, koff, keys), info


def test_refusals_and_buffer_protocol(index):
    eng, present, known = index
    tenants, ot, ops = K.duplicate_batch()
    want = R.plan(tenants, ot, ops, present)
    need = sum(map(len, want["keys"]))
    bad = list(ot)
    bad[70] = len(tenants)                                              # a tenant index out of range: BMQ_E_INVAL, no output is written
    rc, outs, _ = raw_plan(eng, tenants, bad, ops, need)
    assert rc == -1 and all((o == 0xAB).all() for o in outs)
    for cap in (0, need - 1):                                           # BMQ_E_NOSPACE: everything except the key bytes
        rc, (code, act, win, ids, delta, koff, keys), info = raw_plan(eng, tenants, ot, ops, cap)
        assert rc == -3 and int(koff[len(ops)]) == need == info.key_bytes
        assert (code.tolist(), act.tolist(), win.tolist(), ids.tolist(), delta.tolist()) == tuple(want[k] for k in ("code", "action", "winner", "topic_id", "delta"))
        assert np.diff(koff.astype(np.int64)).tolist() == [len(k) for k in want["keys"]] and (keys == 0xAB).all()
    rc, (_, _, _, _, _, koff, keys), _ = raw_plan(eng, tenants, ot, ops, need)
    assert rc == 0 and keys.tobytes() == b"".join(want["keys"])
    # optional outputs may be NULL; n = 0 is BMQ_OK
    td, to = B.pack(tenants)
    koff = np.full(1, 7, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _lib.lib().bmq_retain_plan(eng.h, p(td), p(to), len(tenants), None, None, None, None, 0, None, None, None, None, None, p(koff), None, 0, None) == 0
    assert koff.tolist() == [0]
    pd, po = B.pack([b"s/1"])
    cl = np.zeros(1, dtype=np.uint8)
    keys = np.zeros(64, dtype=np.uint8)
    koff = np.zeros(2, dtype=np.uint64)
    assert _lib.lib().bmq_retain_plan(eng.h, p(td), p(to), len(tenants), None, p(pd), p(po), p(cl), 1, None, None, None, None, None, p(koff), p(keys), 64, None) == 0
    assert keys[:int(koff[1])].tobytes() == retain_message_key(b"t1", b"s/1")


def test_plan_without_an_index():
    eng = B.Engine(device=-1)
    try:
        ops = [(b"a/b", 0), (b"a/b", 1), (b"c", 0)]
        got, want = K.run_and_check(eng, {}, [b"t"], None, ops, where="no index")
        assert want["action"] == [R.SUPERSEDED, R.NONE, R.ADD]
        _, ids = eng.batch_retain([b"t"], None, ops, lambda puts, deletes: None)
        assert ids.tolist() == [R.NO_ID, R.NO_ID, 0] and eng.retain_tenant_counts() == [(b"t", 1)]
    finally:
        eng.close()


def counts_of(present):
    acc = {}
    for t, _ in present:
        acc[t] = acc.get(t, 0) + 1
    return sorted(acc.items())


def test_batch_retain_end_to_end():
    eng = B.Engine(device=-1)
    try:
        present, known = K.build_index(eng)
        kv = {k: b"old" for k in map(lambda tp: retain_message_key(*tp), present)}
        for rnd, (tenants, ot, ops) in enumerate([K.duplicate_batch(), K.state_batch(0), K.random_batch(present, known, 1500, seed=5), K.state_batch(1)]):
            want = R.plan(tenants, ot, ops, present)
            before = dict(eng.retain_tenant_counts())
            epoch = eng.retain_info().epoch

            def kv_commit(puts, deletes):
                for key, i in puts:
                    kv[key] = b"msg %d/%d" % (rnd, i)
                for key in deletes:
                    del kv[key]                                         # a delete is only issued for a key that is there
            stamps = np.arange(len(ops), dtype=np.uint64) + 1000 * (rnd + 1)
            plan, ids = eng.batch_retain(tenants, ot, ops, kv_commit, timestamps=stamps, expiry=np.full(len(ops), 60, dtype=np.uint32))
            R.check(plan, want, "round %d" % rnd)
            R.apply_to(present, tenants, ot, ops, want, ids.tolist())
            assert eng.retain_live_ids() == sorted(present.values())    # the live set is the model's
            assert set(kv) == {retain_message_key(t, p) for t, p in present}
            after = dict(eng.retain_tenant_counts())
            assert after == dict(counts_of(present))
            by_tenant = {}
            for t, d in zip(tenants, want["delta"]):
                by_tenant[t] = by_tenant.get(t, 0) + d
            assert all(after.get(t, 0) - before.get(t, 0) == d for t, d in by_tenant.items())
            changed = [i for i, a in enumerate(want["action"]) if a in (R.ADD, R.UPDATE)]
            for i in changed[:20]:                                      # the winner's stamps are the ones the index holds
                assert eng.retain_topic_info(int(ids[i]))[:2] == (int(stamps[i]), 60)
            assert eng.retain_info().epoch == epoch + (1 if any(a in (R.ADD, R.UPDATE, R.REMOVE) for a in want["action"]) else 0)
    finally:
        eng.close()


def test_stale_plan_and_compaction():
    eng = B.Engine(device=-1)
    try:
        present, known = K.build_index(eng)
        tenants, ot, ops = K.duplicate_batch()
        plan = eng.retain_plan(tenants, ot, ops)
        eng.retain_apply_batch(["t1"], None, [(0, "interleaved")])       # the index moves on between plan and commit
        present[(b"t1", b"interleaved")] = int(eng.retain_info().id_bound) - 1
        state = (info_tuple(eng), eng.retain_live_ids())
        with pytest.raises(B.BmqError) as ei:
            eng.retain_plan_commit(tenants, ot, ops, plan)
        assert ei.value.code == -7 and (info_tuple(eng), eng.retain_live_ids()) == state
        # plan -> commit between compact_begin and _swap: the serving generation answers, the swap replays the commit
        eng.retain_compact_begin()
        want = R.plan(tenants, ot, ops, present)
        plan, ids = eng.batch_retain(tenants, ot, ops, lambda puts, deletes: None)
        R.check(plan, want, "during compaction")
        R.apply_to(present, tenants, ot, ops, want, ids.tolist())
        eng.retain_compact_build()
        assert eng.retain_live_ids() == sorted(present.values())
        gen = eng.retain_info().generation
        eng.retain_compact_swap()
        assert eng.retain_info().generation == gen + 1
        live = eng.retain_live_ids()
        assert len(live) == len(present)
        new_present = dict(zip(_topics_bytes(eng, live), live))
        assert set(new_present) == set(present)
        K.run_and_check(eng, new_present, tenants, ot, ops, where="after the swap")
        with pytest.raises(B.BmqError) as ei:                           # a plan of the old generation is stale too
            eng.retain_plan_commit(tenants, ot, ops, plan)
        assert ei.value.code == -7
    finally:
        eng.close()


def _topics_bytes(eng, ids):
    """(tenant bytes, topic bytes) of ids, through the raw call (special topics are not all UTF-8)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n = len(ids)
    off, tl = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
    cap = 1 << 20
    out = np.zeros(cap, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _lib.lib().bmq_retain_topics(eng.h, p(ids), n, p(out), cap, p(off), p(tl)) == 0
    raw = out.tobytes()
    return [(raw[int(off[i]):int(off[i]) + int(tl[i])], raw[int(off[i]) + int(tl[i]):int(off[i + 1])]) for i in range(n)]
