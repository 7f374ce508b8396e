"""bmq_retain_plan / bmq_retain_plan_commit on the device (k_rp_find, k_rp_group, k_rp_classify, the scan, k_rp_key_write): the comparisons
of tests/test_retain_plan.py against the rule of tests/retain_plan_ref.py, the device against the host executor output for output on a
20 000-op batch, read-only-ness with a fixed match batch, and the stream order behind an apply."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import retain_plan_cases as K
from tests import retain_plan_ref as R

pytestmark = pytest.mark.gpu

FILTERS = ["#", "+/#", "s/+/x", "s/1", "q/3", "p/q/r", "p/+", "a/b", "new/+/z", "k/#"]


@pytest.fixture(scope="module")
def index():
    eng = B.Engine(device=0)
    present, known = K.build_index(eng)
    yield eng, present, known
    eng.close()


def info_tuple(eng):
    i = eng.retain_info()
    return tuple(getattr(i, f) for f, _ in i._fields_)


def fixed_match(eng):
    tn = ["t0", "t1", "t2", "ov", "empty", ""]
    ft = [t for t in range(len(tn)) for _ in FILTERS]
    row, ids = eng.retain_match_batch(tn, ft, FILTERS * len(tn))
    return row.tolist(), ids.tolist()


def test_index_states_and_duplicates_on_the_device(index):
    eng, present, known = index
    K.assert_states(eng, present, known)
    seen = set()
    for clear in (0, 1):
        _, want = K.run_and_check(eng, present, *K.state_batch(clear), where="states clear=%d" % clear)
        seen |= {(a, c) for a, c in zip(want["action"], want["code"])}
    _, want = K.run_and_check(eng, present, *K.duplicate_batch(), where="duplicates")
    seen |= {(a, c) for a, c in zip(want["action"], want["code"])}
    assert {a for a, _ in seen} == {R.NONE, R.ADD, R.UPDATE, R.REMOVE, R.SUPERSEDED} and {c for _, c in seen} == {R.RETAINED, R.CLEARED}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2000])
def test_batch_sizes_on_the_device(index, n):
    eng, present, known = index
    tenants, ot, ops = K.random_batch(present, known, n, seed=n)
    K.run_and_check(eng, present, tenants, ot, ops, where="n=%d" % n)
    if n:
        K.run_and_check(eng, present, [tenants[ot[0]]], None, ops, where="n=%d, tenant 0" % n)


def test_read_only_on_the_device(index):
    eng, present, known = index
    before, rows = info_tuple(eng), fixed_match(eng)
    assert len(rows[1]) > 500
    live = eng.retain_live_ids()
    for clear in (0, 1):
        K.run_and_check(eng, present, *K.state_batch(clear), where="read-only")
    K.run_and_check(eng, present, *K.random_batch(present, known, 3000, seed=11), where="read-only")
    assert info_tuple(eng) == before and fixed_match(eng) == rows       # epoch, ids, overlay nodes and every row as they were
    assert eng.retain_live_ids() == live == sorted(present.values())


def test_device_equals_host_on_20000_ops():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        dp, dk = K.build_index(dev)
        hp, hk = K.build_index(host)
        assert set(dp) == set(hp)
        tenants, ot, ops = K.random_batch(dp, dk, 20000, seed=3, dup=0.3)
        d, h = dev.retain_plan(tenants, ot, ops), host.retain_plan(tenants, ot, ops)
        R.check(d, R.plan(tenants, ot, ops, dp), "device")
        for f in ("code", "action", "winner", "delta", "key_off"):
            assert np.array_equal(getattr(d, f), getattr(h, f)), f
        assert d.key_bytes == h.key_bytes
        base = int(dev.retain_info().loaded_topics)
        assert base == host.retain_info().loaded_topics
        d_by_id, h_by_id = {i: k for k, i in dp.items()}, {i: k for k, i in hp.items()}
        di, hi = d.topic_id.tolist(), h.topic_id.tolist()
        for a, b in zip(di, hi):                                        # ranks are the same ids in both engines; overlay ids go by topic
            assert a == b if (a == R.NO_ID or a < base) else d_by_id[a] == h_by_id[b]
        assert sum(1 for a in di if a != R.NO_ID and a >= base) > 1000
        assert [getattr(d.info, f) for f in ("n_groups", "n_add", "n_update", "n_remove", "n_none", "key_bytes")] == \
               [getattr(h.info, f) for f in ("n_groups", "n_add", "n_update", "n_remove", "n_none", "key_bytes")]
        assert d.info.n_groups < 16000                                  # about 30 % of the ops repeat an earlier key
    finally:
        dev.close(), host.close()


def test_batch_retain_and_stream_order_on_the_device():
    eng = B.Engine(device=0)
    try:
        present, known = K.build_index(eng)
        # a plan queued behind an apply that nobody waited for sees that apply
        ids = eng.retain_apply_batch(["ov", "t1"], [0, 1, 1], [(0, "p/q"), (1, "s/4/x"), (0, "s/4")]).tolist()
        present[(b"ov", b"p/q")], present[(b"t1", b"s/4")] = ids[0], ids[2]
        del present[(b"t1", b"s/4/x")]
        got, want = K.run_and_check(eng, present, *K.state_batch(0), where="behind an apply")
        keys = list(K.STATES.values())
        assert [want["action"][keys.index(k)] for k in ((b"ov", b"p/q"), (b"t1", b"s/4/x"), (b"t1", b"s/4"))] == [R.UPDATE, R.ADD, R.UPDATE]
        for rnd, (tenants, ot, ops) in enumerate([K.duplicate_batch(), K.random_batch(present, known, 1500, seed=5), K.state_batch(1)]):
            want = R.plan(tenants, ot, ops, present)
            plan, out = eng.batch_retain(tenants, ot, ops, lambda puts, deletes: None)
            R.check(plan, want, "round %d" % rnd)
            R.apply_to(present, tenants, ot, ops, want, out.tolist())
            assert eng.retain_live_ids() == sorted(present.values())
        plan = eng.retain_plan(*K.duplicate_batch())
        eng.retain_apply_batch(["t1"], None, [(0, "interleaved")])
        with pytest.raises(B.BmqError) as ei:
            eng.retain_plan_commit(*K.duplicate_batch(), plan)
        assert ei.value.code == -7
    finally:
        eng.close()
