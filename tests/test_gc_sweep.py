"""The key-ordered window (bmq_routes_window, Engine.window) and the dist worker's GC sweep over it (bmq_routes_gc_sweep, Engine.gc_sweep) on
a host-only engine, which runs the per-item functions the gfx950 kernels k_o_* wrap (bifromq_amd/csrc/bmq_order_core.h) under the same
control (DistIndex::window).  The table -- key sets, index states, cursors, window sizes, sweeps -- is tests/order_cases.py, the model
tests/gc_sweep_ref.py; tests/test_gc_sweep_gpu.py runs the table on the device."""
import pytest

import bifromq_amd as B
from tests import gc_sweep_ref as R
from tests import order_cases as T
from tests.test_gc_sweep_ref import case_keys, golden_cases


def test_scenario_table_on_the_host_executor():
    counts = T.Scenario([B.Engine(device=-1)]).run()
    for cls in T.expected_classes():
        assert counts[cls] > 0, cls


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"].split(",")[0].replace(" ", "_")[:48])
def test_golden_cases_of_the_reference(case):
    ks = case_keys(case)
    eng = B.Engine(device=-1).rebuild(ks)
    start = None if case["start"] is None else ks[case["start"]]
    ids, wrapped, nxt = eng.gc_sweep(start, case["step"], case["quota"])
    d = case["derived"]
    assert eng.route_keys(ids) == [ks[p] for p in d["inspected_positions"]]
    assert wrapped == d["wrapped"]
    assert nxt == (None if d["next_position"] is None else ks[d["next_position"]])
    eng.close()


def _fifty():
    ks = sorted(T.K(b"t%d" % (i % 3), "g/%d" % i) for i in range(50))
    order = ks[:]
    __import__("random").Random(9).shuffle(order)
    eng = B.Engine(device=-1).rebuild([])
    eng.apply([(0, k) for k in order])
    return eng, ks


def test_steps_and_quotas_over_fifty_keys():
    eng, ks = _fifty()
    n = len(ks)
    for step in (1, 2, 3, 7, 10):
        for quota in (1, n, n + 1, 0):
            for p0 in (0, 1, 24, 49):
                ids, wrapped, nxt = eng.gc_sweep(ks[p0], step, quota)
                assert (eng.route_keys(ids), wrapped, nxt) == R.sweep(ks, ks[p0], step, quota), (step, quota, p0)
    eng.close()


def test_every_start_position():
    eng, ks = _fifty()
    for step, quota in ((3, 40), (7, 0)):
        for p0 in range(len(ks) + 1):  # p0 % step zero and not; p0 == N: past the end
            start = ks[p0] if p0 < len(ks) else ks[-1] + b"\0"
            ids, wrapped, nxt = eng.gc_sweep(start, step, quota)
            assert (eng.route_keys(ids), wrapped, nxt) == R.sweep(ks, start, step, quota), (step, quota, p0)
    eng.close()


def test_the_boundary_clamp_is_the_callers():
    eng, ks = _fifty()
    b = (ks[10], ks[40])
    for start in (ks[3], ks[10], ks[25], ks[40], ks[45], b"", b"\xff"):
        ids, wrapped, nxt = eng.gc_sweep(start, 2, 6, boundary=b)
        assert (eng.route_keys(ids), wrapped, nxt) == R.sweep(ks, start, 2, 6, boundary=b), start
    ids, _, _ = eng.gc_sweep(ks[45], 1, 1, boundary=(None, ks[40]))  # no start: the clamp seeks to the first key
    assert eng.route_keys(ids) == [ks[0]]
    eng.close()


def test_cap_too_small_and_refusals():
    eng, ks = _fifty()
    rc, rep, out = T.sweep_raw(eng, None, 1, 20, 5)
    assert rc == -3 and rep.inspected == 20 and eng.route_keys(out[:5]) == ks[:5]
    rc, rep, out = T.sweep_raw(eng, None, 1, 20, 20)
    assert rc == 0 and rep.inspected == 20 and rep.has_next == 1 and eng.route_key(rep.next_route_id) == ks[20] and rep.epoch == eng.info().epoch
    assert T.sweep_raw(eng, None, 10, 5120, 1)[0] == -3  # the reference's largest: 51 200 keys
    assert T.sweep_raw(eng, None, 1, 50000, 1)[0] == -3  # the cleaner's first sweep
    assert T.sweep_raw(eng, None, 16, 65537, 1)[0] == -1  # more than 16 windows
    assert T.sweep_raw(eng, None, 0xFFFFFFFF, 0, 1)[0] == -1
    with pytest.raises(B.BmqError) as ex:
        eng.window(None, B.BMQ_WINDOW_MAX + 1)
    assert ex.value.code == -1
    ids, more = eng.window(None, 0)
    assert len(ids) == 0 and more
    eng.close()


def test_an_open_async_batch_is_completed_first():
    eng = B.Engine(device=-1).rebuild([T.K(b"x", "b")])
    eng.apply_async([(0, T.K(b"x", "a")), (0, T.K(b"x", "c")), (1, T.K(b"x", "b"))])
    ids, more = eng.window()
    assert eng.route_keys(ids) == [T.K(b"x", "a"), T.K(b"x", "c")] and not more
    eng.close()


def test_the_window_neither_changes_the_index_nor_the_epoch():
    eng, ks = _fifty()
    before = eng.info()
    ep = before.epoch
    eng.window(ks[7], 9, True)
    eng.gc_sweep(ks[7], 2, 9)
    after = eng.info()
    assert (after.next_route_id, after.n_routes, after.epoch) == (before.next_route_id, before.n_routes, ep)
    eng.close()


def test_split_key_after():
    eng, ks = _fifty()
    assert eng.split_key_after(b"", 0) == ks[0]
    assert eng.split_key_after(ks[5][:-3], 10) == ks[15]  # not bounded by the prefix
    assert eng.split_key_after(ks[45], 4) == ks[49] and eng.split_key_after(ks[45], 5) is None
    eng.close()


def test_bucket_sizes_around_bucket_max():
    eng = B.Engine(device=-1)
    bmax = eng.window_info().bucket_max
    assert eng.window_info().window_max == B.BMQ_WINDOW_MAX and bmax >= 64
    for n in (bmax - 1, bmax, bmax + 1, 3 * bmax + 7):
        d, _ = T.check_sizes([eng], n, windows=((None, None), (None, 1), (None, n), (None, n - 1), (n // 3, bmax), (n // 3, bmax + 1)))
        assert d["n_calls"] == 6 and (d["n_rounds"] > 0) == (n > bmax), (n, d)
    eng.close()


def test_narrowing_and_rebucketing_ran():
    eng = B.Engine(device=-1)
    bmax = eng.window_info().bucket_max
    n = 128 * bmax  # 255 pivots leave bins of n / 256 keys on average, their sizes spread like an exponential: dozens are above bucket_max
    d, info = T.check_sizes([eng], n, windows=((None, None), (n // 5, 4 * bmax), (n // 2, 7)))
    assert d["n_rounds"] > 0 and d["n_bucket_sorts"] > 1 and d["n_rebucketed"] > 0, d
    assert d["n_candidates"] == n + (n - n // 5) + (n - n // 2) and info.max_bucket <= bmax
    eng.close()


def test_rebucketing_with_a_long_shared_prefix():
    eng = B.Engine(device=-1)
    bmax = eng.window_info().bucket_max
    d, _ = T.check_sizes([eng], 128 * bmax, long_prefix=True, windows=((None, None),))
    assert d["n_rebucketed"] > 0, d
    eng.close()
