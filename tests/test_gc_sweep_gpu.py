"""The key-ordered window and the GC sweep on the device: the gfx950 kernels k_o_flag, k_o_pivots, k_o_bucket, k_o_scatter and k_o_leaves
(bifromq_amd/csrc/bmq_order_kernels.h) over the HBM-resident key store, through the table of tests/order_cases.py -- a device engine and a
host-only engine in lockstep through every index state, each answer compared with the model of tests/gc_sweep_ref.py over the scenario's own
set of live keys and the two executors' answers id for id."""
import random

import pytest

import bifromq_amd as B
from tests import gc_sweep_ref as R
from tests import order_cases as T
from tests.test_gc_sweep_ref import case_keys, golden_cases

pytestmark = pytest.mark.gpu


def test_scenario_table_on_the_device_and_against_the_host_executor():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    counts = T.Scenario([dev, host]).run()
    for cls in T.expected_classes():
        assert counts[cls] > 0, cls
    dev.close()
    host.close()


def test_golden_cases_of_the_reference():
    for case in golden_cases():
        ks = case_keys(case)
        eng = B.Engine(device=0).rebuild(ks)
        start = None if case["start"] is None else ks[case["start"]]
        ids, wrapped, nxt = eng.gc_sweep(start, case["step"], case["quota"])
        d = case["derived"]
        assert eng.route_keys(ids) == [ks[p] for p in d["inspected_positions"]], case["name"]
        assert wrapped == d["wrapped"], case["name"]
        assert nxt == (None if d["next_position"] is None else ks[d["next_position"]]), case["name"]
        eng.close()


def test_steps_quotas_and_every_start_position():
    ks = sorted(T.K(b"t%d" % (i % 3), "g/%d" % i) for i in range(50))
    order = ks[:]
    random.Random(9).shuffle(order)
    eng = B.Engine(device=0).rebuild([])
    eng.apply([(0, k) for k in order])
    n = len(ks)
    for step in (1, 2, 3, 7, 10):
        for quota in (1, n, n + 1, 0):
            for p0 in (0, 24, 49):
                ids, wrapped, nxt = eng.gc_sweep(ks[p0], step, quota)
                assert (eng.route_keys(ids), wrapped, nxt) == R.sweep(ks, ks[p0], step, quota), (step, quota, p0)
    for p0 in range(n + 1):
        start = ks[p0] if p0 < n else ks[-1] + b"\0"
        ids, wrapped, nxt = eng.gc_sweep(start, 3, 40)
        assert (eng.route_keys(ids), wrapped, nxt) == R.sweep(ks, start, 3, 40), p0
    rc, rep, out = T.sweep_raw(eng, None, 1, 20, 5)
    assert rc == -3 and rep.inspected == 20 and eng.route_keys(out[:5]) == ks[:5]
    assert eng.split_key_after(ks[5][:-3], 10) == ks[15]
    eng.close()


def test_bucket_sizes_around_bucket_max():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    bmax = dev.window_info().bucket_max
    assert bmax == host.window_info().bucket_max
    for n in (bmax - 1, bmax, bmax + 1, 3 * bmax + 7):
        d, _ = T.check_sizes([dev, host], n, windows=((None, None), (None, 1), (None, n), (None, n - 1), (n // 3, bmax), (n // 3, bmax + 1)))
        assert d["n_calls"] == 6 and (d["n_rounds"] > 0) == (n > bmax), (n, d)
    dev.close()
    host.close()


def test_narrowing_and_rebucketing_ran():
    dev = B.Engine(device=0)
    bmax = dev.window_info().bucket_max
    n = 128 * bmax  # 255 pivots leave bins of n / 256 keys on average, their sizes spread like an exponential: dozens are above bucket_max
    d, info = T.check_sizes([dev], n, windows=((None, None), (n // 5, 4 * bmax), (n // 2, 7)))
    assert d["n_rounds"] > 0 and d["n_bucket_sorts"] > 1 and d["n_rebucketed"] > 0, d
    assert d["n_candidates"] == n + (n - n // 5) + (n - n // 2) and info.max_bucket <= bmax
    dev.close()


def test_rebucketing_with_a_long_shared_prefix():
    dev = B.Engine(device=0)
    d, _ = T.check_sizes([dev], 128 * dev.window_info().bucket_max, long_prefix=True, windows=((None, None),))
    assert d["n_rebucketed"] > 0, d
    dev.close()


def test_a_sweep_that_crosses_a_window_and_a_grid_that_strides():
    """N = 70 000 keys of 7 tenants, step 1, quota 70 000 from a cursor in the middle: both phases fetch a second window behind the last key
    of the first.  Then more candidates than one round of the bounded grid of the per-id passes (2048 workgroups x 256 lanes): 630 000 ids,
    the last 70 000 of them live."""
    n = 70000
    ks = sorted(T.K(b"t%d" % (i % 7), "s/%d/%d" % (i % 251, i), "0\0in%d\0d" % (i % 3)) for i in range(n))
    eng = B.Engine(device=0).rebuild(ks)
    start = ks[n // 2]
    ids, wrapped, nxt = eng.gc_sweep(start, 1, n)
    assert wrapped and nxt == start and len(ids) == n
    assert eng.route_keys(ids) == ks[n // 2:] + ks[:n // 2]
    before = eng.window_info().n_calls
    ids, wrapped, nxt = eng.gc_sweep(ks[n - 10], 7, 0)
    exp = R.sweep(ks, ks[n - 10], 7, 0)
    assert (eng.route_keys(ids), wrapped, nxt) == exp and eng.window_info().n_calls - before == 2
    # churn: every key deleted and put again, eight times over -- 630 000 ids, the last 70 000 of them live
    for _ in range(8):
        for at in range(0, n, 35000):
            eng.apply([(1, k) for k in ks[at:at + 35000]])
            eng.apply([(0, k) for k in ks[at:at + 35000]])
    assert eng.info().next_route_id > 2048 * 256 + n
    ids, more = eng.window(ks[100], 3000)
    assert eng.route_keys(ids) == ks[100:3100] and more
    ids, more = eng.window(ks[n - 50], B.BMQ_WINDOW_MAX, True)
    assert eng.route_keys(ids) == ks[n - 49:] and not more
    eng.close()
