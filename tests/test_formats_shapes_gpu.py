"""BMQ_FMT_RANGES on the device at the shapes its kernels (bifromq_amd/csrc/bmq_format_kernels.h) and its wait (bmq_match_wait_ranges) go wrong
at, every result held to the contract of include/bmq.h by the strict consumer of tests/ranges_ref.py: the count of overlapping rows by
construction, rows of 32 / 33 / 38 ranges, filters emptied by deletes, the slot's own range and side buffers growing inside the wait, the
caller's buffers fitting exactly and one short, the repair paths of the batch (deep topics, waves of many tenants, pair-buffer growth, the
smallest LDS geometry) and a de-duplicating engine.  Expected rows: the semantic oracle over the engine's live route keys (ranges_ref.expected_csr),
which eng.match_batch has to agree with.  The emulator tier below this one: tests/test_format_emu.py."""
import itertools
import time

import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import ranges_ref as R

pytestmark = pytest.mark.gpu


def _key(tenant, tf, recv):
    return B.route_key_from_mqtt(tenant, tf, O.receiver_url(0, recv, "d0"))


def _family(tenant, extra=()):
    """the 32 filters of {x,+}^5 and `extra`, one route each"""
    return [_key(tenant, "/".join(lv), "r") for lv in itertools.product("x+", repeat=5)] + [_key(tenant, f, "r") for f in extra]


O33 = ("#",)
O38 = ("#", "x/#", "x/x/#", "x/x/x/#", "x/x/x/x/#", "+/#")
TOPIC = "x/x/x/x/x"


@pytest.fixture()
def eng():
    e = B.Engine(device=0)  # a fresh engine per test: slot capacities persist in an engine and would hide the growth paths
    yield e
    e.close()


def _timed(label, t0):
    print("[ranges shapes] %s: %.2f s" % (label, time.time() - t0))


def _n_ranges(rptr, i):
    return int(rptr[i + 1]) - int(rptr[i])


def test_g1_the_overlap_count_by_construction(eng):
    """a/+ and a/b with two routes each; one more route on the filter that holds the LOWER ids makes its list reach over the other filter's
    range in every row both match: exactly those rows are counted.  The same on the filter with the HIGHER ids overlaps nothing."""
    t0 = time.time()
    keys = [_key(tn, f, r) for tn in ("v", "w") for f in ("a/+", "a/b") for r in ("r0", "r1")]
    eng.rebuild(keys)
    ids = {k: i for i, k in enumerate(eng.route_keys(list(range(len(keys)))))}
    k_rows, m_rows = 37, 91
    lo = {tn: min(("a/+", "a/b"), key=lambda f: ids[_key(tn, f, "r0")]) for tn in ("v", "w")}
    hi = {tn: "a/b" if lo[tn] == "a/+" else "a/+" for tn in ("v", "w")}
    for tn in ("v", "w"):  # (what the construction rests on: a filter's routes are neighbours, the two filters' id sets do not interleave)
        a, b = sorted(ids[_key(tn, lo[tn], r)] for r in ("r0", "r1")), sorted(ids[_key(tn, hi[tn], r)] for r in ("r0", "r1"))
        assert a[1] == a[0] + 1 and b[1] == b[0] + 1 and a[1] < b[0]
    eng.apply([(0, _key("v", lo["v"], "late")), (0, _key("w", hi["w"], "late"))])
    live = keys + [_key("v", lo["v"], "late"), _key("w", hi["w"], "late")]
    topics = ["a/b"] * k_rows + ["a/c"] * m_rows
    order = np.random.RandomState(5).permutation(len(topics))
    topics = [topics[i] for i in order]
    # v: every row holds the list of three ids; the k rows that also match the other filter overlap
    bv = R.Batch(["v"], np.zeros(len(topics), dtype=np.uint32), topics)
    erow, eids = R.expected_csr(eng, bv, live)
    info, rptr, ranges, side, rows, flags = R.ranges_of(eng, bv, erow, eids)
    assert lo["v"] == "a/+"  # ('+' sorts in front of 'b': the list is a/+'s, every row holds it, and a/b matches both filters)
    assert info.n_overlapping_rows == k_rows and [bool(f) for f in flags] == [t == "a/b" for t in topics]
    assert info.n_side_ids == 3 * (k_rows + m_rows)
    # w: the list lies behind the other filter's range
    bw = R.Batch(["w"], np.zeros(len(topics), dtype=np.uint32), topics)
    erow, eids = R.expected_csr(eng, bw, live)
    info, *_ = R.ranges_of(eng, bw, erow, eids)
    assert info.n_overlapping_rows == 0 and info.n_side_ids == 3 * k_rows > 0
    _timed("G1", t0)


def _boundary_index(eng):
    keys = _family("o32") + _family("o33", O33) + _family("o38", O38)
    eng.rebuild(keys)
    return keys


def _check_boundary(eng, keys, label):
    b = R.Batch(["o32", "o33", "o38"], np.arange(3, dtype=np.uint32), [TOPIC] * 3)
    erow, eids = R.expected_csr(eng, b, keys)
    assert np.diff(erow.astype(np.int64)).tolist() == [32, 33, 38]
    info, rptr, ranges, side, rows, flags = R.ranges_of(eng, b, erow, eids)
    assert [_n_ranges(rptr, i) for i in range(3)] == [32, 33, 38] and info.n_side_ids == 0
    # the row of 32 ranges is ordered (check_ranges_contract (c)) and, after a rebuild, not flagged; rows of more come as matched: the strict
    # consumer reproduced them (a) and counted what the engine counted (b)
    assert not flags[0]
    print("[ranges shapes] %s: n_overlapping_rows after a rebuild = %d (row of 32 ranges: %d, of 33: %d, of 38: %d)" % (label, info.n_overlapping_rows, flags[0], flags[1], flags[2]))
    return info, flags


def test_g2_rows_of_32_33_and_38_ranges(eng):
    """32 ranges are ordered, 33 and more come as the walk matched them: include/bmq.h lets n_overlapping_rows count such rows even after a
    rebuild (the walk does not match in id order), and the strict consumer orders exactly the rows the engine counted"""
    t0 = time.time()
    keys = _boundary_index(eng)
    _check_boundary(eng, keys, "G2 default geometry")
    _timed("G2", t0)


def test_g2_the_same_rows_with_the_smallest_lds_geometry():
    t0 = time.time()
    e = B.Engine(device=0, wave_queue_cap=128, wave_pair_cap=128)
    try:
        keys = _family("o38", O38)
        e.rebuild(keys)
        b = R.Batch(["o38"], np.zeros(5, dtype=np.uint32), [TOPIC] * 5)
        erow, eids = R.expected_csr(e, b, keys)
        info, rptr, *_ = R.ranges_of(e, b, erow, eids)
        assert [_n_ranges(rptr, i) for i in range(5)] == [38] * 5
        print("[ranges shapes] G2 smallest geometry: n_overlapping_rows = %d of 5 rows" % info.n_overlapping_rows)
    finally:
        e.close()
    _timed("G2 smallest geometry", t0)


def test_g3_filters_emptied_by_deletes(eng):
    """e/f gets two routes by apply and loses both; +/f holds one route from the rebuild, gets two by apply (an id LIST: the ids are no
    neighbours) and loses all three; e/# holds two routes from the rebuild and loses both; the sibling e/+ keeps its route: rows for e/f carry
    that id alone and are not flagged.  Whether an emptied filter still shows as a range of count 0 is the index's business;
    where n_ranges says it does, the ranges are there, empty"""
    t0 = time.time()
    base = [_key("e", "e/+", "keep"), _key("e", "e/#", "h0"), _key("e", "e/#", "h1"), _key("e", "q", "other"), _key("e", "+/f", "f0")]
    eng.rebuild(base)
    late = [_key("e", "e/f", "l0"), _key("e", "e/f", "l1"), _key("e", "+/f", "f1"), _key("e", "+/f", "f2")]
    eng.apply([(0, k) for k in late])
    n = 300
    b = R.Batch(["e"], np.zeros(n, dtype=np.uint32), ["e/f" if i % 3 else "e/g" for i in range(n)])
    erow, eids = R.expected_csr(eng, b, base + late)  # before the deletes: every row holds the rebuild's routes, two of three rows the list as well
    info, *_ = R.ranges_of(eng, b, erow, eids)
    assert info.n_side_ids == 3 * sum(1 for t in b.topics if t == "e/f")  # the list of +/f: one id of the rebuild, two far behind it
    eng.apply([(1, late[0]), (1, late[3])])
    eng.apply([(1, late[1]), (1, base[1]), (1, base[4])])
    eng.apply([(1, base[2]), (1, late[2])])
    live = [base[0], base[3]]
    erow, eids = R.expected_csr(eng, b, live)
    keep = eng.find_routes([base[0]])[0]
    assert np.diff(erow.astype(np.int64)).tolist() == [1] * n and (eids == keep).all()
    info, rptr, ranges, side, rows, flags = R.ranges_of(eng, b, erow, eids)
    assert info.n_overlapping_rows == 0 and not any(flags) and info.n_side_ids == 0
    cnt = ranges[:info.n_ranges, 1].astype(np.int64) & 0x7FFFFFFF
    assert int((cnt != 0).sum()) == n  # one non-empty range per row ...
    assert int((cnt == 0).sum()) == info.n_ranges - n  # ... and whatever else n_ranges counts is an empty range
    print("[ranges shapes] G3: %d ranges for %d rows (%d empty ranges emitted)" % (info.n_ranges, n, info.n_ranges - n))
    _timed("G3", t0)


def test_g4_the_slots_range_buffer_grows_inside_the_wait(eng):
    """200 rows of 38 ranges: 7600 ranges against the 8 * n + 1024 = 2624 the slot starts with; the first wait has the whole result"""
    t0 = time.time()
    keys = _family("o38", O38)
    eng.rebuild(keys)
    n = 200
    assert 38 * n > 8 * n + 1024
    b = R.Batch(["o38"], np.zeros(n, dtype=np.uint32), [TOPIC] * n)
    erow, eids = R.expected_csr(eng, b, keys)
    info, *_ = R.ranges_of(eng, b, erow, eids)
    assert info.n_ranges == 38 * n
    info2, *_ = R.ranges_of(eng, b, erow, eids)  # and with the grown buffers
    assert (info2.n_ranges, info2.n_overlapping_rows) == (info.n_ranges, info.n_overlapping_rows)
    _timed("G4 ranges", t0)


def test_g4_the_slots_side_buffer_grows_inside_the_wait(eng):
    """700 rows under a '#' filter that got 100 routes by apply: 70 000 side ids against the 65 536 the slot starts with"""
    t0 = time.time()
    base = [_key("g", "#", "first"), _key("g", "zz", "other")]
    eng.rebuild(base)
    late = [_key("g", "#", "late%03d" % j) for j in range(100)]
    eng.apply([(0, k) for k in late[:60]])
    eng.apply([(0, k) for k in late[60:]] + [(1, base[0])])
    n = 700
    b = R.Batch(["g"], np.zeros(n, dtype=np.uint32), ["t/%d" % (i % 9) for i in range(n)])
    erow, eids = R.expected_csr(eng, b, base[1:] + late)
    assert len(eids) == 100 * n
    info, *_ = R.ranges_of(eng, b, erow, eids)
    assert info.n_side_ids == 100 * n > 65536 and info.n_ranges == n and info.n_overlapping_rows == 0
    _timed("G4 side ids", t0)


def test_g5_the_callers_buffers_exact_and_one_short(eng):
    t0 = time.time()
    keys = [_key("v", f, r) for f in ("a/+", "a/b") for r in ("r0", "r1")]
    eng.rebuild(keys)
    late = _key("v", "a/+", "late")
    eng.apply([(0, late)])
    topics = ["a/b", "a/c", "a/b", "zz", "a/b"] * 13
    b = R.Batch(["v"], np.zeros(len(topics), dtype=np.uint32), topics)
    erow, eids = R.expected_csr(eng, b, keys + [late])
    info, *_ = R.ranges_of(eng, b, erow, eids)
    n_r, n_s = int(info.n_ranges), int(info.n_side_ids)
    assert n_r > 0 and n_s > 0
    exact, *_ = R.ranges_of(eng, b, erow, eids, range_cap=n_r, side_cap=n_s)  # an exact fit of both
    assert (exact.n_ranges, exact.n_side_ids, exact.n_overlapping_rows) == (n_r, n_s, info.n_overlapping_rows)
    for rc, sc in ((n_r - 1, n_s), (n_r, n_s - 1)):
        t = b.submit(eng, eng.FMT_RANGES)
        with pytest.raises(B.BmqError) as ei:
            R.wait_ranges(eng, t, b.n, rc, sc)
        assert ei.value.code == -3 and (ei.value.info.n_ranges, ei.value.info.n_side_ids, ei.value.info.n_ids) == (n_r, n_s, len(eids))
        with pytest.raises(B.BmqError) as ei:  # the ticket was released
            R.wait_ranges(eng, t, b.n, n_r, n_s)
        assert ei.value.code == -7
    _timed("G5", t0)


def _first_batch_ranges_then_ids(make_engine, keys, batch, after=None):
    """RANGES as the FIRST batch of a fresh engine (the repair path runs under it), held to the contract and to the BMQ_FMT_IDS result of the same batch"""
    e = make_engine()
    try:
        e.rebuild(keys)
        t = batch.submit(e, e.FMT_RANGES)
        info, rptr, ranges, side, row = R.wait_ranges(e, t, batch.n, 80 * batch.n + 4096, 80 * batch.n + 4096)
        st = e.stats()
        irow, iids = batch.ids_async(e)
        assert np.array_equal(row, irow)
        R.check_ranges_contract(info, rptr, ranges, side, batch.n, irow, iids)
        erow, eids = R.expected_csr(e, batch, keys)  # and the FMT_IDS result is the oracle's
        assert np.array_equal(irow, erow) and np.array_equal(iids, eids)
        if after is not None:
            after(st, info)
    finally:
        e.close()


def test_g6_deep_topics_as_the_first_batch():
    """topics of 17 and 40 levels: the first launch has no k_walk_slow in it, finish_dist runs the batch again with it -- and the format kernels with it"""
    t0 = time.time()
    keys = [_key("d", "#", "all"), _key("d", "d/#", "under"), _key("d", "d/+", "one")]
    deep17, deep40 = "/".join(["d"] * 17), "/".join(["d"] * 40)
    topics = [deep17, "d/x", deep40, "q", "d"] * 20
    b = R.Batch(["d"], np.zeros(len(topics), dtype=np.uint32), topics)

    def after(st, info):
        assert st.n_slow_topics == 40 and info.n_ranges > 0

    _first_batch_ranges_then_ids(lambda: B.Engine(device=0), keys, b, after)
    _timed("G6 deep topics", t0)


def test_g6_a_batch_alternating_over_70_tenants_as_the_first_batch():
    """256 rows, no two neighbours of one tenant: every wave holds many tenants (the MIXED rerun)"""
    t0 = time.time()
    tenants = ["m%02d" % i for i in range(70)]
    keys = [_key(tn, f, "r%d" % j) for tn in tenants for j, f in enumerate(("#", "s/+", "s/t", "+/t"))]
    b = R.Batch(tenants, np.arange(256, dtype=np.uint32) % 70, ["s/t" if i % 4 else "s/u" for i in range(256)])
    _first_batch_ranges_then_ids(lambda: B.Engine(device=0), keys, b)
    _timed("G6 many tenants", t0)


def test_g6_more_pairs_than_the_slots_pair_buffer_as_the_first_batch():
    """2000 rows of 38 ranges = 76 000 matched ranges against the max(65 536, 4 * n) the slot starts with: the batch runs again with a larger
    pair buffer (bmq_config offers no smaller one; that the rerun happened is arithmetic, the engine reports no count of it)"""
    t0 = time.time()
    n = 2000
    assert 38 * n > max(65536, 4 * n)
    b = R.Batch(["o38"], np.zeros(n, dtype=np.uint32), [TOPIC] * n)

    def after(st, info):
        assert info.n_ranges == 38 * n

    _first_batch_ranges_then_ids(lambda: B.Engine(device=0), _family("o38", O38), b, after)
    _timed("G6 pair growth", t0)


def test_g7_a_de_duplicating_engine():
    """dedup_min_topics = 1: every row three times (not as neighbours), side lists included; every repetition has ranges and a side slice of its own"""
    t0 = time.time()
    e = B.Engine(device=0, dedup_min_topics=1)
    try:
        keys = [_key("v", f, r) for f in ("a/+", "a/b", "c/#") for r in ("r0", "r1")]
        e.rebuild(keys)
        late = [_key("v", "a/+", "late"), _key("v", "c/#", "late")]
        e.apply([(0, k) for k in late])
        distinct = ["a/b", "a/c", "c/d/e", "zz", "c", "a/b/c"]
        topics = distinct * 3
        b = R.Batch(["v"], np.zeros(len(topics), dtype=np.uint32), topics)
        erow, eids = R.expected_csr(e, b, keys + late)
        info, rptr, ranges, side, rows, flags = R.ranges_of(e, b, erow, eids)  # (e): the side slices are disjoint and in row order
        k = len(distinct)
        per_row_side = [sum(int(c) & 0x7FFFFFFF for _, c in ranges[rptr[i]:rptr[i + 1]] if int(c) & 0x80000000) for i in range(b.n)]
        assert per_row_side[:k] == per_row_side[k:2 * k] == per_row_side[2 * k:] and sum(per_row_side) == info.n_side_ids > 0
        assert flags[:k] == flags[k:2 * k] == flags[2 * k:] and info.n_overlapping_rows == 3 * sum(flags[:k]) > 0
        assert e.stats().n_walked in (0, k)  # (the hashing de-duplication does not count; where it does, the walk saw the distinct rows)
    finally:
        e.close()
    _timed("G7", t0)
