"""The strict consumer of tests/ranges_ref.py on hand-made results: it must accept what include/bmq.h allows and refuse every way a RANGES
result can be wrong that the lenient Engine.expand_ranges lets through -- a wrong order in a short row, a wrong n_overlapping_rows, side
slices out of row order.  (No GPU: the checker is checked here, the engine in tests/test_formats_shapes_gpu.py.)"""
from types import SimpleNamespace

import numpy as np
import pytest

from bifromq_amd.engine import Engine
from tests import ranges_ref as R

S = R.SIDE


def _result(rows, side, n_overlapping):
    """rows: lists of (begin, count) -> (info, range_ptr, ranges, side)"""
    rptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    ranges = np.array([rc for r in rows for rc in r] or np.zeros((0, 2)), dtype=np.uint32).reshape(-1, 2)
    side = np.asarray(side, dtype=np.uint32)
    return rptr, ranges, side, n_overlapping


def _check(rows, side, n_overlapping, expected_rows, n_ids=None):
    rptr, ranges, side, _ = _result(rows, side, n_overlapping)
    erow = np.cumsum([0] + [len(r) for r in expected_rows]).astype(np.uint32)
    eids = np.array([x for r in expected_rows for x in r], dtype=np.uint32)
    info = SimpleNamespace(n_ranges=len(ranges), n_side_ids=len(side), n_ids=len(eids) if n_ids is None else n_ids, n_overlapping_rows=n_overlapping)
    return R.check_ranges_contract(info, rptr, ranges, side, len(rows), erow, eids)


GOOD = dict(rows=[[(0, 2), (0, 3 | S), (20, 1)], [], [(3, 0 | S), (9, 0), (3, 2 | S)], [(5, 2 | S), (4, 3)]],
            side=[5, 7, 30, 40, 41, 2, 9], n_overlapping=2,
            expected_rows=[[0, 1, 5, 7, 20, 30], [], [40, 41], [2, 4, 5, 6, 9]])


def test_a_result_the_contract_allows_is_accepted_and_flagged_rows_are_the_ordered_ones():
    rows, flags = _check(**GOOD)
    assert flags == [True, False, False, True]
    assert [r.tolist() for r in rows] == GOOD["expected_rows"]


@pytest.mark.parametrize("what, change", [
    ("a short row in descending order", dict(rows=[[(20, 1), (0, 2)]], side=[], n_overlapping=0, expected_rows=[[0, 1, 20]])),
    ("a short row in descending order that the engine counted", dict(rows=[[(20, 1), (0, 2)]], side=[], n_overlapping=1, expected_rows=[[0, 1, 20]])),
    ("an overlapping row the engine did not count", dict(GOOD, n_overlapping=1)),
    ("a count of overlapping rows without such rows", dict(rows=[[(0, 2), (5, 1)]], side=[], n_overlapping=1, expected_rows=[[0, 1, 5]])),
    ("side slices out of row order", dict(rows=[[(1, 1 | S)], [(0, 1 | S)]], side=[8, 7], n_overlapping=0, expected_rows=[[7], [8]])),
    ("two lists over the same side words", dict(rows=[[(0, 1 | S), (0, 1 | S)]], side=[7], n_overlapping=1, expected_rows=[[7, 7]])),
    ("side ids no row owns", dict(rows=[[(0, 1 | S)]], side=[7, 8], n_overlapping=0, expected_rows=[[7]])),
    ("a wrong n_ids", dict(GOOD, n_ids=3)),
    ("a missing id", dict(rows=[[(0, 2)]], side=[], n_overlapping=0, expected_rows=[[0, 1, 2]])),
])
def test_a_wrong_result_is_refused(what, change):
    with pytest.raises(AssertionError):
        _check(**change)


def test_rows_of_more_than_32_ranges_may_come_in_any_order_if_they_are_counted():
    ranges = [(2 * i, 1) for i in reversed(range(33))]
    _check([ranges], [], 1, [[2 * i for i in range(33)]])
    with pytest.raises(AssertionError):
        _check([ranges], [], 0, [[2 * i for i in range(33)]])
    with pytest.raises(AssertionError):  # ... but 32 ranges may not
        _check([ranges[1:]], [], 1, [[2 * i for i in range(32)]])


def test_the_lenient_consumer_accepts_what_the_strict_one_refuses():
    """why tests/test_formats_gpu.py could not see a wrong order: Engine.expand_ranges orders the row and says nothing"""
    rptr, ranges, side, _ = _result([[(20, 1), (0, 2)]], [], 0)
    assert Engine.expand_ranges(rptr, ranges, side, 1)[0].tolist() == [0, 1, 20]
