"""The counting-sort fast path of the fan-out grouping (bifromq_amd/csrc/bmq_fanout_kernels.h: k_fo_dense, k_fo_hist, the scan, k_fo_scatter,
k_fo_groups2) at the shapes where it can go wrong, against oracle.fanout_groups: totals around 64 and 1024 and up to five tiles, a row
longer than a tile, rows of one pair, runs of more than 64 empty rows, tiles that start behind a run of empty rows, 2 to 1026 bins and the
switch to the generic passes behind them, batches that are all shared or all dead, and the state transitions of one engine.  The table
is tests/fanout_cases.py; tests/test_fanout_shapes.py runs the same cases on a host-only engine.  bmq_fanout_info_get says which path
answered, so a fast path that quietly stopped being taken fails here."""
import pytest

from tests import fanout_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    e = FC.Engines(0)
    yield e
    e.close()


@pytest.mark.parametrize("K", FC.SHAPE_KS)
@pytest.mark.parametrize("shape", sorted(FC.ROW_SHAPES))
def test_row_shapes(engines, K, shape):
    FC.run_row_shape(engines, K, shape)


@pytest.mark.parametrize("K", FC.SHAPE_KS)
@pytest.mark.parametrize("pattern", sorted(FC.KEY_PATTERNS))
def test_key_patterns(engines, K, pattern):
    FC.run_key_pattern(engines, K, pattern)


@pytest.mark.parametrize("K", FC.BIN_KS)
def test_bin_counts(K):
    FC.run_bin_count(0, K)


def test_state_transitions_on_one_engine():
    FC.state_transitions(0)


def test_groups_after_compact_swap():
    FC.swap_sequence(0)
