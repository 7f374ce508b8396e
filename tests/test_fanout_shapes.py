"""The shape-directed cases of the fan-out grouping (tests/fanout_cases.py) on a host-only engine: the generic passes of
bifromq_amd/csrc/bmq_fanout_core.h answer every one of them, which proves that the hand-written CSRs and the reference agree before
tests/test_fanout_shapes_gpu.py runs the same table through the gfx950 fast path."""
import pytest

from tests import fanout_cases as FC


@pytest.fixture(scope="module")
def engines():
    e = FC.Engines(-1)
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
    FC.run_bin_count(-1, K)


def test_state_transitions_on_one_engine():
    FC.state_transitions(-1)
