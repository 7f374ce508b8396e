"""The range fan-out split hinter (bifromq_amd/hinter.py) over a device engine: the mutation script of tests/hinter_cases.py step by step against
the model of tests/hinter_ref.py, and a filter of 70 000 routes whose split key at the scale of 66 000 comes from two chained windows."""
import pytest

import bifromq_amd as B
from bifromq_amd import hinter as H
from tests import hinter_cases as S
from tests.order_cases import K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("granularity", H.GRANULARITIES)
def test_the_mutation_script_against_the_model_on_the_device(granularity):
    eng = B.Engine(device=0)
    counts = S.Script(eng, granularity).run()
    for cls in S.expected_classes(granularity):
        assert counts[cls] > 0, cls
    eng.close()


def test_a_split_key_behind_more_keys_than_one_window_holds():
    n, scale = 70000, 66000
    assert scale > B.BMQ_WINDOW_MAX
    keys = sorted(K(b"big", "hot/+/filter", "0\0in%05d\0d" % i) for i in range(n))
    others = [K(b"a", "in/front"), K(b"big", "hot/+/filtes", "0\0behind\0d"), K(b"zz", "behind")]
    eng = B.Engine(device=0).rebuild(sorted(keys + others))
    h = H.RangeFanoutSplitHinter(eng, scale)
    before = eng.window_info().n_calls
    h.record_mutate([(0, keys[7]), (0, others[0])])
    p = H.filter_prefix(keys[0])
    assert list(h.splits) == [p]
    data_size, record_size, key = h.splits[p]
    assert key == keys[scale] and (data_size, record_size) == (sum(len(k) for k in keys), len(keys[0]))
    assert eng.window_info().n_calls - before == 2  # two chained windows
    assert h.estimate() == {"type": "fanout_split_hinter", "split_key": keys[scale], "load": {"fanout_topicfilters": 1, "fanout_scale": float(n)}}
    assert h.split_key_at(p, n) == others[1] and h.split_key_at(p, n + 2) is None
    eng.close()
