"""The range fan-out split hinter (bifromq_amd/hinter.py: DW/hinter/FanoutSplitHinter.java at per-filter granularity over Engine.prefix_census and
chained key-ordered windows) on a host-only engine, step by step against the model of tests/hinter_ref.py over the mutation script of
tests/hinter_cases.py, at split_at_scale = 5."""
import pytest

import bifromq_amd as B
from bifromq_amd import hinter as H
from tests import hinter_cases as S
from tests import hinter_ref as R
from tests.order_cases import K


@pytest.mark.parametrize("granularity", H.GRANULARITIES)
def test_the_mutation_script_against_the_model(granularity):
    eng = B.Engine(device=-1)
    counts = S.Script(eng, granularity).run()
    for cls in S.expected_classes(granularity):
        assert counts[cls] > 0, cls
    eng.close()


def test_record_mutate_asks_the_index_once_per_batch():
    eng = B.Engine(device=-1).rebuild([])
    h = H.RangeFanoutSplitHinter(eng, 3)
    ops = [(0, K(b"t%d" % (i % 2), "f/%d" % (i % 3), S.recv(i))) for i in range(60)]
    eng.apply(ops)
    before = eng.prefix_census_info()
    h.record_mutate(ops)
    after = eng.prefix_census_info()
    distinct = {R.cut_filter(k) for _, k in ops}
    assert (after.n_calls - before.n_calls, after.n_prefixes - before.n_prefixes) == (1, len(distinct))
    ref = R.Hinter(lambda: sorted(k for _, k in ops), 3)
    ref.record_mutate(ops)
    assert h.splits == ref.map and h.splits


def test_split_key_at_and_the_helpers():
    ks = sorted(K(b"t", "g/%d" % i) for i in range(50))
    eng = B.Engine(device=-1).rebuild(ks)
    h = H.RangeFanoutSplitHinter(eng, 5)
    assert h.split_key_at(b"", 0) == ks[0] and h.split_key_at(ks[5][:-3], 10) == ks[15] == eng.split_key_after(ks[5][:-3], 10)
    assert h.split_key_at(ks[45], 4) == ks[49] and h.split_key_at(ks[45], 5) is None and h.split_key_at(b"\xff", 0) is None
    k = K(b"tenant", "a/b/c", "0\0inbox\0d")
    assert H.tenant_prefix(k) == b"\x00\x00\x06tenant" and H.filter_prefix(k) == b"\x00\x00\x06tenanta\x00b\x00c\x00\x00" and k.startswith(H.filter_prefix(k))
    assert H.filter_prefix(K(b"tenant", "$share/g/a/b/c", "")) == H.filter_prefix(k)  # normal and shared routes of a filter lie under one prefix
    with pytest.raises(ValueError):
        H.filter_prefix(b"\x00\x00\x01a")
    with pytest.raises(ValueError):
        H.RangeFanoutSplitHinter(eng, 5, "range")
    assert H.RangeFanoutSplitHinter(eng).split_at_scale == 100000  # FanoutSplitHinterFactory's default
    eng.close()
