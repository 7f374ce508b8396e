"""The per-prefix census on the device: the gfx950 kernel k_b_prefix_census (bifromq_amd/csrc/bmq_prefix_kernels.h) over the HBM-resident key store,
through the table of tests/prefix_cases.py -- a device engine and a host-only engine in lockstep through every index state, each answer
compared with the model of tests/hinter_ref.py over the scenario's own set of live keys and the two executors' answers number for number."""
import bisect

import pytest

import bifromq_amd as B
from tests import hinter_ref as R
from tests import prefix_cases as P
from tests.order_cases import K

pytestmark = pytest.mark.gpu


def test_the_table_on_the_device_and_against_the_host_executor():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    counts = P.Scenario([dev, host], lambda i: B.Engine(device=0 if i == 0 else -1)).run()
    for cls in P.expected_classes():
        assert counts[cls] > 0, cls
    info = dev.prefix_census_info()
    assert info.n_nested > 0 and info.max_chain >= 3 and info.n_distinct < info.n_prefixes and info.n_keys_scanned > 0
    dev.close()
    host.close()


def test_the_largest_call_over_a_few_thousand_keys():
    keys = sorted(K(b"t%d" % (i % 5), "s/%d/%d" % (i % 41, i), "0\0in%d\0d" % (i % 3)) for i in range(3000))
    dev, host = B.Engine(device=0).rebuild(keys), B.Engine(device=-1).rebuild(keys)
    distinct = sorted({R.cut_filter(k) for k in keys} | {R.cut_tenant(k) for k in keys} | set(keys) | {k[:n] for k in keys[::7] for n in (1, 2, 5, 9, 12)})
    prefixes = (distinct * (B.BMQ_PREFIX_MAX // len(distinct) + 1))[:B.BMQ_PREFIX_MAX]
    want = dict(zip(distinct, R.census(keys, distinct)))
    got = dev.prefix_census(prefixes)
    assert got.tolist() == [want[p] for p in prefixes]
    assert (got == host.prefix_census(prefixes)).all()
    with pytest.raises(B.BmqError) as ex:
        dev.prefix_census(prefixes + [b""])
    assert ex.value.code == -1
    dev.close()
    host.close()


def test_a_key_store_larger_than_one_turn_per_wave():
    """70 000 keys of 7 tenants, every key deleted and put again eight times over: 630 000 ids, the last 70 000 of them live -- more than
    the 2048 x 4 waves of the bounded grid take in one turn of 64, so every wave carries its sums over several turns; 2 000 filter
    prefixes plus their tenants."""
    n = 70000
    keys = sorted(K(b"t%d" % (i % 7), "s/%d/%d" % (i % 251, i), "0\0in%d\0d" % (i % 3)) for i in range(n))
    eng = B.Engine(device=0).rebuild(keys)
    for _ in range(8):
        for at in range(0, n, 35000):
            eng.apply([(1, k) for k in keys[at:at + 35000]])
            eng.apply([(0, k) for k in keys[at:at + 35000]])
    assert eng.info().next_route_id > 2048 * 256 + n
    filters = [R.cut_filter(k) for k in keys[::35]]
    assert len(filters) == 2000
    levels = [R.cut_tenant(k) + b"s\x00%d\x00" % j for k in keys[:1] + keys[-1:] for j in (0, 10, 250)]  # a level of the filters: dozens of keys each
    prefixes = filters + sorted({R.cut_tenant(k) for k in keys}) + [b""] + levels
    got = eng.prefix_census(prefixes).tolist()
    # the model, by bisect: keys are sorted, a prefix's keys are one stretch of them
    for p, row in zip(prefixes, got):
        lo = bisect.bisect_left(keys, p)
        ub = R.upper_bound(p)
        hi = len(keys) if ub is None else bisect.bisect_left(keys, ub)
        under = keys[lo:hi]
        assert all(k.startswith(p) for k in under[:1] + under[-1:])
        assert row == [len(under), 0, 0, sum(len(k) for k in under)], p
    assert sum(r[0] for r in got[2000:2007]) == n == got[2007][0] and all(r[0] > 10 for r in got[2008:])
    eng.close()
