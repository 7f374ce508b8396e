"""The per-prefix census of the route index (bmq_routes_prefix_census: what FanoutSplitHinter.doEstimate asks the KV range per key prefix of a
mutation batch, for all prefixes in one pass) over the host executor (device = -1: the same per-key function as on the device, run on host
threads).  Every expected value is tests/hinter_ref.py's `startswith` over the scenario's own set of live keys (tests/prefix_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from tests import hinter_ref as R
from tests import prefix_cases as P
from tests.order_cases import K, base_keys


def _raw(eng, prefixes, out):
    data, off = B.pack(prefixes)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return _lib.lib().bmq_routes_prefix_census(eng.h, p(data), p(off), len(prefixes), p(out))


def test_the_table_of_prefix_classes_through_every_index_state():
    eng = B.Engine(device=-1)
    counts = P.Scenario([eng], lambda i: B.Engine(device=-1)).run()
    for cls in P.expected_classes():
        assert counts[cls] > 0, cls
    eng.close()


def test_the_model_cuts_keys_as_the_package_does():
    from bifromq_amd import hinter as H
    for k in base_keys() + P.extras():
        assert (R.cut_tenant(k), R.cut_filter(k), R.upper_bound(k)) == (H.tenant_prefix(k), H.filter_prefix(k), H.upper_bound(k))
        if all(x < 0x80 for x in R.cut_tenant(k)):
            flag, tenant, _, _ = B.decode_route_key(k)
            assert R.flag_of(k) == flag and R.cut_tenant(k)[3:] == tenant.encode()
    assert H.upper_bound(b"") is None and H.upper_bound(b"\xff\xff") is None and H.upper_bound(b"a\xff\xff") == b"b" and H.upper_bound(b"a\x00") == b"a\x01"


def test_refusals_and_the_largest_call():
    keys = sorted(set(base_keys()) | set(P.extras()))
    eng = B.Engine(device=-1).rebuild(keys)
    assert B.BMQ_PREFIX_MAX == 65536 == eng.prefix_census_info().prefix_max
    assert eng.prefix_census([]).shape == (0, 4)  # n = 0
    n = B.BMQ_PREFIX_MAX + 1
    prefixes = [keys[i % len(keys)][:1 + i % 40] for i in range(n)]
    out = np.full(4 * n, 0xC0DE, dtype=np.uint64)
    before = (eng.info().epoch, eng.prefix_census_info().n_calls)
    assert _raw(eng, prefixes, out) == -1 and (out == 0xC0DE).all()  # the canary is untouched
    assert (eng.info().epoch, eng.prefix_census_info().n_calls) == before
    with pytest.raises(B.BmqError) as ex:
        eng.prefix_census(prefixes)
    assert ex.value.code == -1
    got = eng.prefix_census(prefixes[:-1])  # n = BMQ_PREFIX_MAX works
    distinct = sorted(set(prefixes[:-1]))
    want = dict(zip(distinct, R.census(keys, distinct)))
    assert got.tolist() == [want[p] for p in prefixes[:-1]]
    # a prefix of 16 MiB: refused, nothing written
    big = np.zeros((1 << 24) + 16, dtype=np.uint8)
    off = np.array([0, 1, 1 + (1 << 24)], dtype=np.uint32)
    out = np.full(8, 0xC0DE, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert _lib.lib().bmq_routes_prefix_census(eng.h, p(big), p(off), 2, p(out)) == -1 and (out == 0xC0DE).all()
    off[2] = 1 << 24  # one byte less: fine (prefixes 00 and 00 * (16 MiB - 1))
    assert _lib.lib().bmq_routes_prefix_census(eng.h, p(big), p(off), 2, p(out)) == 0
    assert out.reshape(2, 4).tolist() == R.census(keys, [b"\x00", b"\x00\x00\x00\x00\x00\x00\x00\x00"])[:1] + [[0, 0, 0, 0]]
    eng.close()


def test_the_info_counters_move_as_stated():
    keys = sorted(set(base_keys()) | set(P.extras()))
    eng = B.Engine(device=-1).rebuild(keys)
    i0 = eng.prefix_census_info()
    assert (i0.struct_size, i0.n_calls, i0.n_prefixes, i0.n_distinct, i0.n_nested, i0.n_keys_scanned, i0.max_chain) == (C.sizeof(_lib.PrefixCensusInfo), 0, 0, 0, 0, 0, 0)
    k = keys[len(keys) // 2]
    eng.prefix_census([b"", R.cut_tenant(k), R.cut_filter(k), k, k, b""])  # a chain of three parent links, two repeats
    i1 = eng.prefix_census_info()
    assert (i1.n_calls, i1.n_prefixes, i1.n_distinct, i1.n_nested, i1.n_keys_scanned, i1.max_chain) == (1, 6, 4, 3, len(keys), 3)
    assert i1.n_distinct < i1.n_prefixes and i1.last_ms > 0
    eng.prefix_census([K(b"sib", "a"), K(b"sib", "b")])  # siblings: no parent
    i2 = eng.prefix_census_info()
    assert (i2.n_calls, i2.n_prefixes, i2.n_distinct, i2.n_nested, i2.n_keys_scanned, i2.max_chain) == (2, 8, 6, 3, 2 * len(keys), 3)
    eng.close()


def test_python_and_library_agree_on_the_abi():
    assert {"bmq_routes_prefix_census", "bmq_routes_prefix_census_info_get"} <= set(_lib.ABI_SYMBOLS)
    assert C.sizeof(_lib.PrefixCensusInfo) == 64
