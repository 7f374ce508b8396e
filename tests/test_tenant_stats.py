"""The per-tenant census of the route index (bmq_routes_tenant_stats: what TenantsStats.doReset counts while it walks the range) over the host
executor (device = -1: the same per-key function as on the device, run on host threads).  Every expected value is tests/tenant_stats_ref.py's
brute force over the key list."""
import ctypes as C

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from tests import range_split_ref as R
from tests import tenant_stats_ref as T


def _directed(device=-1):
    keys = T.directed_keys()
    eng = B.Engine(device=device)
    eng.rebuild(sorted(keys))
    return eng, keys


def test_the_reference_parses_what_the_codec_writes():
    for k in T.directed_keys()[::17] + T.interleaved_keys()[::31]:
        flag, tenant, _, _ = B.decode_route_key(k)
        assert T.parse(k) == (tenant.encode(), flag)
    assert {len(t) for t in T.TENANTS} >= {0, 1, 12, 13, 40} and any(x >= 0x80 for t in T.TENANTS for x in t)


def test_census_of_the_directed_population_over_the_boundary_table():
    eng, keys = _directed()
    try:
        assert B.Engine(device=-1).routes_tenant_stats() == []           # no index yet
        assert T.check(eng, keys) > 20
        full = eng.routes_tenant_stats()
        assert [r[0] for r in full] == sorted(T.TENANTS) and [r[1] + r[2] + r[3] for r in full] == [n for _, n in sorted(zip(T.TENANTS, T.RUNS))]
        assert all(r[1] and r[2] and r[3] for r in full if sum(r[1:4]) >= 20)  # flags mixed inside one tenant
        dead = T.directed_deletes(keys)
        before = (eng.info().epoch, eng.info().next_route_id)
        eng.apply([(1, k) for k in dead])
        live = sorted(set(keys) - set(dead))
        after_apply = (eng.info().epoch, eng.info().next_route_id)
        T.check(eng, live)
        assert b"gone" not in [r[0] for r in eng.routes_tenant_stats()]  # every route deleted: absent
        assert eng.routes_tenant_stats(end=b"") == [] and eng.routes_tenant_stats(start=live[-1] + b"\0") == []
        # the index is unchanged by counting
        assert (eng.info().epoch, eng.info().next_route_id) == after_apply != before
        assert R.live_keys(eng) == live
    finally:
        eng.close()


def test_census_of_tenants_interleaved_through_the_apply_path():
    keys = T.interleaved_keys()
    a, b = B.Engine(device=-1), B.Engine(device=-1)
    try:
        a.apply([(0, k) for k in keys])                                  # ids in op order: round-robin across 70 tenants
        b.rebuild(sorted(keys))
        assert len(a.routes_tenant_stats()) == 70
        T.check(a, keys, other=b, bounds=[(None, None), (None, sorted(keys)[170]), (sorted(keys)[99], sorted(keys)[300]), (None, b"")])
        gone = keys[::3]
        a.apply([(1, k) for k in gone])
        T.check(a, sorted(set(keys) - set(gone)), bounds=[(None, None), (sorted(keys)[60], None)])
    finally:
        a.close(), b.close()


def test_both_nospace_paths_report_the_needed_sizes():
    eng, keys = _directed()
    try:
        want = T.census(keys)
        n_ten, n_bytes = len(want), sum(len(r[0]) for r in want)
        L = _lib.lib()
        n, nb = C.c_uint32(), C.c_uint64()
        names, off, st = np.zeros(n_bytes, dtype=np.uint8), np.zeros(n_ten + 1, dtype=np.uint64), np.full(4 * n_ten, 77, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        # too few rows: nothing but the sizes
        assert L.bmq_routes_tenant_stats(eng.h, 0, None, 0, None, 0, p(names), n_bytes, p(off), p(st), n_ten - 1, C.byref(n), C.byref(nb)) == -3
        assert (n.value, nb.value) == (n_ten, n_bytes) and st[0] == 77
        # rows fit, the name bytes do not: sizes, offsets and numbers
        n.value, nb.value = 0, 0
        assert L.bmq_routes_tenant_stats(eng.h, 0, None, 0, None, 0, p(names), n_bytes - 1, p(off), p(st), n_ten, C.byref(n), C.byref(nb)) == -3
        assert (n.value, nb.value) == (n_ten, n_bytes) and int(off[n_ten]) == n_bytes and st.reshape(-1, 4).tolist() == [list(r[1:]) for r in want]
        assert L.bmq_routes_tenant_stats(eng.h, 0, None, 0, None, 0, p(names), n_bytes, p(off), p(st), n_ten, None, None) == 0
        assert names.tobytes() == b"".join(r[0] for r in want)
        assert eng.routes_tenant_stats(tenants_cap=1, cap=1) == want     # the Python wrapper grows both
        # malformed boundaries are refused as bmq_routes_count_in refuses them
        with pytest.raises(B.BmqError) as ei:
            eng.routes_tenant_stats(start=b"b", end=b"a")
        assert ei.value.code == -1
    finally:
        eng.close()


def test_census_reads_the_serving_generation_during_a_compaction_and_the_new_one_after_the_swap():
    eng, keys = _directed()
    try:
        dead = T.directed_deletes(keys)
        eng.apply([(1, k) for k in dead])
        model = set(keys) - set(dead)
        cut = T.tenant_prefix(b"tenant-12-by")                           # tenants of up to 2 bytes and the shorter ones stay
        eng.compact_begin(end=cut)
        eng.compact_poll(100)
        assert eng.routes_tenant_stats() == T.census(sorted(model))      # between polls: the serving generation, all its keys
        extra = [T.key(b"a", 1000 + i) for i in range(5)] + [T.key(b"zz-late", 1)]
        eng.apply([(0, k) for k in extra])
        model.update(extra)
        assert eng.routes_tenant_stats() == T.census(sorted(model))
        while eng.compact_poll(100) < 1000:
            pass
        assert eng.routes_tenant_stats(start=cut) == T.census(sorted(model), cut, None)
        eng.compact_swap()
        want = T.census(sorted(model), None, cut)
        assert eng.routes_tenant_stats() == want and sum(sum(r[1:4]) for r in want) == eng.info().n_routes
        assert eng.routes_tenant_stats(start=cut) == []
    finally:
        eng.close()
