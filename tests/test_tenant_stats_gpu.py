"""The per-tenant census of the route index on the device (k_b_census, bmq_census_kernels.h) against tests/tenant_stats_ref.py's brute force
and against the host executor: the directed populations and boundaries of tests/test_tenant_stats.py, churn that makes a tenant outgrow its
region, a generation change, and one population with more key references than the saturated grid covers in four turns."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import range_split_ref as R
from tests import tenant_stats_ref as T

pytestmark = pytest.mark.gpu


def test_census_of_the_directed_population_on_the_device():
    keys = T.directed_keys()
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        assert dev.routes_tenant_stats() == []
        for e in (dev, host):
            e.rebuild(sorted(keys))                                      # key order: every tenant a run of ids
        assert T.check(dev, keys, other=host) > 20
        dead = T.directed_deletes(keys)
        for e in (dev, host):
            e.apply([(1, k) for k in dead])
        live = sorted(set(keys) - set(dead))
        epoch = dev.info().epoch
        T.check(dev, live, other=host)
        assert b"gone" not in [r[0] for r in dev.routes_tenant_stats()]
        assert dev.routes_tenant_stats(tenants_cap=1, cap=1) == T.census(live)
        assert dev.info().epoch == epoch and R.live_keys(dev) == live    # the index is unchanged
    finally:
        dev.close(), host.close()


def test_census_of_interleaved_tenants_and_a_match_row_unchanged_on_the_device():
    keys = T.interleaved_keys()
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        for e in (dev, host):
            e.apply([(0, k) for k in keys])                              # ids in op order: 64 tenants in the 64 lanes of a wave
        row0, ids0 = dev.match_batch(["rr-07"], [0], ["a/0/zz"])
        assert len(ids0) == 1
        s = sorted(keys)
        T.check(dev, keys, other=host, bounds=[(None, None), (None, s[170]), (s[99], s[300]), (None, b""), (s[-1] + b"\0", None)])
        gone = keys[::3]
        for e in (dev, host):
            e.apply([(1, k) for k in gone])
        T.check(dev, sorted(set(keys) - set(gone)), other=host, bounds=[(None, None), (s[60], None)])
        row1, ids1 = dev.match_batch(["rr-07"], [0], ["a/0/zz"])
        assert row1.tolist() == row0.tolist() and ids1.tolist() == ids0.tolist()
    finally:
        dev.close(), host.close()


def test_census_after_a_tenant_outgrew_its_region_and_after_a_generation_change():
    keys = T.directed_keys()
    dev = B.Engine(device=0)
    try:
        dev.rebuild(sorted(keys))
        grow = [B.route_key(b"a", "grow/%d/+/x" % i, 1 + i % 3, "0\0g%d\0d" % i if i % 3 == 0 else "g%d" % (i % 5)) for i in range(3000)]
        late = [T.key(b"late-tenant", i) for i in range(70)]
        dev.apply([(0, k) for k in grow + late] + [(1, k) for k in keys[5::9]])
        model = (set(keys) | set(grow) | set(late)) - set(keys[5::9])
        T.check(dev, sorted(model))
        cut = T.tenant_prefix(b"tenant-12-by")
        dev.compact_begin(end=cut)
        dev.compact_poll(500)
        assert dev.routes_tenant_stats() == T.census(sorted(model))      # the serving generation, between polls
        while dev.compact_poll(4096) < 1000:
            pass
        dev.compact_swap()
        want = T.census(sorted(model), None, cut)
        assert dev.routes_tenant_stats() == want and sum(sum(r[1:4]) for r in want) == dev.info().n_routes
    finally:
        dev.close()


def test_census_of_more_references_than_the_saturated_grid_covers_in_four_turns():
    """2.2 M keys of the workload generator: the grid stops growing at 2048 workgroups x 4 waves x 4 turns x 64 ids = 2 097 152 references,
    beyond that every wave takes more turns.  Compared through the sum identities and a per-tenant numpy count."""
    w = B.Workload(0xB1F20071, 275, 8000, 1)
    data, off = w.keys_packed()
    n = len(off) - 1
    assert n > 2048 * 4 * 4 * 64
    end = off[1:].astype(np.int64)
    rl = data[end - 2].astype(np.int64) * 256 + data[end - 1]
    flag = data[end - 3 - rl].astype(np.int64)
    tf = w.tenant_first().astype(np.int64)
    tenant = np.searchsorted(tf[1:], np.arange(n), side="right")
    klen = (off[1:].astype(np.int64) - off[:-1].astype(np.int64))
    names = [t.encode() for t in w.tenants()]
    cnt = np.zeros((len(names), 4), dtype=np.int64)
    np.add.at(cnt, (tenant, flag - 1), 1)
    np.add.at(cnt, (tenant, 3), klen)
    want = sorted((names[t],) + tuple(int(v) for v in cnt[t]) for t in range(len(names)))
    dev = B.Engine(device=0)
    try:
        dev.rebuild(packed=(data, off))
        assert int(dev.info().next_route_id) == n
        got = dev.routes_tenant_stats(cap=512, tenants_cap=1 << 16)
        assert got == want
        assert (sum(r[1] + r[2] + r[3] for r in got), sum(r[4] for r in got)) == dev.count_in() == (n, int(klen.sum()))
        mid = bytes(data[off[n // 2]:off[n // 2 + 1]])
        half = dev.routes_tenant_stats(end=mid, cap=512, tenants_cap=1 << 16)
        assert (sum(r[1] + r[2] + r[3] for r in half), sum(r[4] for r in half)) == dev.count_in(end=mid)
    finally:
        dev.close()
