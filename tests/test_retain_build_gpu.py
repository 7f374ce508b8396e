"""The executor builder of the retained-topic index on the GPU (bmq_config.retain_builder = 1: the k_rb_* kernels of
bifromq_amd/csrc/bmq_retain_build_kernels.h, a device merge sort, radix sorts and scans between them) against the host builder on the same
device and against the oracle's TopicLevelTrie + RetainMatcher, on every load of tests/retain_build_ref.py: ids, stamps, match rows for an
exhaustive set of short filters, match(limit, now), then churn / removal by id / compaction / import on the generation the device built.
The same source on host threads, the image under sanitizers and under the wave emulator: tests/test_retain_build.py."""
import random

import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import retain_build_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

CASES = ["EDGE", "GOLDEN", "DUPS", "WIDE", "DEEP-128", "TENANTS", "SIZE-0", "SIZE-1", "SIZE-63", "SIZE-64", "SIZE-65", "SIZE-257", "WORKLOAD-20000"]
FILTERS = R.filters_up_to_3()


@pytest.fixture(scope="module")
def corpus():
    loads = {ld.name: ld for ld in R.corpus()}
    assert sorted(loads) == sorted(CASES)
    return {name: (ld, R.Model(ld)) for name, ld in loads.items()}


@pytest.fixture(scope="module")
def engines():
    made = []

    def make(rb):
        made.append(B.Engine(device=0, retain_builder=rb))
        return made[-1]
    yield make
    for e in made:
        e.close()


def state(eng, stride=1):
    """what the engine tells of its retained topics by id (stride: the stamps of every stride-th live id -- one call each)"""
    info = eng.retain_info()
    live = eng.retain_live_ids()
    counts = eng.retain_tenant_counts(tenants_cap=1 << 16, cap=1024)
    now = 1_000_000 + 37 * (len(live) // 2) + 2500 * 1000                              # about half of the corpus' stamps have expired by then
    return {"info": (int(info.n_topics), int(info.id_bound), int(info.loaded_topics), int(info.loaded_removed), int(info.added_ids)), "live": live,
            "topics": eng.retain_topics(list(range(int(info.id_bound)))), "stamps": [eng.retain_topic_info(i) for i in live[::stride]],
            "tenant_counts": counts, "expired": [eng.retain_expired(t, now) for t, _ in counts[:3]]}   # (the GC scan skips the tenant's '$' run)


def rows_of(eng, names, ft, filters):
    rp, ids = eng.retain_match_batch(names, ft, filters)
    return U.csr_rows(rp, ids)


@pytest.mark.parametrize("case", CASES)
def test_a_device_built_generation_serves_what_the_host_built_one_and_the_oracle_serve(corpus, engines, case):
    ld, m = corpus[case]
    a, b = engines(0), engines(1)
    ld.rebuild(a), ld.rebuild(b)
    bi = b.retain_build_info()
    assert (bi.builder, bi.fallback) == (1, 0)                                          # a condition: nothing here passes by falling back
    assert a.retain_build_info().builder == 0
    got = {f: int(getattr(bi, f)) for f in ("n_items", "n_topics", "n_tenants", "n_nodes", "n_edges", "n_posts", "n_gp_runs", "n_tokens", "max_depth")}
    assert got == {f: getattr(m, f) for f in got}
    if case == "WIDE":
        assert {31, 32, 33, 300} <= set(m.widths) and m.n_posts and bi.n_edge_overflows > 0 and bi.n_gp_overflows > 0   # else the case proves nothing
    # ---- every id -> topic and stamps ----
    sa, sb = state(a), state(b)
    assert sb["topics"] == m.order and sb["live"] == list(range(m.n_topics))
    assert sb["stamps"] == [(ts, ex, m.expire_at(i)) for i, (ts, ex) in enumerate(m.stamps)]
    assert sb["tenant_counts"] == m.tenant_counts
    assert sa == sb
    # ---- match rows: every filter of <= 3 levels per tenant (+ one nobody holds), against both references ----
    lt = O.LevelTrie(1)
    for i, (t, p) in enumerate(m.order):
        lt.add(t, p, i)
    names = [t.decode() for t in m.tenants] + ["nobody"]
    ft = [t for t in range(len(names)) for _ in FILTERS]
    fl = FILTERS * len(names)
    rows_b = rows_of(b, names, ft, fl)
    assert rows_b == rows_of(a, names, ft, fl)
    exp = [sorted(lt.match(names[t], f)) for t, f in zip(ft, fl)]
    bad = [(names[t], f, g[:8], e[:8]) for t, f, g, e in zip(ft, fl, rows_b, exp) if g != e]
    assert not bad, bad[:5]
    if case == "GOLDEN":
        for t in names[:-1]:
            for f, topics in R.golden_rows():
                assert sorted(m.order[i][1] for i in b.retain_match(t, f)) == topics and all(m.order[i][0] == t for i in b.retain_match(t, f)), (t, f)
    # ---- match(limit, now) with a third of the stamps expired ----
    if m.n_topics:
        now = sorted(m.expire_at(i) for i in range(m.n_topics))[m.n_topics // 3]
        for limit in (1, 10, 65):
            rp_b, ids_b, cnt_b = b.retain_match_limited(names, ft, fl, [limit] * len(fl), now_ms=now)
            rp_a, ids_a, cnt_a = a.retain_match_limited(names, ft, fl, [limit] * len(fl), now_ms=now)
            assert rp_b.tolist() == rp_a.tolist() and ids_b.tolist() == ids_a.tolist() and cnt_b.tolist() == cnt_a.tolist()
            assert U.csr_rows(rp_b, ids_b) == [[i for i in e if m.expire_at(i) > now][:limit] for e in exp], limit


@pytest.mark.parametrize("case", [c for c in CASES if c != "SIZE-0"])
def test_churn_remove_ids_compact_and_import_on_a_generation_the_device_built(corpus, engines, case):
    ld, m = corpus[case]
    rnd = random.Random(11)
    a, b = engines(0), engines(1)
    ld.rebuild(a), ld.rebuild(b)
    names = [t.decode() for t in m.tenants] + ["fresh-tenant"]
    probe = ["#", "+", "+/+", "a/#", "a/+", "+/b", "a/b/added", "+/+/added", "sibling", "x/y", "$a/#", "w0/#", "+/sibling"]
    ft = [t for t in range(len(names)) for _ in probe]
    fl = probe * len(names)

    stride = max(1, m.n_topics // 256)

    def same():
        assert state(a, stride) == state(b, stride)
        assert rows_of(a, names, ft, fl) == rows_of(b, names, ft, fl)
    cn, ot, ops = R.churn_ops(m, rnd)
    assert list(a.retain_apply_batch(cn, ot, ops)) == list(b.retain_apply_batch(cn, ot, ops))   # adds below loaded prefixes find them in the device-built index
    same()
    gone = rnd.sample(range(m.n_topics), min(m.n_topics, 5))
    assert a.retain_remove_ids(gone, a.retain_info().generation) == b.retain_remove_ids(gone, b.retain_info().generation)
    same()
    for _ in range(2):                                                                  # ids are ranks again; the second load starts from a load the device made
        a.retain_compact(), b.retain_compact()
        same()
        assert b.retain_live_ids() == list(range(int(b.retain_info().n_topics)))
        assert (b.retain_build_info().builder, b.retain_build_info().fallback) == (1, 0)
    c, d = engines(0), engines(1)
    assert c.retain_import(a) == d.retain_import(b) == (int(b.retain_info().n_topics), 0)       # into an empty engine: a bulk load on the device
    assert (d.retain_build_info().builder, d.retain_build_info().fallback) == (1, 0)
    sd, sb = state(d, stride), state(b, stride)
    assert state(c, stride) == sd and sd["topics"] == sb["topics"] and sd["stamps"] == sb["stamps"]
    assert rows_of(d, names, ft, fl) == rows_of(b, names, ft, fl)


def test_a_topic_of_129_levels_is_built_by_the_host_builder_and_served_the_same(engines):
    ld = R.deep(levels=(17, R.RB_MAX_DEPTH, R.RB_MAX_DEPTH + 1))
    m = R.Model(ld)
    a, b = engines(0), engines(1)
    ld.rebuild(a), ld.rebuild(b)
    bi = b.retain_build_info()
    assert (bi.builder, bi.fallback, bi.max_depth) == (0, 1, R.RB_MAX_DEPTH + 1)
    assert state(a) == state(b) and state(b)["topics"] == m.order
    names = [t.decode() for t in m.tenants]
    ft = [t for t in range(len(names)) for _ in FILTERS]
    assert rows_of(a, names, ft, FILTERS * len(names)) == rows_of(b, names, ft, FILTERS * len(names))
