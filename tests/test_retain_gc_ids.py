"""The retain census and the id-based half of RetainStoreCoProc.gc (bmq_retain_tenant_counts, bmq_retain_remove_ids, bmq_retain_message_keys)
over the host executor (device = -1: the same per-item functions as on the device, run on host threads; host engines do not match, so live id
sets, tenant counts and the engine's counters are compared -- the rows of filters are compared on the device, tests/test_retain_gc_ids_gpu.py)."""
import pytest

import bifromq_amd as B
from bifromq_amd.engine import retain_message_key
from oracle import oracle as O
from tests import retain_gc_ref as G


def test_tenant_counts_over_bulk_load_and_churn():
    eng = B.Engine(device=-1)
    try:
        assert eng.retain_tenant_counts() == []                           # no index yet
        m = G.Model(eng).load(G.bulk_items())
        m.check()
        assert eng.retain_tenant_counts() == [(t.encode(), 150) for t in G.BULK]
        G.churn(m)
        m.check()
        got = dict(eng.retain_tenant_counts())
        assert b"empty" not in got and got[b"sys-only"] == 5 and got[b"ov"] == 130
        assert got[b"t1"] == 150 + 97                                     # a bulk-loaded tenant with topics under its shadow: once, the sum
        assert got[b"t0"] == 150 - 19 and len([t for t in got if t.startswith(b"rr-")]) == 70
        assert eng.retain_tenant_counts(tenants_cap=1, cap=1) == m.counts()   # both BMQ_E_NOSPACE paths report the needed sizes
    finally:
        eng.close()


def test_remove_ids_cases_and_readding_gives_the_old_id():
    eng = B.Engine(device=-1)
    try:
        m = G.populated(eng)
        gen = eng.retain_info().generation
        for name, ids in G.removal_cases(m):
            want = m.remove_ids(ids)
            epoch = eng.retain_info().epoch
            assert eng.retain_remove_ids(ids, gen) == want, name
            assert (want > 0) == (name != "dead already"), name
            assert eng.retain_info().epoch == epoch + 1 and eng.retain_info().generation == gen
            m.check()
            assert all(k == b"" for k in eng.retain_message_keys(ids)), name
        # a later add of the same topic gets the same id back
        back = [k for k, i in m.known.items() if k not in m.ids][:40]
        assert len(back) == 40
        out = m.apply([(0, t, p) for t, p in back])
        assert out.tolist() == [m.known[k] for k in back]
        m.check()
        assert eng.retain_remove_ids([], gen) == 0
    finally:
        eng.close()


def test_refusals_change_nothing():
    eng = B.Engine(device=-1)
    try:
        with pytest.raises(B.BmqError) as ei:
            eng.retain_remove_ids([0], 0)                                 # no index: no generation to belong to
        assert ei.value.code == -7
        m = G.populated(eng)
        info = eng.retain_info()
        for ids, gen, code in (([1, 2], info.generation + 1, -7), ([1, 2], info.generation - 1, -7), ([1, 2, int(info.id_bound)], info.generation, -1),
                               ([0xFFFFFFFF], info.generation, -1)):
            with pytest.raises(B.BmqError) as ei:
                eng.retain_remove_ids(ids, gen)
            assert ei.value.code == code
        after = eng.retain_info()
        assert (after.epoch, after.n_topics, after.loaded_removed) == (info.epoch, info.n_topics, info.loaded_removed)
        m.check()
    finally:
        eng.close()


def test_removals_between_compact_begin_and_swap_are_replayed():
    eng = B.Engine(device=-1)
    try:
        m = G.populated(eng)
        gen = eng.retain_info().generation
        eng.retain_compact_begin()
        ids = sorted(m.ids.values())[10:400:3]
        gone = [k for k, i in m.ids.items() if i in set(ids)]
        assert eng.retain_remove_ids(ids + ids[:5], gen) == m.remove_ids(ids) == len(ids)
        assert eng.retain_remove_ids(ids[:7], gen) == 0                   # dead ids are not logged again
        eng.retain_compact_build()
        carried, replayed = eng.retain_compact_swap()
        assert replayed == len(ids) and carried == len(m.ids) + len(ids)
        assert eng.retain_info().generation == gen + 1 and eng.retain_info().n_topics == len(m.ids)
        live = eng.retain_live_ids()
        assert sorted(eng.retain_topics(live)) == sorted(m.ids) and not set(gone) & set(eng.retain_topics(live))
        assert eng.retain_tenant_counts() == m.counts()
        with pytest.raises(B.BmqError) as ei:                             # ids of the generation before the swap
            eng.retain_remove_ids(ids, gen)
        assert ei.value.code == -7
    finally:
        eng.close()


def test_message_keys_equal_the_per_id_composition():
    eng = B.Engine(device=-1)
    try:
        assert eng.retain_message_keys([0, 7]) == [b"", b""]              # no index
        m = G.populated(eng)
        # the topics of the key-schema vectors (KVSchemaUtilTest.java:45-79, the filters without wildcards) under their tenant
        vec = ["/a", "a/b", "a", "/", "a/b/c/"]
        out = m.apply([(0, "tenantA", p) for p in vec])
        assert eng.retain_message_keys(out) == [O.retain_message_key("tenantA", p) for p in vec]
        bound = int(eng.retain_info().id_bound)
        ids = list(range(0, bound, 7)) + [bound - 1, bound, bound + 5, 0xFFFFFFFF]
        live = set(m.ids.values())
        keys = eng.retain_message_keys(ids)
        topics = eng.retain_topics(ids)
        assert len(keys) == len(ids)
        for i, k, (t, p) in zip(ids, keys, topics):
            assert k == (retain_message_key(t, p) if i in live else b""), i
        assert any(k == b"" for k in keys[:-4]) and any(k for k in keys)  # dead ids inside the range, and live ones
        assert [k for k in keys if k] == [O.retain_message_key(*kv) for kv, i in sorted(m.ids.items(), key=lambda x: x[1]) if i in set(ids)]
    finally:
        eng.close()


def test_topics_are_found_by_string_after_the_overlay_table_grew():
    eng = B.Engine(device=-1)
    try:
        G.growth_case(eng, n=6000)
    finally:
        eng.close()
