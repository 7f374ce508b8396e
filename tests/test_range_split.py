"""Split and merge of the route index by KV boundary (bmq_routes_count_in, bmq_compact_begin_in, bmq_routes_import) over the host
executor (device = -1: the same index code and the same boundary predicate as on the device, run on host threads; host engines do not match,
so key sets are compared).  Every expected value is Python's `start <= k < end` on bytes."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import range_split_ref as R


def _key(i, t):
    return B.route_key(t, ["a/%d/+", "b/%d/#", "%d/x", "+/%d"][i % 4] % i, 1, "0\0inbox%d\0d%d" % (i, i % 3))


def _model(n_per_tenant=60):
    return set(_key(i, t) for t in R.TENANTS for i in range(n_per_tenant))


def _tenants_of(keys):
    return {k[3:3 + int.from_bytes(k[1:3], "big")] for k in keys}


def test_the_directed_table_is_what_the_issue_asks_for():
    R.assert_table_covers(R.table_keys())


def test_count_in_over_the_directed_boundary_table():
    keys = R.table_keys()
    assert 35 <= len(keys) <= 45
    eng = B.Engine(device=-1)
    try:
        assert eng.count_in() == (0, 0) and eng.count_in(start=b"", end=b"\xff") == (0, 0)   # no index yet
        eng.rebuild(keys)
        assert R.check_table(eng, keys) > 1000
        dead = keys[::3]
        eng.apply([(1, k) for k in dead])                      # dead ids between the live ones
        live = sorted(set(keys) - set(dead))
        R.check_table(eng, live)
        assert eng.count_in(end=b"") == (0, 0)                 # NULL_BOUNDARY: valid, holds nothing
        assert eng.count_in(start=b"") == (len(live), sum(map(len, live)))
        assert R.live_keys(eng) == live                        # the index is not changed by counting
    finally:
        eng.close()


@pytest.mark.parametrize("chunk", [1, 63, 64, 65, None])
def test_bounded_compaction_keeps_what_is_inside(chunk):
    """deleted ids interleaved, blocking mutations inside and outside the boundary between the polls; after the swap the live keys are the
    model restricted to the boundary, `replayed` counts the ops inside only, tenants that left are gone"""
    model = _model()
    eng = B.Engine(device=-1)
    try:
        eng.rebuild(sorted(model))
        dels = sorted(model)[::3]
        eng.apply([(1, k) for k in dels])
        model.difference_update(dels)
        # keys order by tenant LENGTH first (00 | u16be(len) | tenant): from inside tenant "a", over all of "b", to inside tenant "ab";
        # the tenants "" and "租户" leave as a whole
        start, end = R.tenant_prefix("a") + b"b", _key(30, "ab")
        n_ids = int(eng.info().next_route_id)
        step = n_ids + 7 if chunk is None else chunk
        eng.compact_begin(start=start, end=end)
        serial, inside_ops, polls, done = 1000, 0, 0, 0
        while done < 1000:
            done = eng.compact_poll(step)
            polls += 1
            if polls % max(1, (n_ids // step) // 6) == 0 or chunk is None:
                adds = [_key(serial + j, t) for j, t in enumerate(R.TENANTS)] + [_key(serial, "born-%d" % serial), _key(serial, "aa")]   # "aa": a tenant born inside
                gone = sorted(model)[serial % 7::41]
                ops = [(1, k) for k in gone] + [(0, k) for k in adds] + [(0, gone[0]), (1, gone[0])]
                eng.apply(ops)
                inside_ops += len(R.inside([k for _, k in ops], start, end))
                model.difference_update(gone)
                model.update(adds)
                serial += 10
                assert R.live_keys(eng) == sorted(model)       # the serving generation holds everything until the swap
        assert polls >= (1 if chunk is None else n_ids // step)
        carried, replayed = eng.compact_swap()
        want = R.inside(sorted(model), start, end)
        assert R.live_keys(eng) == want
        assert replayed == inside_ops and inside_ops > 0
        info = eng.info()
        assert info.n_routes == len(want) and info.n_tenants == len(_tenants_of(want))
        assert carried <= len(want) + replayed and carried >= len(want) - replayed
        assert eng.count_in() == (len(want), sum(map(len, want)))
        # the engine does not police later mutations against the boundary
        eng.apply([(0, _key(1, "zzz-outside"))])
        assert R.live_keys(eng) == sorted(want + [_key(1, "zzz-outside")])
    finally:
        eng.close()


def test_a_tenant_that_leaves_takes_no_room_and_abort_changes_nothing():
    model = sorted(_model())
    a, b = B.Engine(device=-1), B.Engine(device=-1)
    try:
        for e in (a, b):
            e.rebuild(model)
            e.apply([(1, k) for k in model[::5]])
        live = sorted(set(model) - set(model[::5]))
        a.compact_begin()
        while a.compact_poll(64) < 1000:
            pass
        a.compact_swap()
        cut = R.tenant_prefix("b")                              # "" and "a" stay; "b", "ab" and "租户" leave as a whole
        before = b.info()
        b.compact_begin(end=cut)
        b.compact_poll(64)
        b.compact_abort()                                       # abort: the serving generation is untouched
        after = b.info()
        assert (after.generation, after.n_routes, after.trie_slots, after.next_route_id) == (before.generation, before.n_routes, before.trie_slots, before.next_route_id)
        assert R.live_keys(b) == live
        b.compact_begin(end=cut)
        while b.compact_poll(64) < 1000:
            pass
        carried, replayed = b.compact_swap()
        want = R.inside(live, None, cut)
        assert (carried, replayed) == (len(want), 0) and R.live_keys(b) == want
        assert b.info().n_tenants == 2 and a.info().n_tenants == 5
        assert b.info().trie_slots < a.info().trie_slots
        assert b.info().generation == before.generation + 1
    finally:
        a.close()
        b.close()


def _split_points(model):
    ks = sorted(model)
    return {"tenant border": R.tenant_prefix("ab"), "inside a tenant": ks[len(ks) // 2], "below every key": b"\0", "above every key": b"\xff",
            "empty start": b""}


@pytest.mark.parametrize("where", ["tenant border", "inside a tenant", "below every key", "above every key", "empty start"])
def test_split(where):
    model = _model(40)
    s = _split_points(model)[where]
    a, b = B.Engine(device=-1), B.Engine(device=-1)
    try:
        a.rebuild(sorted(model))
        dels = sorted(model)[1::4]
        a.apply([(1, k) for k in dels])
        model.difference_update(dels)
        upper = R.inside(sorted(model), s, None)
        assert b.import_routes(a, start=s) == (len(upper), 0)   # the new sibling: [s, end)
        assert R.live_keys(a) == sorted(model)                  # the source is not changed by lending its keys
        a.compact_begin(end=s)                                  # the range that shrinks: [start, s)
        while a.compact_poll(4096) < 1000:
            pass
        a.compact_swap()
        ka, kb = R.live_keys(a), R.live_keys(b)
        assert kb == upper and ka == R.inside(sorted(model), None, s)
        assert not set(ka) & set(kb) and sorted(ka + kb) == sorted(model)
        assert b.info().n_routes == len(kb) and b.info().n_tenants == len(_tenants_of(kb))
    finally:
        a.close()
        b.close()


def test_merge_keeps_the_ids_of_the_destination_and_counts_duplicates():
    model = sorted(_model(50))
    s = model[len(model) // 3]
    a, b = B.Engine(device=-1), B.Engine(device=-1)
    try:
        a.rebuild(R.inside(model, None, s))
        shared = R.inside(model, None, s)[::9]                  # keys both ranges hold: stored once, counted as dups
        b.rebuild(sorted(R.inside(model, s, None) + shared))
        b.apply([(1, k) for k in shared[:3]] + [(0, k) for k in shared[:3]])   # dead ids in the source
        ids = np.arange(int(a.info().next_route_id), dtype=np.uint32)
        before = a.route_keys(ids)
        info0 = a.info()
        imported, dups = a.import_routes(b)
        assert (imported, dups) == (len(R.inside(model, s, None)), len(shared))
        assert R.live_keys(a) == model
        assert a.route_keys(ids) == before                      # ids a handed out stay valid
        info1 = a.info()
        assert info1.generation == info0.generation and info1.epoch > info0.epoch and info1.n_routes == len(model)
        assert a.import_routes(b) == (0, info1.n_routes - len(R.inside(model, None, s)) + len(shared))   # again: everything is a duplicate
        assert a.import_routes(b, start=s, end=s + b"\x00") == (0, 1)
        assert B.Engine(device=-1).import_routes(B.Engine(device=-1)) == (0, 0)    # nothing to import from an engine without an index
        assert R.live_keys(b) == sorted(R.inside(model, s, None) + shared)
    finally:
        a.close()
        b.close()


def test_an_import_of_more_than_one_chunk():
    """70 000 ids in the source: two chunks of the import, with dead ids, into an engine that knows none of the tenants"""
    keys = sorted(B.route_key("t%d" % (i % 7), "c/%d" % i, 1, "0\0r\0d") for i in range(70000))
    a, b = B.Engine(device=-1), B.Engine(device=-1)
    try:
        a.rebuild(keys)
        a.apply([(1, k) for k in keys[::1000]])
        live = sorted(set(keys) - set(keys[::1000]))
        s = R.tenant_prefix("t3")
        assert b.import_routes(a, start=s) == (len(R.inside(live, s, None)), 0)
        assert R.live_keys(b) == R.inside(live, s, None)
        assert b.count_in(end=s) == (0, 0) and a.count_in(start=s)[0] == b.info().n_routes
    finally:
        a.close()
        b.close()


def test_refusals():
    model = sorted(_model(10))
    a, b = B.Engine(device=-1), B.Engine(device=-1)

    def code(f, *args, **kw):
        with pytest.raises(B.BmqError) as ei:
            f(*args, **kw)
        return ei.value.code

    try:
        a.rebuild(model)
        b.rebuild(model[:5])
        assert code(a.import_routes, a) == -1                                   # dst is src
        for bad in ((b"b", b"a"), (b"a", b"a"), (b"", b""), (b"a\x00", b"a")):  # start >= end, on all three calls
            assert code(a.count_in, *bad) == -1
            assert code(a.compact_begin, *bad) == -1
            assert code(a.import_routes, b, *bad) == -1
        a.compact_begin(end=b"\xff")
        assert code(a.import_routes, b) == -7                                   # the destination's compaction is running
        assert code(b.import_routes, a) == -7                                   # the source's
        assert code(a.compact_begin) == -7
        a.compact_abort()
        assert b.import_routes(a) == (len(model) - 5, 5)
        assert R.live_keys(b) == model
    finally:
        a.close()
        b.close()
