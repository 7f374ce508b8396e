"""Split and merge of the retained-topic index by KV boundary on the device: k_r_boundary behind bmq_retain_count_in / bmq_retain_ids_in /
bmq_retain_compact_begin_in / bmq_retain_import, against Python's `start <= k < end` over oracle.retain_message_key, against a host engine
that holds the same topics, and -- device engines match -- against an oracle.LevelTrie restricted to each half."""
import threading

import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import retain_gc_ref as G
from tests import retain_split_ref as R

pytestmark = pytest.mark.gpu

FILTERS = ["#", "+/+", "s/+/x", "$sys/#", "a/b/c"]
NOW = 1_700_000_000_000


def _populate(eng, which):
    """retain_gc_ref's population (dead ids, overlay ids of neighbouring lanes in different tenants) with one half of the table bulk-loaded
    beside it and the other half added as overlay ids -> (tenant, topic) -> id"""
    items = R.table_items()
    bulk = [tp for j, tp in enumerate(items) if j % 2 == which]
    rest = [tp for j, tp in enumerate(items) if j % 2 != which]
    m = G.churn(G.Model(eng).load(G.bulk_items() + bulk))
    m.apply([(0, t, p) for t, p in rest])
    m.apply([(1,) + rest[4], (1,) + bulk[9], (1,) + bulk[-1]])
    m.apply([(0,) + rest[4]])
    if int(eng.retain_info().id_bound) % 64 == 0:
        m.apply([(0, "pad", "x")])
    return m


@pytest.mark.parametrize("which", [0, 1])
def test_the_table_on_the_device(which):
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    try:
        assert dev.retain_count_in() == (0, 0) and dev.retain_ids_in() == []
        m, h = _populate(dev, which), _populate(host, which)
        info = dev.retain_info()
        assert info.id_bound % 64 != 0 and info.id_bound > 3 * 64 and info.loaded_removed > 0 and info.added_ids > 300
        assert set(m.ids) == set(h.ids)
        assert R.check_table(dev, m.ids, other=host, live_other=h.ids) > 2000
        m.check()                                                              # nothing is changed by counting
    finally:
        dev.close(), host.close()


def test_one_tenant_with_70000_topics():
    """boundary keys inside the tenant: every lane takes the long path, and the id list crosses 65 536"""
    n = 70000
    topics = ["dev/%d/room/%d" % (i % 977, i) if i % 3 else "d/%d" % i for i in range(n)]
    dev = B.Engine(device=0)
    try:
        dev.retain_rebuild(["big", "z"], [0] * n + [1], topics + ["other"])
        ids = dev.retain_live_ids()
        assert len(ids) == n + 1
        keyed = sorted((R.key(t, p), i) for i, (t, p) in zip(ids, dev.retain_topics(ids)))
        ks = [k for k, _ in keyed]
        cuts = [ks[1000], ks[n // 2], ks[n // 2][:-3], ks[n - 1500] + b"\0", R.tenant_prefix("big") + b"\0\x03"]
        cases = [(None, None), (cuts[0], None), (None, cuts[3]), (cuts[0], cuts[3]), (cuts[2], None), (None, cuts[1]), (cuts[4], None), (None, cuts[4])]
        crossed = 0
        for s, e in cases:
            exp = [(k, i) for k, i in keyed if R.is_inside(k, s, e)]
            assert dev.retain_count_in(start=s, end=e) == (len(exp), sum(len(k) for k, _ in exp)), (s, e)
            assert dev.retain_ids_in(start=s, end=e) == sorted(i for _, i in exp), (s, e)
            crossed += len(exp) > 65536
        assert crossed >= 3
    finally:
        dev.close()


def test_an_overlay_only_tenant_with_17_level_topics():
    """the chain walk that reaches forward level j from the last level; boundary keys end inside the hash bytes and inside the body"""
    dev = B.Engine(device=0)
    try:
        dev.retain_rebuild(["t"], [0] * 3, ["a", "b", "c"])
        deep = ["/".join(("v%d" % (i if lv == i % 17 else lv) if (i + lv) % 5 else "") for lv in range(17)) for i in range(200)]
        deep += ["/".join("n%d" % lv for lv in range(17)), "/".join("n%d" % lv for lv in range(16)) + "/n17"]
        out = dev.retain_apply_batch(["ov17"], None, [(0, p) for p in sorted(set(deep))])
        live = {("ov17", p): i for p, i in zip(sorted(set(deep)), out.tolist())}
        live.update(zip(dev.retain_topics([0, 1, 2]), [0, 1, 2]))
        keyed = sorted((R.key(t, p), i) for (t, p), i in live.items())
        head = len(R.tenant_prefix("ov17")) + 2
        cuts = set()
        for k, _ in keyed[3::17]:
            cuts.update([k[:head + 1], k[:head + 9], k[:head + 17], k[:head + 17 + 5], k[:-1], k, k + b"\0"])   # inside the hash bytes, inside the body
        cuts = sorted(cuts)
        assert len(cuts) > 50
        for j, c in enumerate(cuts):
            for s, e in ((c, None), (None, c), (c, cuts[j + 5]) if j + 5 < len(cuts) else (None, None)):
                exp = [(k, i) for k, i in keyed if R.is_inside(k, s, e)]
                assert dev.retain_count_in(start=s, end=e) == (len(exp), sum(len(k) for k, _ in exp)), (s, e)
                assert dev.retain_ids_in(start=s, end=e) == sorted(i for _, i in exp), (s, e)
    finally:
        dev.close()


def _stamped(eng):
    """retain_gc_ref's bulk items and the table, with stamps: every second topic has expired at NOW"""
    items = sorted(set(G.bulk_items(60) + R.table_items()))
    m = R.Model(eng).load([(t, p) + ((((NOW - 5000) << 16), 1) if i % 2 else ((NOW << 16), 100)) for i, (t, p) in enumerate(items[::2])])
    m.apply([(0, t, p) + ((((NOW - 5000) << 16), 1) if i % 2 else ((NOW << 16), 100)) for i, (t, p) in enumerate(items[1::2])])
    m.apply([(1,) + items[10], (1,) + items[11]])
    return m


def _check_matches(eng, model):
    """rows of retain_match_batch and retain_match_limited(now = NOW) mapped through retain_topics against an oracle.LevelTrie over `model`"""
    where = sorted(model)
    lt = O.LevelTrie(1)
    for v, (t, p) in enumerate(where):
        lt.add(t, p, v)
    tn = sorted({t for t, _ in where} | {"nobody"})
    ft = [i for i in range(len(tn)) for _ in FILTERS]
    fl = FILTERS * len(tn)
    row, ids = eng.retain_match_batch(tn, ft, fl)
    names = eng.retain_topics(ids)
    lrow, lids, _ = eng.retain_match_limited(tn, ft, fl, [100000] * len(fl), now_ms=NOW)
    lnames = eng.retain_topics(lids)
    hits = 0
    for j in range(len(fl)):
        want = sorted(where[v] for v in lt.match(tn[ft[j]], fl[j]))
        assert sorted(names[row[j]:row[j + 1]]) == want, (tn[ft[j]], fl[j])
        alive = [tp for tp in want if (model[tp][0] >> 16) + 1000 * model[tp][1] > NOW]
        assert sorted(lnames[lrow[j]:lrow[j + 1]]) == alive, (tn[ft[j]], fl[j])      # the stamps travelled
        hits += len(want)
    return hits


@pytest.mark.parametrize("cut", range(5))
def test_split_and_merge_with_matches(cut):
    c = R.cuts()[cut]
    a, b = B.Engine(device=0), B.Engine(device=0)
    try:
        m = _stamped(a)
        lower, upper = m.restricted(end=c), m.restricted(start=c)
        assert lower and upper
        assert _check_matches(a, m.d) > 100
        assert b.retain_import(a, start=c) == (len(upper), 0)
        assert b.retain_info().loaded_topics == len(upper)
        a.retain_compact_begin(end=c)
        a.retain_compact_build()
        assert a.retain_compact_swap() == (len(lower), 0)
        _check_matches(a, lower), _check_matches(b, upper)
        assert R.live_state(a) == lower and R.live_state(b) == upper
        assert a.retain_import(b) == (len(upper), 0)
        assert _check_matches(a, m.d) > 100
        assert R.live_state(a) == m.d
    finally:
        a.close(), b.close()


def test_import_out_of_a_serving_engine():
    """the import runs while a thread runs match batches on the source: every row that thread sees is the unrestricted model's"""
    c = R.cuts()[1]
    a, b, host = B.Engine(device=0), B.Engine(device=0), B.Engine(device=-1)
    try:
        m = _stamped(a)
        done, seen, errors = threading.Event(), [], []

        def serve():
            try:
                while True:
                    seen.append(_check_matches(a, m.d))
                    if done.is_set():
                        return
            except BaseException as ex:   # noqa: B902 -- reported by the main thread
                errors.append(ex)

        th = threading.Thread(target=serve)
        th.start()
        try:
            got = b.retain_import(a, start=c)
            got_host = host.retain_import(a, start=c)          # a device engine into a host-only one
        finally:
            done.set()
            th.join()
        assert not errors, errors
        assert seen and all(s == seen[0] for s in seen)
        upper = m.restricted(start=c)
        assert got == got_host == (len(upper), 0)
        assert R.live_state(b) == R.live_state(host) == upper
        _check_matches(b, upper)
    finally:
        a.close(), b.close(), host.close()
