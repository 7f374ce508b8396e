"""Shared by test_retain_generation.py (host-only engines) and test_retain_generation_gpu.py (device engines): the scenarios of the
non-blocking generation change of the retained-topic index -- bmq_retain_compact_begin[_in] / _build / _swap -- run side by side on an engine
with retain_builder = 0 and one with retain_builder = 3, over the corpus and model of tests/retain_build_ref.py, and a set model of which
(tenant, topic) pairs are retained after every step."""
import random

from tests import retain_build_ref as R

# bmq_config.retain_builder by the builder that serves begin / build / swap (what bmq_retain_compact_info.builder reports): 0 = the host builder,
# 1 = the executor builder.  The value for the latter is 3, not 1: under 1 the executor builder bulk-loads only and the three calls stay the host
# builder's, which tests/test_retain_build.py::test_the_switch_and_the_info_call holds it to.
RETAIN_BUILDER = {0: 0, 1: 3}

PROBE = ["#", "+", "+/+", "a/#", "a/+", "+/b", "a/b/added", "+/+/added", "sibling", "x/y", "$a/#", "w0/#", "+/sibling", "gen/#", "gen/+"]


def state(eng, stride=1):
    """what the engine tells of its retained topics by id (as tests/test_retain_build_gpu.py's: info, live ids, id -> topic, stamps, tenant counts,
    expired; stride: the stamps of every stride-th live id -- one call each)"""
    info = eng.retain_info()
    live = eng.retain_live_ids()
    counts = eng.retain_tenant_counts(tenants_cap=1 << 16, cap=1024)
    now = 1_000_000 + 37 * (len(live) // 2) + 2500 * 1000
    return {"info": (int(info.n_topics), int(info.id_bound), int(info.loaded_topics), int(info.loaded_removed), int(info.added_ids)), "live": live,
            "topics": eng.retain_topics(list(range(int(info.id_bound)))), "stamps": [eng.retain_topic_info(i) for i in live[::stride]],
            "tenant_counts": counts, "expired": [eng.retain_expired(t, now) for t, _ in counts[:3]]}


def apply_both(a, b, live, names, ot, ops):
    """one apply batch on both engines and on the set model (ops of a batch take effect in order)"""
    assert list(a.retain_apply_batch(names, ot, ops)) == list(b.retain_apply_batch(names, ot, ops))
    for t, (op, p) in zip(ot, ops):
        (live.add if op == 0 else live.discard)((names[t], p))
    return len(ops)


def later_batches(m, names, ot, ops, gone_topics):
    """the batch between begin and build, and the one between build and swap: they re-add a topic the churn removed and one removed by id, remove
    one the churn added and one the first of them adds, add topics nobody held, remove loaded topics that are still there"""
    removed = [(t, p) for t, (op, p) in zip(ot, ops) if op == 1]
    added = [(t, p) for t, (op, p) in zip(ot, ops) if op == 0]
    t0 = 0
    two_t, two = [t0, len(names) - 1], [(0, "gen/two"), (0, "gen/fresh/two")]
    three_t, three = [t0, t0], [(0, "gen/three"), (1, "gen/two")]                      # an add of the second batch goes in the third
    if removed:
        two_t.append(removed[0][0]), two.append((0, removed[0][1]))                      # re-add a removed topic
    if added:
        two_t.append(added[0][0]), two.append((1, added[0][1]))                          # remove an added one
    if len(added) > 1:
        three_t.append(added[1][0]), three.append((1, added[1][1]))
    for k, (t, p) in enumerate(gone_topics[:2]):                                          # removed by id before the begin: back again
        (two_t if k == 0 else three_t).append(names.index(t)), (two if k == 0 else three).append((0, p))
    still = [x for x in m.order if x not in gone_topics and (names.index(x[0]), x[1]) not in removed]
    for k, (t, p) in enumerate(still[:: max(1, len(still) // 4)][:4]):                    # loaded topics go, two per batch
        (two_t if k % 2 == 0 else three_t).append(names.index(t)), (two if k % 2 == 0 else three).append((1, p))
    return (two_t, two), (three_t, three)


def full_round(a, b, ld, m, seed=11):
    """load, churn, remove five ids, begin, a second batch, build, a third batch, swap -- on both engines; -> (the set model's live pairs, the ops
    applied after the begin, what the two swaps returned)"""
    rnd = random.Random(seed)
    ld.rebuild(a), ld.rebuild(b)
    live = set(m.order)
    names, ot, ops = R.churn_ops(m, rnd)
    apply_both(a, b, live, names, ot, ops)
    gone = rnd.sample(range(m.n_topics), min(m.n_topics, 5))
    assert a.retain_remove_ids(gone, a.retain_info().generation) == b.retain_remove_ids(gone, b.retain_info().generation)
    gone_topics = [m.order[i] for i in gone]
    for x in gone_topics:
        live.discard(x)
    (two_t, two), (three_t, three) = later_batches(m, names, ot, ops, gone_topics)
    a.retain_compact_begin(), b.retain_compact_begin()
    after = apply_both(a, b, live, names, two_t, two)
    a.retain_compact_build(), b.retain_compact_build()
    after += apply_both(a, b, live, names, three_t, three)
    return live, after, (a.retain_compact_swap(), b.retain_compact_swap()), names


def check_round(a, b, live, after, swaps, stride=1):
    """what must hold after full_round, on any executor"""
    sa, sb = state(a, stride), state(b, stride)
    assert sa == sb
    assert sorted(sb["topics"][i] for i in sb["live"]) == sorted(live)                    # ... and both hold what the set model holds
    assert swaps[0] == swaps[1] and swaps[1][1] == after
    bi = b.retain_build_info()
    assert (bi.builder, bi.fallback) == (1, 0)                                          # (on the parent commit _swap reports the host builder here)
    assert a.retain_build_info().builder == 0
    ci = b.retain_compact_info()
    assert (ci.state, ci.builder, ci.fallback, int(ci.replayed)) == (3, 1, 0, after)
    assert (a.retain_compact_info().state, a.retain_compact_info().builder, int(a.retain_compact_info().replayed)) == (3, 0, after)
    ids = sb["live"]
    assert b.retain_keys_by_id(ids) == b.retain_message_keys(ids)                       # the key store the build left behind, and the overlay beside it
    # a second round straight after, nothing between: ids are ranks again
    for e in (a, b):
        e.retain_compact_begin().retain_compact_build()
        assert e.retain_compact_swap() == (len(live), 0)
    sa, sb = state(a, stride), state(b, stride)
    assert sa == sb and sb["live"] == list(range(len(live))) and sorted(sb["topics"]) == sorted(live)
    assert sb["info"] == (len(live), len(live), len(live), 0, 0)
    assert (b.retain_build_info().builder, b.retain_build_info().fallback, int(b.retain_build_info().n_topics)) == (1, 0, len(live))
    ids = sb["live"]
    assert b.retain_keys_by_id(ids) == b.retain_message_keys(ids)
    return sb


def one_round(e):
    e.retain_compact_begin().retain_compact_build()
    return e.retain_compact_swap()


def locked_copy_bytes_of_an_idle_round(make, ld, rb, prepare=True):
    """locked_copy_bytes of begin / build / swap rounds with an empty log on a fresh engine that holds `ld`: the first round (prepare: the key store is
    built ahead, as a caller that minds the lock does) and the round straight after it"""
    e = make(rb)
    ld.rebuild(e)
    if prepare:
        e.retain_keys_prepare()
    out = []
    for _ in range(2):
        one_round(e)
        ci = e.retain_compact_info()
        assert (ci.state, int(ci.replayed), ci.builder) == (3, 0, rb)
        out.append(int(ci.locked_copy_bytes))
    return out
