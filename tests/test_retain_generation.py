"""The non-blocking generation change of the retained-topic index -- bmq_retain_compact_begin[_in] / _build / _swap -- with the executor builder
(bmq_config.retain_builder = 3) on host-only engines: the snapshot functions the k_rs_* kernels wrap (bifromq_amd/csrc/bmq_retain_snap_core.h),
run by HostExec, against the host builder's path (retain_builder = 0) on every load of tests/retain_build_ref.py, the edges, the lock condition
on bmq_retain_compact_info.locked_copy_bytes, and the snapshot under sanitizers (tools/retain_snapshot_check.cpp).  What a GPU makes of the same
source, match rows included: tests/test_retain_generation_gpu.py."""
import os
import subprocess

import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import retain_build_ref as R
from tests import retain_generation_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus():
    return {ld.name: (ld, R.Model(ld)) for ld in R.corpus()}


@pytest.fixture()
def engines():
    made = []

    def make(rb):
        made.append(B.Engine(device=-1, retain_builder=G.RETAIN_BUILDER[rb]))
        return made[-1]
    yield make
    for e in made:
        e.close()


CASES = ["EDGE", "GOLDEN", "DUPS", "WIDE", "DEEP-128", "TENANTS", "SIZE-0", "SIZE-1", "SIZE-63", "SIZE-64", "SIZE-65", "SIZE-257", "WORKLOAD-20000"]


@pytest.mark.parametrize("case", CASES)
def test_a_round_with_churn_around_every_call_equals_the_host_builders_round(corpus, engines, case):
    ld, m = corpus[case]
    a, b = engines(0), engines(1)
    live, after, swaps, _ = G.full_round(a, b, ld, m)
    G.check_round(a, b, live, after, swaps, stride=max(1, m.n_topics // 256))


def test_nothing_live_at_begin_gives_an_empty_generation(corpus, engines):
    ld, m = corpus["SIZE-65"]
    a, b = engines(0), engines(1)
    for e in (a, b):
        ld.rebuild(e)
        e.retain_apply("s0", [(0, "added/one")])
        ids = e.retain_live_ids()
        assert e.retain_remove_ids(ids, e.retain_info().generation) == len(ids)
        assert G.one_round(e) == (0, 0)
    assert G.state(a) == G.state(b) and G.state(b)["info"] == (0, 0, 0, 0, 0)
    assert (b.retain_build_info().builder, int(b.retain_compact_info().n_items)) == (1, 0)
    for e in (a, b):                                                                    # ... and it takes topics again
        e.retain_apply("s0", [(0, "a/b")])
        assert G.one_round(e) == (1, 0) and e.retain_topic(0) == ("s0", "a/b")


def test_only_overlay_topics_live_and_only_bulk_ids_live(corpus, engines):
    ld, m = corpus["SIZE-64"]
    a, b = engines(0), engines(1)
    adds = [(0, "x/%d" % i) for i in range(70)] + [(0, ""), (0, "$sys/x")]
    for e in (a, b):                                                                    # every bulk id dead, the overlay holds two tenants (one of them loaded too)
        ld.rebuild(e)
        e.retain_apply("s1", adds), e.retain_apply("brand-new", adds[:3])
        assert e.retain_remove_ids(list(range(m.n_topics)), e.retain_info().generation) == m.n_topics
        assert G.one_round(e) == (len(adds) + 3, 0)
    sa, sb = G.state(a), G.state(b)
    assert sa == sb and sb["live"] == list(range(len(adds) + 3)) and sorted(sb["topics"]) == sorted([("s1", p) for _, p in adds] + [("brand-new", p) for _, p in adds[:3]])
    assert b.retain_build_info().builder == 1 and b.retain_keys_by_id(sb["live"]) == b.retain_message_keys(sb["live"])
    c, d = engines(0), engines(1)
    for e in (c, d):                                                                    # bulk ids only, some of them dead
        ld.rebuild(e)
        assert e.retain_remove_ids([0, 1, 63], e.retain_info().generation) == 3
        assert G.one_round(e) == (m.n_topics - 3, 0)
    sc, sd = G.state(c), G.state(d)
    assert sc == sd and sd["topics"] == [x for i, x in enumerate(m.order) if i not in (0, 1, 63)]
    assert d.retain_build_info().builder == 1 and d.retain_keys_by_id(sd["live"]) == d.retain_message_keys(sd["live"])


def test_begin_in_with_a_boundary_through_a_tenant_and_one_that_keeps_nothing(corpus, engines):
    ld, m = corpus["SIZE-257"]
    keys = sorted(O.retain_message_key(t, p) for t, p in m.order)
    cut = keys[len(keys) // 2]                                                         # inside tenant s1's keys (three tenants of equal length)
    for start, end in ((None, cut), (cut, None), (keys[-1] + b"\xff", None)):
        a, b = engines(0), engines(1)
        for e in (a, b):
            ld.rebuild(e)
            e.retain_apply("s1", [(0, "added/below"), (1, m.order[100][1] if m.order[100][0] == "s1" else "nothing")])
        inside = [b.retain_topic(i) for i in b.retain_ids_in(start, end)]               # taken before the begin
        for e in (a, b):
            e.retain_compact_begin(start, end)
            e.retain_apply("s0", [(0, "logged/op")]), e.retain_apply("s2", [(0, "logged/op")])
            e.retain_compact_build()
        assert a.retain_compact_swap() == b.retain_compact_swap()
        sa, sb = G.state(a), G.state(b)
        assert sa == sb
        logged = [x for x in (("s0", "logged/op"), ("s2", "logged/op"))
                  if (start is None or O.retain_message_key(*x) >= start) and (end is None or O.retain_message_key(*x) < end)]
        assert sorted(sb["topics"][i] for i in sb["live"]) == sorted(inside + logged)
        assert sb["info"][2] == len(inside) and (b.retain_build_info().builder, b.retain_build_info().fallback) == (1, 0)
        if start is not None and end is None and start > keys[-1]:
            assert inside == []


def test_a_topic_of_129_levels_added_before_the_begin_falls_back_with_the_same_results(corpus, engines):
    ld, m = corpus["SIZE-63"]
    deep = "/".join("l%d" % (k % 5) for k in range(R.RB_MAX_DEPTH + 1))
    a, b = engines(0), engines(1)
    for e in (a, b):
        ld.rebuild(e)
        e.retain_apply("s1", [(0, deep), (0, "shallow")])
        e.retain_compact_begin()
        e.retain_apply("s1", [(0, "meanwhile")])
        e.retain_compact_build()
        assert e.retain_compact_swap() == (m.n_topics + 2, 1)
    assert G.state(a) == G.state(b) and ("s1", deep) in G.state(b)["topics"]
    bi, ci = b.retain_build_info(), b.retain_compact_info()
    assert (bi.builder, bi.fallback, bi.max_depth) == (0, 1, R.RB_MAX_DEPTH + 1) and (ci.state, ci.builder, ci.fallback) == (3, 0, 1)
    b.retain_apply("s1", [(1, deep)])                                                  # without it the executor builder takes the next round
    assert G.one_round(b) == (m.n_topics + 2, 0) and (b.retain_build_info().builder, b.retain_build_info().fallback) == (1, 0)


def test_abort_after_begin_and_after_build_then_a_full_round(corpus, engines):
    ld, m = corpus["SIZE-65"]
    a, b = engines(0), engines(1)
    for e in (a, b):
        ld.rebuild(e)
        assert e.retain_compact_info().state == 0
        e.retain_compact_begin()
        assert e.retain_compact_info().state == 1
        e.retain_compact_abort()
        assert e.retain_compact_info().state == 0                                      # nothing has ended in a swap yet
        e.retain_compact_begin().retain_compact_build()
        assert e.retain_compact_info().state == 2
        e.retain_apply("s0", [(0, "during/the/aborted/one")])
        e.retain_compact_abort()
        with pytest.raises(B.BmqError):
            e.retain_compact_swap()                                                    # nothing to swap
    assert G.state(a) == G.state(b) and G.state(b)["info"][4] == 1
    live, after, swaps, _ = G.full_round(a, b, ld, m)
    G.check_round(a, b, live, after, swaps)
    b.retain_compact_begin()
    b.retain_compact_abort()
    assert b.retain_compact_info().state == 3                                          # the last one that ended in a swap


def test_swap_before_build_and_begin_twice_are_refused_as_under_the_host_builder(corpus, engines):
    ld, m = corpus["SIZE-1"]
    codes = []
    for rb in (0, 1):
        e = engines(rb)
        got = []
        with pytest.raises(B.BmqError) as ei:
            e.retain_compact_begin()                                                   # no index
        got.append(ei.value.code)
        ld.rebuild(e)
        e.retain_compact_begin()
        for call in (e.retain_compact_swap, e.retain_compact_begin, e.retain_compact, lambda: ld.rebuild(e)):
            with pytest.raises(B.BmqError) as ei:
                call()
            got.append(ei.value.code)
        e.retain_compact_build().retain_compact_build()                                # (a second build is a no-op)
        assert e.retain_compact_swap() == (1, 0)
        with pytest.raises(B.BmqError) as ei:
            e.retain_compact_build()
        got.append(ei.value.code)
        codes.append(got)
    assert codes[0] == codes[1] == [-7] * 6                                            # BMQ_E_STATE


def test_the_first_round_without_a_key_store_and_with_one_prepared_ahead(corpus, engines):
    ld, m = corpus["SIZE-257"]
    a, b, c = engines(0), engines(1), engines(1)
    for e in (a, b, c):
        ld.rebuild(e)
    assert c.retain_keys_prepare() > 0
    for e in (a, b, c):
        assert G.one_round(e) == (m.n_topics, 0)
    assert G.state(a) == G.state(b) == G.state(c) and G.state(b)["topics"] == m.order
    lazy, ahead = int(b.retain_compact_info().locked_copy_bytes), int(c.retain_compact_info().locked_copy_bytes)
    assert lazy > ahead + sum(len(p) for _, p in m.order)                              # the store crossed under the lock where nobody had prepared it
    assert b.retain_keys_prepare() == c.retain_keys_prepare() > 0                      # both generations brought their store along: nothing is built now


def test_the_lock_condition_no_copy_under_the_lock_grows_with_the_number_of_topics(corpus, engines):
    """bmq_retain_compact_info.locked_copy_bytes of idle rounds on SIZE-257 and WORKLOAD-20000: under builder 1 the two differ by less than 2048 bytes
    (anything per topic, even one dead bit, is 20 000 / 8 = 2 500 bytes more); under builder 0 by more than 20 000 (else the counter counts nothing)."""
    small, large = corpus["SIZE-257"][0], corpus["WORKLOAD-20000"][0]
    s1, l1 = G.locked_copy_bytes_of_an_idle_round(engines, small, 1), G.locked_copy_bytes_of_an_idle_round(engines, large, 1)
    print("locked_copy_bytes, builder 1: SIZE-257", s1, "WORKLOAD-20000", l1)
    for k in range(2):
        assert abs(l1[k] - s1[k]) < 2048
    s0, l0 = G.locked_copy_bytes_of_an_idle_round(engines, small, 0, prepare=False), G.locked_copy_bytes_of_an_idle_round(engines, large, 0, prepare=False)
    print("locked_copy_bytes, builder 0: SIZE-257", s0, "WORKLOAD-20000", l0)
    for k in range(2):
        assert l0[k] - s0[k] > 20000


@pytest.fixture(scope="module")
def long_log():
    """300 loaded topics over two tenants and 65 537 ops for the time between begin and build -- one more than a chunk of the replay (65 536): adds
    of distinct short topics, and 300 removes, of loaded topics and of topics added a moment before, in turn.  -> (tenants, loaded, ops as
    (tenant index, op, topic), the set model after them)"""
    names = ["s0", "s1"]
    loaded = [(names[i % 2], "base/%d" % i) for i in range(300)]
    live, ops, n_adds, n_removes = set(loaded), [], 65537 - 300, 0
    for i in range(n_adds):
        ops.append((i % 2, 0, "n/%d" % i))
        if i % 217 == 216 and n_removes < 300:
            t, p = loaded[n_removes] if n_removes % 2 == 0 else (names[(i - 5) % 2], "n/%d" % (i - 5))
            ops.append((names.index(t), 1, p))
            n_removes += 1
    assert len(ops) == 65537 and n_removes == 300
    for t, op, p in ops:
        (live.add if op == 0 else live.discard)((names[t], p))
    return names, loaded, ops, live


def topics_by_tenant(e, tenants):
    """per tenant what '#' (and '$'-filters: no topic here starts with '$') would give -- a host-only engine cannot match, so: the tenant's live ids"""
    return {t: sorted(p for _, p in e.retain_topics(e.retain_live_ids(t))) for t in tenants}


def test_a_log_of_65537_ops_is_replayed_in_two_chunks_and_the_result_merges_in_two(long_log, engines):
    names, loaded, ops, live = long_log
    got = []
    for rb in (0, 1):
        e, dst = engines(rb), engines(rb)
        e.retain_rebuild(names, [names.index(t) for t, _ in loaded], [p for _, p in loaded])
        e.retain_compact_begin()
        for lo in range(0, len(ops), 9000):                                            # (batches of its own size: the chunks are the replay's)
            part = ops[lo:lo + 9000]
            e.retain_apply_batch(names, [t for t, _, _ in part], [(op, p) for _, op, p in part])
        e.retain_compact_build()
        assert e.retain_compact_swap() == (300, 65537)
        assert int(e.retain_compact_info().replayed) == 65537
        by_tenant = topics_by_tenant(e, names)
        assert int(e.retain_info().n_topics) == len(live) and by_tenant == {t: sorted(p for tt, p in live if tt == t) for t in names}
        got.append((by_tenant, e.retain_live_ids()))
        # the merge leg of bmq_retain_import: dst holds topics already, 70 of them src's too; src has more than 65 536 to give
        more = [(0, "late/%d" % i) for i in range(500)]
        e.retain_apply("s1", more)
        src_live = live | {("s1", p) for _, p in more}
        own = [("s1", "base/%d" % i) for i in range(101, 241, 2)] + [("s2", "own/%d" % i) for i in range(30)]
        dst.retain_rebuild(["s1", "s2"], [0 if t == "s1" else 1 for t, _ in own], [p for _, p in own])
        dst.retain_apply("s2", [(0, "own/added")])
        n_src = int(e.retain_info().n_topics)
        assert n_src == len(src_live) > 65536
        imported, replaced = dst.retain_import(e)
        both = src_live & set(own)
        assert imported + replaced == n_src and replaced == len(both) > 0
        union = src_live | set(own) | {("s2", "own/added")}
        assert int(dst.retain_info().n_topics) == len(union)
        assert topics_by_tenant(dst, ["s0", "s1", "s2"]) == {t: sorted(p for tt, p in union if tt == t) for t in ("s0", "s1", "s2")}
    assert got[0] == got[1]                                                             # the two builders agree, id for id


def test_the_switch_has_a_value_of_its_own_and_under_1_the_three_calls_stay_the_host_builders(corpus):
    ld, m = corpus["SIZE-65"]
    for bad in (2, 4):
        with pytest.raises(B.BmqError):
            B.Engine(device=-1, retain_builder=bad)                                    # BMQ_E_INVAL at create
    a, b, c = (B.Engine(device=-1, retain_builder=rb) for rb in (0, 1, 3))
    try:
        for e in (a, b, c):
            ld.rebuild(e)
            e.retain_apply("s0", [(0, "added/one"), (1, m.order[3][1])])
        assert G.one_round(a) == G.one_round(b) == G.one_round(c)
        assert G.state(a) == G.state(b) == G.state(c)
        assert [(e.retain_build_info().builder, e.retain_compact_info().builder) for e in (a, b, c)] == [(0, 0), (0, 0), (1, 1)]
        for e in (b, c):                                                               # the bulk loads are the executor builder's under both
            e.retain_compact()
            assert e.retain_build_info().builder == 1
    finally:
        a.close(), b.close(), c.close()


def test_the_ctypes_mirror_of_the_compact_info_has_the_layout_of_the_header(tmp_path):
    import ctypes as C

    from bifromq_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_retain_compact_info));']
    for fname, _ in _lib.RetainCompactInfo._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(bmq_retain_compact_info, %s));' % (fname, fname))
    lines += ['return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.RetainCompactInfo)
    for fname, _ in _lib.RetainCompactInfo._fields_:
        assert int(got[fname]) == getattr(_lib.RetainCompactInfo, fname).offset, fname


def test_the_snapshot_under_sanitizers():
    """tools/retain_snapshot_check.cpp (a program of its own, nothing preloaded): random loads + churn -> snapshot, item for item against the strings and
    stamps of the existing host path; the image built from it against the executor build of the same items handed in from host memory; the next
    generation's key store and payload -- under ASan/UBSan, and under TSan with a thread mutating the serving generation while another builds."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "bifromq_amd", "csrc"), "rscheck"], check=True, capture_output=True, timeout=900)
    exe = os.path.join(ROOT, "tools", "retain_snapshot_check")
    for seed in ("1", "2"):
        r = subprocess.run([exe, "24", seed, "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "retain_snapshot_check ok" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe + "_tsan", "12", "3", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "retain_snapshot_check ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
