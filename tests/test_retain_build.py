"""The executor builder of the retained-topic index (bmq_config.retain_builder = 1: bifromq_amd/csrc/bmq_retain_build_core.h) on host-only engines --
the functions the k_rb_* kernels wrap, run by HostExec on host threads -- against the host builder (retain_builder = 0) and the model of
tests/retain_build_ref.py, id for id; the image itself under sanitizers (tools/retain_build_check.cpp) and under k_retain_walk in the wave emulator
(tools/emu/rwalk_build_emu.cpp).  What a GPU makes of the same source: tests/test_retain_build_gpu.py."""
import os
import random
import subprocess

import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import retain_build_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus():
    return [(ld, R.Model(ld)) for ld in R.corpus()]


def snapshot(eng):
    """everything a host-only engine tells of its retained topics, by id"""
    info = eng.retain_info()
    bound = int(info.id_bound)
    ids = list(range(bound))
    live = eng.retain_live_ids()
    now = 1_000_000 + 37 * (len(live) // 2) + 2500 * 1000                              # about half of the corpus' stamps have expired by then
    return {
        "info": (int(info.n_topics), int(info.n_tenants), bound, int(info.loaded_topics), int(info.loaded_removed), int(info.added_ids)),
        "live": live,
        "topics": eng.retain_topics(ids),
        "stamps": [eng.retain_topic_info(i) for i in live],
        "tenant_counts": eng.retain_tenant_counts(tenants_cap=1 << 16, cap=1024),
        "keys": eng.retain_keys_by_id(ids),
        "expired": [eng.retain_expired(t, now) for t, _ in eng.retain_tenant_counts(tenants_cap=1 << 16, cap=1024)[:3]],   # (the GC scan skips the tenant's '$' run)
    }


def check_against_model(eng, m):
    s = snapshot(eng)
    assert s["info"] == (m.n_topics, m.n_tenants, m.n_topics, m.n_topics, 0, 0)
    assert s["live"] == list(range(m.n_topics))
    assert s["topics"] == m.order                                                       # id = rank of (tenant bytes, level list)
    assert s["stamps"] == [(ts, ex, m.expire_at(i)) for i, (ts, ex) in enumerate(m.stamps)]   # the last add of a duplicate wins
    assert s["tenant_counts"] == m.tenant_counts
    assert s["keys"] == [O.retain_message_key(t, p) for t, p in m.order]
    return s


def test_corpus_on_host_engines_builder_1_equals_builder_0_and_the_model(corpus):
    for ld, m in corpus:
        a, b = B.Engine(device=-1, retain_builder=0), B.Engine(device=-1, retain_builder=1)
        try:
            ld.rebuild(a), ld.rebuild(b)
            bi = b.retain_build_info()
            assert (bi.builder, bi.fallback) == (1, 0), ld.name                         # no case passes by falling back
            assert a.retain_build_info().builder == 0
            assert check_against_model(b, m) == check_against_model(a, m), ld.name
            got = {f: int(getattr(bi, f)) for f in ("n_items", "n_topics", "n_tenants", "n_nodes", "n_edges", "n_posts", "n_gp_runs", "n_tokens", "max_depth")}
            assert got == {f: getattr(m, f) for f in got}, ld.name
            ai = a.retain_build_info()
            assert all(int(getattr(ai, f)) == got[f] for f in got), ld.name            # the host builder's own counts agree
            if ld.name == "WIDE":
                assert {31, 32, 33, 300} <= set(m.widths) and m.n_posts and bi.n_edge_overflows > 0 and bi.n_gp_overflows > 0   # else the case proves nothing
            if m.n_topics:
                keys = sorted(O.retain_message_key(t, p) for t, p in m.order)
                k = keys[m.n_topics // 2]                                              # a median key: count_in on both sides of it
                for lo, hi in ((None, k), (k, None)):
                    inside = [x for x in keys if (lo is None or x >= lo) and (hi is None or x < hi)]
                    assert a.retain_count_in(lo, hi) == b.retain_count_in(lo, hi) == (len(inside), sum(len(x) for x in inside)), ld.name
        finally:
            a.close(), b.close()


def test_churn_remove_ids_compact_and_import_on_a_generation_the_executor_built(corpus):
    rnd = random.Random(7)
    for ld, m in corpus:
        if m.n_topics == 0:
            continue
        a, b = B.Engine(device=-1, retain_builder=0), B.Engine(device=-1, retain_builder=1)
        c = d = None
        try:
            ld.rebuild(a), ld.rebuild(b)
            names, ot, ops = R.churn_ops(m, rnd)
            assert list(a.retain_apply_batch(names, ot, ops)) == list(b.retain_apply_batch(names, ot, ops)), ld.name   # adds below loaded prefixes find them
            assert snapshot(a) == snapshot(b), ld.name
            gone = rnd.sample(range(m.n_topics), min(m.n_topics, 5))
            assert a.retain_remove_ids(gone, a.retain_info().generation) == b.retain_remove_ids(gone, b.retain_info().generation), ld.name
            assert snapshot(a) == snapshot(b), ld.name
            for _ in range(2):                                                         # ids are ranks again, twice (the second load starts from a load the builder made)
                a.retain_compact(), b.retain_compact()
                sa, sb = snapshot(a), snapshot(b)
                assert sa == sb and sb["live"] == list(range(len(sb["live"]))), ld.name
                assert (b.retain_build_info().builder, b.retain_build_info().fallback) == (1, 0), ld.name
            c, d = B.Engine(device=-1, retain_builder=0), B.Engine(device=-1, retain_builder=1)
            assert c.retain_import(a) == d.retain_import(b) == (len(sb["live"]), 0), ld.name   # into an empty engine: a bulk load
            assert (d.retain_build_info().builder, d.retain_build_info().fallback) == (1, 0), ld.name
            assert snapshot(c) == snapshot(d) and snapshot(d)["topics"] == sb["topics"] and snapshot(d)["stamps"] == sb["stamps"], ld.name
        finally:
            for e in (a, b, c, d):
                if e is not None:
                    e.close()


def test_a_topic_of_129_levels_falls_back_to_the_host_builder_with_the_same_results():
    ld = R.deep(levels=(17, R.RB_MAX_DEPTH, R.RB_MAX_DEPTH + 1))
    m = R.Model(ld)
    a, b = B.Engine(device=-1, retain_builder=0), B.Engine(device=-1, retain_builder=1)
    try:
        ld.rebuild(a), ld.rebuild(b)
        bi = b.retain_build_info()
        assert (bi.builder, bi.fallback, bi.max_depth) == (0, 1, R.RB_MAX_DEPTH + 1)
        assert check_against_model(b, m) == check_against_model(a, m)
        b.retain_compact()                                                             # ... and again through the compaction's load
        assert (b.retain_build_info().builder, b.retain_build_info().fallback) == (0, 1) and snapshot(b)["topics"] == m.order
    finally:
        a.close(), b.close()


def test_the_switch_and_the_info_call():
    with pytest.raises(B.BmqError):
        B.Engine(device=-1, retain_builder=2)                                          # BMQ_E_INVAL at create
    e = B.Engine(device=-1, retain_builder=1)
    try:
        with pytest.raises(B.BmqError) as ei:
            e.retain_build_info()                                                      # nothing is loaded
        assert ei.value.code == -7                                                     # BMQ_E_STATE
        e.retain_apply("t", [(0, "a/b")])                                              # the empty load a fresh engine starts from: the host builder's
        assert (e.retain_build_info().builder, e.retain_build_info().n_topics) == (0, 0)
        e.retain_compact()
        assert (e.retain_build_info().builder, e.retain_build_info().n_topics) == (1, 1) and e.retain_topic(0) == ("t", "a/b")
        e.retain_compact_begin(), e.retain_compact_build(), e.retain_compact_swap()    # the non-blocking form keeps the host builder
        assert e.retain_build_info().builder == 0 and e.retain_topic(0) == ("t", "a/b")
        e.retain_compact()
        assert e.retain_build_info().builder == 1 and e.retain_topic(0) == ("t", "a/b")
    finally:
        e.close()


def test_the_ctypes_mirror_of_the_build_info_has_the_layout_of_the_header(tmp_path):
    """_lib.RetainBuildInfo against what the compiler makes of bmq_retain_build_info (bmq_config's mirror: tests/test_host.py reads both sides)"""
    import ctypes as C

    from bifromq_amd import _lib
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_retain_build_info));']
    for fname, _ in _lib.RetainBuildInfo._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(bmq_retain_build_info, %s));' % (fname, fname))
    lines += ['return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.RetainBuildInfo)
    for fname, _ in _lib.RetainBuildInfo._fields_:
        assert int(got[fname]) == getattr(_lib.RetainBuildInfo, fname).offset, fname
    assert C.sizeof(_lib.Config) == 13 * 4 and _lib.Config.retain_builder.offset == 11 * 4   # one of the two reserved words: struct_size unchanged


def test_the_image_of_both_builders_under_sanitizers():
    """tools/retain_build_check.cpp (a program of its own, nothing preloaded): RNode slices bitwise equal per tenant, edge sets and postings equal,
    every edge and run reachable under the overflow rule, '$' runs, the dictionary -- under ASan/UBSan, and under TSan with 8 host threads."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "bifromq_amd", "csrc"), "rbcheck"], check=True, capture_output=True, timeout=900)
    exe = os.path.join(ROOT, "tools", "retain_build_check")
    for seed in ("1", "2"):
        r = subprocess.run([exe, "24", seed, "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "retain_build_check ok" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe + "_tsan", "16", "3", "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "retain_build_check ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr


def test_k_retain_walk_under_the_wave_emulator_over_the_executor_builders_image(tmp_path):
    """tools/emu/rwalk_build_emu.cpp: rwalk_emu's rounds (every third one wide) and brute force, the index built by the executor builder."""
    exe = str(tmp_path / "rwalk_build_emu")
    cmd = ["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "bifromq_amd", "csrc"), "-I", os.path.join(ROOT, "tools", "emu"),
           os.path.join(ROOT, "tools", "emu", "rwalk_build_emu.cpp"), os.path.join(ROOT, "bifromq_amd", "csrc", "bmq_retain.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "24", "12345"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("ok: G") == 3, r.stdout[-2000:]
