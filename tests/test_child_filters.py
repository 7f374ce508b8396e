"""Child filter words of the filter trie (bmq_config.child_filters, bmq_layout.h): the begin word of a node's empty route range holds 32 more filter bits
over the node's literal children; the builder maintains them, the walk asks them before it probes for a literal child.  They only ever spare a probe:
rows, ids and the count of discovered nodes are the same with the walk reading them and ignoring them."""
import os
import subprocess

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd.workload import unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")


@pytest.mark.parametrize("seed", [1, 99])
def test_no_filter_word_lacks_a_childs_bit_through_churn_growth_and_compaction(tmp_path, seed):
    """tools/child_filter_check.cpp on the host executor: after rebuilds, apply batches (children below route-less nodes, the first route of such a
    node, its last route leaving again, put + delete of one key in one batch), region growth and compaction, every node with an empty range has the
    bit of each of its literal children in that range's begin word; the words of a rebuilt / compacted image are exact (never all-ones)."""
    exe = str(tmp_path / "child_filter_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(ROOT, "tools", "child_filter_check.cpp"),
                    os.path.join(CSRC, "bmq_codec.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "16", str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("child filter check ok:"), r.stdout
    assert int(r.stdout.split(" (node, literal child) pairs")[0].split()[-1]) > 10000, r.stdout
    assert int(r.stdout.split(" of them all-ones")[0].split()[-1]) > 0, r.stdout
    assert int(r.stdout.split(" rounds with region growth")[0].split()[-1]) > 0, r.stdout


def test_the_bloom_census_finds_fewer_line_fetches_on_the_survey_population(tmp_path):
    """tools/bloom_census.cpp on 8 C3 tenants, 50 k publishes, region slack 6: with the child filter words the walk discovers the same nodes and
    fetches at least 0.4 lines per publish fewer (the planning runs gave 0.55-0.65 with 32 bits per empty range)."""
    exe = str(tmp_path / "bloom_census")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(ROOT, "tools", "bloom_census.cpp"), os.path.join(CSRC, "bmq_gen.cpp"),
                    os.path.join(CSRC, "bmq_codec.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "8", "50000", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        if not line.startswith("slack"):
            continue
        name = line[9:27].strip()
        rows[name] = (float(line.split("nodes discovered")[0].split()[-1]), float(line.split("line fetches")[0].split(",")[-1]),
                      float(line.split("false positives")[0].split(",")[-1]))
    print(r.stdout)
    assert rows["child filters"][0] == rows["Bloom word alone"][0], rows
    assert rows["child filters"][1] <= rows["Bloom word alone"][1] - 0.4, rows
    assert rows["child filters"][2] < rows["Bloom word alone"][2], rows


def _engines(**kw):
    return B.Engine(device=0, child_filters=0, **kw), B.Engine(device=0, child_filters=1, **kw)


def _rows(row_ptr, ids):
    return [sorted(ids[row_ptr[k]:row_ptr[k + 1]].tolist()) for k in range(len(row_ptr) - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,grouped", [({}, True), ({"region_slack": 1}, True), ({"wave_queue_cap": 128, "wave_pair_cap": 128}, True), ({}, False)],
                         ids=["default", "region_slack_1", "smallest_geometry", "ungrouped_mixed"])
def test_rows_ids_and_visits_are_the_same_with_and_without_child_filters(kw, grouped):
    """A batch grouped by tenant runs the grouped instantiation (the root's '+' child and its '+' child are resolved at the wave's start, with their
    filter words); one that is not grouped runs the MIXED one."""
    from oracle import oracle as O
    from tests import util as U
    w = B.Workload(0xB1F20003, 8, 4000, 1)
    kv = O.KV(packed=w.keys_packed())
    on, off = _engines(**kw)
    try:
        tn = w.tenants()
        for eng in (on, off):
            eng.rebuild(packed=w.keys_packed())
        data, off_, tt = w.topics(0xB1F20003 + 5, 20000, grouped=grouped)
        r_on, i_on = on.match_batch(tn, tt, packed_topics=(data, off_))
        v_on = on.stats().n_visit
        r_off, i_off = off.match_batch(tn, tt, packed_topics=(data, off_))
        v_off = off.stats().n_visit
        assert np.array_equal(r_on, r_off)
        assert np.array_equal(i_on, i_off)
        assert v_on == v_off == int(kv.count_visits(tn, tt, (data, off_)).sum())
        # a sample against the brute force
        rows_on = _rows(r_on, i_on)
        topics = [t.decode() for t in unpack(data, off_)]
        sel = list(range(0, len(topics), 97))
        exp = U.semantic_rows(kv, tn, [tt[i] for i in sel], [topics[i] for i in sel])
        assert [rows_on[i] for i in sel] == exp
    finally:
        on.close()
        off.close()


@pytest.mark.gpu
def test_churn_keeps_the_filter_words_supersets_and_compaction_makes_them_exact_again():
    """Children below route-less nodes, the first route of such nodes, those routes leaving again, put + delete of one key in one batch beside a new
    child, many new nodes (regions grow), then compact(): after every step the rows of the engine whose walk reads the filter words equal those of the
    engine whose walk ignores them, and so do the counts of discovered nodes."""
    w = B.Workload(0xB1F20007, 4, 3000, 1)
    keys = list(w.keys())
    on, off = _engines()
    try:
        tn = w.tenants()
        data, off_, tt = w.topics(0xB1F20007 + 3, 20000, grouped=True)
        topics = [t.decode() for t in unpack(data, off_)]

        def same():
            r_on, i_on = on.match_batch(tn, tt, packed_topics=(data, off_))
            v_on = on.stats().n_visit
            r_off, i_off = off.match_batch(tn, tt, packed_topics=(data, off_))
            assert off.stats().n_visit == v_on
            assert np.array_equal(r_on, r_off)
            for k in range(len(r_on) - 1):
                a, b = i_on[r_on[k]:r_on[k + 1]], i_off[r_off[k]:r_off[k + 1]]
                if not np.array_equal(a, b):  # (ids are handed out alike in both engines; if they ever are not, the keys decide)
                    assert sorted(on.route_keys(a.tolist())) == sorted(off.route_keys(b.tolist()))

        for eng in (on, off):
            eng.rebuild(keys)
        same()
        rnd = np.random.default_rng(11)
        # route-less inner nodes: proper prefixes of filters (most hold no route of their own); children are named after levels publishes use, so
        # that topics really probe for them
        decoded = [B.decode_route_key(keys[i]) for i in rnd.choice(len(keys), 400, replace=False)]
        prefixes = []
        for flag, tenant, filt, recv in decoded:
            levels = filt.split("/")
            if levels[-1] == "#":
                levels = levels[:-1]
            if len(levels) >= 2:
                prefixes.append((tenant, "/".join(levels[:int(rnd.integers(1, len(levels)))])))
        words = sorted({lv for t in topics[:2000] for lv in t.split("/") if lv})[:200]
        held = []
        for step in range(5):
            ops = []
            for n, (tenant, p) in enumerate(prefixes):
                word = words[int(rnd.integers(0, len(words)))]
                if step == 0:
                    ops.append((0, B.route_key_from_mqtt(tenant, p + "/" + word, "c%d" % n)))  # a child below a (mostly) route-less node
                elif step == 1:
                    k = B.route_key_from_mqtt(tenant, p if n % 2 else p + "/#", "first%d" % n)  # the node's first route (own / '#')
                    held.append(k)
                    ops.append((0, k))
                elif step == 2:
                    ops.append((1, held[n]))  # ... leaves again: the word becomes all-ones
                elif step == 3:
                    k = B.route_key_from_mqtt(tenant, p if n % 2 else p + "/#", "blink%d" % n)
                    ops += [(0, k), (0, B.route_key_from_mqtt(tenant, p + "/" + word, "d%d" % n)), (1, k)]  # put + delete in one batch, a new child beside
                else:
                    for j in range(12):  # many new nodes: the tenants' regions grow
                        ops.append((0, B.route_key_from_mqtt(tenant, "%s/g%d/%s" % (p, j, word), "g%d" % n)))
            for eng in (on, off):
                eng.apply(ops)
            same()
        for eng in (on, off):
            eng.compact()
        same()
    finally:
        on.close()
        off.close()
