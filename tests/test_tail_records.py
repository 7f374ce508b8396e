"""Tail records of the filter trie (bmq_config.tail_records, bmq_layout.h): a node whose subtree is a short unary chain carries the chain's tokens and
its leaf's payload in the free slot of its line, and the walk resolves the chain from the line it already holds."""
import os
import subprocess

import numpy as np
import pytest

import bifromq_amd as B
from bifromq_amd.workload import unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bifromq_amd", "csrc")


@pytest.mark.parametrize("seed", [1, 99])
def test_every_tail_record_equals_its_chain_through_churn_growth_and_compaction(tmp_path, seed):
    """tools/tail_check.cpp on the host executor: after rebuilds, apply batches (puts inside tails, routes added to and removed from their leaves,
    id lists), region growth and compaction, every record equals its chain; apply batches leave tombstones; tail_records off leaves no record."""
    exe = str(tmp_path / "tail_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(ROOT, "tools", "tail_check.cpp"), os.path.join(CSRC, "bmq_codec.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "16", str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("tail check ok:"), r.stdout
    assert int(r.stdout.split(" records")[0].split()[-1]) > 1000, r.stdout


def test_the_tail_census_finds_records_on_the_survey_population(tmp_path):
    """tools/tail_census.cpp: on a few C3 tenants the records remove line fetches and change no count of discovered nodes."""
    exe = str(tmp_path / "tail_census")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(ROOT, "tools", "tail_census.cpp"), os.path.join(CSRC, "bmq_gen.cpp"),
                    os.path.join(CSRC, "bmq_codec.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "2", "20000", "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        name = line[9:27].strip()
        rows[name] = (float(line.split("nodes discovered")[0].split()[-1]), float(line.split("line fetches")[0].split(",")[-1]))
    assert rows["K=4, one range"][0] == rows["no records"][0], rows
    assert rows["K=4, one range"][1] < rows["no records"][1] - 0.5, rows


def _engines(**kw):
    return B.Engine(device=0, tail_records=0, **kw), B.Engine(device=0, tail_records=1, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"region_slack": 1}, {"wave_queue_cap": 128, "wave_pair_cap": 128}])
def test_rows_and_visits_are_the_same_with_and_without_tail_records(kw):
    from oracle import oracle as O
    w = B.Workload(0xB1F20003, 8, 4000, 1)
    kv = O.KV(packed=w.keys_packed())
    on, off = _engines(**kw)
    try:
        tn = w.tenants()
        for eng in (on, off):
            eng.rebuild(packed=w.keys_packed())
        data, off_, tt = w.topics(0xB1F20003 + 5, 20000)
        r_on, i_on = on.match_batch(tn, tt, packed_topics=(data, off_))
        v_on = on.stats().n_visit
        r_off, i_off = off.match_batch(tn, tt, packed_topics=(data, off_))
        v_off = off.stats().n_visit
        assert np.array_equal(r_on, r_off)
        rows_on = [sorted(i_on[r_on[k]:r_on[k + 1]].tolist()) for k in range(len(r_on) - 1)]
        rows_off = [sorted(i_off[r_off[k]:r_off[k + 1]].tolist()) for k in range(len(r_off) - 1)]
        assert rows_on == rows_off
        assert v_on == v_off == int(kv.count_visits(tn, tt, (data, off_)).sum())
        # a sample against the brute force
        topics = [t.decode() for t in unpack(data, off_)]
        sel = list(range(0, len(topics), 97))
        from tests import util as U
        exp = U.semantic_rows(kv, tn, [tt[i] for i in sel], [topics[i] for i in sel])
        assert [rows_on[i] for i in sel] == exp
    finally:
        on.close()
        off.close()


@pytest.mark.gpu
def test_churn_splits_tails_and_compaction_forms_them_again():
    """Deletes and puts on tail leaves, puts below them (new children inside tails), then a compaction: rows of the engine with records equal those of
    the engine without after every step, and so do the counts of discovered nodes."""
    w = B.Workload(0xB1F20007, 4, 3000, 1)
    keys = list(w.keys())
    on, off = _engines()
    try:
        tn = w.tenants()
        data, off_, tt = w.topics(0xB1F20007 + 3, 20000)

        def same():
            r_on, i_on = on.match_batch(tn, tt, packed_topics=(data, off_))
            v_on = on.stats().n_visit
            r_off, i_off = off.match_batch(tn, tt, packed_topics=(data, off_))
            assert off.stats().n_visit == v_on
            assert np.array_equal(r_on, r_off)
            for k in range(len(r_on) - 1):
                a, b = i_on[r_on[k]:r_on[k + 1]], i_off[r_off[k]:r_off[k + 1]]
                assert sorted(on.route_keys(a.tolist())) == sorted(off.route_keys(b.tolist()))

        for eng in (on, off):
            eng.rebuild(keys)
        same()
        rnd = np.random.default_rng(7)
        for step in range(3):
            ops = []
            for i in rnd.choice(len(keys), 300, replace=False):
                flag, tenant, filt, recv = B.decode_route_key(keys[i])
                if step == 0:
                    ops.append((1, keys[i]))  # routes leave leaves
                elif step == 1:
                    if filt.endswith("#"):
                        continue
                    ops.append((0, B.route_key_from_mqtt(tenant, filt + "/zz%d" % (i % 3), "r%d" % i)))  # a child inside a tail
                else:
                    ops.append((0, B.route_key_from_mqtt(tenant, filt, "extra%d" % i)))  # more routes on a leaf (id lists)
            for eng in (on, off):
                eng.apply(ops)
            same()
        for eng in (on, off):
            eng.compact()
        same()
    finally:
        on.close()
        off.close()
