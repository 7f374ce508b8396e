"""k_walk on the device over the index states the CPU tier walks under the emulator (tools/emu/walk_emu.cpp): a directed family of unary chains for the
tail records -- every chain length 1 .. TAIL_K + 2, every '+'/literal mask, own routes and '#' routes at the leaf, topics that end inside a chain with a row
behind them whose first levels continue it -- on a fresh index, after each directed churn step and after compact(), for tail records x child filters on and
off, both LDS geometries, batches grouped by tenant and not (the MIXED instantiation, which is also what the persistent matcher k_poll runs).  Every row
against the brute force over the live keys, the count of discovered nodes against the trie of the keys put since the last rebuild / compaction."""
import random

import numpy as np
import pytest

import bifromq_amd as B
from oracle import oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

V = ["a", "b", "c"]  # chain tokens: levels topics also START with
TAIL_K = 4
N_TENANTS = 6  # (a wave of an ungrouped batch must hold more than four)


def family():
    """-> [(idx, k, is_hash, stem levels, chain levels, chain levels with known tokens for '+')]"""
    chains = []
    for k in range(1, TAIL_K + 3):
        full = (1 << k) - 1
        masks = range(1 << k) if k <= TAIL_K else [0, full, 0x15 & full, 0x2A & full]
        for m in masks:
            for is_hash in (False, True):
                idx = len(chains)
                name = "%s0k%dm%d%s" % (V[idx % 3], k, m, "h" if is_hash else "o")
                stem = ["st", name] if idx % 4 == 1 else ["$fam", name] if idx % 4 == 3 else [name]
                lv = ["+" if (m >> l) & 1 else V[(l + idx) % 3] for l in range(k)]
                fill = [V[(l + idx + 1) % 3] if (m >> l) & 1 else lv[l] for l in range(k)]
                chains.append((idx, k, is_hash, stem, lv, fill))
    return chains


def chain_topics(c):
    """blocks of rows that stay together in batch order: [short topic, the row that continues its chain] pairs, the others alone"""
    idx, k, _, stem, lv, fill = c
    base, ns = stem + fill, len(stem)
    blocks = [["/".join(base)]]
    for n in range(1, len(base)):  # every proper prefix
        if n < ns:
            blocks.append(["/".join(base[:n])])
        else:
            blocks.append(["/".join(base[:n]), "/".join(fill[n - ns:] + (["a"] if (idx + n) & 1 else []))])
    blocks += [["/".join(base + ["a"])], ["/".join(base + ["a", "b"])]]  # one and two levels beyond the leaf
    for i in range(k):  # one level off at each position; '+' positions: an unknown level, the empty level
        for lvl in ["zz", V[(i + idx + 2) % 3]] + (["qq%d" % idx, ""] if lv[i] == "+" else []):
            blocks.append(["/".join(base[:ns + i] + [lvl] + base[ns + i + 1:])])
    if ns == 1:
        blocks.append(["$" + "/".join(base)])
    for lvl in ("n", "m"):  # the children the churn steps put below the chain's inner node
        blocks.append(["/".join(base[:ns + idx % k] + [lvl])])
    return blocks


def filt(c, n_chain, tail=""):
    return "/".join(c[3] + c[4][:n_chain]) + tail


def key(tenant, f, rcv):
    return B.route_key_from_mqtt(tenant, f, O.receiver_url(0, rcv, "d"))


def leaf_keys(tenant, c):
    f = filt(c, c[1], "/#" if c[2] else "")
    return [key(tenant, f, "leaf%d" % c[0])] + ([key(tenant, f, "second%d" % c[0])] if c[0] % 3 == 0 else [])


CHAINS = family()
TENANTS = ["fam%d" % t for t in range(N_TENANTS)]
STEPS = ["own_on_inner", "other_kind", "leave", "back", "below_inner", "blink", "grow"]


def initial_keys():
    keys = []
    for tn in TENANTS:
        for c in CHAINS:
            keys += leaf_keys(tn, c)
        keys += [key(tn, "+", "p0"), key(tn, "+/+", "pp0")]  # the root's '+' child and its '+' child: resolved at the wave's start (grouped batches)
        for i in range(40):
            keys += [key(tn, "+/f%d" % i, "p0c"), key(tn, "+/+/f%d" % i, "pp0c")]
    return keys


def step_ops(step):
    """the directed churn steps of walk_emu.cpp, each on a part of the family of its own (chain index mod 8)"""
    ops = []
    part = STEPS.index(step)
    for tn in TENANTS:
        for c in CHAINS:
            idx, k, is_hash = c[0], c[1], c[2]
            j, tag = idx % k, str(idx)
            if step == "back":
                if idx % 8 == STEPS.index("leave"):
                    ops += [(0, kk) for kk in leaf_keys(tn, c)]
                continue
            if idx % 8 != part:
                continue
            if step == "own_on_inner":
                ops.append((0, key(tn, filt(c, j), "inner" + tag)))
            elif step == "other_kind":
                ops.append((0, key(tn, filt(c, k, "" if is_hash else "/#"), "other" + tag)))
            elif step == "leave":
                ops += [(1, kk) for kk in leaf_keys(tn, c)]
            elif step == "below_inner":
                ops.append((0, key(tn, filt(c, j, "/n"), "below" + tag)))
            elif step == "blink":
                kk = key(tn, filt(c, k, "/#" if is_hash else ""), "blink" + tag)
                ops += [(0, kk), (0, key(tn, filt(c, j, "/m"), "beside" + tag)), (1, kk)]
        if step == "leave":
            ops += [(1, key(tn, "+", "p0")), (1, key(tn, "+/+", "pp0"))]
        elif step == "back":
            ops += [(0, key(tn, "+", "p0")), (0, key(tn, "+/+", "pp0"))]
        elif step == "grow":  # more new nodes than the region has buckets
            ops += [(0, key(tn, "grow/g%d/w" % g, "grow")) for g in range(1500)]
    return ops


def batch(grouped):
    """-> (topic_tenant, packed topics): every topic of every chain for every tenant; grouped by tenant, or the blocks of all tenants shuffled"""
    blocks = [(t, b) for t in range(N_TENANTS) for c in CHAINS for b in chain_topics(c)]
    if not grouped:
        random.Random(5).shuffle(blocks)
    tt = np.asarray([t for t, b in blocks for _ in b], dtype=np.uint32)
    return tt, O.pack([x for _, b in blocks for x in b])


class Model:
    def __init__(self, keys):
        self.live, self.put = set(keys), set(keys)

    def apply(self, ops):
        for op, k in ops:
            if op:
                self.live.discard(k)
            else:
                self.live.add(k)
                self.put.add(k)

    def compacted(self):
        self.put = set(self.live)


def check(eng, model, tt, packed, what):
    row, ids = eng.match_batch(TENANTS, tt, packed_topics=packed)
    n_visit = eng.stats().n_visit
    keys_sorted = sorted(model.live)
    res, _ = O.KV(keys_sorted).match_semantic_batch(TENANTS, tt, packed, threads=U.host_threads())
    got = U.rows_as_ranks(eng, row, ids, keys_sorted)
    exp = res.per_topic()
    bad = [i for i in range(len(exp)) if got[i] != sorted(exp[i])]
    assert not bad, (what, bad[:5], len(bad))
    want_visit = int(O.KV(sorted(model.put)).count_visits(TENANTS, tt, packed).sum())
    print("%s: %d rows, %d ids, n_visit %d (model %d)" % (what, len(exp), len(ids), n_visit, want_visit))
    assert n_visit == want_visit, what


@pytest.mark.parametrize("child_filters", [0, 1], ids=["filters_read", "filters_ignored"])
@pytest.mark.parametrize("tail_records", [0, 1], ids=["records_on", "records_off"])
@pytest.mark.parametrize("kw,grouped", [({}, True), ({"wave_queue_cap": 128, "wave_pair_cap": 128}, True), ({}, False),
                                        ({"wave_queue_cap": 128, "wave_pair_cap": 128}, False)],
                         ids=["default_grouped", "smallest_grouped", "default_ungrouped_mixed", "smallest_ungrouped_mixed"])
def test_the_tail_family_through_the_index_states(kw, grouped, tail_records, child_filters):
    model = Model(initial_keys())
    tt, packed = batch(grouped)
    eng = B.Engine(device=0, tail_records=tail_records, child_filters=child_filters, **kw)
    try:
        eng.rebuild(sorted(model.live))
        check(eng, model, tt, packed, "fresh")
        for step in STEPS:
            garbage = eng.info().garbage_bytes
            ops = step_ops(step)
            eng.apply(ops)
            model.apply(ops)
            check(eng, model, tt, packed, step)
            if step == "grow":
                assert eng.info().garbage_bytes > garbage  # the regions really grew (the step adds no id list: the garbage is abandoned regions)
        eng.compact()
        model.compacted()
        check(eng, model, tt, packed, "compacted")
    finally:
        eng.close()


def test_the_persistent_matcher_on_the_churned_and_the_compacted_index():
    """The same topics in generations of at most 64 through the batching front with the poller enabled: the resident waves (k_poll) run the MIXED
    walk on an index with tombstones, grown regions and id lists, then on the compacted one with its records formed again."""
    model = Model(initial_keys())
    eng = B.Engine(device=0)
    try:
        eng.rebuild(sorted(model.live))
        for step in STEPS:
            ops = step_ops(step)
            eng.apply(ops)
            model.apply(ops)
        eng.poller_control(eng.POLLER_ENABLE)
        assert eng.poller_stats().enabled
        for what in ("churned", "compacted"):
            if what == "compacted":
                eng.compact()
                model.compacted()
            keys_sorted = sorted(model.live)
            kv = O.KV(keys_sorted)
            rank = {k: i for i, k in enumerate(keys_sorted)}
            b = eng.batcher()
            s0 = eng.poller_stats()
            n_gen = 0
            for t, tn in enumerate(TENANTS):
                topics = [x for c in CHAINS[t::2] for blk in chain_topics(c) for x in blk]  # (half of the chains per tenant, all of them over two tenants)
                for g in range(0, len(topics), 64):
                    gen = list(dict.fromkeys(topics[g:g + 64]))  # matchAll takes a set
                    rows, epoch = b.match_all(tn, gen)
                    exp = kv.match_bruteforce(tn, gen).per_topic()
                    got = [sorted(rank[k] for k in eng.route_keys(r)) if r else [] for r in rows]
                    assert got == [sorted(e) for e in exp], (what, tn, g)
                    assert epoch == eng.info().epoch
                    n_gen += 1
            s1 = eng.poller_stats()
            print("%s: %d generations, poller served %d, fallback %d, timeouts %d" % (what, n_gen, s1.n_served - s0.n_served, s1.n_fallback - s0.n_fallback, s1.n_timeouts))
            assert s1.n_served > s0.n_served and s1.n_timeouts == 0
            b.close()
    finally:
        eng.close()
