"""Shared by test_retain_gc_ids.py and test_retain_gc_ids_gpu.py: the population of the retain census / removal-by-id tests and its model --
a dict (tenant, topic) -> topic id of the retained topics beside an oracle.LevelTrie that holds the same ids."""
import numpy as np

from oracle import oracle as O

BULK = ["t0", "t1", "t2"]
NEVER = 0xFFFFFFFF


class Model:
    def __init__(self, eng):
        self.eng = eng
        self.ids = {}          # (tenant, topic) -> id, retained now
        self.known = {}        # (tenant, topic) -> id, every id ever seen in this generation
        self.lt = O.LevelTrie(1)

    def load(self, items):
        tn = sorted({t for t, _ in items})
        self.eng.retain_rebuild(tn, [tn.index(t) for t, _ in items], [p for _, p in items])
        ids = self.eng.retain_live_ids()
        for i, (t, p) in zip(ids, self.eng.retain_topics(ids)):
            self._add(t, p, i)
        assert len(self.ids) == len(set(items))
        return self

    def _add(self, t, p, i):
        assert self.known.setdefault((t, p), i) == i, "a topic's id changed inside a generation"
        if (t, p) not in self.ids:
            self.ids[(t, p)] = i
            self.lt.add(t, p, i)

    def _drop(self, t, p):
        i = self.ids.pop((t, p), None)
        if i is not None:
            self.lt.remove(t, p, i)

    def apply(self, ops):
        """ops: (0 = add | 1 = remove, tenant, topic) through bmq_retain_apply_batch"""
        tn = sorted({t for _, t, _ in ops})
        out = self.eng.retain_apply_batch(tn, [tn.index(t) for _, t, _ in ops], [(o, p) for o, _, p in ops])
        for (o, t, p), i in zip(ops, out.tolist()):
            if o == 0:
                assert i != NEVER
                self._add(t, p, i)
            else:
                self._drop(t, p)
        return out

    def remove_ids(self, ids):
        """the model's side of bmq_retain_remove_ids -> topics that stop being retained"""
        by_id = {i: k for k, i in self.ids.items()}
        n = 0
        for i in ids:
            if i in by_id and by_id[i] in self.ids:
                self._drop(*by_id[i])
                n += 1
        return n

    def counts(self):
        acc = {}
        for t, _ in self.ids:
            acc[t.encode()] = acc.get(t.encode(), 0) + 1
        return sorted(acc.items())

    def check(self):
        """tenant counts, live ids and the engine's counters against the model"""
        eng = self.eng
        got = eng.retain_tenant_counts()
        assert got == self.counts(), (got, self.counts())
        assert sum(n for _, n in got) == eng.retain_info().n_topics == len(self.ids) == eng.retain_find_all()[0]
        for t, n in got:
            assert len(eng.retain_live_ids(t.decode())) == n, t
        assert eng.retain_live_ids() == sorted(self.ids.values()) == sorted(self.lt.find_all())
        base = eng.retain_info().loaded_topics
        assert eng.retain_info().loaded_removed == base - sum(1 for i in self.ids.values() if i < base)


def bulk_items(per_tenant=150):
    """3 bulk-loaded tenants; first levels that start with '$' among them"""
    items = []
    for t in BULK:
        for i in range(per_tenant):
            items.append((t, ["s/%d/x", "s/%d", "$sys/%d/y", "a/b/%d"][i % 4] % i))
    return items


def churn(m: Model):
    """removes inside the bulk load, adds under a bulk tenant, a tenant that exists only in the overlay, a tenant with only '$' topics, a
    tenant all of whose topics are removed, a topic removed and retained again"""
    m.apply([(1, "t0", "s/%d/x" % i) for i in range(0, 150, 8)] + [(1, "t2", "$sys/%d/y" % i) for i in range(2, 150, 12)])
    m.apply([(0, "t1", "new/%d/z" % i) for i in range(90)] + [(0, "t1", "$new/%d" % i) for i in range(7)])
    m.apply([(0, "ov", "q/%d" % i) for i in range(130)] + [(0, "sys-only", "$SYS/broker/%d" % i) for i in range(5)])
    m.apply([(0, "empty", "e/%d" % i) for i in range(9)])
    m.apply([(1, "empty", "e/%d" % i) for i in range(9)])
    m.apply([(1, "t0", "s/1"), (1, "ov", "q/3")])
    m.apply([(0, "t0", "s/1"), (0, "ov", "q/3")])
    m.apply([(0, "rr-%02d" % (i % 70), "k/%d" % i) for i in range(210)])  # overlay ids of neighbouring lanes belong to different tenants
    return m


def populated(eng):
    return churn(Model(eng).load(bulk_items()))


def removal_cases(m: Model):
    """(name, ids): 64 consecutive ids of one word; ids across word ends; bulk-loaded and overlay ids mixed; repeats; ids that are dead"""
    base = int(m.eng.retain_info().loaded_topics)
    bound = int(m.eng.retain_info().id_bound)
    assert base >= 448 and bound >= base + 300
    return [
        ("one word", list(range(128, 192))),
        ("word ends", [255, 256, 257, 319, 320, 321] + list(range(base + 63, base + 66)) + list(range(base + 127, base + 130))),
        ("mixed", list(range(300, 310)) + list(range(base + 200, base + 230)) + [5, base + 1]),
        ("repeats", [400, 400, 401, 400, base + 250, base + 250, 401]),
        ("dead already", list(range(128, 192)) + [400, base + 250]),
    ]


def growth_case(eng, n=30000):
    """topics added in ONE batch below shared levels (on the device thousands of lanes race for the nodes of "churn" and "n<k>": the losers'
    nodes stay behind, never published), then a batch big enough to make the overlay's edge table grow and be re-filled, then the first
    topics removed by string: every one must still be found"""
    eng.retain_rebuild(["t"], [0] * 50, ["base/%d" % i for i in range(50)])
    first = ["churn/n%d/x%d" % (j % 97, j) for j in range(n)]
    ids = eng.retain_apply_batch(["t"], None, [(0, p) for p in first])
    assert len(set(ids.tolist())) == n and NEVER not in ids.tolist()
    nodes = int(eng.retain_info().overlay_nodes)
    deep = ["g/a/b/c/d/e/f/%d" % j for j in range(2 * n)]
    eng.retain_apply_batch(["t"], None, [(0, p) for p in deep])
    assert eng.retain_info().n_topics == 50 + 3 * n and eng.retain_info().overlay_nodes > 2 * nodes
    out = eng.retain_apply_batch(["t"], None, [(1, p) for p in first])
    assert out.tolist() == ids.tolist()                       # found, each under the id it was given
    assert eng.retain_info().n_topics == 50 + 2 * n
    assert eng.retain_tenant_counts() == [(b"t", 50 + 2 * n)]
    back = eng.retain_apply_batch(["t"], None, [(0, p) for p in first[::7]])
    assert back.tolist() == ids.tolist()[::7]                 # and a later add gets the same id back
