"""Shape-directed cases of the fan-out grouping (bmq_fanout_group), shared by tests/test_fanout_shapes.py (host-only engine: the generic
passes; proves that the inputs and the reference agree without a GPU) and tests/test_fanout_shapes_gpu.py (device 0: the counting-sort fast
path of bifromq_amd/csrc/bmq_fanout_kernels.h, FO_TILE = 1024 pairs per wave, 64 pairs per segment, 64 bins per prefix chunk, at most
FO_MAX_BINS = 1026 bins).

No match is involved: bmq_fanout_group accepts any CSR, so row_ptr and ids are written by hand over a synthetic index of one tenant with
three routes for each of exactly K distinct (subBrokerId, delivererKey) pairs (the receiverId varies inside a key) and 40 $share / $oshare
routes.  The reference is oracle.fanout_groups through tests/util.py::fanout_check; everything is integer-exact.

A CSR row keeps its ids ascending, as a match would leave them (fanout_check asserts (topic, route) order inside a group)."""
import ctypes as C
import random

import numpy as np

import bifromq_amd as B
from bifromq_amd import _lib
from oracle import oracle as O
from tests import util as U

TENANT = "tenantA"
N_SHARED = 40


def index_keys(K, tag="d"):
    """sorted route keys: 3 routes for each of K deliverer keys + N_SHARED shared-subscription routes.  Route j of key k has the filter
    f/<j>/<k>, so ids (ranks) run through all keys before a key repeats; neighbouring deliverer keys differ in ONE of (subBrokerId, delivererKey)."""
    keys = []
    for k in range(K):
        for j in range(3):
            keys.append(O.route_key_from_mqtt(TENANT, "f/%d/%04d" % (j, k), O.receiver_url(k % 3, "inbox%d" % (7 * k + j), "%s%d" % (tag, k // 3))))
    for i in range(N_SHARED):
        keys.append(O.route_key_from_mqtt(TENANT, "$%sshare/g%d/s/%d" % ("o" if i % 2 else "", i % 4, i)))
    keys = sorted(set(keys))
    assert len(keys) == 3 * K + N_SHARED
    return keys


class Ctx:
    """what the cases need to know of an index: key bytes of every id handed out (None: deleted), ids by deliverer key, shared ids"""

    def __init__(self, keys_by_id):
        self.keys = [k if k else None for k in keys_by_id]
        by = {}
        self.shared, self.deleted = [], []
        for i, k in enumerate(self.keys):
            if k is None:
                self.deleted.append(i)
                continue
            dk = O.deliverer_key_of(k)
            if dk is None:
                self.shared.append(i)
            else:
                by.setdefault(dk, []).append(i)
        self.groups = sorted(by.values())  # by first id
        self.K = len(self.groups)
        self.next_id = len(self.keys)

    def key_of(self, i):
        return self.keys[i] if i < len(self.keys) else None

    def never_issued(self, rnd):
        return rnd.choice([self.next_id, self.next_id + 1, self.next_id + rnd.randrange(2, 5000), 0x7FFFFFFF, 0xFFFFFFFD])

    def without(self, gone):
        c = Ctx([None if i in gone else k for i, k in enumerate(self.keys)])
        return c


# ---- row shapes: name -> list of row lengths ---------------------------------------------------------------------------------------------
def _small_rows(total, seed):
    rnd = random.Random(seed)
    out = []
    while total > 0:
        n = min(total, rnd.choice([0, 0, 1, 1, 2, 3, 5, 9]))
        out.append(n)
        total -= n
    return out + [0] * rnd.randrange(3)


def _random_mix(seed):
    rnd = random.Random(seed)
    out, total = [], 0
    while total < 7000:
        n = 0 if rnd.random() < 0.5 else (rnd.randint(700, 1500) if rnd.random() < 0.01 else rnd.randint(1, 6))
        out.append(n)
        total += n
    return out


ROW_SHAPES = {"T%d" % t: (lambda t=t: _small_rows(t, t)) for t in (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4097)}
ROW_SHAPES.update({
    "one_row_3000": lambda: [3000],                       # a row spanning three tiles
    "rows_of_one_2500": lambda: [1] * 2500,               # the row window moves on in nearly every segment
    # runs of empty rows before, between and behind the pairs
    "empty_runs": lambda: [0] * 300 + [5] + [0] * 63 + [7] + [0] * 64 + [3] + [0] * 65 + [9] + [0] * 129 + [70] + [0] * 1000 + [4] + [0] * 400,
    # pairs 1024, 2048 and 3072 are each the first pair behind a run of empty rows (129, 64 + ..., 65): the row of a tile's first pair is the
    # LAST of several equal row_ptr entries
    "tile_behind_empty_run": lambda: [1024] + [0] * 129 + [1024] + [0] * 64 + [10] + [0] * 63 + [1014] + [0] * 65 + [500] + [0] * 300,
    "tile_behind_1000_empty_rows": lambda: [0] * 500 + [1] * 1024 + [0] * 1000 + [1] * 1024 + [0] * 65 + [1] * 100 + [0] * 500,
    "random_mix_1": lambda: _random_mix(1),
    "random_mix_2": lambda: _random_mix(2),
})
for _name, _mk in ROW_SHAPES.items():
    assert sum(_mk()) <= 10000, _name
for _name in ("tile_behind_empty_run", "tile_behind_1000_empty_rows"):  # tile borders with more than 64 equal row_ptr entries in front
    _ends = np.cumsum(ROW_SHAPES[_name]()).tolist()
    assert any(_ends.count(p) > 64 for p in (1024, 2048, 3072)), _name
assert [np.cumsum(ROW_SHAPES["tile_behind_empty_run"]()).tolist().count(p) for p in (1024, 2048, 3072)] == [130, 65, 66]


# ---- key patterns: (ctx, n pairs, rnd) -> route ids ----------------------------------------------------------------------------------------
def _pat_one_group(c, n, rnd):
    return [rnd.choice(c.groups[c.K // 2]) for _ in range(n)]


def _pat_round_robin(c, n, rnd):  # the 64 pairs of a segment all differ when K >= 64 (ids ascend through a whole round of the keys)
    return [c.groups[p % c.K][(p // c.K) % len(c.groups[p % c.K])] for p in range(n)]


def _pat_long_runs(c, n, rnd):
    out = []
    while len(out) < n:
        g = c.groups[rnd.randrange(c.K)]
        out += [rnd.choice(g) for _ in range(rnd.randint(50, 400))]
    return out[:n]


def _pat_skewed(c, n, rnd):
    return [rnd.choice(c.groups[int(c.K * rnd.random() ** 4)]) for _ in range(n)]


def _pat_shared(c, n, rnd):
    return [rnd.choice(c.shared) for _ in range(n)]


def _pat_dead(c, n, rnd):  # ids at or beyond next_route_id, and ids deleted after the CSR was made
    return [rnd.choice(c.deleted) if c.deleted and rnd.random() < 0.6 else c.never_issued(rnd) for _ in range(n)]


def _pat_mix(c, n, rnd):
    out = []
    pats = [_pat_one_group, _pat_round_robin, _pat_long_runs, _pat_skewed, _pat_shared, _pat_dead]
    while len(out) < n:
        out += rnd.choice(pats)(c, min(n - len(out), rnd.randint(1, 300)), rnd)
    return out


def _pat_default(c, n, rnd):  # for the row shapes: mostly live routes, a skewed draw, some shared, a few ids never handed out
    out = []
    for _ in range(n):
        u = rnd.random()
        out.append(rnd.choice(c.shared) if u < 0.08 else c.never_issued(rnd) if u < 0.1 else rnd.choice(c.groups[int(c.K * rnd.random() ** 2)]))
    return out


KEY_PATTERNS = {"one_group": _pat_one_group, "round_robin": _pat_round_robin, "long_runs": _pat_long_runs, "skewed": _pat_skewed,
                "only_shared": _pat_shared, "only_dead": _pat_dead, "mix": _pat_mix}
CHURNED = ("only_dead", "mix")  # patterns that want routes deleted after the first grouping: they run on an engine of their own


def make_rows(lengths, ids):
    rows, at = [], 0
    for n in lengths:
        rows.append(sorted(ids[at:at + n]))
        at += n
    assert at == len(ids)
    return rows


def rows_for(c, shape, pattern, seed):
    lengths = ROW_SHAPES[shape]()
    rnd = random.Random(seed)
    fn = KEY_PATTERNS.get(pattern, _pat_default)
    return make_rows(lengths, fn(c, sum(lengths), rnd))


# ---- engines -----------------------------------------------------------------------------------------------------------------------------
class Engines:
    """one engine per (K, churned) for a test module, over one device (-1: host-only)"""

    def __init__(self, device):
        self.device = device
        self.made = {}

    def get(self, K, churned=False):
        if (K, churned) not in self.made:
            keys = index_keys(K)
            eng = B.Engine(device=self.device).rebuild(keys)
            c = Ctx(keys)
            if churned:
                # group first, so that the per-route cache holds the routes that go: the builder then marks them dead in the cache itself
                rows = rows_for(c, "T1025", "round_robin", 5)
                U.fanout_check(eng, rows, c.key_of, eng.fanout_group(*U.csr_of_rows(rows), group_cap=2048))
                rnd = random.Random(K)
                gone = set(rnd.sample(range(len(keys)), len(keys) // 4))
                eng.apply([(1, keys[i]) for i in sorted(gone)])
                c = c.without(gone)
            self.made[(K, churned)] = (eng, c)
        return self.made[(K, churned)]

    def close(self):
        for eng, _ in self.made.values():
            eng.close()
        self.made = {}


def group(eng, rows, group_cap=2048):
    return eng.fanout_group(*U.csr_of_rows(rows), group_cap=group_cap)


def raw_group(eng, rows, group_cap):
    """bmq_fanout_group as it is, without Engine.fanout_group's retry -> (rc, n_groups, result or None)"""
    row, ids = U.csr_of_rows(rows)
    total = int(row[-1])
    ot, orr = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.uint32)
    goff, grep = np.zeros(group_cap + 1, dtype=np.uint32), np.zeros(max(group_cap, 1), dtype=np.uint32)
    ng, sp = C.c_uint32(), C.c_uint32()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().bmq_fanout_group(eng.h, p(row), p(ids), len(row) - 1, p(ot), p(orr), total, p(goff), p(grep), group_cap, C.byref(ng), C.byref(sp))
    res = (ot[:total], orr[:total], goff[:ng.value + 1], grep[:ng.value], sp.value) if rc == 0 else None
    return rc, ng.value, res


def calls(eng):
    i = eng.fanout_info()
    return int(i.n_fast_calls), int(i.n_generic_calls), int(i.n_refill_calls)


def assert_path(eng, before, fast, refill=None):
    """one grouping since `before` (= calls(eng)): answered by the fast path (device engines with at most 1024 deliverer keys) or by the
    generic passes; a host-only engine never takes the fast path"""
    now = calls(eng)
    fast = fast and eng.device >= 0
    assert (now[0] - before[0], now[1] - before[1]) == ((1, 0) if fast else (0, 1)), (before, now)
    if eng.device < 0:
        assert now[0] == 0 and now[2] == 0
    elif refill is not None:
        assert now[2] - before[2] == (1 if refill else 0), (before, now)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
SHAPE_KS = (63, 1024)


def run_row_shape(engines, K, shape):
    eng, c = engines.get(K)
    rows = rows_for(c, shape, None, 100 + K)
    before = calls(eng)
    U.fanout_check(eng, rows, c.key_of, group(eng, rows))
    assert_path(eng, before, fast=True)


def run_key_pattern(engines, K, pattern):
    eng, c = engines.get(K, churned=pattern in CHURNED)
    for shape in ("random_mix_1", "random_mix_2"):
        rows = rows_for(c, shape, pattern, 200 + K)
        before = calls(eng)
        res = group(eng, rows)
        n = U.fanout_check(eng, rows, c.key_of, res)
        assert_path(eng, before, fast=True)
        if pattern == "one_group":
            assert n == 1 and res[4] == 0
        elif pattern == "round_robin":
            assert n == K
        elif pattern == "only_shared":
            assert n == 0 and res[4] == 1 and res[3].tolist() == [U.FANOUT_SHARED]
        elif pattern == "only_dead":
            assert n == 0 and res[4] == 2 and res[3].tolist() == [U.FANOUT_DEAD]
            assert any(i < c.next_id for r in rows for i in r) and any(i >= c.next_id for r in rows for i in r)
        elif pattern == "mix":
            assert n > 1 and res[4] == 3


BIN_KS = (0, 1, 62, 63, 126, 127, 513, 1023, 1024, 1025)


def run_bin_count(device, K):
    """a new engine with exactly K deliverer keys: n_bins = K + 2 on the fast path (2: K = 0; one 64-bin chunk up to K = 62; key_bits 7 -> 8
    between 126 and 127; the 1024-slot table grows from 513 on; 1024 is n_bins == FO_MAX_BINS; 1025 must take the generic passes)"""
    keys = index_keys(K)
    eng = B.Engine(device=device).rebuild(keys)
    try:
        c = Ctx(keys)
        rnd = random.Random(K)
        lengths = ROW_SHAPES["random_mix_1"]()
        n = sum(lengths)
        if K:
            ids = _pat_round_robin(c, 3 * K, rnd) + _pat_default(c, n - 3 * K, rnd)  # every route of every key, then a random draw
        else:
            ids = [rnd.choice(c.shared) if rnd.random() < 0.7 else c.never_issued(rnd) for _ in range(n)]
        rows = make_rows(lengths, ids)
        fast = K <= 1024
        assert eng.fanout_info().generation == 0 and calls(eng) == (0, 0, 0)
        for call in range(3):
            before = calls(eng)
            res = group(eng, rows)
            assert U.fanout_check(eng, rows, c.key_of, res) == K
            assert res[4] == 3
            # the first call after a rebuild maps the route ids (the refill), a repeated one finds them mapped
            assert_path(eng, before, fast=fast, refill=call == 0)
        inf = eng.fanout_info()
        assert inf.n_keys == K and inf.generation == eng.info().generation
        # the table is kept at most half full: 1024 slots hold up to 512 keys, one growth (x 4) holds all the others here
        assert (inf.table_slots, inf.n_table_grows, inf.n_table_reseeds) == ((4096, 1, 0) if K > 512 else (1024, 0, 0))
    finally:
        eng.close()


def swap_sequence(device, K=200):
    """group, churn, compact and swap, group over the new ids, mutate and group again: the grouping state belongs to the index it was built
    over, and the swap replaces that index"""
    keys = index_keys(K)
    eng = B.Engine(device=device).rebuild(keys)
    try:
        c = Ctx(keys)
        rows = rows_for(c, "T2049", None, 1)
        U.fanout_check(eng, rows, c.key_of, group(eng, rows))
        gen0 = eng.fanout_info().generation
        gone = set(range(0, len(keys), 3))
        eng.apply([(1, keys[i]) for i in sorted(gone)])
        eng.compact_begin()
        while eng.compact_poll(256) < 1000:
            pass
        eng.compact_swap()
        assert calls(eng) == (0, 0, 0)  # the state went with the generation it belonged to
        live = eng.route_keys(np.arange(int(eng.info().next_route_id), dtype=np.uint32))
        assert sorted(live) == sorted(k for i, k in enumerate(keys) if i not in gone)
        c = Ctx(live)
        rows = rows_for(c, "T2049", None, 2)
        before = calls(eng)
        U.fanout_check(eng, rows, c.key_of, group(eng, rows))
        assert_path(eng, before, fast=True, refill=True)
        assert eng.fanout_info().generation == gen0 + 1 == eng.info().generation
        # mutate the new generation: routes with a new deliverer key, a few deleted, an old CSR and one that uses the new ids
        first = int(eng.info().next_route_id)
        new = [O.route_key_from_mqtt(TENANT, "n/%d" % i, O.receiver_url(9, "inbox%d" % i, "fresh")) for i in range(5)]
        gone = set(range(1, len(live), 7))
        eng.apply([(0, k) for k in new] + [(1, live[i]) for i in sorted(gone)])
        c = Ctx(list(live) + new).without(gone)
        res = group(eng, rows)
        U.fanout_check(eng, rows, c.key_of, res)
        assert res[4] & 2
        rows2 = [sorted(r + [first + t % 5]) if t % 4 == 0 else r for t, r in enumerate(rows)]
        U.fanout_check(eng, rows2, c.key_of, group(eng, rows2))
    finally:
        eng.close()


def state_transitions(device):
    """one engine through: first call, repeated call, group_cap too small + retry, 1024 -> 1025 deliverer keys (the path changes, the
    answers do not), deletes under an old CSR, compact_begin .. compact_swap, rebuild"""
    keys = index_keys(1024)
    eng = B.Engine(device=device).rebuild(keys)
    try:
        c = Ctx(keys)
        rows = rows_for(c, "random_mix_1", "round_robin", 3)
        for call in range(2):  # first call, repeated call
            before = calls(eng)
            assert U.fanout_check(eng, rows, c.key_of, group(eng, rows)) == 1024
            assert_path(eng, before, fast=True, refill=call == 0)
        # group_cap too small: BMQ_E_NOSPACE and the count that is needed, then the retry with it
        rc, need, _ = raw_group(eng, rows, 5)
        assert (rc, need) == (-3, 1024)
        rc, ng, res = raw_group(eng, rows, need)
        assert (rc, ng) == (0, 1024)
        U.fanout_check(eng, rows, c.key_of, res)
        # three routes of a 1025th deliverer key
        first = int(eng.info().next_route_id)
        assert first == len(keys)
        new = [O.route_key_from_mqtt(TENANT, "n/%d" % i, O.receiver_url(9, "inbox%d" % i, "fresh")) for i in range(3)]
        eng.apply([(0, k) for k in new])
        c = Ctx(keys + new)
        rows2 = [sorted(r + [first + t % 3]) if t % 50 == 0 else r for t, r in enumerate(rows)]
        for call in range(2):
            before = calls(eng)
            assert U.fanout_check(eng, rows2, c.key_of, group(eng, rows2)) == 1025
            assert_path(eng, before, fast=False, refill=call == 0)
        assert eng.fanout_info().n_keys == 1025
        # deletes: every route of keys 0 .. 9 and a scattering of single routes; the CSR was made before
        gone = {i for g in c.groups[:10] for i in g} | set(range(100, len(keys), 37))
        eng.apply([(1, c.keys[i]) for i in sorted(gone)])
        c = c.without(gone)
        assert c.K == 1015
        res = group(eng, rows2)
        U.fanout_check(eng, rows2, c.key_of, res)
        assert res[4] & 2 and int(res[3][-1]) == U.FANOUT_DEAD
        # the next generation: dense ids, 1015 keys -- on the device the fast path again
        gen = eng.info().generation
        eng.compact_begin()
        while eng.compact_poll(1024) < 1000:
            pass
        eng.compact_swap()
        assert calls(eng) == (0, 0, 0)
        live = eng.route_keys(np.arange(int(eng.info().next_route_id), dtype=np.uint32))
        assert sorted(live) == sorted(k for k in c.keys if k)
        c = Ctx(live)
        rows3 = rows_for(c, "random_mix_2", "round_robin", 4)
        for call in range(2):
            before = calls(eng)
            assert U.fanout_check(eng, rows3, c.key_of, group(eng, rows3)) == 1015
            assert_path(eng, before, fast=True, refill=call == 0)
        assert eng.fanout_info().generation == gen + 1
        # rebuild: ranks of the sorted keys again, the counts restart
        keys4 = index_keys(63, tag="r")
        eng.rebuild(keys4)
        c = Ctx(keys4)
        rows4 = rows_for(c, "T4097", None, 5)
        U.fanout_check(eng, rows4, c.key_of, group(eng, rows4))
        inf = eng.fanout_info()
        assert inf.n_fast_calls + inf.n_generic_calls == 1 and inf.n_keys == 63 and inf.generation == eng.info().generation != gen + 1
    finally:
        eng.close()
