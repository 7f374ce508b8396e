"""The scenario table of the key-ordered window (Engine.window) and the GC sweep over it (Engine.gc_sweep) that tests/test_gc_sweep.py runs
on a host-only engine and tests/test_gc_sweep_gpu.py on a device engine and a host-only engine in lockstep (not a conftest; nothing here
is collected).  The truth is a Python set of the live keys that the scenario keeps itself; every answer is turned into keys with
Engine.route_keys, an existing call that shares nothing with the code under test, and compared with tests/gc_sweep_ref.py; the engines'
answers are also compared with each other id for id.  Every class of the table is counted: the callers assert each count above zero."""
import collections
import ctypes as C
import random

import numpy as np

import bifromq_amd as B
from bifromq_amd import _lib
from tests import gc_sweep_ref as R

RECV = "0\0inbox\0d0"


def K(tenant, mqtt_filter, recv=RECV):
    return B.route_key_from_mqtt(tenant, mqtt_filter, recv)


def _common(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def shared_prefix_pair(tenant, total):
    """two keys of one tenant whose first `total` bytes agree and whose next byte differs"""
    head = _common(K(tenant, "a"), K(tenant, "b"))
    stem = "x" * (total - head)
    a, b = K(tenant, stem + "a"), K(tenant, stem + "b")
    assert _common(a, b) == total, (total, _common(a, b))
    return [a, b]


def base_keys():
    keys = set()
    for total in (15, 16, 17, 31, 32, 33, 300):  # around the 16-byte steps of the compare; 300: past the LDS staging of a cursor
        keys.update(shared_prefix_pair(b"p", total))
    long_filter = "/".join(["y" * 59] * 5)  # a 299-byte filter: keys that agree in 300 bytes and more, told apart by receiver and flag
    for r in ("0\0in1\0d", "0\0in10\0d", "0\0in100\0d", "0\0in2\0d"):  # receivers that are proper prefixes of one another
        keys.add(K(b"p", long_filter, r))
        keys.add(K(b"q", "a/b", r))
    for t in (b"b", b"aa", b"", b"a", b"ab", b"t" * 40):  # `b` sorts before `aa`: the u16 length leads the tenant id
        for f in ("#", "a", "a/b", "a/+", "+/#", "$share/g/a", "$oshare/g/a", "$share/g/#", "$oshare/h/a/b"):  # flags 1, 2, 3
            keys.add(K(t, f))
    for t in (b"\xc3\xa9\xff\x80\xfe", b"\x80", b"\x7f"):  # bytes >= 0x80: the order is unsigned
        for f in ("a", "é/ÿ", "é", "z/\u0080"):
            keys.add(K(t, f))
    return sorted(keys)


def extra_keys(n, seed):
    rnd = random.Random(seed)
    return [K(b"t%d" % rnd.randrange(7), "s/%d/%d" % (rnd.randrange(97), i), "0\0in%d\0d" % rnd.randrange(3)) for i in range(n)]


def cursors(live):
    """(class, cursor bytes or None) for a sorted list of live keys"""
    out = [("cursor: absent", None)]
    if not live:
        return out + [("cursor: any key, empty index", K(b"x", "a")), ("cursor: empty key", b"")]
    mid = live[len(live) // 2]
    out += [("cursor: equal to a key", mid), ("cursor: equal to the first key", live[0]), ("cursor: equal to the last key", live[-1]),
            ("cursor: between keys (a proper prefix of a key)", mid[:-1]), ("cursor: between keys (a key plus a byte)", mid + b"\0"),
            ("cursor: below all keys", b""), ("cursor: below all keys", live[0][:1]), ("cursor: above all keys", live[-1] + b"\xff"),
            ("cursor: above all keys", b"\xff\xff"), ("cursor: not a route key", b"\x00\x00\x01b\x00")]
    long_keys = [k for k in live if len(k) > 300]
    if long_keys:
        out += [("cursor: longer than the LDS staging", long_keys[len(long_keys) // 2]), ("cursor: longer than the LDS staging", long_keys[0][:-2])]
    return out


class Scenario:
    def __init__(self, engines):
        self.engines = engines
        self.live = set()
        self.counts = collections.Counter()

    # ---- one state: every cursor x window size, and a few sweeps ----
    def keys_of(self, eng, ids):
        ks = eng.route_keys(ids) if len(ids) else []
        assert all(ks), "a dead id in an answer"
        return ks

    def check_window(self, cls, lo, n, exclusive):
        exp, exp_more = R.window(self.live, lo, n, exclusive)
        first = None
        for eng in self.engines:
            ids, more = eng.window(lo, n, exclusive)
            assert ids.dtype == np.uint32
            assert (self.keys_of(eng, ids), more) == (exp, exp_more), (cls, lo, n, exclusive)
            if first is None:
                first = ids
            assert (ids == first).all(), (cls, lo, n, exclusive)
        self.counts[cls] += 1
        self.counts["window: exclusive" if exclusive else "window: inclusive"] += 1
        self.counts["window: more follows" if exp_more else "window: the last one"] += 1

    def check_sweep(self, cls, start, step, quota, boundary=None):
        exp = R.sweep(self.live, start, step, quota, boundary)
        first = None
        for eng in self.engines:
            ids, wrapped, nxt = eng.gc_sweep(start, step, quota, boundary)
            assert (self.keys_of(eng, ids), wrapped, nxt) == exp, (cls, start, step, quota)
            if first is None:
                first = ids
            assert (ids == first).all(), (cls, start, step, quota)
        self.counts[cls] += 1
        self.counts["sweep: wrapped" if exp[1] else "sweep: not wrapped"] += 1
        self.counts["sweep: next key" if exp[2] is not None else "sweep: no next key"] += 1
        if exp[0] and exp[1] and exp[2] is None:  # (no position is inspected twice: the two phases differ in p0 % step then)
            self.counts["sweep: the stride jumps over the start key after the wrap"] += 1

    def check(self, state):
        live = sorted(self.live)
        n_live = len(live)
        for cls, lo in cursors(live):
            for n in sorted({1, 2, max(n_live // 2, 1), max(n_live, 1), n_live + 5}):
                for exclusive in (False, True):
                    if lo is None and exclusive:
                        continue
                    self.check_window(cls, lo, n, exclusive)
        for cls, lo in cursors(live)[:6]:
            for step, quota in ((1, 0), (3, 0), (2, 5), (1, max(n_live, 1)), (7, n_live + 1)):
                self.check_sweep("sweep " + cls, lo, step, quota)
        self.counts["state: " + state] += 1

    def apply(self, ops):
        for eng in self.engines:
            eng.apply(ops)
        for op, k in ops:
            (self.live.discard if op else self.live.add)(k)

    def run(self):
        engines = self.engines
        self.check("no index")
        for eng in engines:
            eng.rebuild([])
        self.check("empty index")
        one = K(b"p", "only")
        self.apply([(0, one)])
        self.check("one key")
        base = base_keys()
        for eng in engines:
            eng.rebuild(base)
        self.live = set(base)
        self.check("after rebuild")
        rnd = random.Random(5)
        puts = extra_keys(150, 1)
        rnd.shuffle(puts)
        self.apply([(0, k) for k in puts])  # ids no longer follow the key order
        self.check("after puts that break the id order")
        gone = rnd.sample(sorted(self.live), 90)
        self.apply([(1, k) for k in gone])
        self.check("after deletes")
        self.apply([(0, k) for k in gone[:30]])  # the same keys under new ids
        self.check("a deleted key put again")
        for eng in engines:
            eng.compact()
        self.check("after compact")
        self.apply([(0, k) for k in extra_keys(40, 2)] + [(1, k) for k in gone[:10]])
        for eng in engines:
            eng.compact_begin()
            while eng.compact_poll(64) < 1000:
                pass
            eng.compact_swap()
        self.check("after compact_swap")
        live = sorted(self.live)
        lo, hi = live[len(live) // 4], live[3 * len(live) // 4]
        for eng in engines:
            eng.compact_begin(lo, hi)
            while eng.compact_poll(64) < 1000:
                pass
            eng.compact_swap()
        self.live = {k for k in self.live if lo <= k < hi}
        self.check("after a bounded compact_begin and swap")
        return self.counts


def expected_classes():
    return ["cursor: absent", "cursor: equal to a key", "cursor: equal to the first key", "cursor: equal to the last key",
            "cursor: between keys (a proper prefix of a key)", "cursor: between keys (a key plus a byte)", "cursor: below all keys", "cursor: above all keys",
            "cursor: not a route key", "cursor: longer than the LDS staging", "cursor: any key, empty index", "cursor: empty key", "window: exclusive",
            "window: inclusive", "window: more follows", "window: the last one", "sweep: wrapped", "sweep: not wrapped", "sweep: next key", "sweep: no next key",
            "sweep: the stride jumps over the start key after the wrap", "state: no index", "state: empty index", "state: one key", "state: after rebuild",
            "state: after puts that break the id order", "state: after deletes", "state: a deleted key put again", "state: after compact",
            "state: after compact_swap", "state: after a bounded compact_begin and swap"]


# ---- bucket sizes: N around bucket_max and beyond, ids in a shuffled order so that the pivots split unevenly ----
def sized_keys(n, long_prefix=False):
    stem = "/".join(["w" * 59] * 5) + "/" if long_prefix else "n/"  # long_prefix: every key shares 300 bytes and more
    return [K(b"big", stem + "%06d" % i, "0\0in%d\0d" % (i % 3)) for i in range(n)]


def load_shuffled(engines, keys, seed):
    order = list(keys)
    random.Random(seed).shuffle(order)
    for eng in engines:
        eng.rebuild([])
        for at in range(0, len(order), 8192):
            eng.apply([(0, k) for k in order[at:at + 8192]])
    return sorted(keys)


def check_sizes(engines, n, long_prefix=False, windows=((None, None),)):
    """-> the window_info deltas of the first engine over the windows asked"""
    live = load_shuffled(engines, sized_keys(n, long_prefix), n)
    before = engines[0].window_info()
    for lo_pos, size in windows:
        lo = None if lo_pos is None else live[lo_pos]
        m = B.BMQ_WINDOW_MAX if size is None else size
        exp, exp_more = R.window(live, lo, m)
        first = None
        for eng in engines:
            ids, more = eng.window(lo, m)
            assert more == exp_more and len(ids) == len(exp), (n, lo_pos, size, len(ids), len(exp))
            assert eng.route_keys(ids) == exp, (n, lo_pos, size)
            if first is None:
                first = ids
            assert (ids == first).all()
    after = engines[0].window_info()
    return {f: getattr(after, f) - getattr(before, f) for f in ("n_calls", "n_candidates", "n_rounds", "n_bucket_sorts", "n_rebucketed")}, after


def sweep_raw(eng, start, step, quota, cap):
    """bmq_routes_gc_sweep with a caller's cap -> (rc, reply, ids)"""
    out = np.zeros(max(cap, 1), dtype=np.uint32)
    rep = _lib.GcSweepReply()
    rc = _lib.lib().bmq_routes_gc_sweep(eng.h, start, 0 if start is None else len(start), step, quota, out.ctypes.data_as(C.c_void_p), cap, C.byref(rep))
    return rc, rep, out
