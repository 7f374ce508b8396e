"""The table of prefix classes of the per-prefix census (Engine.prefix_census) and the index states it is run through: tests/test_prefix_census.py
on a host-only engine, tests/test_prefix_census_gpu.py on a device engine and a host-only engine in lockstep (not a conftest; nothing here is
collected).  The truth is a Python set of the live keys that the scenario keeps itself and tests/hinter_ref.py's `startswith` census over it;
the engines' answers are also compared with each other number for number, with Engine.count_in over [p, upper_bound(p)), with the rows of
Engine.routes_tenant_stats and with info().n_routes.  Every class of the table is counted: the callers assert each count above zero."""
import collections
import random

import numpy as np

from tests import hinter_ref as R
from tests.order_cases import K, base_keys, extra_keys


def extras():
    """keys beside order_cases.base_keys(): one filter with many receivers (a run of ids under one filter prefix), and tenant `sib` for
    the floor-is-a-sibling case"""
    out = [K(b"hot", "room/+/temp", "0\0in%d\0d" % i) for i in range(70)]
    out += [K(b"sib", f) for f in ("a", "b", "c/d", "c/e", "z")]
    return out


def below_all(live):
    """a string below every live key that is a prefix of none"""
    k = live[0]
    j = next(i for i, x in enumerate(k) if x > 0)
    return k[:j] + bytes([k[j] - 1])


def calls(live):
    """[(class, [prefixes])]: every entry is one prefix_census call over the sorted list of live keys `live`"""
    if not live:
        some = K(b"p", "a/b")
        return [("the empty prefix", [b""]), ("a key of an index that holds none", [some, R.cut_filter(some), R.cut_tenant(some)]),
                ("absent: above all keys", [b"\xff\xff"]), ("n = 64", [b"%d" % i for i in range(64)])]
    mid = live[len(live) // 2]
    out = [("the empty prefix", [b""]),
           ("tenant prefix, filter prefix and full key of a live key", [R.cut_tenant(mid), R.cut_filter(mid), mid]),
           ("cut in the middle of a level", [mid[:len(R.cut_filter(mid)) - 3], mid[:len(R.cut_tenant(mid)) + 1]]),
           ("cut in the middle of the u16 tenant length", [mid[:2], mid[:1]]),
           ("absent: between keys", [mid + b"\x00", mid[:-1] + bytes([mid[-1] ^ 0x80])]),
           ("absent: below all keys", [below_all(live)]),
           ("absent: above all keys", [b"\xff\xff", live[-1] + b"\xff"]),
           ("absent: longer than every key", [max(live, key=len) + b"x"]),
           ("all 0xFF", [b"\xff", b"\xff" * 9])]
    # receivers in1 / in10 / in100: the key of in1 up to the end of `...in1` is a proper prefix of the keys of in10 and in100
    in1 = [k for k in live if k.endswith(b"0\x00in1\x00d\x00\x07")]
    if in1:
        stem = in1[0][:-4]  # ... 0 NUL in1
        out.append(("a prefix that covers keys which are prefixes of one another up to the receiver", [in1[0], stem, stem + b"0", stem + b"00", stem + b"\x00"]))
    ff = [k for k in live if b"\xa9\xff" in k[:8]]
    if ff:
        cut = ff[0].index(b"\xa9\xff") + 2
        out.append(("ending in a 0xFF byte", [ff[0][:cut], ff[0][:cut - 1]]))
    for total in (15, 16, 17, 300):
        pair = [k for k in live if len(k) > total and sum(o[:total] == k[:total] for o in live) >= 2 and k[3:4] == b"p"]
        if pair:
            out.append(("%d bytes" % total, [pair[0][:total]]))
    chain = [b"", R.cut_tenant(mid), R.cut_filter(mid), mid]
    out.append(("a nested chain of depth 4", chain))
    sib = [k for k in live if R.cut_tenant(k) == R.cut_tenant(K(b"sib", "a"))]
    if len(sib) >= 3:
        # the table holds P and P + x, live keys P + y with y > x: their floor is the sibling P + x, which is no prefix of them
        P = R.cut_tenant(sib[0])
        out.append(("the floor is a sibling", [P, sib[0]]))
        out.append(("the floor is a sibling", [P, R.cut_filter(sib[0]), sib[1], b""]))
    hot = [k for k in live if R.cut_tenant(k) == R.cut_tenant(K(b"hot", "a"))]
    if hot:
        out.append(("a filter with many receivers", [R.cut_filter(hot[0]), hot[len(hot) // 2], R.cut_tenant(hot[0])]))
    a, b, c = R.cut_filter(live[0]), R.cut_tenant(live[-1]), live[len(live) // 3]
    out.append(("duplicates at both ends of the input", [a, b, c, b, a]))
    out.append(("duplicates at both ends of the input", [b""] + chain[1:] + [b""]))
    every = sorted({R.cut_filter(k) for k in live} | {R.cut_tenant(k) for k in live} | set(live[::3]))
    out.append(("input in descending order", every[::-1]))
    shuffled = every[:]
    random.Random(11).shuffle(shuffled)
    out.append(("input in a shuffled order", shuffled))
    for n in (1, 63, 64, 65):
        out.append(("n = %d" % n, (shuffled * (n // len(shuffled) + 1))[:n]))
    return out


def expected_classes():
    return ["the empty prefix", "tenant prefix, filter prefix and full key of a live key", "cut in the middle of a level", "cut in the middle of the u16 tenant length",
            "absent: between keys", "absent: below all keys", "absent: above all keys", "absent: longer than every key", "all 0xFF",
            "a prefix that covers keys which are prefixes of one another up to the receiver", "ending in a 0xFF byte", "15 bytes", "16 bytes", "17 bytes",
            "300 bytes", "a nested chain of depth 4", "the floor is a sibling", "a filter with many receivers", "duplicates at both ends of the input",
            "input in descending order", "input in a shuffled order", "n = 1", "n = 63", "n = 64", "n = 65", "a key of an index that holds none",
            "answer: zero", "answer: one key", "answer: more than 64 keys", "answer: every key", "cross: count_in", "cross: tenant stats", "cross: n_routes",
            "state: no index", "state: empty index", "state: after rebuild", "state: after deletes", "state: the same keys put again", "state: after compact",
            "state: an apply_async batch is open", "state: while a compaction runs", "state: while a compaction runs, keys mutated since",
            "state: after compact_swap", "state: after import_routes"]


class Scenario:
    def __init__(self, engines, make_engine):
        self.engines, self.make_engine = engines, make_engine
        self.live = set()
        self.counts = collections.Counter()

    def check(self, state, built=True):
        live = sorted(self.live)
        seen = set()
        for cls, prefixes in calls(live):
            exp = R.census(live, prefixes)
            first = None
            for eng in self.engines:
                got = eng.prefix_census(prefixes)
                assert got.dtype == np.uint64 and got.shape == (len(prefixes), 4)
                assert got.tolist() == exp, (state, cls, prefixes)
                if first is None:
                    first = got
                assert (got == first).all(), (state, cls)
            self.counts[cls] += 1
            for p, row in zip(prefixes, exp):
                n = sum(row[:3])
                self.counts["answer: zero" if n == 0 else "answer: one key" if n == 1 else "answer: every key" if n == len(live) else
                            "answer: more than 64 keys" if n > 64 else "answer: a few keys"] += 1
                if p in seen:
                    continue
                seen.add(p)
                ub = R.upper_bound(p)
                if ub is not None:  # what the parent commit answers with one call per prefix
                    for eng in self.engines:
                        assert eng.count_in(p, ub) == (n, row[3]), (state, cls, p)
                    self.counts["cross: count_in"] += 1
        for eng in self.engines:
            for name, n1, n2, n3, nbytes in eng.routes_tenant_stats():
                tp = b"\x00" + len(name).to_bytes(2, "big") + name
                assert eng.prefix_census([tp]).tolist() == [[n1, n2, n3, nbytes]], (state, name)
                self.counts["cross: tenant stats"] += 1
            if built:
                assert int(eng.prefix_census([b""])[0, :3].sum()) == eng.info().n_routes == len(live), state
                self.counts["cross: n_routes"] += 1
        self.counts["state: " + state] += 1

    def apply(self, ops):
        for eng in self.engines:
            eng.apply(ops)
        for op, k in ops:
            (self.live.discard if op else self.live.add)(k)

    def run(self):
        engines = self.engines
        self.check("no index", built=False)
        for eng in engines:
            eng.rebuild([])
        self.check("empty index")
        base = sorted(set(base_keys()) | set(extras()))
        for eng in engines:
            eng.rebuild(base)
        self.live = set(base)
        self.check("after rebuild")
        before = [(eng.info().epoch, eng.info().next_route_id) for eng in engines]
        rnd = random.Random(5)
        puts = extra_keys(150, 1)
        rnd.shuffle(puts)
        self.apply([(0, k) for k in puts])  # ids no longer follow the key order
        gone = rnd.sample(sorted(self.live), 120)
        self.apply([(1, k) for k in gone])
        state = [(eng.info().epoch, eng.info().next_route_id) for eng in engines]
        self.check("after deletes")  # dead ids are not counted
        assert [(eng.info().epoch, eng.info().next_route_id) for eng in engines] == state != before  # the call is read-only
        self.apply([(0, k) for k in gone[:60]])  # the same keys under new ids
        self.check("the same keys put again")
        for eng in engines:
            eng.compact()
        self.check("after compact")
        ops = [(0, k) for k in extra_keys(40, 2)] + [(1, k) for k in gone[60:70] if k in self.live] + [(0, k) for k in gone[60:80]]
        for eng in engines:
            eng.apply_async(ops)  # the census completes it first
        for op, k in ops:
            (self.live.discard if op else self.live.add)(k)
        self.check("an apply_async batch is open")
        for eng in engines:
            eng.apply_wait()
            eng.compact_begin()
            eng.compact_poll(64)
        self.check("while a compaction runs")  # the serving generation answers
        self.apply([(0, k) for k in extra_keys(30, 3)] + [(1, k) for k in sorted(self.live)[::9]])
        for eng in engines:
            eng.compact_poll(64)
        self.check("while a compaction runs, keys mutated since")
        for eng in engines:
            while eng.compact_poll(4096) < 1000:
                pass
            eng.compact_swap()
        self.check("after compact_swap")
        live = sorted(self.live)
        lo, hi = live[len(live) // 4], live[3 * len(live) // 4]
        fresh = [self.make_engine(i) for i in range(len(engines))]
        for src, dst in zip(engines, fresh):
            dst.rebuild([live[0]])
            dst.import_routes(src, lo, hi)
        self.engines, self.live = fresh, {live[0]} | {k for k in live if lo <= k < hi}
        self.check("after import_routes")
        for eng in fresh:
            eng.close()
        self.engines = engines
        return self.counts
