"""The mutation script of the range fan-out split hinter (bifromq_amd/hinter.py) that tests/test_fanout_hinter.py runs on a host-only engine and
tests/test_fanout_hinter_gpu.py on a device engine (not a conftest; nothing here is collected).  After every step the hinter's map and, where
the script says so, its estimate() are compared with tests/hinter_ref.py's model over the script's own set of live keys.  Every class of the
script is counted: the callers assert each count above zero."""
import collections

from bifromq_amd.hinter import RangeFanoutSplitHinter
from tests import hinter_ref as R
from tests.order_cases import K

SCALE = 5


def recv(i):
    return "0\0in%02d\0d" % i


def keys_of(tenant, mqtt_filter, receivers):
    return [K(tenant, mqtt_filter, recv(i)) for i in receivers]


class Script:
    def __init__(self, engine, granularity):
        self.eng, self.gran = engine, granularity
        self.live = set()
        self.h = RangeFanoutSplitHinter(engine, SCALE, granularity)
        self.ref = R.Hinter(lambda: sorted(self.live), SCALE, granularity)
        self.counts = collections.Counter()

    def mutate(self, ops):
        self.eng.apply(ops)
        for op, k in ops:
            (self.live.discard if op else self.live.add)(k)
        self.h.record_mutate(ops)  # after commit
        self.ref.record_mutate(ops)
        self.same()

    def same(self):
        assert self.h.splits == self.ref.map, (self.gran, self.h.splits, self.ref.map)

    def estimate(self):
        got, exp = self.h.estimate(), self.ref.estimate()
        assert got == exp, (self.gran, got, exp)
        self.same()
        return got

    def run(self):
        c, h = self.counts, self.h
        self.eng.rebuild([])
        A, B_, C_ = (b"T", "a"), (b"T", "b"), (b"T", "c")
        pa, pb = R.cut_filter(K(*A, recv(0))), R.cut_filter(K(*B_, recv(0)))
        filt = self.gran == "filter"
        self.mutate([(0, k) for k in keys_of(*A, range(10, 14))] + [(0, k) for k in keys_of(*B_, range(10, 13))])
        if self.gran != "tenant":  # (the tenant holds seven keys already)
            assert not h.splits
        c["below the scale: no entry"] += 1
        self.mutate([(0, k) for k in keys_of(*A, range(14, 17))])  # 7 under a, 3 under b behind them
        if filt:
            assert h.splits[pa][2] == sorted(self.live)[5] and h.splits[pa][2].startswith(pa)
            c["a filter crosses the scale and gets its split key"] += 1
        # the last filter of the key space reaches exactly the scale: there is no key at index `scale`
        Z = (b"\xff\xff", "zz")
        self.mutate([(0, k) for k in keys_of(*Z, range(SCALE))])
        if filt:
            assert R.cut_filter(K(*Z, recv(0))) not in h.splits and self.eng.prefix_census([R.cut_filter(K(*Z, recv(0)))])[0, 0] == SCALE
            c["exactly the scale with nothing behind it: no entry"] += 1
        # b reaches the scale with the first key of c behind it: the split key lies outside the prefix
        self.mutate([(0, K(*C_, recv(50)))])
        self.mutate([(0, k) for k in keys_of(*B_, range(13, 15))])
        if filt:
            assert h.splits[pb][2] == K(*C_, recv(50)) and not h.splits[pb][2].startswith(pb)
            c["the split key lies outside the prefix"] += 1
        hint = self.estimate()
        if filt:
            assert hint["split_key"] == h.splits[pa][2] and hint["load"]["fanout_topicfilters"] == 2 and hint["load"]["fanout_scale"] > 0
            c["estimate reports the smallest prefix"] += 1
        # hysteresis: between half the scale and the scale the entry stays, below half it goes
        self.mutate([(1, k) for k in keys_of(*A, range(10, 14))])  # 3 left: 2 * 3 >= 5
        if filt:
            assert pa in h.splits
            c["hysteresis: the entry stays between half the scale and the scale"] += 1
        self.mutate([(1, k) for k in keys_of(*A, range(14, 15))])  # 2 left
        if filt:
            assert pa not in h.splits and pb in h.splits
            c["hysteresis: the entry goes below half the scale"] += 1
        # computeIfAbsent: keys put in front of b's receivers would move the key at index `scale`; the entry keeps its old one
        old = dict(h.splits)
        self.mutate([(0, k) for k in keys_of(*B_, range(0, 3))])
        if filt:
            assert h.splits[pb] == old[pb] and R.split_key_at(sorted(self.live), pb, SCALE) != old[pb][2]
            c["computeIfAbsent: an entry keeps its old key"] += 1
        # reset to a boundary that excludes b's split key: dropped, estimated again (now the key at index `scale` of today)
        end = K(*C_, recv(50)) if filt else (h.splits[min(h.splits)][2] if h.splits else b"\xff")
        h.reset((None, end))
        self.ref.reset((None, end))
        self.same()
        if filt:
            assert h.splits[pb][2] == R.split_key_at(sorted(self.live), pb, SCALE) != old[pb][2]
            c["reset drops an entry outside the boundary and estimates it again"] += 1
        elif self.gran == "tenant":
            c["reset drops an entry outside the boundary and estimates it again"] += 1
        # estimate with a key that cannot split the boundary (equal to its start): removed, counted from before, no key
        if h.splits:
            p = min(h.splits)
            start = h.splits[p][2]
            h.reset((start, None))
            self.ref.reset((start, None))
            self.same()
            assert p in h.splits  # (in range: key >= start)
            n = len(h.splits)
            hint = self.estimate()
            assert hint["split_key"] is None and hint["load"] == {"fanout_topicfilters": n, "fanout_scale": 0.0} and p not in h.splits
            c["estimate removes an entry whose key cannot split"] += 1
            assert self.estimate()["load"]["fanout_topicfilters"] == n - 1
        h.reset((None, b""))  # the NULL boundary: nothing is in range, nothing is splittable
        self.ref.reset((None, b""))
        self.same()
        assert self.estimate()["split_key"] is None
        if self.gran == "key":
            assert not h.splits
            c["granularity key never reaches the scale"] += 1
        return c


def expected_classes(granularity):
    common = ["below the scale: no entry"]
    if granularity == "filter":
        return common + ["a filter crosses the scale and gets its split key", "exactly the scale with nothing behind it: no entry",
                         "the split key lies outside the prefix", "estimate reports the smallest prefix",
                         "hysteresis: the entry stays between half the scale and the scale", "hysteresis: the entry goes below half the scale",
                         "computeIfAbsent: an entry keeps its old key", "reset drops an entry outside the boundary and estimates it again",
                         "estimate removes an entry whose key cannot split"]
    if granularity == "tenant":
        return common + ["reset drops an entry outside the boundary and estimates it again", "estimate removes an entry whose key cannot split"]
    return common + ["granularity key never reaches the scale"]
