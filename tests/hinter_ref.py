"""A model of the per-prefix census and of the range fan-out split hinter in plain Python over a sorted list of live route keys (not a
conftest; nothing here is collected).  It shares no code with the engine nor with bifromq_amd/hinter.py: the census is `startswith`,
the split key a `bisect`, the key is taken apart here again, and the state machine restates DW/hinter/FanoutSplitHinter.java on its own."""
import bisect


def flag_of(key):
    """the flag byte of a route key: ... | bucket | flag | receiver | u16be(len receiver)"""
    rlen = (key[-2] << 8) | key[-1]
    return key[len(key) - 2 - rlen - 1]


def census(live, prefixes):
    """[[keys with flag 1, with flag 2, with flag 3, bytes]] per prefix"""
    out = []
    for p in prefixes:
        row = [0, 0, 0, 0]
        for k in live:
            if k.startswith(p):
                row[flag_of(k) - 1] += 1
                row[3] += len(k)
        out.append(row)
    return out


def split_key_at(live, prefix, index):
    """the key at `index` among the sorted live keys >= prefix, None if there are not that many"""
    at = bisect.bisect_left(live, prefix) + index
    return live[at] if at < len(live) else None


def upper_bound(key):
    k = key
    while k and k[-1] == 0xFF:
        k = k[:-1]
    return k[:-1] + bytes([k[-1] + 1]) if k else None


def cut_tenant(key):
    return key[:3 + ((key[1] << 8) | key[2])]


def cut_filter(key):
    rlen = (key[-2] << 8) | key[-1]
    return key[:len(key) - rlen - 4]


class Hinter:
    """`live` is a callable that returns the sorted live keys at the moment of the call"""

    def __init__(self, live, split_at_scale, granularity="filter", boundary=(None, None)):
        self.live, self.scale, self.boundary = live, split_at_scale, boundary
        self.cut = {"filter": cut_filter, "tenant": cut_tenant, "key": lambda k: k}[granularity]
        self.map = {}

    def _estimate(self, prefixes):
        live = self.live()
        cand = []
        for p in sorted(set(prefixes)):
            under = [k for k in live if k.startswith(p)]
            if len(under) >= self.scale:
                size = sum(len(k) for k in under)
                cand.append((p, size, size // len(under)))
            elif p in self.map and len(under) < 0.5 * self.scale:
                del self.map[p]
        for p, size, rec in cand:
            if p not in self.map:
                key = split_key_at(live, p, self.scale)
                if key is not None:
                    self.map[p] = (size, rec, key)

    def record_mutate(self, ops):
        self._estimate([self.cut(k) for _, k in ops])

    def reset(self, boundary):
        self.boundary = boundary
        start, end = boundary
        out = [p for p, (_, _, key) in self.map.items() if not ((start is None or key >= start) and (end is None or key < end))]
        for p in out:
            del self.map[p]
        self._estimate(out)

    def estimate(self):
        n = len(self.map)
        split_key, scale = None, 0.0
        if self.map:
            p = sorted(self.map)[0]
            size, rec, key = self.map[p]
            start, end = self.boundary
            ok = not (start is None and end == b"") and key != b"" and (start is None or start < key) and (end is None or key < end)
            if ok:
                split_key, scale = key, size / rec
            else:
                del self.map[p]
        return {"type": "fanout_split_hinter", "split_key": split_key, "load": {"fanout_topicfilters": n, "fanout_scale": scale}}
