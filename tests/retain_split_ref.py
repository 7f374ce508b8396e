"""Shared by test_retain_split.py and test_retain_split_gpu.py: the directed (tenant, topic) / boundary table of the KV-boundary predicate
over the retained-topic index, its Python reference and the model of the split / merge tests.  Every expected set is Python's
`start <= k < end` on bytes (BoundaryUtil.inRange: unsigned lexicographic, a proper prefix first) over oracle.retain_message_key, the
oracle's own encoder -- never the engine's keys.

    retainMessageKey = 00 | u16be(len tenant) | tenant | u16be(#levels) | one LevelHash byte per level | topic, '/' -> 00
"""
import bisect

from oracle import oracle as O

LONG = "L" * 280          # longer than any LDS staging of a boundary key
TENANTS = ["", "a", "ab", "b", "租户", LONG]


def _same_hash_pair():
    """two last levels with the SAME LevelHash byte (FNV-1a's last step is a bijection of the last unit, so they differ in two characters):
    keys that differ first in the body"""
    seen = {}
    for c in "abcdefghijklmnopqrstuvwxyz":
        for d in "0123456789":
            h = O.retain_level_hash(["v" + c + d])
            if h in seen and seen[h][0] != c:
                return "pair/v" + seen[h], "pair/v" + c + d
            seen.setdefault(h, c + d)
    raise AssertionError("no two suffixes share a LevelHash byte")


def topics():
    deep = "/".join("n%d" % i for i in range(17))
    same = _same_hash_pair()
    return [
        "one", "a/b", "a/b/c", "l1/l2/l3/l4/l5", deep,          # 1, 2, 3, 5 and 17 levels
        "a//b", "/", "a/",                                      # empty levels
        "$sys/x",                                               # a '$' first level
        "é/€",                                        # 2-byte and 3-byte UTF-8
        "e/\U0001F600",                                         # a 4-byte code point: the surrogate pair in the hash
        "last/x1", "last/x2", same[0], same[1],                 # differ only in the last body byte; equal hash bytes: the body decides
        "h/x/z", "h/y/z", "x/h/z",                              # equal level count, differ in one hash byte position
    ]


def table_items():
    return [(t, p) for t in TENANTS for p in topics()]


def key(t, p):
    return O.retain_message_key(t, p)


def tenant_prefix(tenant):
    return O.retain_tenant_begin_key(tenant)


def upper_bound(p):
    p = p.rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def is_inside(k, start=None, end=None):
    return (start is None or k >= start) and (end is None or k < end)


_BK = {}


def boundary_keys(keys):
    """every key the table derives a boundary from (as tests/range_split_ref.boundary_keys does)"""
    memo = tuple(keys)
    if memo in _BK:
        return _BK[memo]
    out = {b"", b"\xff" * 3, max(keys, key=len) + b"\x01" * 40}
    for k in keys:
        out.add(k)
        out.update(k[:j] for j in range(len(k)))
        out.add(k + b"\x00")
        out.add(k[:-1] + bytes([(k[-1] + 1) & 0xFF]) if k[-1] != 0xFF else k + b"\x01")
    for t in TENANTS:
        out.add(tenant_prefix(t))
        out.add(upper_bound(tenant_prefix(t)))
    _BK[memo] = sorted(out)
    return _BK[memo]


def boundaries(keys):
    """(start, end) pairs: every derived key as start only and as end only, neither side, and two-sided ones from neighbours at distances
    1 / 7 / 101 in the sorted list (start < end always: the refusals have their own test)"""
    bk = boundary_keys(keys)
    out = [(None, None)]
    out += [(b, None) for b in bk] + [(None, b) for b in bk]
    for d in (1, 7, 101):
        out += [(bk[i], bk[i + d]) for i in range(0, len(bk) - d, 3)]
    return out


def table_keys():
    return sorted(key(t, p) for t, p in table_items())


def segment(k, pos):
    """which segment of retainMessageKey k byte `pos` lies in"""
    tl = int.from_bytes(k[1:3], "big")
    levels = int.from_bytes(k[3 + tl:5 + tl], "big")
    if pos == 0:
        return "zero"
    if pos < 3:
        return "tenant-length"
    if pos < 3 + tl:
        return "tenant"
    if pos < 5 + tl:
        return "level-count"
    if pos < 5 + tl + levels:
        return "hash"
    return "body"


def assert_table_covers(items):
    """the first difference between some key and some boundary key falls in each segment of the key; some boundary key equals a head
    (00 | len | tenant) exactly and some is shorter than a head"""
    keys = sorted(key(t, p) for t, p in items)
    bk = boundary_keys(keys)
    heads = {tenant_prefix(t) for t, _ in items}
    seen = set()
    for k in keys:
        for b in bk:
            n = min(len(k), len(b))
            d = next((i for i in range(n) if k[i] != b[i]), None)
            if d is not None:
                seen.add(segment(k, d))
    assert {"tenant-length", "tenant", "level-count", "hash", "body"} <= seen, sorted(seen)
    assert any(b in heads for b in bk)
    assert any(len(b) < len(h) and h.startswith(b) for b in bk for h in heads)
    by_levels = {len(p.split("/")) for _, p in items}
    assert {1, 2, 3, 5, 17} <= by_levels
    a, b = _same_hash_pair()
    ka, kb = key("a", a), key("a", b)
    assert segment(ka, next(i for i in range(len(ka)) if ka[i] != kb[i])) == "body"


def _slice(ks, s, e):
    """[lo, hi) of the sorted byte strings ks with s <= k < e"""
    return (0 if s is None else bisect.bisect_left(ks, s)), (len(ks) if e is None else bisect.bisect_left(ks, e))


def check_table(eng, live, other=None, live_other=None):
    """retain_count_in and retain_ids_in of every boundary of the table against Python; the ids also against the composer (the live ids whose
    retain_keys_by_id key passes Python's compare) and, with `other` (an engine that holds the same topics, ids in live_other), counts and
    topics against it.  live: (tenant, topic) -> id of the retained topics.  Returns the number of boundaries."""
    want = sorted((key(t, p), i) for (t, p), i in live.items())
    ks = [k for k, _ in want]
    run = [0]
    for k in ks:
        run.append(run[-1] + len(k))
    bound = int(eng.retain_info().id_bound)
    composed = sorted((k, i) for i, k in enumerate(eng.retain_keys_by_id(list(range(bound + 8)))) if k)   # ids past id_bound too
    cks = [k for k, _ in composed]
    if other is not None:
        topic_of = {i: tp for tp, i in live.items()}
        owant = sorted((key(t, p), i) for (t, p), i in live_other.items())
        assert [k for k, _ in owant] == ks
    n = 0
    for s, e in boundaries(table_keys()):
        lo, hi = _slice(ks, s, e)                                   # Python's start <= k < end over the oracle's keys
        got = eng.retain_count_in(start=s, end=e)
        assert got == (hi - lo, run[hi] - run[lo]), (s, e, got, hi - lo)
        ids = eng.retain_ids_in(start=s, end=e)
        assert ids == sorted(i for _, i in want[lo:hi]), (s, e)
        clo, chi = _slice(cks, s, e)                                # ... and over the keys the composer makes of the ids
        assert ids == sorted(i for _, i in composed[clo:chi]), (s, e)
        if other is not None:
            assert other.retain_count_in(start=s, end=e) == got, (s, e)
            assert other.retain_ids_in(start=s, end=e) == sorted(i for _, i in owant[lo:hi]), (s, e)
        n += 1
    return n


class Model:
    """(tenant, topic) -> (timestamp_hlc, expiry_seconds) of the retained topics, driven beside an engine"""

    def __init__(self, eng=None):
        self.eng = eng
        self.d = {}

    def load(self, items):
        """items: (tenant, topic, ts, expiry) through bmq_retain_rebuild_ex"""
        tn = sorted({t for t, _, _, _ in items})
        self.eng.retain_rebuild(tn, [tn.index(t) for t, _, _, _ in items], [p for _, p, _, _ in items], timestamps=[s for _, _, s, _ in items],
                                expiry=[x for _, _, _, x in items])
        self.d = {(t, p): (s, x) for t, p, s, x in items}
        return self

    def apply(self, ops):
        """ops: (0, tenant, topic, ts, expiry) | (1, tenant, topic) through bmq_retain_apply_batch -> the ids"""
        tn = sorted({o[1] for o in ops})
        out = self.eng.retain_apply_batch(tn, [tn.index(o[1]) for o in ops], [(o[0], o[2]) + ((o[3], o[4]) if o[0] == 0 else (0, 0xFFFFFFFF)) for o in ops])
        self.note(ops)
        return out

    def note(self, ops):
        for o in ops:
            if o[0] == 0:
                self.d[(o[1], o[2])] = (o[3], o[4])
            else:
                self.d.pop((o[1], o[2]), None)

    def restricted(self, start=None, end=None):
        return {tp: v for tp, v in self.d.items() if is_inside(key(*tp), start, end)}


def live_state(eng):
    """(tenant, topic) -> (timestamp_hlc, expiry_seconds) of what the engine retains now"""
    ids = eng.retain_live_ids()
    return {tp: eng.retain_topic_info(i)[:2] for i, tp in zip(ids, eng.retain_topics(ids))}


def live_ids(eng):
    ids = eng.retain_live_ids()
    return dict(zip(eng.retain_topics(ids), ids))


def stamps(i):
    """distinct, recognisable stamps: an HLC (ms << 16 | counter) and an expiry interval"""
    return ((1_700_000_000_000 + 1000 * i) << 16) | (i & 0xFFFF), 60 + i % 1000


CUTS = [("ab", "a/b/c"), ("b", "h/y/z"), ("租户", "one"), (LONG, "a//b")]  # inside tenants; the fifth cut is a tenant prefix


def cuts():
    return [key(t, p) for t, p in CUTS] + [tenant_prefix("b")]
