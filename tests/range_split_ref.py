"""Shared by test_range_split.py and test_range_split_gpu.py: the directed key / boundary table of the KV-boundary predicate and its Python
reference.  `start <= k < end` on bytes IS BoundaryUtil.inRange (unsigned lexicographic, a proper prefix first)."""
import numpy as np

import bifromq_amd as B

TENANTS = ["", "a", "ab", "b", "租户"]  # the last one: bytes >= 0x80 inside the first compared words
_BASE = "abcdefghijklmnop/q"
# filters that differ from _BASE at character 3, 4, 11, 12: for tenant "a" (4 bytes in front of the filter) at key byte 7, 8, 15, 16
_FILTERS = [_BASE] + [_BASE[:p] + "X" + _BASE[p + 1:] for p in (3, 4, 11, 12)] + ["+", "x/#", "s/+/t"]


def table_keys():
    keys = []
    for t in TENANTS:
        for i, f in enumerate(_FILTERS):
            keys.append(B.route_key(t, f, 1, "0\0" + "r" * ((i + len(t)) % 9) + "\0d"))  # receiver lengths vary: key lengths around multiples of 8
    return sorted(set(keys))


def tenant_prefix(tenant):
    t = tenant.encode() if isinstance(tenant, str) else bytes(tenant)
    return b"\0" + len(t).to_bytes(2, "big") + t


def upper_bound(p):
    p = p.rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def inside(keys, start=None, end=None):
    return [k for k in keys if (start is None or k >= start) and (end is None or k < end)]


def boundary_keys(keys):
    """every key the table derives a boundary from"""
    out = {b"", b"\xff" * 3, max(keys, key=len) + b"\x01" * 40}
    for k in keys:
        out.add(k)
        out.update(k[:j] for j in range(len(k)))
        out.add(k + b"\x00")
        out.add(k[:-1] + bytes([k[-1] + 1]))
    for t in TENANTS:
        out.add(tenant_prefix(t))
        out.add(upper_bound(tenant_prefix(t)))
    return sorted(out)


def boundaries(keys):
    """(start, end) pairs: every derived key as start only and as end only, neither side, and two-sided ones from neighbours at several
    distances in the sorted list (start < end always: the refusals have their own test)"""
    bk = boundary_keys(keys)
    out = [(None, None)]
    out += [(b, None) for b in bk] + [(None, b) for b in bk]
    for d in (1, 7, 101):
        out += [(bk[i], bk[i + d]) for i in range(0, len(bk) - d, 3)]
    return out


def first_difference(a, b):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i
    return None  # one is a prefix of the other


def assert_table_covers(keys):
    """what the table has to contain for the 8-byte compare steps: first differences at byte 0, 7, 8, 15, 16 and key lengths on both sides of
    a multiple of 8"""
    diffs = set()
    bk = boundary_keys(keys)
    for k in keys:
        for b in bk:
            d = first_difference(k, b)
            if d is not None:
                diffs.add(d)
    assert {0, 7, 8, 15, 16} <= diffs, sorted(diffs)
    assert {7, 0, 1} <= {len(k) % 8 for k in keys}, sorted(len(k) for k in keys)
    assert any(x >= 0x80 for k in keys for x in k[:16])


def check_table(eng, live, other=None):
    """count_in of every boundary of the table against Python (and against `other`, an engine that holds the same keys)"""
    keys = table_keys()
    n = 0
    for s, e in boundaries(keys):
        exp = inside(live, s, e)
        got = eng.count_in(start=s, end=e)
        assert got == (len(exp), sum(map(len, exp))), (s, e, got, len(exp))
        if other is not None:
            assert other.count_in(start=s, end=e) == got, (s, e)
        n += 1
    return n


def live_keys(eng):
    n = int(eng.info().next_route_id)
    return sorted(k for k in eng.route_keys(np.arange(n, dtype=np.uint32)) if k)
