"""Shared by test_tenant_stats.py and test_tenant_stats_gpu.py: the directed populations and boundaries of the per-tenant census
(bmq_routes_tenant_stats) and its Python reference -- a brute force over the key list with a pure-Python key parse and `start <= k < end` on
bytes, which IS BoundaryUtil.inRange (unsigned lexicographic, a proper prefix first)."""
import bifromq_amd as B

# the empty id; 1, 12, 13 and 40 bytes (the directory compares 12 bytes inline, the rest against the name pool); bytes >= 0x80; two that share
# their first 12 bytes; one whose every route is deleted below
TENANTS = [b"", b"a", b"tenant-12-by", b"tenant-13-byt", b"q" * 40, "租户".encode(), "\U0010ffff".encode(), b"tenant-12-by2", b"gone"]
RUNS = [1, 63, 64, 65, 200, 3, 130, 64, 20]  # keys per tenant: loaded in key order, the runs end on both sides of a wave's border


def parse(key: bytes):
    """route key -> (tenant id, flag): 00 | u16be(len tenant) | tenant | levels | 00 | bucket | flag | receiver | u16be(len receiver)"""
    assert key[0] == 0
    tl = int.from_bytes(key[1:3], "big")
    rl = int.from_bytes(key[-2:], "big")
    flag = key[len(key) - 2 - rl - 1]
    assert flag in (1, 2, 3)
    return key[3:3 + tl], flag


def census(keys, start=None, end=None):
    """[(tenant, normal, unordered share, ordered share, key_bytes)] in byte order of the tenant ids; tenants with nothing inside are left out"""
    acc = {}
    for k in keys:
        if (start is not None and k < start) or (end is not None and not k < end):
            continue
        t, flag = parse(k)
        row = acc.setdefault(t, [0, 0, 0, 0])
        row[flag - 1] += 1
        row[3] += len(k)
    return [(t,) + tuple(acc[t]) for t in sorted(acc)]


def key(tenant, i):
    """flags 1 / 2 / 3 mixed inside every tenant"""
    flag = 1 + (i * 7 + i // 5) % 3
    f = ["a/%d/+", "b/%d/#", "%d/x", "+/%d"][i % 4] % i
    return B.route_key(tenant, f, flag, "0\0inbox%d\0d%d" % (i, i % 3) if flag == 1 else "g%d" % (i % 4))


def directed_keys():
    return [key(t, i) for t, n in zip(TENANTS, RUNS) for i in range(n)]


def directed_deletes(keys):
    """dead references scattered through the runs, and every route of the tenant b"gone" """
    return [k for j, k in enumerate(keys) if j % 7 == 3 or parse(k)[0] == b"gone"]


def interleaved_keys(n_tenants=70, per_tenant=5):
    """round-robin across 70 tenants: handed to bmq_routes_apply in this order, every lane of a wave has a different tenant"""
    return [key(b"rr-%02d" % t, i) for i in range(per_tenant) for t in range(n_tenants)]


def tenant_prefix(t: bytes) -> bytes:
    return b"\0" + len(t).to_bytes(2, "big") + t


def upper_bound(p: bytes):
    p = p.rstrip(b"\xff")
    return p[:-1] + bytes([p[-1] + 1]) if p else None


def boundaries(keys):
    """(start, end): none; cuts inside a tenant; an end exactly at a tenant's prefix and at its upper bound (and the same as starts);
    NULL_BOUNDARY; boundaries that hold nothing"""
    s = sorted(keys)
    mid, third = s[len(s) // 2], s[len(s) // 3]
    out = [(None, None), (None, mid), (third, None), (third, mid), (None, b""), (s[-1] + b"\0", None), (mid + b"\0", mid + b"\0\0")]
    for t in (b"a", b"tenant-13-byt", b"q" * 40, "\U0010ffff".encode()):
        p = tenant_prefix(t)
        out += [(None, p), (None, upper_bound(p)), (p, None), (upper_bound(p), None), (p, upper_bound(p))]
    return out


def check(eng, live, other=None, bounds=None):
    """the census of every boundary against Python, the sum identities, the order of the tenants"""
    n = 0
    for s, e in (bounds or boundaries(live)):
        exp = census(live, s, e)
        got = eng.routes_tenant_stats(start=s, end=e)
        assert got == exp, (s, e, got[:3], exp[:3])
        assert [r[0] for r in got] == sorted(r[0] for r in got)
        assert (sum(r[1] + r[2] + r[3] for r in got), sum(r[4] for r in got)) == eng.count_in(start=s, end=e), (s, e)
        if other is not None:
            assert other.routes_tenant_stats(start=s, end=e) == got, (s, e)
        n += 1
    full = eng.routes_tenant_stats()
    assert sum(r[1] + r[2] + r[3] for r in full) == eng.info().n_routes
    return n
