"""Cases and the reference of the fan-out caps over a match CSR (bmq_routes_cap_batch / bmq_routes_cap_dev / bmq_delivery_wait_capped),
shared by the CPU tier (tests/test_routes_cap_batch.py, a host-only engine) and the GPU tier (tests/test_routes_cap_gpu.py).

The reference is the function the engine had before: bmq_routes_cap, one call per row under that row's caps.  Its events interleave the
two types by key; the batch call orders a row's events by (type, key), so the reference's are sorted that way."""
import random

import numpy as np

from oracle import oracle as O
from tests import util as U

T = "T"
INT_MAX = 2**31 - 1
RANK_MAX = 4096  # CAPS_RANK_MAX (bifromq_amd/csrc/bmq_caps_core.h): a larger class over its cap is sorted on the host


def persistent(flt, i, tenant=T):
    return O.route_key(tenant, flt, O.FLAG_NORMAL, O.receiver_url(1, "inbox%05d" % i, "d%d" % (i % 3)))


def transient(flt, i, tenant=T):
    return O.route_key(tenant, flt, O.FLAG_NORMAL, O.receiver_url(i % 2 * 10, "mqtt%05d" % i, "d0"))  # subBrokerId 0 or 10


def group(flt, i, tenant=T):
    return O.route_key(tenant, flt, O.FLAG_ORDERED if i % 3 == 0 else O.FLAG_UNORDERED, "g%05d" % i)


def odd_receivers(flt, tenant=T):
    """receiverUrls that try the digit-prefix rule: "1abc" and "01" count as sub-broker 1 (the prefix is "1" / its value is 1), an empty
    prefix, "11" and "2" do not"""
    return [O.route_key(tenant, flt, O.FLAG_NORMAL, r) for r in ("1abc\0r\0d", "01\0r\0d", "\0r\0d", "11\0r\0d", "2\0r\0d", "x1\0r\0d")]


def class_of(key):
    """0 transient, 1 persistent, 2 group -- the rule of bmq_routes_cap, restated"""
    flag, _t, _f, recv = O.parse_route_key(key)
    if flag != 1:
        return 2
    digits = ""
    for ch in recv:
        if not ch.isdigit() or not ch.isascii():
            break
        digits += ch
    return 1 if digits and int(digits) == 1 else 0


def expected(eng, rows, caps, row_caps=None):
    """per row bmq_routes_cap under the row's caps -> (rows, class counts, events ordered per row by (type, key))"""
    out_rows, counts, events = [], [], []
    table = np.asarray(caps, dtype=np.int64).reshape(-1, 2).tolist()  # (pf, gf) or a list of such pairs
    for r, row in enumerate(rows):
        pf, gf = table[int(row_caps[r]) if row_caps is not None else 0]
        rp, ids = U.csr_of_rows([row])
        kept, cnt, ev = eng.routes_cap(rp, ids, pf, gf)
        out_rows.append(kept[0])
        counts.append(cnt[0])
        keys = eng.route_keys(np.array([e[2] for e in ev], dtype=np.uint32)) if ev else []
        events += [(typ, r, rid, mx) for (typ, _r, rid, mx), _k in sorted(zip(ev, keys), key=lambda p: (p[0][0], p[1]))]
    return out_rows, counts, events


def plain(result):
    """what Engine.routes_cap_batch returns -> (rows, class counts, events, info) in lists and tuples"""
    o_row, o_ids, cls, ev, info = result
    return U.csr_rows(o_row, o_ids), [tuple(int(x) for x in c) for c in cls], [tuple(int(x) for x in e) for e in ev], info


def batch(eng, rows, caps, row_caps=None, **kw):
    rp, ids = U.csr_of_rows(rows)
    return plain(eng.routes_cap_batch(rp, ids, caps, row_caps, **kw))


def assert_batch_equals_per_row(eng, rows, caps, row_caps=None, got=None):
    want = expected(eng, rows, caps, row_caps)
    got = got or batch(eng, rows, caps, row_caps)
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert got[2] == want[2]
    info = got[3]
    assert (info.n_in, info.n_kept, info.n_events) == (sum(len(r) for r in rows), sum(len(r) for r in want[0]), len(want[2]))
    assert info.n_rows_classified == sum(1 for c in want[1] if c != (0xFFFFFFFF, 0xFFFFFFFF))
    return got


def random_case(seed, n_keys=260, n_rows=40, max_len=70):
    """keys of three tenants, every class on a handful of filters -> (sorted keys, rows of ascending ids, row_caps)"""
    rng = random.Random(seed)
    keys = set()
    for i in range(n_keys):
        tenant = "T%d" % (i % 3)
        flt = rng.choice(["a", "a/b", "+/b", "#"])
        keys.add(rng.choice([persistent, persistent, transient, group, group])(flt, rng.randrange(10 ** 5), tenant))
    keys |= set(odd_receivers("a", "T0"))
    keys = sorted(keys)
    rows = [sorted(rng.sample(range(len(keys)), rng.choice([0, 1, 2, 5, 17, 40, max_len]))) for _ in range(n_rows)]
    return keys, rows, [rng.randrange(3) for _ in range(n_rows)]


def out_of_order_case(eng_of):
    """A rebuild, then puts whose keys sort BEFORE the persistent and group keys of the same filter: the late routes carry the largest ids and
    the smallest keys -> (engine, all keys by id, the row of every route of the filter)"""
    base = [persistent("s/t", i) for i in range(100, 112)] + [group("s/t", i) for i in range(100, 108)] + [transient("s/t", i) for i in range(4)]
    late = [persistent("s/t", i) for i in range(0, 6)] + [group("s/t", i) for i in range(0, 5)]
    eng = eng_of().rebuild(sorted(base))
    eng.apply([(0, k) for k in late])
    by_id = sorted(base) + late
    assert eng.route_keys(np.arange(len(by_id), dtype=np.uint32)) == by_id
    return eng, by_id, list(range(len(by_id)))


def sizes_case(sizes, n_transient=3):
    """one row per size m: m persistent routes, m groups and a few transient ones on a filter of its own -> (sorted keys, rows)"""
    keys = []
    for j, m in enumerate(sizes):
        flt = "f/%d" % j
        keys += [persistent(flt, i) for i in range(m)] + [group(flt, i) for i in range(m)] + [transient(flt, i) for i in range(n_transient)]
    keys = sorted(keys)
    filt = [O.parse_route_key(k)[2].split("/")[-1] for k in keys]
    return keys, [[i for i, f in enumerate(filt) if f == str(j)] for j in range(len(sizes))]
