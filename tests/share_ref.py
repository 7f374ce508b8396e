"""Restatement of DeliverExecutorGroup.send(GroupMatching, ...) for the shared-subscription tests (not a conftest; nothing here touches
the library): MurmurHash3_x64_128 in pure Python, RendezvousHash.get over a member list, the unordered pick as include/bmq.h documents
it, and the delivery rows of a batch grouped by DelivererKey bytes.  Written from the description in include/bmq.h."""
M64 = (1 << 64) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
NONE = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def murmur3_x64_128(data: bytes, seed: int = 0):
    """-> (h1, h2), unsigned"""
    h1 = h2 = seed
    n = len(data)
    for o in range(0, n - n % 16, 16):
        k1 = int.from_bytes(data[o:o + 8], "little")
        k2 = int.from_bytes(data[o + 8:o + 16], "little")
        k1 = (_rotl((k1 * C1) & M64, 31) * C2) & M64
        h1 ^= k1
        h1 = (_rotl(h1, 27) + h2) & M64
        h1 = (h1 * 5 + 0x52DCE729) & M64
        k2 = (_rotl((k2 * C2) & M64, 33) * C1) & M64
        h2 ^= k2
        h2 = (_rotl(h2, 31) + h1) & M64
        h2 = (h2 * 5 + 0x38495AB5) & M64
    tail = data[n - n % 16:]
    if len(tail) > 8:
        k2 = int.from_bytes(tail[8:], "little")
        h2 ^= (_rotl((k2 * C2) & M64, 33) * C1) & M64
    if tail:
        k1 = int.from_bytes(tail[:8], "little")
        h1 ^= (_rotl((k1 * C1) & M64, 31) * C2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = fmix64(h1), fmix64(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def score_unsigned(sender: int, url) -> int:
    return murmur3_x64_128((sender & 0xFFFFFFFF).to_bytes(4, "little") + _b(url))[0]


def score(sender: int, url) -> int:
    """HashCode.asLong(): h1 as a signed 64-bit value"""
    u = score_unsigned(sender, url)
    return u - (1 << 64) if u >> 63 else u


def rendezvous(sender: int, urls, signed: bool = True) -> int:
    """index of the member RendezvousHash.get picks: the highest score, strict '>' in list order"""
    f = score if signed else score_unsigned
    best, best_s = 0, f(sender, urls[0])
    for m in range(1, len(urls)):
        s = f(sender, urls[m])
        if s > best_s:
            best, best_s = m, s
    return best


def pick(nonce: int, topic: int, route_id: int, n: int) -> int:
    """the unordered pick of include/bmq.h"""
    x = fmix64(((nonce ^ ((route_id << 32) | topic)) + 0x9E3779B97F4A7C15) & M64)
    return ((x >> 32) * n) >> 32


def deliverer_key(url) -> bytes:
    """DelivererKey(subBrokerId, delivererKey) of a member's receiverUrl, as bytes"""
    p = _b(url).split(b"\0")
    assert len(p) == 3
    return p[0] + b"\0" + p[2]


def resolve_ref(pairs, senders, tables, nonce):
    """pairs: [(topic, route id)]; senders: per topic the list of sender hashes; tables: {route id: (ordered, [urls])} of the LIVE group routes.
    -> ({DelivererKey bytes: [(pair, sender, member), ...] in (pair, sender) order}, [unresolved (pair, NONE, NONE)]); sender = index into the
    concatenation of `senders`, NONE for an unordered share."""
    first = [0]
    for s in senders:
        first.append(first[-1] + len(s))
    groups, unresolved = {}, []
    for i, (t, rid) in enumerate(pairs):
        tab = tables.get(rid)
        if tab is None:
            unresolved.append((i, NONE, NONE))
            continue
        ordered, urls = tab
        if not ordered:
            m = pick(nonce, t, rid, len(urls))
            groups.setdefault(deliverer_key(urls[m]), []).append((i, NONE, m))
            continue
        for k, sh in enumerate(senders[t]):
            m = rendezvous(sh, urls)
            groups.setdefault(deliverer_key(urls[m]), []).append((i, first[t] + k, m))
    return groups, unresolved


# ---- workloads and the comparison both test files use ------------------------------------------------------------------------------
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
SPECIAL_SENDERS = [0, 1, -1, INT_MIN, INT_MAX]
MEMBER_COUNTS = [1, 2, 63, 64, 65, 200, 1000]
# 4 + len(url): tail and block edges of the 16-byte blocks
EDGE_LENGTHS = [15, 16, 17, 31, 32, 33, 48, 64]


def url_of_len(rnd, total_len, broker, dkey, uniq):
    """a receiverUrl of exactly total_len - 4 UTF-8 bytes (so that [sender | url] is total_len long), multi-byte characters included when
    there is room; `uniq` keeps the receiver ids of one list apart where the length allows"""
    head, tail = ("%d\0" % broker).encode(), b"\0" + dkey.encode()
    room = total_len - 4 - len(head) - len(tail)
    assert room >= 0
    rid = ("%x" % uniq).encode()[:room]
    for ch in ("你".encode(), "é".encode()):
        if room - len(rid) >= len(ch) and rnd.random() < 0.7:
            rid += ch
    rid += b"r" * (room - len(rid))
    return (head + rid + tail).decode("utf-8")


def member_list(rnd, n, brokers=(0, 1, 2), dkeys=9):
    urls = []
    for m in range(n):
        total = rnd.choice(EDGE_LENGTHS) if rnd.random() < 0.6 else rnd.randint(15, 90)
        urls.append(url_of_len(rnd, total, rnd.choice(brokers), "d%d" % rnd.randrange(dkeys), m))
    return urls


def senders_for(rnd, n_topics, max_senders=4):
    out = []
    for _ in range(n_topics):
        out.append([rnd.choice(SPECIAL_SENDERS) if rnd.random() < 0.4 else rnd.randint(INT_MIN, INT_MAX) for _ in range(rnd.randint(0, max_senders))])
    return out


def sender_arrays(senders):
    import numpy as np
    off = np.zeros(len(senders) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(s) for s in senders])
    return off, np.array([x for s in senders for x in s], dtype=np.int32)


def check_rows(member_url, pairs, senders, tables, nonce, result):
    """result of Engine.share_resolve vs resolve_ref: the same groups with the same rows in (pair, sender) order; the groups partition the
    rows; the unresolved group is last.  member_url(route id, index) -> receiverUrl bytes.  -> number of resolved groups"""
    op, os_, om, goff, special = result
    exp, exp_unres = resolve_ref(pairs, senders, tables, nonce)
    n_rows = sum(len(v) for v in exp.values()) + len(exp_unres)
    assert len(op) == len(os_) == len(om) == n_rows
    assert goff[0] == 0 and goff[-1] == n_rows and all(goff[g] < goff[g + 1] for g in range(len(goff) - 1))
    got = {}
    for g in range(len(goff) - 1):
        rows = list(zip(op[goff[g]:goff[g + 1]].tolist(), os_[goff[g]:goff[g + 1]].tolist(), om[goff[g]:goff[g + 1]].tolist()))
        assert rows == sorted(rows)  # (pair, sender) order inside a group
        if rows[0][2] == NONE:
            assert g == len(goff) - 2 and rows == exp_unres
            continue
        keys = {deliverer_key(member_url(pairs[p][1], m)) for p, _, m in rows}
        assert len(keys) == 1  # a group = one DelivererKey
        dk = keys.pop()
        assert dk not in got
        got[dk] = rows
    assert got == exp
    assert special == (1 if exp_unres else 0)
    return len(got)
