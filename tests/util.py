"""Shared helpers for the parity tests: random topic/filter generators and oracle adapters."""
import random

import numpy as np

from oracle import oracle as O

ALPHABET = ["a", "b", "c", "", "$sys", "$x", "你好", "😄", "dev", "+x", "a b", "#a", "x" * 17, "y" * 40]


def host_threads():
    """threads for the oracle's parallel legs: the CPUs the cgroup really grants (the GPU boxes show 256 and grant 16)"""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 8)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:  # noqa: BLE001
        pass
    return max(1, n)


def rand_level(rnd, alphabet=ALPHABET):
    return rnd.choice(alphabet)


def rand_topic(rnd, max_levels=5, alphabet=ALPHABET):
    return "/".join(rand_level(rnd, alphabet) for _ in range(rnd.randint(1, max_levels)))


def rand_filter(rnd, max_levels=5, alphabet=ALPHABET):
    n = rnd.randint(1, max_levels)
    lv = []
    for i in range(n):
        p = rnd.random()
        if p < 0.2:
            lv.append("+")
        elif p < 0.3 and i == n - 1:
            lv.append("#")
        else:
            lv.append(rand_level(rnd, alphabet))
    return "/".join(lv)


def rand_route_key(rnd, tenant, topic_filter, rid):
    p = rnd.random()
    if p < 0.1:
        return O.route_key_from_mqtt(tenant, "$share/g%d/%s" % (rnd.randint(0, 3), topic_filter))
    if p < 0.15:
        return O.route_key_from_mqtt(tenant, "$oshare/g%d/%s" % (rnd.randint(0, 3), topic_filter))
    broker = rnd.choice([0, 1, 1, 2])
    return O.route_key_from_mqtt(tenant, topic_filter, O.receiver_url(broker, "inbox%d" % rid, "d%d" % (rid % 7)))


def oracle_rows(kv, tenants, topic_tenant, topics):
    """Per-topic sorted route ranks from the structural oracle, one matchAll per tenant (whole-batch mode)."""
    rows = [None] * len(topics)
    by_tenant = {}
    for i, ti in enumerate(topic_tenant):
        by_tenant.setdefault(int(ti), []).append(i)
    for ti, idxs in by_tenant.items():
        res = kv.match_all(tenants[ti], [topics[i] for i in idxs]).per_topic()
        for j, i in enumerate(idxs):
            rows[i] = sorted(res[j])
    return rows


def semantic_rows(kv, tenants, topic_tenant, topics):
    """Authoritative rows: the reference's own brute-force TopicMatcher (TRIET/TopicMatcher.java:39-101, restated
    in bmq_oracle.cpp) applied to every key of the tenant.  O(topics x keys of tenant)."""
    rows = [None] * len(topics)
    by_tenant = {}
    for i, ti in enumerate(topic_tenant):
        by_tenant.setdefault(int(ti), []).append(i)
    for ti, idxs in by_tenant.items():
        res = kv.match_bruteforce(tenants[ti], [topics[i] for i in idxs]).per_topic()
        for j, i in enumerate(idxs):
            rows[i] = res[j]
    return rows


def csr_rows(row_ptr, ids):
    return [ids[row_ptr[i]:row_ptr[i + 1]].tolist() for i in range(len(row_ptr) - 1)]


def rows_as_ranks(eng, row_ptr, ids, keys_sorted, rows=None):
    """Engine route ids are stable handles (ranks after a rebuild, later ids for routes added by bmq_routes_apply); the oracles
    speak in ranks of the sorted key list.  Maps every id through bmq_route_keys to its key and then to the key's rank in
    `keys_sorted` (KeyError: the engine returned a route the model does not hold), rows sorted ascending.
    rows: only these row indices (default all)."""
    rows = range(len(row_ptr) - 1) if rows is None else rows
    if len(ids) == 0:
        return [[] for _ in rows]
    want = np.unique(np.concatenate([ids[row_ptr[i]:row_ptr[i + 1]] for i in rows] + [np.zeros(0, dtype=ids.dtype)]))
    rank = {k: i for i, k in enumerate(keys_sorted)}
    m = {int(u): rank[k] for u, k in zip(want, eng.route_keys(want))}
    return [sorted(m[int(x)] for x in ids[row_ptr[i]:row_ptr[i + 1]]) for i in rows]


def quirk_ii_filters(keys):
    """(tenant, filter F) pairs for which the KV also holds a filter F + "/" + "" + ... (next level empty).
    The reference's probe-then-seek loop can skip F's keys in that situation (SURVEY.md 8c quirk ii,
    DW/cache/TenantRouteMatcher.java:127-137): keys of "F/" sort between the seek target of F and F's own keys
    with a non-zero bucket byte.  The semantic oracle is authoritative there."""
    filters = set()
    for k in keys:
        flag, tenant, mqtt, _ = O.parse_route_key(k)
        if flag != 1:
            mqtt = mqtt.split("/", 2)[2]
        filters.add((tenant, mqtt))
    out = set()
    for tenant, f in filters:
        parts = f.split("/")
        for i in range(1, len(parts)):
            if parts[i] == "":
                out.add((tenant, "/".join(parts[:i])))
    return out


def assert_rows_equal_modulo_quirk_ii(keys, tenants, topic_tenant, reference_rows, engine_rows):
    """reference_rows come from the structural restatement in the reference's production call pattern (one
    matchAll per topic); they may only differ from the engine by routes LOST to quirk (ii)."""
    quirk = None
    differ = []
    for i, (ref, got) in enumerate(zip(reference_rows, engine_rows)):
        if ref == got:
            continue
        differ.append(i)
        if quirk is None:
            quirk = quirk_ii_filters(keys)
        assert set(ref) <= set(got), i
        for r in set(got) - set(ref):
            flag, tenant, mqtt, _ = O.parse_route_key(keys[r])
            if flag != 1:
                mqtt = mqtt.split("/", 2)[2]
            assert (tenant, mqtt) in quirk, (i, mqtt)
    return differ  # the rows the reference loses routes in (callers check every one of them against the semantic oracle)


def retain_order(tenant_names, topic_tenant, topics):
    """The id order of the retained-topic index, computed independently of the engine: distinct (tenant, topic) pairs, tenants
    in byte order of their ids, a tenant's topics ordered level list by level list (levels compared as bytes, a shorter list
    first).  -> list of (tenant str, topic str); the engine's topic id must be the index in this list."""
    def b(x):
        return x if isinstance(x, bytes) else x.encode()
    pairs = {(b(tenant_names[int(t)]), tuple(b(tp).split(b"/"))) for t, tp in zip(topic_tenant, topics)}
    return [(t.decode(), b"/".join(lv).decode()) for t, lv in sorted(pairs)]


def csr_select(row_ptr, ids, sel):
    """the CSR restricted to rows `sel` -> (row_ptr', ids')"""
    sel = np.asarray(sel, dtype=np.int64)
    cnt = (row_ptr[sel + 1].astype(np.int64) - row_ptr[sel].astype(np.int64))
    rp = np.concatenate([[0], np.cumsum(cnt)])
    idx = np.repeat(row_ptr[sel].astype(np.int64) - rp[:-1], cnt) + np.arange(rp[-1], dtype=np.int64)
    return rp, ids[idx]


def csr_sorted(rp, vals):
    """every row sorted ascending (vectorised; rows that already ascend -- the oracle's matchAll walks the KV in key order -- cost one diff)"""
    if len(vals) > 1:
        d = np.diff(vals.astype(np.int64)) > 0
        starts = np.asarray(rp[1:-1], dtype=np.int64)
        starts = starts[(starts > 0) & (starts < len(vals))]
        d[starts - 1] = True  # row boundaries do not count
        if d.all():
            return vals
    r = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    return vals[np.lexsort((vals, r))]


def assert_csr_equal_modulo_quirk_ii(all_keys_fn, key_of, tenants, topic_tenant, ref_rp, ref_vals, got_rp, got_vals, quirk_cache=None):
    """Whole-CSR comparison for the full-size tests (millions of ids: no Python loop over rows that agree).
    ref_*: the structural oracle in the production call pattern, rows in any order; got_*: the engine, rows ascending.
    Rows may differ only by routes the reference LOSES to quirk (ii) (see assert_rows_equal_modulo_quirk_ii).
    all_keys_fn() -> every key of the index (only called if some row differs); key_of(rank) -> key.  Returns the indices of the
    rows that differed (the caller checks a sample of them against the semantic oracle)."""
    ref_vals = csr_sorted(ref_rp, ref_vals)
    n = len(ref_rp) - 1
    assert len(got_rp) - 1 == n
    if np.array_equal(ref_rp, got_rp) and np.array_equal(ref_vals, got_vals):
        return np.zeros(0, dtype=np.int64)
    rc, gc = np.diff(ref_rp), np.diff(got_rp)

    def row_sums(rp, vals):  # order-independent 64-bit checksum per row (empty rows: 0)
        x = (vals.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        cs = np.concatenate([[np.uint64(0)], np.cumsum(x, dtype=np.uint64)])
        return cs[rp[1:]] - cs[rp[:-1]]

    differ = (rc != gc) | (row_sums(ref_rp, ref_vals) != row_sums(got_rp, got_vals))
    same = np.nonzero(~differ)[0]
    a_rp, a = csr_select(ref_rp, ref_vals, same)
    b_rp, b = csr_select(got_rp, got_vals, same)
    assert np.array_equal(a, b)  # the rows whose checksums agree are really equal
    if quirk_cache is not None and "quirk" in quirk_cache:  # (a caller that compares one KV in several chunks parses its keys once)
        quirk = quirk_cache["quirk"]
    else:
        quirk = quirk_ii_filters(all_keys_fn())
        if quirk_cache is not None:
            quirk_cache["quirk"] = quirk
    for i in np.nonzero(differ)[0]:
        ref = set(ref_vals[ref_rp[i]:ref_rp[i + 1]].tolist())
        got = set(got_vals[got_rp[i]:got_rp[i + 1]].tolist())
        assert ref <= got, i
        for r in got - ref:
            flag, tenant, mqtt, _ = O.parse_route_key(key_of(r))
            if flag != 1:
                mqtt = mqtt.split("/", 2)[2]
            assert (tenant, mqtt) in quirk, (i, mqtt)
    return np.nonzero(differ)[0]


def sub_packed(data, off, sel):
    """the packed strings `sel` of (data, off) as a packed pair of their own (padded for the engine / oracle readers)"""
    sel = np.asarray(sel, dtype=np.int64)
    raw = data.tobytes() if not isinstance(data, (bytes, bytearray)) else data
    o = np.concatenate([[0], np.cumsum((off[sel + 1].astype(np.int64) - off[sel].astype(np.int64)))]).astype(np.uint32)
    d = np.zeros(int(o[-1]) + 32, dtype=np.uint8)
    d[:int(o[-1])] = np.frombuffer(b"".join(raw[off[i]:off[i + 1]] for i in sel), dtype=np.uint8)
    return d, o


def parity_report(config, **fields):
    """One line per full-size parity comparison: how far the engine's rows are from the STRUCTURAL restatement of the reference
    (rows the reference loses routes in: quirks (ii)/(iv) of DESIGN.md section 2) and that every such row equals the semantic oracle.
    Printed (pytest -s / a failing test shows it) and appended to gpurun_out/parity_report.jsonl when that directory is writable."""
    import json
    import os
    import sys
    line = json.dumps(dict(config=config, **fields))
    print("[parity] " + line, file=sys.stderr)  # (stderr: bench.py's stdout carries its ONE JSON line and nothing else)
    try:
        d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_report.jsonl"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def assert_differing_rows_semantic(config, kv, tenants, topic_tenant, packed_topics, differ, got_rp, got, livelocks=None, extra_rows=()):
    """EVERY row that differs from the structural restatement (+ extra_rows, a sub-sample of the others) against the semantic oracle A
    (the reference's own brute-force TopicMatcher over all keys of the row's tenant, on all host cores): equal id for id.
    topic_tenant / packed_topics / got_rp / got describe the compared rows (row j of one is row j of the others); differ = indices."""
    rows = np.unique(np.concatenate([np.asarray(differ, dtype=np.int64), np.asarray(list(extra_rows), dtype=np.int64)])) if (len(differ) or len(extra_rows)) else np.zeros(0, dtype=np.int64)
    n_rows = len(got_rp) - 1
    sec = 0.0
    if len(rows):
        data, off = packed_topics
        sd, so = sub_packed(data, off, rows)
        stt = np.asarray(topic_tenant, dtype=np.uint32)[rows] if topic_tenant is not None else np.zeros(len(rows), dtype=np.uint32)
        res, sec = kv.match_semantic_batch(tenants, stt, (sd, so), threads=host_threads())
        a_rp, a = csr_select(np.asarray(got_rp), np.asarray(got), rows)
        assert np.array_equal(a_rp, res.row_ptr.astype(np.int64)), "row lengths differ from the semantic oracle"
        assert np.array_equal(np.asarray(a, dtype=np.int64), res.routes.astype(np.int64)), "ids differ from the semantic oracle"
    parity_report(config, rows_compared=int(n_rows), rows_differing_from_reference_restatement=int(len(differ)),
                  differing_rows_equal_semantic_oracle=int(len(differ)), other_rows_checked_vs_semantic_oracle=int(len(rows) - len(differ)),
                  reference_livelocks=None if livelocks is None else int(livelocks), semantic_oracle_s=round(sec, 2))
    return len(differ)


def kv_after_mutations(kb, ko, hi_old, del_ids, add_keys):
    """The key set of a KV after deletes and adds, and the rank every id maps to, WITHOUT a Python object per key (10 M of them at full
    size): the first hi_old keys of the packed, sorted (kb, ko) minus the ids del_ids plus the sorted, distinct byte strings add_keys (none
    of them an old key).  -> (oracle KV, old_rank[hi_old] (-1: deleted), add_rank[len(add_keys)], all_keys() -> the sorted key list)."""
    import bisect
    raw_k = kb.tobytes() if hasattr(kb, "tobytes") else bytes(kb)
    ko64 = np.asarray(ko, dtype=np.int64)
    dels = np.unique(np.asarray(list(del_ids), dtype=np.int64))
    alive = np.ones(hi_old, dtype=bool)
    alive[dels] = False

    class _Old:  # the old keys as a sorted sequence for bisect
        def __len__(self):
            return hi_old

        def __getitem__(self, i):
            return raw_k[ko64[i]:ko64[i + 1]]
    pos = np.asarray([bisect.bisect_left(_Old(), k) for k in add_keys], dtype=np.int64)  # old keys (deleted ones included) below the added key
    dead_below = np.concatenate([[0], np.cumsum(~alive)]).astype(np.int64)            # deleted old ids below i
    old_rank = np.arange(hi_old, dtype=np.int64) - dead_below[:-1] + np.searchsorted(pos, np.arange(hi_old), side="right")
    old_rank[~alive] = -1
    add_rank = pos - dead_below[pos] + np.arange(len(add_keys), dtype=np.int64)
    # the packed key set: the old bytes without the deleted keys' (runs between two deleted keys are copied whole) + the added keys; KV sorts
    cuts = np.concatenate([[-1], dels, [hi_old]])
    parts = [raw_k[ko64[int(cuts[x]) + 1]:ko64[int(cuts[x + 1])]] for x in range(len(cuts) - 1) if int(cuts[x]) + 1 < int(cuts[x + 1])]
    surv_len = (ko64[1:hi_old + 1] - ko64[:hi_old])[alive]
    all_len = np.concatenate([surv_len, np.asarray([len(k) for k in add_keys], dtype=np.int64)])
    m_off = np.concatenate([[0], np.cumsum(all_len)]).astype(np.uint32)
    m_raw = b"".join(parts) + b"".join(add_keys)
    assert len(m_raw) == int(m_off[-1])
    m_data = np.zeros(len(m_raw) + 32, dtype=np.uint8)
    m_data[:len(m_raw)] = np.frombuffer(m_raw, dtype=np.uint8)
    kv = O.KV(packed=(m_data, m_off))  # (sorts: rank = position in byte order = what old_rank / add_rank compute)
    n_kv = len(m_off) - 1
    assert len(kv) == n_kv == int(alive.sum()) + len(add_keys)

    def all_keys():
        so = np.concatenate([[0], np.cumsum(all_len)])
        return sorted(m_raw[so[i]:so[i + 1]] for i in range(n_kv))
    return kv, old_rank, add_rank, all_keys


def churn_case(eng, match_fn, n_tenants, per_tenant, n_ops, n_topics, sample_tenants=16, n_sample=2000, seed=0xB1F20005):
    """configs[4]: an index of n_tenants x per_tenant generated routes, then ONE batch of n_ops mutations (50 % unsubscribes of
    existing routes, 50 % subscribes of new filters, spread over all tenants) through bmq_routes_apply, then a batch of
    publishes.  Checked: route count, id stability (surviving routes keep their rank ids, deleted ids are dead, the j-th new
    route got id n_keys + j), CSR well-formed and ascending, tenant isolation of every id, and the rows of the first
    `sample_tenants` tenants bit-exact vs the oracle on the updated key set: n_sample of them, or (n_sample=None) every one.
    match_fn(tenants, topic_tenant, (data, off)) -> (row_ptr, ids): the engine's batch match (GPU), or a stand-in in the CPU test
    of this helper."""
    import random

    import numpy as np

    import bifromq_amd as B
    from oracle import oracle as O

    w = B.Workload(seed, n_tenants, per_tenant, 1)
    kb, ko = w.keys_packed()
    eng.rebuild(packed=(kb, ko))
    assert eng.info().n_routes == w.n_keys
    tn = w.tenants()
    first = np.asarray(w.tenant_first(), dtype=np.int64)
    rnd = random.Random(seed & 0xFFFF)
    mv = memoryview(kb)  # no copy of the (large) key bytes

    def key_at(i):
        return bytes(mv[int(ko[i]):int(ko[i + 1])])

    del_ids = sorted(set(rnd.randrange(w.n_keys) for _ in range(n_ops // 2)))
    ops = [(1, key_at(i)) for i in del_ids]
    per_tenant_delta = np.zeros(n_tenants, dtype=np.int64)
    owner = np.searchsorted(first, np.asarray(del_ids), side="right") - 1
    np.subtract.at(per_tenant_delta, owner, 1)
    added = {}      # key -> tenant index
    added_id = {}   # key -> the id the engine must have given it: n_keys + (number of puts before it in the batch)
    n_del = len(ops)
    for q in range(n_ops - n_ops // 2):
        t = rnd.randrange(n_tenants)
        # two in three new filters match nothing published ("churn/..."), the third is "<first level>/#" and matches a lot
        f = "churn/l1_%d/+/l3_%d" % (q % 64, q % 4096) if q % 3 else "l0_%d/#" % (q % 8)
        k = B.route_key(tn[t], f, 1, "0\0c%d\0d%d" % (q, q % 64))
        if k not in added:
            added[k] = t
            added_id[k] = w.n_keys + q
            per_tenant_delta[t] += 1
        ops.append((0, k))
    eng.apply(ops)
    assert len(ops) - n_del == n_ops - n_ops // 2
    n_new = w.n_keys - len(del_ids) + len(added)
    info = eng.info()
    assert info.n_routes == n_new and info.next_route_id == w.n_keys + (n_ops - n_ops // 2)
    # ids are stable: survivors keep their ranks, deleted ids are dead, new routes carry the ids the ABI promises
    deleted = set(del_ids)
    probe = sorted(rnd.sample(range(w.n_keys), min(300, w.n_keys))) + del_ids[:50]
    for i, k in zip(probe, eng.route_keys(probe)):
        assert k == (b"" if i in deleted else key_at(i)), i
    some_added = rnd.sample(sorted(added), min(200, len(added)))
    assert eng.route_keys([added_id[k] for k in some_added]) == some_added
    owner_of_new = {added_id[k]: t for k, t in added.items()}
    S = min(sample_tenants, n_tenants)
    hi_old = int(first[S])
    data, off, tt = w.topics(seed + 1000, n_topics)
    row, ids = match_fn(tn, tt, (data, off))
    assert row[0] == 0 and row[-1] == len(ids) and (np.diff(row.astype(np.int64)) >= 0).all()
    if len(ids):
        d = np.diff(ids.astype(np.int64))
        starts = row[1:-1][row[1:-1] < len(ids)]
        d[(starts - 1)[starts > 0]] = 1
        assert (d > 0).all()
        # tenant isolation: an old id lies in its tenant's rank range, a new id belongs to the tenant its put named
        own = np.repeat(tt.astype(np.int64), np.diff(row.astype(np.int64)))
        old = ids < w.n_keys
        assert ((ids[old] >= first[own[old]]) & (ids[old] < first[own[old] + 1])).all()
        assert not np.isin(ids[old], np.asarray(del_ids)).any()
        for x, o in zip(ids[~old].tolist(), own[~old].tolist()):
            assert owner_of_new[x] == o
    cand = np.nonzero(tt < S)[0]
    if n_sample is None:
        # EVERY publish addressed to the first S tenants (S = all of them at full size), whole-CSR comparison: the post-churn index --
        # indirect id lists, re-hashed regions, dead ids -- is where a wrong row would hide from a sample.  The key set after the batch and
        # the rank every id must map to are computed without a Python object per key (10 M of them at full size): the old keys are sorted,
        # a deleted one leaves, an added one enters at its bisection point.
        add_keys = sorted(k for k, t in added.items() if t < S)
        kv, old_rank, add_rank, all_keys = kv_after_mutations(kb, ko, hi_old, [i for i in del_ids if i < hi_old], add_keys)
        new_rank = np.full(n_ops - n_ops // 2, -1, dtype=np.int64)
        for k, rk in zip(add_keys, add_rank.tolist()):
            new_rank[added_id[k] - w.n_keys] = rk
        for rk in rnd.sample(range(len(kv)), min(50, len(kv))):  # the computed ranks are the KV's
            src = np.nonzero(old_rank == rk)[0]
            assert kv.key(rk) == (key_at(int(src[0])) if len(src) else add_keys[int(np.nonzero(add_rank == rk)[0][0])])
        traw = data.tobytes()
        t_off = np.concatenate([[0], np.cumsum((off[cand + 1] - off[cand]).astype(np.int64))]).astype(np.uint32)
        t_data = np.zeros(int(t_off[-1]) + 32, dtype=np.uint8)
        t_data[:int(t_off[-1])] = np.frombuffer(b"".join(traw[off[i]:off[i + 1]] for i in cand), dtype=np.uint8)
        stt = tt[cand]
        res, _ = kv.match_singletons(tn[:S], stt, (t_data, t_off), threads=host_threads())
        got_rp, got = csr_select(row, ids, cand)
        got = got.astype(np.int64)
        is_old = got < w.n_keys
        assert (got[is_old] < hi_old).all()
        mapped = np.where(is_old, old_rank[np.where(is_old, got, 0)], new_rank[np.where(is_old, 0, got - w.n_keys)])
        assert (mapped >= 0).all()  # no deleted id, no id of another tenant's new route
        mapped = csr_sorted(got_rp, mapped)

        differ = assert_csr_equal_modulo_quirk_ii(all_keys, kv.key, tn[:S], stt, res.row_ptr.astype(np.int64), res.routes.astype(np.int64), got_rp, mapped)
        # the semantic oracle on EVERY row that differs from the restatement + a sub-sample of the others, counted in the parity report
        assert_differing_rows_semantic("c5: %d tenants x %d routes after one batch of %d mutations, %d publishes (every publish of the first %d tenants)"
                                       % (n_tenants, per_tenant, n_ops, n_topics, S), kv, tn[:S], stt, (t_data, t_off), differ, got_rp, mapped,
                                       livelocks=res.livelocks, extra_rows=rnd.sample(range(len(cand)), min(200, len(cand))))
        assert np.isin(mapped, add_rank).any()  # routes subscribed by the batch are matched
        return n_new
    keys_s = [key_at(i) for i in range(hi_old) if i not in deleted] + [k for k, t in added.items() if t < S]
    kv = O.KV(keys_s)  # sorts
    keys_sorted = sorted(keys_s)
    sample = sorted(rnd.sample(cand.tolist(), min(n_sample, len(cand))))
    traw = data.tobytes()
    topics = [traw[off[i]:off[i + 1]] for i in sample]
    stt = tt[sample]
    import os
    res, _ = kv.match_singletons(tn[:S], stt, O.pack(topics), threads=host_threads())
    got = rows_as_ranks(eng, row, ids, keys_sorted, rows=sample)
    assert_rows_equal_modulo_quirk_ii(keys_sorted, tn[:S], stt.tolist(), [sorted(r) for r in res.per_topic()], got)
    assert any(keys_sorted[r] in added for g in got for r in g)  # routes subscribed by the batch are matched
    return n_new


# ---- fan-out grouping: bmq_fanout_group against oracle.fanout_groups (tests/test_fanout.py, tests/fanout_cases.py) ----
FANOUT_SHARED, FANOUT_DEAD = 0xFFFFFFFE, 0xFFFFFFFF


def csr_of_rows(rows):
    row = np.zeros(len(rows) + 1, dtype=np.uint32)
    row[1:] = np.cumsum([len(r) for r in rows])
    ids = np.array([x for r in rows for x in r], dtype=np.uint32)
    return row, ids


def fanout_check(eng, rows, key_of, result):
    """result of Engine.fanout_group vs the oracle: the same groups, each with the same pairs in (topic, route) order"""
    ot, orr, goff, grep, special = result
    exp, exp_shared, exp_dead = O.fanout_groups(key_of, rows)
    n_groups = len(goff) - 1
    assert goff[0] == 0 and goff[-1] == sum(len(r) for r in rows) and (np.diff(goff.astype(np.int64)) > 0).all()
    got = {}
    kinds = []
    for g in range(n_groups):
        pairs = list(zip(ot[goff[g]:goff[g + 1]].tolist(), orr[goff[g]:goff[g + 1]].tolist()))
        assert pairs == sorted(pairs)  # (topic, route id) order inside a group
        rep = int(grep[g])
        kinds.append(rep)
        if rep == FANOUT_SHARED:
            assert pairs == exp_shared
        elif rep == FANOUT_DEAD:
            assert pairs == exp_dead
        else:
            assert (any(p[1] == rep for p in pairs))  # the group is named by one of its own routes
            dk = O.deliverer_key_of(eng.route_key(rep))
            assert dk not in got
            got[dk] = pairs
    assert got == exp
    assert special == (1 if exp_shared else 0) | (2 if exp_dead else 0)
    # the special groups come last: shared, then dead
    tail = [k for k in kinds if k >= FANOUT_SHARED]
    assert kinds[len(kinds) - len(tail):] == tail == sorted(tail)
    return len(exp)
