"""The cases of bmq_config.share_carry (member tables of shared subscriptions follow their route keys through bmq_compact /
bmq_compact_swap) that tests/test_share_carry.py runs on a host-only engine and tests/test_share_carry_gpu.py on the device (not a
conftest; nothing here is collected).  Built on tests/test_share_resolve.py and tests/share_ref.py: the workload of build_case, member
lists of R.member_list, rows checked by R.check_rows.

The model: `mirror` = every table the engine holds as {route id: (route key when it was applied, ordered, urls)}.  A generation change
keeps the tables whose id still has that key (the route was not deleted since) and whose key has an id in the new generation, re-keyed to
that id; everything expected below is computed from the KEYS in Python -- ids come from Engine.route_keys, an existing call."""
import random

import numpy as np

import bifromq_amd as B
from oracle import oracle as O
from tests import share_ref as R
from tests import util as U
from tests.test_fanout import _workload
from tests.test_share_resolve import member_url_of

NONE = 0xFFFFFFFF


def flag_of(key):
    return O.parse_route_key(key)[0]


class Model:
    def __init__(self, device, seed, share_carry=1, shared=0.4, counts=R.MEMBER_COUNTS, tables="all", **kw):
        self.rnd = random.Random(seed)
        self.tenants, keys, self.topics, self.tt = _workload(seed, shared=shared, **kw)
        self.eng = B.Engine(device=device, share_carry=share_carry).rebuild(keys)
        self.carry = share_carry == 1
        self.mirror = {}
        self.deliverers = set()
        self.senders = R.senders_for(self.rnd, len(self.topics))
        group = [k for k in keys if flag_of(k) in (2, 3)]
        chosen = {"none": [], "one": group[len(group) // 2:len(group) // 2 + 1], "all": group}[tables]
        self.give({k: R.member_list(self.rnd, counts[j % len(counts)]) for j, k in enumerate(chosen)})

    def close(self):
        self.eng.close()

    # ---- the engine's view ----
    def id_keys(self):
        n = int(self.eng.info().next_route_id)
        return self.eng.route_keys(np.arange(n, dtype=np.uint32)) if n else []

    def ref(self):
        return {k: i for i, k in enumerate(self.id_keys()) if k}

    # ---- mutations ----
    def give(self, by_key):
        """share_members_apply for the routes with these keys"""
        if not by_key:
            return
        ref = self.ref()
        self.eng.share_members_apply({ref[k]: urls for k, urls in by_key.items()})
        for k, urls in by_key.items():
            self.mirror[ref[k]] = (k, flag_of(k) == 3, list(urls))
            self.deliverers |= {R.deliverer_key(u) for u in urls}

    def apply(self, ops):
        self.eng.apply(ops)

    # ---- the expectation ----
    def survivors(self, inside=lambda k: True):
        """(tables that a generation change carries as {key: (ordered, urls)}, number of tables it drops) -- from the engine's state NOW"""
        keys = self.id_keys()
        keep = {}
        for rid, (k, ordered, urls) in self.mirror.items():
            if keys[rid] == k and inside(k):
                keep[k] = (ordered, urls)
        return keep, len(self.mirror) - len(keep)

    def generation_changed(self, keep, dropped, from_generation, replayed_deletes=()):
        """after compact() / compact_swap(): checks everything against `keep` and re-keys the mirror; -> the state as the ENGINE reports it"""
        eng = self.eng
        ref = self.ref()
        for k in replayed_deletes:
            assert k not in ref
        if not self.carry:
            inf = eng.share_info()
            assert inf.n_tables == 0 and inf.n_members == 0 and inf.generation == eng.info().generation
            ci = eng.share_carry_info()
            assert (ci.status, ci.from_generation, ci.to_generation, ci.n_carried) == (0, 0, 0, 0)
            self.mirror = {}
            return {}
        assert all(k in ref for k in keep)
        self.mirror = {ref[k]: (k, ordered, urls) for k, (ordered, urls) in keep.items()}
        tables = {rid: (ordered, urls) for rid, (_, ordered, urls) in self.mirror.items()}
        n_members = sum(len(u) for _, u in keep.values())
        inf = eng.share_info()
        assert (inf.n_tables, inf.n_members, inf.n_deliverers) == (len(keep), n_members, len(self.deliverers))
        assert inf.generation == eng.info().generation != from_generation
        ci = eng.share_carry_info()
        assert (ci.status, ci.from_generation, ci.to_generation) == (1, from_generation, eng.info().generation)
        assert (ci.n_carried, ci.n_dropped, ci.n_members_carried) == (len(keep), dropped, n_members)
        state = {}
        for rid, (k, ordered, urls) in self.mirror.items():
            got = [eng.share_member(rid, m) for m in range(len(urls))]
            assert got == [u.encode() for u in urls], k
            with_more = False
            try:
                eng.share_member(rid, len(urls))
                with_more = True
            except B.BmqError:
                pass
            assert not with_more
            state[k] = got
        # resolve over the shared pairs of a batch: rows of the brute-force matcher over the live keys (ids there = ranks), mapped to this generation's ids
        live = sorted(ref)
        rows = U.semantic_rows(O.KV(live), self.tenants, self.tt, self.topics)
        flags = [flag_of(k) for k in live]
        pairs = [(t, ref[live[r]]) for t, row in enumerate(rows) for r in row if flags[r] in (2, 3)]
        so, sh = R.sender_arrays(self.senders)
        res = eng.share_resolve([p[0] for p in pairs], [p[1] for p in pairs], so, sh, nonce=11)
        n_groups = R.check_rows(member_url_of(eng), pairs, self.senders, tables, 11, res)
        assert len(pairs) > 50 and (n_groups > 0 or not tables)
        state["rows"] = [a.tolist() if hasattr(a, "tolist") else a for a in res]
        return state


def moved_ids(before, after, keep):
    changed = sum(1 for k in keep if before[k] != after[k])
    return changed, len(keep) - changed


# ---- the cases: each returns the engine-reported state(s), so that two executors can be compared -------------------------------------
def case_compact(device, tables, seed=31):
    m = Model(device, seed, tables=tables)
    eng = m.eng
    keys = sorted(m.ref())
    group = [k for k in keys if flag_of(k) in (2, 3)]
    normal = [k for k in keys if flag_of(k) == 1]
    # normal routes that sort below group keys go, others come: ranks move -- but not those in front of the first deleted key
    cut = keys.index(group[len(group) // 3])
    ops = [(1, k) for k in normal if keys.index(k) > cut][::7][:25]
    ops += [(0, O.route_key_from_mqtt(m.rnd.choice(m.tenants), "new/%d/x" % i, O.receiver_url(0, "n%d" % i, "d1"))) for i in range(12)]
    dead = reput = new_group = None
    if tables == "all":
        dead, reput = group[1], group[-2]
        ops += [(1, dead), (1, reput)]
    m.apply(ops)
    if tables == "all":
        m.apply([(0, reput)])  # the same key again: another route, its table does not come back
        new_group = O.route_key_from_mqtt(m.tenants[0], "$oshare/late/a/+")
        m.apply([(0, new_group)])
        appended = int(eng.find_routes([new_group])[0])
        assert appended == eng.info().next_route_id - 1
        m.give({new_group: R.member_list(m.rnd, 5)})
    before = m.ref()
    keep, dropped = m.survivors()
    if tables == "all":
        assert dropped == 2 and dead not in keep and reput not in keep and new_group in keep
    gen = eng.info().generation
    eng.compact()
    states = [m.generation_changed(keep, dropped, gen)]
    after = m.ref()
    if tables == "all":
        changed, same = moved_ids(before, after, keep)
        assert changed > 0 and same > 0
        assert after[new_group] != before[new_group] and after[new_group] == sorted(after).index(new_group)  # from an appended id to its rank
    if tables == "none":
        assert not keep and eng.share_info().n_tables == 0
    # a second compact right after: a carry of carried tables
    keep2, dropped2 = m.survivors()
    assert keep2 == keep and dropped2 == 0
    gen = eng.info().generation
    eng.compact()
    states.append(m.generation_changed(keep2, 0, gen))
    assert m.ref() == after
    m.close()
    return states


def case_id_space(device, grow, seed=32):
    """the id space shrinks (next_route_id smaller after than before) or has grown since the tables were applied"""
    m = Model(device, seed, n_filters=300)
    eng = m.eng
    n0 = int(eng.info().next_route_id)
    keys = sorted(m.ref())
    if grow:
        m.apply([(0, O.route_key_from_mqtt(m.tenants[i % 2], "grown/%d/%d" % (i % 13, i), O.receiver_url(1, "g%d" % i, "d2"))) for i in range(2 * n0)])
    else:
        m.apply([(1, k) for k in keys if flag_of(k) == 1][::2] + [(1, k) for k in keys if flag_of(k) != 1][::3])
    keep, dropped = m.survivors()
    gen = eng.info().generation
    eng.compact()
    n1 = int(eng.info().next_route_id)
    assert n1 > 2 * n0 if grow else n1 < n0 - 50
    assert dropped == (0 if grow else len([k for k in keys if flag_of(k) != 1][::3]))
    state = m.generation_changed(keep, dropped, gen)
    m.close()
    return [state]


def case_swap(device, bounded, share_carry=1, seed=33):
    """compact_begin / compact_poll / compact_swap with route mutations and a share_members_apply between polls; bounded: the boundary cuts
    through the group routes -- inside carried, outside dropped"""
    m = Model(device, seed, share_carry=share_carry, counts=[1, 2, 5, 63, 65, 200])
    eng = m.eng
    keys = sorted(m.ref())
    group = [k for k in keys if flag_of(k) in (2, 3)]
    end = group[len(group) // 2] if bounded else None
    inside = (lambda k: k < end) if bounded else (lambda k: True)
    gen = eng.info().generation
    eng.compact_begin(None, end)
    assert eng.compact_poll(150) < 1000
    late_a, late_b = O.route_key_from_mqtt(m.tenants[1], "$share/late/q"), O.route_key_from_mqtt(m.tenants[0], "$oshare/late/zz/#")
    gone = [group[2], group[-3]]
    m.apply([(1, k) for k in gone] + [(0, late_a), (0, late_b), (0, O.route_key_from_mqtt(m.tenants[0], "late/normal", O.receiver_url(2, "x", "d3")))])
    eng.compact_poll(150)
    # a table given while the next generation is being built is keyed by the SERVING generation's id ...
    serving = eng.find_routes([late_a, late_b])
    assert (serving >= len(keys)).all()
    m.give({late_a: R.member_list(m.rnd, 3), late_b: R.member_list(m.rnd, 17)})
    assert eng.share_info().generation == gen
    while eng.compact_poll(150) < 1000:
        pass
    keep, dropped = m.survivors(inside)
    assert gone[0] not in keep and gone[1] not in keep
    if bounded:
        n_in = sum(1 for rid, (k, _, _) in m.mirror.items() if k < end)
        assert 0 < len(keep) < len(m.mirror) - 2 and len(keep) <= n_in and dropped == len(m.mirror) - len(keep)
    else:
        assert late_a in keep and late_b in keep and dropped == 2  # ... and is carried
    eng.compact_swap()
    state = m.generation_changed(keep, dropped, gen, replayed_deletes=gone)
    if bounded:
        assert all(k < end for k in m.ref())
    m.close()
    return [state]
