"""Shared by test_retain_plan.py (host executor) and test_retain_plan_gpu.py: the index the plan tests run on -- the churned population of
tests/retain_gc_ref.py plus a handful of explicit topics --, the index states and duplicate patterns a plan has to tell apart, and random
batches.  The model is `present`: (tenant bytes, topic bytes) -> live topic id, what tests/retain_plan_ref.py takes."""
import random

from tests import retain_gc_ref as G
from tests import retain_plan_ref as R
from tests.test_retain_keys import SPECIAL, TENANT

T = TENANT.encode()

# name -> (tenant, topic): every state of the index a lookup can meet
STATES = {
    "bulk live": (b"t1", b"s/4/x"),
    "bulk removed": (b"t0", b"s/8/x"),
    "bulk interior": (b"t1", b"s/4"),            # "s/4/x" is retained, "s/4" is a node on the way
    "below bulk leaf": (b"t1", b"s/1/s"),
    "overlay live": (b"ov", b"q/5"),
    "overlay removed": (b"empty", b"e/3"),
    "overlay interior": (b"ov", b"p/q"),         # "p/q/r" is retained
    "below overlay leaf": (b"ov", b"p/q/r/s"),
    "unknown level": (b"t1", b"s/never-seen"),
    "unknown tenant": (b"nobody", b"s/1"),
    "empty tenant live": (b"", b"a/b"),
    "empty tenant absent": (b"", b"a"),
}


def build_index(eng):
    """-> (present, known): known = every (tenant, topic) that ever had an id in this generation"""
    m = G.populated(eng)
    m.apply([(0, "ov", "p/q/r"), (0, "", "a/b")])
    present = {(t.encode(), p.encode()): i for (t, p), i in m.ids.items()}
    known = {(t.encode(), p.encode()): i for (t, p), i in m.known.items()}
    half = SPECIAL[::2]                                            # every other special topic is retained, the others are not
    ids = eng.retain_apply_batch([TENANT], None, [(0, p) for p in half]).tolist()
    for p, i in zip(half, ids):
        present[(T, p)] = known[(T, p)] = i
    assert len(set(present.values())) == len(present) == eng.retain_info().n_topics
    return present, known


def assert_states(eng, present, known):
    """each state of STATES is what its name says"""
    base = int(eng.retain_info().loaded_topics)
    s = STATES

    def under(key, bulk):
        return any(t == key[0] and p.startswith(key[1] + b"/") and (i < base) == bulk for (t, p), i in present.items())

    def parent(key):
        return (key[0], key[1].rsplit(b"/", 1)[0])

    assert present[s["bulk live"]] < base <= present[s["overlay live"]]
    assert s["bulk removed"] not in present and known[s["bulk removed"]] < base
    assert s["overlay removed"] not in present and known[s["overlay removed"]] >= base
    assert s["bulk interior"] not in known and under(s["bulk interior"], True)
    assert s["overlay interior"] not in known and under(s["overlay interior"], False)
    assert s["below bulk leaf"] not in known and present[parent(s["below bulk leaf"])] < base
    assert s["below overlay leaf"] not in known and present[parent(s["below overlay leaf"])] >= base
    levels = {lv for _, p in known for lv in p.split(b"/")}
    assert s["unknown level"] not in known and s["unknown level"][1].split(b"/")[-1] not in levels
    assert all(t != s["unknown tenant"][0] for t, _ in known)
    assert s["empty tenant live"] in present and s["empty tenant absent"] not in known
    assert any((T, p) in present for p in SPECIAL) and any((T, p) not in present for p in SPECIAL)


def table_of(keys, extra=()):
    """tenant table of a list of (tenant, topic) keys -> (tenants, op_tenant)"""
    tenants = list(extra)
    for t, _ in keys:
        if t not in tenants:
            tenants.append(t)
    return tenants, [tenants.index(t) for t, _ in keys]


def state_batch(clear):
    """every state and every special topic once, all retains or all clears"""
    keys = list(STATES.values()) + [(T, p) for p in SPECIAL]
    tenants, ot = table_of(keys)
    return tenants, ot, [(p, clear) for _, p in keys]


def duplicate_batch():
    """-> (tenants, op_tenant, ops): [retain, clear] and [clear, retain] on a present and on an absent topic; one topic 64 times in one
    wave; one topic once in each of three waves; one topic under two tenants; one tenant's bytes at two table indices.  The rest are
    distinct filler topics nobody retains."""
    tenants = [b"t1", b"t2", b"ov", b"nobody", b"t1"]              # "t1" twice: index 0 and index 4 are the same tenant
    n = 5 * 64
    ops = [(0, b"fill/%d" % i, 1 if i % 3 == 0 else 0) for i in range(n)]

    def put(at, seq):
        for k, o in enumerate(seq):
            ops[at + k] = o
    put(0, [(0, b"s/4/x", 0), (0, b"s/4/x", 1)])                  # present: retain then clear -> REMOVE
    put(2, [(0, b"dup/absent-1", 0), (0, b"dup/absent-1", 1)])    # absent: retain then clear -> NONE
    put(4, [(2, b"q/5", 1), (2, b"q/5", 0)])                      # present: clear then retain -> UPDATE
    put(6, [(0, b"dup/absent-2", 1), (0, b"dup/absent-2", 0)])    # absent: clear then retain -> ADD
    put(8, [(0, b"s/1", 0), (1, b"s/1", 1), (3, b"s/1", 0)])      # one topic under t1 (present), t2 (present), nobody: three groups
    put(12, [(0, b"s/5", 0), (4, b"s/5", 1)])                     # one group across the two indices of "t1": REMOVE, filed under index 4
    put(14, [(4, b"two/idx", 1), (0, b"two/idx", 0)])             # ... and an ADD filed under index 0
    put(64, [(0, b"s/9", k % 2) for k in range(63)] + [(0, b"s/9", 0)])     # 64 times in the second wave, the last one retains
    for w in (2, 3, 4):
        put(64 * w + 5, [(1, b"a/b/3", 1 if w < 4 else 0)])       # once per wave, the third one retains
    return tenants, [o[0] for o in ops], [(o[1], o[2]) for o in ops]


def random_batch(present, known, n, seed, dup=0.3):
    """n ops over retained topics, removed ones, neighbours of both and fresh ones; about `dup` of them repeat an earlier key"""
    rnd = random.Random(seed)
    pool = sorted(present) + sorted(set(known) - set(present)) + list(STATES.values()) + [(T, p) for p in SPECIAL]
    keys = []
    for i in range(n):
        r = rnd.random()
        if keys and r < dup:
            keys.append(rnd.choice(keys))
        elif r < dup + 0.45:
            keys.append(rnd.choice(pool))
        elif r < dup + 0.55:
            t, p = rnd.choice(pool)
            keys.append((t, p + rnd.choice([b"/", b"/x", b"x"])))
        else:
            keys.append((rnd.choice([b"t0", b"t1", b"ov", b"fresh", b""]), b"new/%d/%d" % (seed, i)))
    tenants, ot = table_of(keys, extra=[b"unused"])
    return tenants, ot, [(p, 1 if rnd.random() < 0.3 else 0) for _, p in keys]


def run_and_check(eng, present, tenants, ot, ops, where):
    want = R.plan(tenants, ot, ops, present)
    got = eng.retain_plan(tenants, ot, ops)
    R.check(got, want, where)
    return got, want
