"""The rule of the retain plan, written from the reference's Java: RetainStoreCoProc.batchRetain (RS/RetainStoreCoProc.java:193-255) for one
(tenant, topic, message), in front of it the grouping of BatchRetainCallHelper.makeBatch (a map per tenant: the LAST request of a topic stays,
scheduler/BatchRetainCallHelper.java:31-44) and BatchRetainCall.handleOutput (:57-86: every request of a topic gets the stored result).

Shared by test_retain_plan.py (host executor), test_retain_plan_gpu.py and tools/retain_plan_probe.py.  Nothing here calls the product:
`present` is a dict (tenant bytes, topic bytes) -> live topic id that the caller keeps."""
from bifromq_amd.engine import retain_message_key

NONE, ADD, UPDATE, REMOVE, SUPERSEDED = range(5)
RETAINED, CLEARED = 0, 1          # RetainResult.Code, RetainStoreCoProc.proto:50-53
NO_ID = 0xFFFFFFFF


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def plan(tenants, op_tenant, ops, present):
    """tenants: the tenant table; op_tenant: index per op (None: tenant 0); ops: (topic, clear); present: {(tenant bytes, topic bytes): id}.
    -> dict of lists: code, action, winner, topic_id, keys (per op), delta (per tenant-table entry)"""
    n = len(ops)
    tn = [_b(t) for t in tenants]
    ot = [0] * n if op_tenant is None else list(op_tenant)
    # makeBatch: requests.computeIfAbsent(tenant).put(topic, message) -- a later put of the same topic replaces the earlier one
    last = {}
    for i, (topic, _) in enumerate(ops):
        last[(tn[ot[i]], _b(topic))] = i
    code, action, winner, topic_id, keys = [0] * n, [SUPERSEDED] * n, [0] * n, [NO_ID] * n, [b""] * n
    delta = [0] * len(tn)
    for i, (topic, _) in enumerate(ops):
        k = (tn[ot[i]], _b(topic))
        w = last[k]
        clear = bool(ops[w][1])
        retained = k in present                                  # :213 index.match(tenantId, topic) is not empty
        code[i] = CLEARED if clear else RETAINED                 # :220 / :234, handed to every request of the topic
        winner[i] = w
        topic_id[i] = present.get(k, NO_ID)
        if i != w:
            continue
        if clear:                                                # :214-222
            action[i] = REMOVE if retained else NONE
        else:                                                    # :223-233
            action[i] = UPDATE if retained else ADD
        if action[i] != NONE:
            keys[i] = retain_message_key(k[0], k[1])             # :212, written by :217 / :225 / :230
        if action[i] == ADD:
            delta[ot[i]] += 1                                    # :244
        if action[i] == REMOVE:
            delta[ot[i]] -= 1                                    # :252
    return {"code": code, "action": action, "winner": winner, "topic_id": topic_id, "keys": keys, "delta": delta}


def check(got, want, where=""):
    """a RetainPlan of the engine against plan()'s dict, output for output"""
    assert got.code.tolist() == want["code"], where
    assert got.action.tolist() == want["action"], where
    assert got.winner.tolist() == want["winner"], where
    assert got.topic_id.tolist() == want["topic_id"], where
    assert got.delta.tolist() == want["delta"], where
    assert got.keys == want["keys"], where
    a = want["action"]
    info = got.info
    assert (info.n_add, info.n_update, info.n_remove, info.n_none) == (a.count(ADD), a.count(UPDATE), a.count(REMOVE), a.count(NONE)), where
    assert info.n_groups == len(a) - a.count(SUPERSEDED) and info.key_bytes == sum(map(len, want["keys"])), where


def apply_to(present, tenants, op_tenant, ops, want, ids):
    """the post-commit closure (:240-255) on the model: ids = out_topic_ids of the commit"""
    tn = [_b(t) for t in tenants]
    for i, (topic, _) in enumerate(ops):
        k = (tn[0 if op_tenant is None else op_tenant[i]], _b(topic))
        if want["action"][i] in (ADD, UPDATE):
            assert ids[i] != NO_ID
            if want["action"][i] == UPDATE:
                assert ids[i] == present[k]                      # the id of an updated topic does not change
            present[k] = ids[i]
        elif want["action"][i] == REMOVE:
            assert ids[i] == present.pop(k)
        else:
            assert ids[i] == NO_ID
