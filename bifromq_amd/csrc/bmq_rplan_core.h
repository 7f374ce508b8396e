// bmq_rplan_core.h -- the PLAN of a batch of retain ops: the pre-commit half of RetainStoreCoProc.batchRetain (RS/RetainStoreCoProc.java:193-239)
// for a whole batch, where the retained-topic index lives.  Per (tenant, topic, message) the reference asks the index whether the topic is
// retained now (index.match(tenantId, topic), :213), decides CLEARED / RETAINED (:214-234), issues a put or a delete of
// retainMessageKey(tenant, topic) (:212,217,225,230) and files the topic under add / update / remove for the post-commit closure and the
// per-tenant topic count (:240-255).  Equal (tenant, topic) pairs of one batch are grouped as BatchRetainCallHelper.makeBatch groups them
// (bifromq-retain-server/.../scheduler/BatchRetainCallHelper.java:31-44: a map per tenant, the LAST request of a topic stays) and every op
// of a group reports the winner's code, as BatchRetainCall.handleOutput hands it out (:57-86).
//
// Every function is BMQ_HD: bmq_rplan_kernels.h wraps them in gfx950 kernels on the engine stream (one lane per op), bmq_exec_host.h runs
// the very same code on host threads for host-only engines, the emulator harness (tools/emu/rplan_emu.cpp) and the sanitizer checker
// (tools/retain_plan_check.cpp) -- there is no second implementation.  Nothing here writes the index: the lookups are base_find / ov_find /
// id_dead of bmq_retain_core.h with plain loads, no node, token or id is created, last_op, the counters and the epoch stay as they are.
//
// Passes, each one lane per op:
//   find      found[i] = the live id of (tenant, topic) in the serving generation, NONE if the topic is not retained now.  The bulk-loaded
//             index first (its answer counts only if the id is not dead), then the overlay trie (a node's topic_id, not dead).
//   group     an open-addressing table (rep + 1 per slot, a power of two >= 2 n slots, zeroed before) keyed by the op's tenant BYTES and
//             topic BYTES.  The lane that claims an empty slot by CAS is the group's representative; a lane that meets an occupied slot
//             compares its bytes with the representative's INPUT bytes (immutable: nothing is published between lanes), on a match notes
//             rep_of[i] and bids for the group with atom_max(last[rep], i), otherwise goes on to the next slot.  No lane ever waits for
//             another one: a lost CAS returns the occupant and the lane goes on with it.
//   classify  code / winner / action / key length per op, and what the op adds to its tenant's delta (the caller sums: per wave on the device)
//   key write (behind the 64-bit scan of the key lengths) the winners' keys from the batch's own strings: retain_key_head / retain_key_tail
#pragma once
#include <stdint.h>

#include "bmq_retain_core.h"

namespace bmq {

enum : uint32_t { RP_NONE = 0, RP_ADD = 1, RP_UPDATE = 2, RP_REMOVE = 3, RP_SUPERSEDED = 4 }; // BMQ_PLAN_* of include/bmq.h
enum : uint32_t { RP_RETAINED = 0, RP_CLEARED = 1 };                                           // RetainResult.Code (RetainStoreCoProc.proto:50-53)
enum : uint32_t { RPERR_TENANT = 1u, RPERR_TABLE = 2u };
enum : uint32_t { RP_C_ERR = 0, RP_C_ACTION = 1, RP_C_N = 8 }; // ctr[RP_C_ACTION + action] = winners with that action (NONE .. REMOVE)

struct RplanBatch {
    // the ops (exec memory)
    const uint8_t* tenants;     // packed tenant ids (readable 16 bytes past the end)
    const uint32_t* tenant_off; // [n_tenants + 1]
    uint32_t n_tenants;
    const uint32_t* op_tenant;  // [n] index into the tenant table; null: every op belongs to tenant 0
    const uint8_t* topics;      // packed topics (readable 16 bytes past the end)
    const uint32_t* topic_off;  // [n + 1]
    const uint8_t* clear;       // [n] != 0: the message's payload is empty
    uint32_t n;
    // scratch
    uint32_t* table;            // [table_mask + 1] rep + 1, zeroed before
    uint32_t table_mask;
    uint32_t* rep_of;           // [n] the representative of the op's group (NONE: a refused op)
    uint32_t* last;             // [n] last[rep] = the last op of rep's group, zeroed before
    // results
    uint32_t* found;            // [n] out of find: the topic's live id or NONE (what out_topic_id reports)
    uint8_t* code;              // [n]
    uint8_t* action;            // [n]
    uint32_t* winner;           // [n]
    int32_t* delta;             // [n_tenants] zeroed before
    unsigned long long* key_len; // [n + 1] with a closing 0 for the scan
    uint32_t* ctr;              // [RP_C_N] zeroed before
};

BMQ_HD uint32_t rp_tenant(const RplanBatch& b, uint32_t i) { return b.op_tenant ? b.op_tenant[i] : 0u; }

// ---- find: is (tenant, topic) retained now?  Read-only on the index. ----
BMQ_HD void rp_find_one(const RetainMut& m, const RplanBatch& b, uint32_t i, bool have_index) {
    b.found[i] = NONE;
    const uint32_t ti = rp_tenant(b, i);
    if (ti >= b.n_tenants) { // (the entry point refuses such a batch before anything is launched)
        atom_or(&b.ctr[RP_C_ERR], (uint32_t)RPERR_TENANT);
        return;
    }
    if (!have_index) return;
    const unsigned long long tb = b.tenant_off[ti], te = b.tenant_off[ti + 1], pb = b.topic_off[i], pe = b.topic_off[i + 1];
    const uint32_t id = base_find(m.base, m.base_n, b.tenants, tb, te, b.topics, pb, pe);
    if (id != NONE && !id_dead(m.dead_bits, id)) {
        b.found[i] = id;
        return;
    }
    LevelScan lv;
    unsigned long long pos = tb;
    lv.start = pos;
    scan_level_bytes<0u>(b.tenants, pos, te, lv.h, lv.inl, lv.len);
    uint32_t node = ov_find(m.onodes, m.oedges, m.oedge_mask, m.opool, 0u, lv.h.h1, lv.h.h2, lv.len, b.tenants, tb);
    pos = pb;
    while (node != NONE) {
        next_level(b.topics, pos, pe, lv);
        node = ov_find(m.onodes, m.oedges, m.oedge_mask, m.opool, node, lv.h.h1, lv.h.h2, lv.len, b.topics, lv.start);
        if (!lv.more) break;
    }
    if (node == NONE) return;
    const uint32_t tid = m.onodes[node].topic_id; // NONE: the node is only a level on the way to other topics
    if (tid != NONE && tid < m.id_cap && !id_dead(m.dead_bits, tid)) b.found[i] = tid;
}

// ---- group: equal tenant bytes and equal topic bytes ----
BMQ_HD uint32_t rp_hash(const RplanBatch& b, uint32_t i) {
    const uint32_t ti = rp_tenant(b, i);
    uint32_t h = FNV1A_INIT;
    for (unsigned long long p = b.tenant_off[ti]; p < b.tenant_off[ti + 1]; p++) h = fnv1a_step(h, b.tenants[p]);
    h = fnv1a_step(h, 0x100u); // (no byte has this value: "ab" + "c" and "a" + "bc" part here)
    for (unsigned long long p = b.topic_off[i]; p < b.topic_off[i + 1]; p++) h = fnv1a_step(h, b.topics[p]);
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    h ^= h >> 13;
    return h;
}
BMQ_HD bool rp_same(const RplanBatch& b, uint32_t i, uint32_t j) {
    const uint32_t ti = rp_tenant(b, i), tj = rp_tenant(b, j);
    const unsigned long long tl = b.tenant_off[ti + 1] - b.tenant_off[ti], pl = b.topic_off[i + 1] - b.topic_off[i];
    if (ti != tj && (b.tenant_off[tj + 1] - b.tenant_off[tj] != tl || !bytes_equal(b.tenants, b.tenant_off[ti], b.tenants, b.tenant_off[tj], tl))) return false;
    return b.topic_off[j + 1] - b.topic_off[j] == pl && bytes_equal(b.topics, b.topic_off[i], b.topics, b.topic_off[j], pl);
}
// mask: the table's (a parameter, so that a harness can run the table nearly full)
BMQ_HD void rp_group_one(const RplanBatch& b, uint32_t i, uint32_t mask) {
    b.rep_of[i] = NONE;
    if (rp_tenant(b, i) >= b.n_tenants) return;
    uint32_t s = rp_hash(b, i) & mask;
    for (uint32_t probes = 0; probes <= mask; probes++) {
        uint32_t e = atom_load(&b.table[s]);
        if (e == 0) {
            e = atom_cas(&b.table[s], 0u, i + 1u); // the value found: 0 = the slot is this lane's, else whoever claimed it in between
            if (e == 0) e = i + 1u;
        }
        const uint32_t rep = e - 1u;
        if (rep == i || rp_same(b, i, rep)) {
            b.rep_of[i] = rep;
            atom_max(&b.last[rep], i); // the LAST op of a group decides
            return;
        }
        s = (s + 1) & mask;
    }
    atom_or(&b.ctr[RP_C_ERR], (uint32_t)RPERR_TABLE);
}

// ---- classify: returns the action of a winner (RP_NONE .. RP_REMOVE), RP_SUPERSEDED for every other op.  dv = what the op adds to
// delta[dt] (+1 an ADD, -1 a REMOVE, else 0): the CALLER adds it -- a wave sums its lanes per table entry first, because a batch of one tenant
// would otherwise send every winner's atomic to the same word (a single hot word serialises in the L2 atomic unit: bmq_build_core.h) ----
BMQ_HD uint32_t rp_classify_one(const RplanBatch& b, uint32_t i, uint32_t& dt, int32_t& dv) {
    dt = 0, dv = 0;
    b.key_len[i] = 0ull;
    const uint32_t rep = b.rep_of[i];
    if (rep == NONE) { // a refused op: the call fails, nothing of this is handed out
        b.code[i] = 0, b.action[i] = (uint8_t)RP_SUPERSEDED, b.winner[i] = NONE;
        return RP_SUPERSEDED;
    }
    const uint32_t w = b.last[rep];
    const bool clear = b.clear[w] != 0, present = b.found[i] != NONE;
    b.code[i] = (uint8_t)(clear ? RP_CLEARED : RP_RETAINED);
    b.winner[i] = w;
    uint32_t action = RP_SUPERSEDED;
    if (i == w) {
        action = clear ? (present ? RP_REMOVE : RP_NONE) : (present ? RP_UPDATE : RP_ADD);
        if (action != RP_NONE) {
            const uint32_t ti = rp_tenant(b, i);
            const unsigned long long pb = b.topic_off[i], pe = b.topic_off[i + 1];
            uint32_t levels = 1;
            for (unsigned long long p = pb; p < pe; p++) levels += b.topics[p] == '/';
            b.key_len[i] = retain_key_len(b.tenant_off[ti + 1] - b.tenant_off[ti], (uint32_t)(pe - pb), levels);
            dt = ti;
            if (action == RP_ADD) dv = 1;
            if (action == RP_REMOVE) dv = -1;
        }
    }
    b.action[i] = (uint8_t)action;
    return action;
}

// ---- the key of a winner into out + offs[i]: offs = the exclusive scan of key_len (nothing is written for an empty key) ----
BMQ_HD void rp_key_write_one(const RplanBatch& b, uint32_t i, const unsigned long long* offs, uint8_t* out) {
    const unsigned long long len = offs[i + 1] - offs[i];
    if (len == 0) return;
    const uint32_t ti = rp_tenant(b, i);
    const uint32_t tl = b.tenant_off[ti + 1] - b.tenant_off[ti], pl = b.topic_off[i + 1] - b.topic_off[i];
    const uint32_t levels = (uint32_t)(len - 5u - tl - pl);
    uint8_t* k = out + offs[i];
    const uint32_t at = retain_key_head(k, b.tenants + b.tenant_off[ti], tl);
    retain_key_tail(k + at, b.topics + b.topic_off[i], pl, levels);
}

} // namespace bmq
