// bmq_retain_core.h -- MUTATION of the retained-topic index where it lives (HBM), with STABLE topic ids: the per-item functions
// behind bmq_retain_apply* / bmq_retain_expired / bmq_retain_topic*.  Every function is BMQ_HD: bmq_exec_dev.h wraps them in gfx950
// kernels on the engine stream (one lane per op / per id), bmq_exec_host.h runs the very same code on host threads for host-only
// engines and the sanitizer fuzzers (tools/retain_fuzz.cpp) -- there is no second implementation.
//
// What it replaces: TopicLevelTrie.add / remove (UTIL/index/TopicLevelTrie.java:49-182: lock-free CAS on INode.main, CNode copies,
// tomb contraction) as RetainTopicIndex drives it (RS/index/RetainTopicIndex.java:126-134) from the post-commit closure of
// RetainStoreCoProc.batchRetain / gc (RS/RetainStoreCoProc.java:240-255,270-275).
//
// Design.  The bulk-loaded index (bmq_retain.h: topic id = rank, every subtree ONE id range, the children of a node range ONE
// node range) stays immutable between rebuilds -- that layout is what makes '+' and '#' O(1) per node range -- and is overlaid by
//   * a DEAD bitmap over the ids (+ a rank directory: dead ids in front of every 64-id word), so that a removed topic keeps its
//     id, matched id ranges give exact live counts in O(1) and the expansion just skips dead ids.  A re-added topic gets its id
//     back (the bit is cleared);
//   * an OVERLAY trie for topics the bulk load did not hold: nodes keyed (parent node, 64-bit level hash) in one open-addressing
//     table, labels verified byte for byte in a string pool, child lists for '+' / '#'; a new topic gets the next unused id.
//     One trie for all tenants, the tenant id is level 0 (as in the reference: RetainTopicIndex keys [tenantId, levels...]).
// An id therefore never changes and is never reused until the next bmq_retain_rebuild* / bmq_retain_compact (a new generation),
// which merges the overlay into a fresh bulk-loaded index.
//
// One batch of ops = three kernels in stream order with the match batches (which therefore never see half a batch):
//   locate   one lane per op (the adds, then the removes): find the topic in the bulk-loaded index (dictionary + edge hash:
//            O(levels) line fetches), else find -- for an add: find or create, lock-free CAS claims -- its overlay node; remember
//            the target and bid for it (64-bit atomic max of the op's position: the LAST op on a topic decides, so ops apply "in order")
//   commit   one lane per op: the winning op of every target sets / clears the dead bit, stores timestamp / expiry / expireAt,
//            hands out the id of a brand-new topic
//   rank     dead ids in front of every 64-id word (exclusive prefix popcount)
#pragma once
#include <stdint.h>

#include "bmq_build_core.h"
#include "bmq_key_core.h"
#include "bmq_retain.h"

namespace bmq {

#if defined(__HIP_DEVICE_COMPILE__)
template <class T> BMQ_HD T atom_max(T* p, T v) { return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> BMQ_HD T atom_and(T* p, T v) { return __hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> BMQ_HD T atom_xchg(T* p, T v) { return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
BMQ_HD void atom_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } // this lane's stores have left for memory
#else
template <class T> BMQ_HD T atom_max(T* p, T v) {
    T cur = __atomic_load_n(p, __ATOMIC_ACQUIRE);
    while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
    }
    return cur;
}
template <class T> BMQ_HD T atom_and(T* p, T v) { return __atomic_fetch_and(p, v, __ATOMIC_ACQ_REL); }
template <class T> BMQ_HD T atom_xchg(T* p, T v) { return __atomic_exchange_n(p, v, __ATOMIC_ACQ_REL); }
BMQ_HD void atom_drain() {}
#endif

constexpr uint32_t RT_OVERLAY = 0x80000000u; // op target: an overlay node (low bits) instead of a bulk-loaded id
constexpr uint32_t ID_SYS = 0x80000000u;     // id_tnode flag: the topic's first level starts with '$'
enum : uint32_t { RERR_NODES = 1u, RERR_POOL = 2u, RERR_IDS = 4u, RERR_STUCK = 8u, RERR_BAD_OP = 16u };

struct RetainCounters { // device memory; the host reads it back after every batch
    uint32_t ov_nodes;   // overlay nodes handed out (node 0 = the root)
    uint32_t opool_used; // bytes of the overlay string pool handed out
    uint32_t next_id;    // ids handed out (bulk-loaded + overlay, live or not)
    uint32_t err;
    // per batch, N_CTR_LANES copies each (a single hot word serialises in the L2 atomic unit: bmq_build_core.h)
    uint32_t went_live[N_CTR_LANES], went_dead[N_CTR_LANES];           // topics that became retained / stopped being retained
    uint32_t base_went_live[N_CTR_LANES], base_went_dead[N_CTR_LANES]; // ... among the bulk-loaded ids (the dead-aware paths switch on them)
};

// Everything the mutation kernels touch (device pointers; host pointers under HostExec).
struct RetainMut {
    RetainIndexView base; // the bulk-loaded index (not written here)
    uint32_t base_n;
    ONode* onodes;
    uint32_t ov_cap;
    uint32_t* oedges;
    uint32_t oedge_mask;
    uint8_t* opool;
    uint32_t opool_cap;
    // per id
    unsigned long long* expire_at; // ms; 0 while the id is dead (so that "expire_at > now" alone rejects removed topics)
    unsigned long long* ts;        // Message.timestamp (HLC) given to IRetainTopicIndex.add
    uint32_t* expiry;              // Message.expiryInterval; 0xFFFFFFFF with ts 0: never expires
    uint32_t* id_node;             // overlay node of an overlay id (NONE for bulk-loaded ids)
    uint32_t* id_tnode;            // overlay node of its tenant | ID_SYS (NONE for bulk-loaded ids)
    uint32_t id_cap;
    unsigned long long* dead_bits;
    uint32_t* dead_rank;
    unsigned long long* last_op;   // [id_cap + ov_cap] bids of the running batch: (batch sequence << 32) | (op position + 1)
    RetainCounters* ctr;
};

struct RetainOps {
    const uint8_t* tenants;       // packed tenant ids
    const uint32_t* tenant_off;   // [n_tenants + 1]
    uint32_t n_tenants;
    const uint32_t* op_tenant;    // [n] index into the tenant table; null: every op belongs to tenant 0
    const uint8_t* topics;        // packed topics (readable 16 bytes past the end)
    const uint32_t* topic_off;    // [n + 1]
    const uint8_t* op;            // [n] 0 = add, 1 = remove
    const unsigned long long* ts; // [n] or null
    const uint32_t* expiry;       // [n] or null (together with ts)
    uint32_t n;
    unsigned long long seq;       // batch sequence number (> 0, ascending)
    uint32_t* target;             // [n] out of locate: id, RT_OVERLAY | node, or NONE
    uint32_t* out_ids;            // [n] out of commit: the topic's id, or NONE (absent topic removed / op superseded by a later one)
};

// ------------------------------------------------------------------------------------------------------------
// the bulk-loaded index, read with plain loads (it is immutable between rebuilds)
// ------------------------------------------------------------------------------------------------------------
BMQ_HD uint32_t rdict_find(const RetainIndexView& ix, const LevelHash& h, uint32_t len, const uint32_t inl[4], const uint8_t* bytes,
                           unsigned long long start) {
    const uint32_t tag = level_hash_tag(h);
    uint32_t g = level_hash_slot(h, len) & ix.dict_group_mask;
    for (uint32_t probes = 0; probes <= ix.dict_group_mask; probes++) {
        bool free_slot = false;
        for (uint32_t j = 0; j < DICT_GROUP; j++) {
            const DictSlot& s = ix.dict[DICT_GROUP * (size_t)g + j];
            if (s.tag == 0) {
                free_slot = true;
                continue;
            }
            if (s.tag != tag || s.len != len || s.inl[0] != inl[0] || s.inl[1] != inl[1] || s.inl[2] != inl[2] || s.inl[3] != inl[3]) continue;
            bool eq = true;
            for (uint32_t i = 16; i < len && eq; i++) eq = ix.pool[s.pool_off + i] == bytes[start + i];
            if (eq) return s.token;
        }
        if (free_slot) return TOK_UNKNOWN;
        g = (g + 1) & ix.dict_group_mask;
    }
    return TOK_UNKNOWN;
}
BMQ_HD uint32_t redge_find(const RetainIndexView& ix, uint32_t edge_base, uint32_t mask, uint32_t parent, uint32_t token) {
    uint32_t bk = redge_bucket(parent, token, mask);
    for (uint32_t probes = 0; probes <= mask; probes++) {
        bool free_slot = false;
        for (uint32_t j = 0; j < 4; j++) {
            const REdge& e = ix.edges[edge_base + 4 * (size_t)bk + j];
            if (e.parent == parent && e.token == token) return e.child & ~RE_OVERFLOW;
            free_slot = free_slot || e.parent == NONE;
        }
        if (free_slot) return NONE;
        bk = (bk + 1) & mask;
    }
    return NONE;
}
BMQ_HD const RTenantSlot* rtenant_find(const RetainIndexView& ix, uint32_t token) {
    uint32_t d = tenant_hash(token) & ix.tenant_mask;
    for (uint32_t probes = 0; probes <= ix.tenant_mask; probes++) {
        const RTenantSlot& t = ix.tenants[d];
        if (t.token == token) return &t;
        if (t.token == 0) return nullptr;
        d = (d + 1) & ix.tenant_mask;
    }
    return nullptr;
}
// The next level of a '/'-separated topic: [pos, level end); pos moves behind the separator.  `more` = another level follows
// (TopicUtil.parse keeps empty levels, UTIL/TopicUtil.java:206-225: "a/" has two).
struct LevelScan {
    LevelHash h;
    uint32_t inl[4];
    uint32_t len;
    unsigned long long start;
    bool more;
};
BMQ_HD void next_level(const uint8_t* bytes, unsigned long long& pos, unsigned long long end, LevelScan& lv) {
    lv.start = pos;
    scan_level_bytes<0x2F2F2F2Fu>(bytes, pos, end, lv.h, lv.inl, lv.len);
    lv.more = pos < end;
    if (lv.more) pos++; // the '/'
}
// id of (tenant, topic) in the bulk-loaded index, or NONE
BMQ_HD uint32_t base_find(const RetainIndexView& ix, uint32_t base_n, const uint8_t* tenants, unsigned long long tb, unsigned long long te,
                          const uint8_t* topics, unsigned long long pb, unsigned long long pe) {
    if (base_n == 0) return NONE;
    LevelScan lv;
    unsigned long long pos = tb;
    lv.start = pos;
    scan_level_bytes<0u>(tenants, pos, te, lv.h, lv.inl, lv.len); // the whole id is ONE level (SEP4 = NUL bytes: an id holds none)
    if (pos != te) return NONE;
    const uint32_t ttok = rdict_find(ix, lv.h, lv.len, lv.inl, tenants, tb);
    if (ttok == TOK_UNKNOWN) return NONE;
    const RTenantSlot* ten = rtenant_find(ix, ttok);
    if (!ten) return NONE;
    uint32_t node = 0;
    pos = pb;
    for (;;) {
        next_level(topics, pos, pe, lv);
        const uint32_t tok = rdict_find(ix, lv.h, lv.len, lv.inl, topics, lv.start);
        if (tok == TOK_UNKNOWN) return NONE;
        node = redge_find(ix, ten->edge_base, ten->edge_bucket_mask, node, tok);
        if (node == NONE) return NONE;
        if (!lv.more) break;
    }
    const RNode& n = ix.nodes[ten->node_base + node];
    return (n.child_count & RN_TERM) ? ten->id_base + n.sub_begin : NONE;
}

// ------------------------------------------------------------------------------------------------------------
// the overlay trie
// ------------------------------------------------------------------------------------------------------------
BMQ_HD uint32_t ov_slot(uint32_t parent, uint32_t h1, uint32_t h2, uint32_t mask) {
    uint32_t x = (parent * 0x9E3779B1u) ^ h1 ^ rotl32(h2, 13);
    x ^= x >> 15;
    x *= 0x85EBCA77u;
    x ^= x >> 13;
    return x & mask;
}
// child of `parent` labelled bytes[start, start + len), or NONE.  Read side of the MATCH kernels and of lookups between batches:
// plain loads (nothing writes while they run).
BMQ_HD uint32_t ov_find(const ONode* onodes, const uint32_t* oedges, uint32_t mask, const uint8_t* opool, uint32_t parent, uint32_t h1, uint32_t h2,
                        uint32_t len, const uint8_t* bytes, unsigned long long start) {
    uint32_t s = ov_slot(parent, h1, h2, mask);
    for (uint32_t probes = 0; probes <= mask; probes++) {
        const uint32_t e = oedges[s];
        if (e == 0) return NONE;
        const ONode& n = onodes[e];
        if (n.parent == parent && n.h1 == h1 && n.h2 == h2 && (n.str_len & ~ON_SYS) == len && bytes_equal(opool, n.str_off, bytes, start, len)) return e;
        s = (s + 1) & mask;
    }
    return NONE;
}
// The same from INSIDE a mutation batch: other lanes insert concurrently, so table entries are claimed by CAS and a node is
// complete in memory (shared_store + drain) before its index is published; insert = false only looks.
BMQ_HD uint32_t ov_child(const RetainMut& m, uint32_t parent, const LevelScan& lv, const uint8_t* bytes, bool insert) {
    uint32_t s = ov_slot(parent, lv.h.h1, lv.h.h2, m.oedge_mask), mine = NONE;
    for (uint32_t probes = 0; probes <= m.oedge_mask; probes++) {
        uint32_t e = atom_load(&m.oedges[s]);
        if (e == 0) {
            if (!insert) return NONE;
            if (mine == NONE) { // build the node first, publish it with the CAS
                mine = atom_add(&m.ctr->ov_nodes, 1u);
                if (mine >= m.ov_cap) {
                    atom_or(&m.ctr->err, (uint32_t)RERR_NODES);
                    return NONE;
                }
                uint32_t off = 0;
                if (lv.len) {
                    off = atom_add(&m.ctr->opool_used, lv.len);
                    if ((unsigned long long)off + lv.len > m.opool_cap) {
                        atom_or(&m.ctr->err, (uint32_t)RERR_POOL);
                        return NONE;
                    }
                    for (uint32_t i = 0; i < lv.len; i++) shared_store(m.opool + off + i, bytes[lv.start + i]);
                }
                ONode* n = m.onodes + mine;
                shared_store(&n->parent, parent);
                shared_store(&n->h1, lv.h.h1);
                shared_store(&n->h2, lv.h.h2);
                shared_store(&n->str_off, off);
                shared_store(&n->str_len, lv.len | ((lv.len && bytes[lv.start] == '$') ? ON_SYS : 0u));
                shared_store(&n->first_child, NONE);
                shared_store(&n->next_sibling, NONE);
                shared_store(&n->topic_id, NONE);
                atom_drain();
            }
            e = atom_cas(&m.oedges[s], 0u, mine);
            if (e == 0) { // ours: hang it into the parent's child list (read by later kernels only)
                const uint32_t old = atom_xchg(&m.onodes[parent].first_child, mine);
                shared_store(&m.onodes[mine].next_sibling, old);
                return mine;
            }
            // somebody claimed the slot in between: e is their node -- maybe the very label we are after
        }
        const ONode* n = m.onodes + e;
        const uint32_t sl = shared_load(&n->str_len) & ~ON_SYS;
        if (shared_load(&n->parent) == parent && shared_load(&n->h1) == lv.h.h1 && shared_load(&n->h2) == lv.h.h2 && sl == lv.len) {
            const uint32_t so = shared_load(&n->str_off);
            bool eq = true;
            for (uint32_t i = 0; i < sl && eq; i++) eq = shared_load(m.opool + so + i) == bytes[lv.start + i];
            if (eq) return e; // (a node built for nothing stays behind as garbage until the next rebuild: rare)
        }
        s = (s + 1) & m.oedge_mask;
    }
    atom_or(&m.ctr->err, (uint32_t)RERR_STUCK);
    return NONE;
}
BMQ_HD bool id_dead(const unsigned long long* dead_bits, uint32_t id) { return (dead_bits[id >> 6] >> (id & 63u)) & 1ull; }
// dead ids in [0, x)
BMQ_HD uint32_t dead_before(const unsigned long long* dead_bits, const uint32_t* dead_rank, uint32_t x) {
    const uint32_t w = x >> 6, b = x & 63u;
    return dead_rank[w] + (b ? (uint32_t)__builtin_popcountll(dead_bits[w] & ((1ull << b) - 1ull)) : 0u);
}

// ------------------------------------------------------------------------------------------------------------
// one batch: locate, commit
// ------------------------------------------------------------------------------------------------------------
// Two launches per batch: phase 0 places the adds (creating overlay nodes), phase 1 the removes -- a remove must find the node an
// add of the SAME batch created for its topic, whatever the lanes' timing.
BMQ_HD void rlocate_one(const RetainMut& m, const RetainOps& ob, uint32_t i, uint32_t phase) {
    if (ob.op[i] > 1) {
        if (phase == 0) {
            ob.target[i] = NONE;
            atom_or(&m.ctr->err, (uint32_t)RERR_BAD_OP);
        }
        return;
    }
    if (ob.op[i] != phase) return;
    ob.target[i] = NONE;
    const bool add = ob.op[i] == 0;
    const uint32_t ti = ob.op_tenant ? ob.op_tenant[i] : 0u;
    if (ti >= ob.n_tenants) {
        atom_or(&m.ctr->err, (uint32_t)RERR_BAD_OP);
        return;
    }
    const unsigned long long tb = ob.tenant_off[ti], te = ob.tenant_off[ti + 1], pb = ob.topic_off[i], pe = ob.topic_off[i + 1];
    uint32_t target = base_find(m.base, m.base_n, ob.tenants, tb, te, ob.topics, pb, pe);
    if (target == NONE) { // not a bulk-loaded topic: the overlay holds it, or will
        LevelScan lv;
        unsigned long long pos = tb;
        lv.start = pos;
        scan_level_bytes<0u>(ob.tenants, pos, te, lv.h, lv.inl, lv.len);
        lv.more = false;
        uint32_t node = ov_child(m, 0u, lv, ob.tenants, add);
        pos = pb;
        while (node != NONE) {
            next_level(ob.topics, pos, pe, lv);
            node = ov_child(m, node, lv, ob.topics, add);
            if (!lv.more) break;
        }
        if (node != NONE) target = RT_OVERLAY | node;
    }
    ob.target[i] = target;
    if (target != NONE) {
        const size_t slot = (target & RT_OVERLAY) ? (size_t)m.id_cap + (target & ~RT_OVERLAY) : (size_t)target;
        atom_max(&m.last_op[slot], (ob.seq << 32) | (unsigned long long)(i + 1u));
    }
}

BMQ_HD void rcommit_one(const RetainMut& m, const RetainOps& ob, uint32_t i) {
    ob.out_ids[i] = NONE;
    const uint32_t target = ob.target[i];
    if (target == NONE) return; // removal of a topic nobody retains (or a refused op)
    const bool ov = (target & RT_OVERLAY) != 0;
    const uint32_t node = target & ~RT_OVERLAY;
    const size_t slot = ov ? (size_t)m.id_cap + node : (size_t)target;
    if (m.last_op[slot] != ((ob.seq << 32) | (unsigned long long)(i + 1u))) return; // a later op of this batch decides for the topic
    const bool add = ob.op[i] == 0;
    uint32_t id = target;
    if (ov) {
        id = m.onodes[node].topic_id;
        if (id == NONE) {
            if (!add) return; // the node is only a level on the way to other topics
            id = atom_add(&m.ctr->next_id, 1u);
            if (id >= m.id_cap) {
                atom_or(&m.ctr->err, (uint32_t)RERR_IDS);
                return;
            }
            m.onodes[node].topic_id = id;
            m.id_node[id] = node;
            uint32_t t = node, first = node; // the tenant's node and the topic's first level
            while (m.onodes[t].parent != 0u) {
                first = t;
                t = m.onodes[t].parent;
            }
            m.id_tnode[id] = t | ((m.onodes[first].str_len & ON_SYS) && first != t ? ID_SYS : 0u);
        }
    }
    const unsigned long long bit = 1ull << (id & 63u);
    const bool was_dead = (atom_load(&m.dead_bits[id >> 6]) & bit) != 0; // only this lane touches this id's BIT (others: the same word)
    const uint32_t c = i & (N_CTR_LANES - 1);
    if (add) {
        if (was_dead) {
            atom_and(&m.dead_bits[id >> 6], ~bit);
            atom_add(&m.ctr->went_live[c], 1u);
            if (!ov) atom_add(&m.ctr->base_went_live[c], 1u);
        }
        const bool has = ob.ts != nullptr;
        const unsigned long long ts = has ? ob.ts[i] : 0ull;
        const uint32_t ex = has ? ob.expiry[i] : 0xFFFFFFFFu;
        m.ts[id] = ts;
        m.expiry[id] = ex;
        m.expire_at[id] = (ts == 0 && ex == 0xFFFFFFFFu) ? RETAIN_NEVER : retain_expire_at(ts, ex);
    } else if (!was_dead) {
        atom_or(&m.dead_bits[id >> 6], bit);
        atom_add(&m.ctr->went_dead[c], 1u);
        if (!ov) atom_add(&m.ctr->base_went_dead[c], 1u);
        m.expire_at[id] = 0ull;
    }
    ob.out_ids[i] = id;
}

// Removal BY ID: the post-commit half of RetainStoreCoProc.gc (RS/RetainStoreCoProc.java:270-275), for ids the engine itself handed out
// (bmq_retain_expired / bmq_retain_live_ids / a match) -- the id names its slot, nothing is looked up.  A live id goes dead exactly as a
// remove op leaves it in rcommit_one.  64 ids of one word may arrive in 64 lanes and an id may be listed twice: the lane whose OR flipped
// the bit is the one that counts.  ids[i] < n_ids (the host checked every id before anything was launched).
BMQ_HD void remove_id_one(const RetainMut& m, const uint32_t* ids, uint32_t i, uint32_t n_ids) {
    const uint32_t id = ids[i];
    if (id >= n_ids || id >= m.id_cap) return;
    const unsigned long long bit = 1ull << (id & 63u);
    if (atom_or(&m.dead_bits[id >> 6], bit) & bit) return; // dead already, or listed twice: another lane took it
    m.expire_at[id] = 0ull;
    const uint32_t c = i & (N_CTR_LANES - 1);
    atom_add(&m.ctr->went_dead[c], 1u);
    if (id < m.base_n) atom_add(&m.ctr->base_went_dead[c], 1u);
}

// ------------------------------------------------------------------------------------------------------------
// retained topics per tenant (RetainStoreCoProc.load(), RS/RetainStoreCoProc.java:279-296: tenantsStats.increaseTopicCount per key)
// ------------------------------------------------------------------------------------------------------------
// a bulk-loaded tenant owns the rank range [lo, hi): its live topics are the range minus the dead ids inside -- no pass over the ids
BMQ_HD void census_bulk_one(const RetainMut& m, const uint32_t* ranges, uint32_t t, uint32_t* out) {
    const uint32_t lo = ranges[2 * t], hi = ranges[2 * t + 1];
    out[t] = (hi - lo) - (dead_before(m.dead_bits, m.dead_rank, hi) - dead_before(m.dead_bits, m.dead_rank, lo));
}
// an id handed out since the bulk load: the overlay node of its tenant if the topic is retained now, NONE otherwise ('$' topics count)
BMQ_HD uint32_t census_topic_one(const RetainMut& m, uint32_t id) {
    if (id >= m.id_cap || id_dead(m.dead_bits, id)) return NONE;
    const uint32_t tn = m.id_tnode[id];
    return tn == NONE ? NONE : (tn & ~ID_SYS);
}
// the census table holds a word per overlay node and only the tenant nodes can have a count: the non-zero entries go into a list
// ((node << 32) | count, any order) on the executor's side, so that the host reads the list and never the table
BMQ_HD void census_pick_one(const unsigned long long* table, uint32_t i, unsigned long long* list, uint32_t* count) {
    const unsigned long long c = table[i];
    if (c) list[atom_add(count, 1u)] = ((unsigned long long)i << 32) | c;
}
// labels of overlay nodes (the tenant ids of tenant nodes): lengths, then bytes at offs[i]
BMQ_HD void ov_node_len_one(const RetainMut& m, const uint32_t* nodes, uint32_t i, uint32_t* lens) { lens[i] = m.onodes[nodes[i]].str_len & ~ON_SYS; }
BMQ_HD void ov_node_write_one(const RetainMut& m, const uint32_t* nodes, uint32_t i, const unsigned long long* offs, uint8_t* out) {
    const ONode& n = m.onodes[nodes[i]];
    const uint32_t l = n.str_len & ~ON_SYS;
    for (uint32_t k = 0; k < l; k++) out[offs[i] + k] = m.opool[n.str_off + k];
}

// re-insert overlay node i into a larger edge table (all nodes in parallel, after the table was cleared)
BMQ_HD void ov_rehash_one(const RetainMut& m, uint32_t i) {
    if (i == 0) return;
    const ONode& n = m.onodes[i];
    // A node that lost the race for its table slot (ov_child: "built for nothing") was never published: it hangs in no child list, no
    // topic ends at it and nothing hangs below it.  It must not enter the new table -- it carries the same (parent, label) as the node
    // that won, and a lookup that meets it first finds neither the topic nor the children.  (A batch of 50 k adds below one first level
    // leaves thousands of them on the device; a published node always has a topic or a child.)
    if (n.first_child == NONE && n.topic_id == NONE) return;
    uint32_t s = ov_slot(n.parent, n.h1, n.h2, m.oedge_mask);
    for (uint32_t probes = 0; probes <= m.oedge_mask; probes++) {
        if (atom_cas(&m.oedges[s], 0u, i) == 0u) return;
        s = (s + 1) & m.oedge_mask;
    }
    atom_or(&m.ctr->err, (uint32_t)RERR_STUCK);
}

// ------------------------------------------------------------------------------------------------------------
// id -> retained topic, GC scan
// ------------------------------------------------------------------------------------------------------------
// overlay id -> bytes of tenant id + topic: lens[2 i] = tenant length, lens[2 i + 1] = total length (0 / 0: not an overlay topic)
BMQ_HD void ov_topic_len_one(const RetainMut& m, const uint32_t* ids, uint32_t i, uint32_t* lens) {
    const uint32_t id = ids[i];
    lens[2 * i] = lens[2 * i + 1] = 0;
    if (id < m.base_n || id >= m.id_cap || m.id_node[id] == NONE) return;
    uint32_t total = 0, levels = 0, t = m.id_node[id];
    while (m.onodes[t].parent != 0u) {
        total += m.onodes[t].str_len & ~ON_SYS;
        levels++;
        t = m.onodes[t].parent;
    }
    const uint32_t tl = m.onodes[t].str_len & ~ON_SYS;
    lens[2 * i] = tl;
    lens[2 * i + 1] = tl + total + (levels ? levels - 1 : 0);
}
BMQ_HD void ov_topic_write_one(const RetainMut& m, const uint32_t* ids, uint32_t i, const unsigned long long* offs, uint8_t* out) {
    const uint32_t id = ids[i];
    unsigned long long end = offs[i + 1];
    if (end == offs[i]) return;
    uint32_t t = m.id_node[id];
    for (;;) { // back to front: the last level first
        const ONode& n = m.onodes[t];
        const uint32_t l = n.str_len & ~ON_SYS;
        end -= l;
        for (uint32_t k = 0; k < l; k++) out[end + k] = m.opool[n.str_off + k];
        if (n.parent == 0u) break; // that was the tenant id
        if (m.onodes[n.parent].parent != 0u) out[--end] = '/';
        t = n.parent;
    }
}
// ------------------------------------------------------------------------------------------------------------
// id -> retainMessageKey (RetainStoreCoProc.match: reader.get(retainMessageKey(tenant, topic)) per hit, RS/RetainStoreCoProc.java:167-190;
// gc deletes the same keys, :258-277).  The encoder is bmq_key_core.h's.
// ------------------------------------------------------------------------------------------------------------
// The strings of the BULK-LOADED ids of one generation in exec memory (the index itself holds no parent pointers and no node -> label map:
// bmq_retain.h).  An id is a rank, so the topics lie back to back in id order and a tenant is a rank range.  Built on first use from the
// host's copy of the load, dropped with the generation (RetainDyn: bmq_retain_dyn.h).  Overlay ids need none: their ONode chain has parents.
struct RetainKeyStore {
    const uint8_t* topics;               // topic bytes of id 0, 1, ... back to back
    const unsigned long long* topic_off; // [n_ids + 1]
    const uint32_t* tenant_lo;           // [n_tenants + 1] first rank of every tenant that has topics, ascending; [n_tenants] = n_ids
    const uint8_t* tenants;              // their ids, back to back
    const uint32_t* tenant_off;          // [n_tenants + 1]
    uint32_t n_tenants;
    uint32_t n_ids;                      // == RetainMut.base_n of the generation it was built for (0: no store / nothing bulk-loaded)
};
// the tenant (index into tenant_lo) that owns rank id; id < ks.n_ids, so ks.n_tenants >= 1
BMQ_HD uint32_t key_store_tenant(const RetainKeyStore& ks, uint32_t id) {
    uint32_t lo = 0, hi = ks.n_tenants; // tenant_lo[lo] <= id < tenant_lo[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ks.tenant_lo[mid] <= id) lo = mid;
        else hi = mid;
    }
    return lo;
}
// is `id` a topic that is retained now, and whose strings this call can reach?  Decided from dead_bits where the index lives.
BMQ_HD bool key_id_live(const RetainMut& m, const RetainKeyStore& ks, uint32_t id) {
    if (id >= m.id_cap || id_dead(m.dead_bits, id)) return false; // out of range, never handed out (those bits are set), or removed
    if (id < m.base_n) return id < ks.n_ids;
    const uint32_t node = m.id_node[id];
    return node != NONE && node < m.ov_cap && node != 0u;
}
// length of the key of ids[i]; 0: the id is out of range, was never handed out, or its topic is not retained now
BMQ_HD unsigned long long key_len_one(const RetainMut& m, const RetainKeyStore& ks, uint32_t id) {
    if (!key_id_live(m, ks, id)) return 0ull;
    if (id < m.base_n) {
        const uint32_t t = key_store_tenant(ks, id);
        const unsigned long long pb = ks.topic_off[id], pe = ks.topic_off[id + 1];
        uint32_t levels = 1;
        for (unsigned long long p = pb; p < pe; p++) levels += ks.topics[p] == '/';
        return retain_key_len(ks.tenant_off[t + 1] - ks.tenant_off[t], (uint32_t)(pe - pb), levels);
    }
    uint32_t total = 0, levels = 0, t = m.id_node[id]; // as ov_topic_len_one: up the chain to the tenant's node
    while (m.onodes[t].parent != 0u) {
        total += m.onodes[t].str_len & ~ON_SYS;
        levels++;
        t = m.onodes[t].parent;
    }
    if (levels == 0) return 0ull; // (a tenant node carries no topic)
    return retain_key_len(m.onodes[t].str_len & ~ON_SYS, total + levels - 1, levels);
}
// the key of `id` into out[0, len): len = key_len_one(m, ks, id) of the same state (nothing is written for len 0)
BMQ_HD void key_write_one(const RetainMut& m, const RetainKeyStore& ks, uint32_t id, uint8_t* out, unsigned long long len) {
    if (len == 0 || !key_id_live(m, ks, id)) return;
    if (id < m.base_n) {
        const uint32_t t = key_store_tenant(ks, id);
        const uint32_t tl = ks.tenant_off[t + 1] - ks.tenant_off[t];
        const unsigned long long pb = ks.topic_off[id];
        const uint32_t pl = (uint32_t)(ks.topic_off[id + 1] - pb);
        const uint32_t levels = (uint32_t)(len - 5u - tl - pl);
        const uint32_t at = retain_key_head(out, ks.tenants + ks.tenant_off[t], tl);
        retain_key_tail(out + at, ks.topics + pb, pl, levels);
        return;
    }
    // an overlay topic: one label per node, the last level first (as ov_topic_write_one).  The hash bytes fill up from the back too.
    uint32_t levels = 0, t = m.id_node[id];
    while (m.onodes[t].parent != 0u) {
        levels++;
        t = m.onodes[t].parent;
    }
    const ONode& tn = m.onodes[t];
    const uint32_t tl = tn.str_len & ~ON_SYS;
    uint32_t at = retain_key_head(out, m.opool + tn.str_off, tl);
    out[at] = (uint8_t)((levels >> 8) & 0xFF);
    out[at + 1] = (uint8_t)(levels & 0xFF);
    uint8_t* hash = out + at + 2;
    unsigned long long end = len;
    uint32_t lv = levels;
    for (uint32_t n = m.id_node[id]; n != t; n = m.onodes[n].parent) {
        const ONode& o = m.onodes[n];
        const uint32_t l = o.str_len & ~ON_SYS;
        end -= l;
        for (uint32_t k = 0; k < l; k++) out[end + k] = m.opool[o.str_off + k];
        hash[--lv] = level_hash_byte(m.opool + o.str_off, l);
        if (o.parent != t) out[--end] = 0; // TopicUtil.escape of the '/' in front of this level
    }
}
// ------------------------------------------------------------------------------------------------------------
// KV boundary of the retain store's range (RetainStoreCoProc.reset(Boundary), RS/RetainStoreCoProc.java:133-137): is the key of id inside?
// ------------------------------------------------------------------------------------------------------------
// No id range is a key range (tenants are ranked in byte order, keys sort by tenant LENGTH first; inside a tenant by level count and hash
// bytes before the topic), so the answer is a predicate over ids.  The key is never written anywhere: its four segments are walked in
// order against the boundary key and the first difference decides -- almost always inside `00 | u16be(tl) | tenant`.
struct KeyCursor { // the byte string the key is compared with, and how far the compare has come
    const uint8_t* k;
    unsigned long long n, p;
};
// the key's next byte against the cursor's: < 0 / > 0 decides the compare (a cursor at its end: the key is the longer one), 0 = go on
BMQ_HD int key_cursor_step(KeyCursor& c, uint32_t b) {
    if (c.p >= c.n) return 1;
    const uint32_t y = c.k[c.p++];
    return b == y ? 0 : (b < y ? -1 : 1);
}
// `00 | u16be(tl) | tenant`
BMQ_HD int key_cursor_head(KeyCursor& c, const uint8_t* tenant, uint32_t tl) {
    int r;
    if ((r = key_cursor_step(c, 0u)) || (r = key_cursor_step(c, (tl >> 8) & 0xFFu)) || (r = key_cursor_step(c, tl & 0xFFu))) return r;
    for (uint32_t k = 0; k < tl; k++)
        if ((r = key_cursor_step(c, tenant[k]))) return r;
    return 0;
}
// overlay node of forward level j of a topic of `levels` levels that ends at node `last`: the chain has parents only
BMQ_HD uint32_t ov_level_node(const RetainMut& m, uint32_t last, uint32_t levels, uint32_t j) {
    uint32_t n = last;
    for (uint32_t up = levels - 1u - j; up != 0u; up--) n = m.onodes[n].parent;
    return n;
}
// retainMessageKey(id) against key[0, key_len) in unsigned byte order, a proper prefix first (the order of key_compare, bmq_build_core.h):
// < 0, 0, > 0.  id is a live id of this state (key_id_live); an id that is not compares as the empty key.
BMQ_HD int retain_key_cmp(const RetainMut& m, const RetainKeyStore& ks, uint32_t id, const uint8_t* key, unsigned long long key_len) {
    KeyCursor c{key, key_len, 0ull};
    int r = 0;
    if (!key_id_live(m, ks, id)) return key_len ? -1 : 0;
    if (id < m.base_n) { // a rank: tenant and topic lie in the key store, the topic in one piece
        const uint32_t t = key_store_tenant(ks, id);
        if ((r = key_cursor_head(c, ks.tenants + ks.tenant_off[t], ks.tenant_off[t + 1] - ks.tenant_off[t]))) return r;
        const uint8_t* p = ks.topics + ks.topic_off[id];
        const uint32_t pl = (uint32_t)(ks.topic_off[id + 1] - ks.topic_off[id]);
        uint32_t levels = 1;
        for (uint32_t i = 0; i < pl; i++) levels += p[i] == '/';
        if ((r = key_cursor_step(c, (levels >> 8) & 0xFFu)) || (r = key_cursor_step(c, levels & 0xFFu))) return r;
        for (uint32_t i = 0, b = 0; i <= pl; i++) { // a LevelHash byte per level
            if (i < pl && p[i] != '/') continue;
            if ((r = key_cursor_step(c, level_hash_byte(p + b, i - b)))) return r;
            b = i + 1;
        }
        for (uint32_t i = 0; i < pl; i++) // the topic, TopicUtil.escape
            if ((r = key_cursor_step(c, p[i] == '/' ? 0u : p[i]))) return r;
        return c.p < c.n ? -1 : 0;
    }
    // an overlay topic: the tenant's node is on record per id; the levels hang on a chain that is walked from the LAST level up
    const uint32_t last = m.id_node[id], t = m.id_tnode[id] & ~ID_SYS;
    if (t >= m.ov_cap) return key_len ? -1 : 0;
    const ONode& tn = m.onodes[t];
    if ((r = key_cursor_head(c, m.opool + tn.str_off, tn.str_len & ~ON_SYS))) return r;
    uint32_t levels = 0;
    for (uint32_t n = last; n != t && n != 0u; n = m.onodes[n].parent) levels++;
    if ((r = key_cursor_step(c, (levels >> 8) & 0xFFu)) || (r = key_cursor_step(c, levels & 0xFFu))) return r;
    // forward level j = levels - 1 - j steps up: quadratic in the level count, no per-lane array -- and only for ids whose tenant is the
    // tenant of the boundary key (everything else was decided above)
    for (uint32_t j = 0; j < levels; j++) {
        const ONode& o = m.onodes[ov_level_node(m, last, levels, j)];
        if ((r = key_cursor_step(c, level_hash_byte(m.opool + o.str_off, o.str_len & ~ON_SYS)))) return r;
    }
    for (uint32_t j = 0; j < levels; j++) {
        const ONode& o = m.onodes[ov_level_node(m, last, levels, j)];
        const uint32_t l = o.str_len & ~ON_SYS;
        if (j && (r = key_cursor_step(c, 0u))) return r;
        for (uint32_t k = 0; k < l; k++)
            if ((r = key_cursor_step(c, m.opool[o.str_off + k]))) return r;
    }
    return c.p < c.n ? -1 : 0;
}
// BoundaryUtil.inRange (base-kv/.../utils/BoundaryUtil.java:241-252) for the key of id; an id that is not live is never inside
BMQ_HD bool retain_key_in_boundary(const RetainMut& m, const RetainKeyStore& ks, uint32_t id, const KeyBoundary& b) {
    if (!key_id_live(m, ks, id)) return false;
    if ((b.flags & 1u) && retain_key_cmp(m, ks, id, b.start, b.start_len) < 0) return false;
    if ((b.flags & 2u) && retain_key_cmp(m, ks, id, b.end, b.end_len) >= 0) return false;
    return true;
}
// one id of the boundary pass: 0 = outside (or not live), else 1 -- or the key's length when the caller wants the bytes.  flags (may be
// null): a byte per id for the select that lists the ids.
BMQ_HD unsigned long long boundary_id_one(const RetainMut& m, const RetainKeyStore& ks, uint32_t id, const KeyBoundary& b, uint8_t* flags, uint32_t want_bytes) {
    const bool in = retain_key_in_boundary(m, ks, id, b);
    if (flags) flags[id] = in ? 1 : 0;
    if (!in) return 0ull;
    return want_bytes ? key_len_one(m, ks, id) : 1ull;
}

// The scan of RetainStoreCoProc.gc (RS/RetainStoreCoProc.java:257-277): flag[id] = 1 for every retained id whose message has
// expired at `now` (expireTime <= now; override_expiry >= 0 replaces the stored interval: GCRequest.expirySeconds).
// tenant scan (has_tenant): only ids of that tenant -- bulk-loaded ranks [t_lo, t_hi), overlay ids below tenant node t_node -- and,
// because the reference obtains them with index.match(tenantId, "#"), NOT the topics whose first level starts with '$'
// (bulk-loaded ranks [sys_lo, sys_hi), overlay ids flagged ID_SYS).  live_only = list every retained id (findAll).
struct GcQuery {
    unsigned long long now;
    long long override_expiry; // < 0: none
    uint32_t has_tenant, t_lo, t_hi, sys_lo, sys_hi, t_node;
    uint32_t live_only;
    uint32_t skip_sys;         // tenant scan: leave out the topics whose first level starts with '$' (what match(tenant, "#") cannot reach)
    uint32_t n_ids;            // ids handed out
};
BMQ_HD uint32_t gc_flag_one(const RetainMut& m, const GcQuery& q, uint32_t id) {
    if (id >= q.n_ids || id_dead(m.dead_bits, id)) return 0u;
    if (q.has_tenant) {
        if (id < m.base_n) {
            if (id < q.t_lo || id >= q.t_hi || (q.skip_sys && id >= q.sys_lo && id < q.sys_hi)) return 0u;
        } else {
            const uint32_t tn = m.id_tnode[id];
            if ((tn & ~ID_SYS) != q.t_node || (q.skip_sys && (tn & ID_SYS))) return 0u;
        }
    }
    if (q.live_only) return 1u;
    unsigned long long at = m.expire_at[id];
    if (q.override_expiry >= 0) at = retain_expire_at(m.ts[id], (uint32_t)(q.override_expiry > 0xFFFFFFFFll ? 0xFFFFFFFFll : q.override_expiry));
    return at <= q.now ? 1u : 0u;
}

} // namespace bmq
