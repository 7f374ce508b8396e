// bmq_retain_snap_core.h -- the per-item functions of the SNAPSHOT of the retained-topic index (bmq_retain_compact_begin with
// bmq_config.retain_builder = 3) and of what the next generation's mutable part is made of.  A snapshot is the live topics of the serving
// generation, gathered where the index lives into the layout the executor builder reads (RbInput, bmq_retain_build.h): a packed tenant
// table, item -> tenant index, packed topics with their offsets, stamps.  Nothing of it crosses to the host under the engine lock.
//   * the strings of bulk-loaded ids come from the generation's key store (RetainKeyStore, bmq_retain_core.h): contiguous runs of one array,
//     copied output-ordered by rs_gather_chunk (16 bytes per call, a search of the offsets for the first item);
//   * the strings of overlay ids come from their ONode chain, one item per call, the last level first (the shape of ov_topic_write_one);
//   * the tenant table is the key store's tenants followed by one entry per overlay tenant node that owns a selected id -- a tenant with
//     both parts appears twice, which RbInput allows (the builder de-duplicates by bytes).
// After the build the same gather, indexed through the builder's permutation rank -> item, lays the next generation's key store out in rank
// order, and rs_next_one writes its per-id payload.  Wrapped by the k_rs_* kernels (bmq_retain_snap_kernels.h) and by HostExec's loops.
#pragma once
#include "bmq_retain_core.h"

namespace bmq {

constexpr uint32_t RS_OV = 0x80000000u; // RsSnap.item_tenant between rs_len_one and rs_item_write_one: an overlay tenant NODE, not yet a table entry

struct RsSnap { // exec memory, RbInput's layout
    uint8_t* tenants;       // packed tenant ids (readable 16 bytes past the end)
    uint32_t* tenant_off;   // [n_tenants + 1]
    uint32_t n_tenants;
    uint32_t* item_tenant;  // [n]
    uint8_t* topics;        // packed topics (zero-filled 16 bytes past the end)
    uint32_t* topic_off;    // [n + 1]
    uint32_t n;
    unsigned long long* ts; // [n]
    uint32_t* expiry;       // [n]
};

struct RsArgs {
    const uint32_t* ids; // [S.n] the selected ids, ascending: the bulk-loaded ones first
    RsSnap S;
    uint32_t* len;       // [S.n] topic lengths (the scan's input)
    uint32_t n_bulk;     // items [0, n_bulk) are bulk-loaded ids (known after rs_len_one: totals[1])
    // overlay tenant nodes that own a selected id, per overlay node
    uint32_t* tn_flag;   // [ov_nodes] 1: the node is such a tenant
    uint32_t* tn_len;    // [ov_nodes] its label's length, 0 for the others
    uint32_t* tn_rank;   // [ov_nodes] inclusive scan of tn_flag
    uint32_t* tn_end;    // [ov_nodes] inclusive scan of tn_len
    uint32_t ov_nodes;
    uint32_t ks_tenants, ks_tenant_bytes; // the first entries of the table are the key store's
    unsigned long long* totals; // [0] topic bytes, [1] bulk-loaded items, [2] overlay tenants, [3] their bytes
};

// sets a flag word that many lanes share: the word is read first, so that a hot one is not hammered with atomics
BMQ_HD void rs_mark(uint32_t* u) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (__hip_atomic_load(u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atom_or(u, 1u);
#else
    if (__atomic_load_n(u, __ATOMIC_RELAXED) == 0u) atom_or(u, 1u);
#endif
}

// length, tenant and stamps of selected id i -> its topic length; *bulk = it is a bulk-loaded id
BMQ_HD uint32_t rs_len_one(const RetainMut& m, const RetainKeyStore& ks, const RsArgs& A, uint32_t i, bool* bulk) {
    const uint32_t id = A.ids[i];
    uint32_t len = 0, ten = 0;
    *bulk = id < m.base_n;
    if (id < m.base_n) {
        if (id < ks.n_ids) {
            len = (uint32_t)(ks.topic_off[id + 1] - ks.topic_off[id]);
            ten = key_store_tenant(ks, id);
        }
    } else if (id < m.id_cap && m.id_node[id] != NONE) { // as ov_topic_len_one: up the chain to the tenant's node
        uint32_t total = 0, levels = 0, t = m.id_node[id];
        while (m.onodes[t].parent != 0u) {
            total += m.onodes[t].str_len & ~ON_SYS;
            levels++;
            t = m.onodes[t].parent;
        }
        len = total + (levels ? levels - 1 : 0);
        ten = RS_OV | t;
        rs_mark(&A.tn_flag[t]);
    }
    A.len[i] = len;
    A.S.item_tenant[i] = ten;
    A.S.ts[i] = id < m.id_cap ? m.ts[id] : 0ull;
    A.S.expiry[i] = id < m.id_cap ? m.expiry[id] : 0xFFFFFFFFu;
    return len;
}
BMQ_HD void rs_tenant_len_one(const RetainMut& m, const RsArgs& A, uint32_t node) { A.tn_len[node] = A.tn_flag[node] ? (m.onodes[node].str_len & ~ON_SYS) : 0u; }
BMQ_HD void rs_totals_one(const RsArgs& A) {
    A.totals[2] = A.ov_nodes ? A.tn_rank[A.ov_nodes - 1] : 0u;
    A.totals[3] = A.ov_nodes ? A.tn_end[A.ov_nodes - 1] : 0u;
}
// the table entry of an overlay tenant node: its offset and its bytes, behind the key store's tenants
BMQ_HD void rs_tenant_write_one(const RetainMut& m, const RsArgs& A, uint32_t node) {
    if (!A.tn_flag[node]) return;
    const ONode& n = m.onodes[node];
    const uint32_t l = n.str_len & ~ON_SYS, end = A.ks_tenant_bytes + A.tn_end[node];
    A.S.tenant_off[A.ks_tenants + A.tn_rank[node]] = end;
    for (uint32_t k = 0; k < l; k++) A.S.tenants[end - l + k] = m.opool[n.str_off + k];
}
// overlay item i (>= A.n_bulk): its tenant's table entry, and its topic back to front into [topic_off[i], topic_off[i + 1])
BMQ_HD void rs_item_write_one(const RetainMut& m, const RsArgs& A, uint32_t i) {
    const uint32_t ten = A.S.item_tenant[i];
    if (!(ten & RS_OV)) return;
    A.S.item_tenant[i] = A.ks_tenants + A.tn_rank[ten & ~RS_OV] - 1u;
    uint32_t end = A.S.topic_off[i + 1], t = m.id_node[A.ids[i]];
    while (m.onodes[t].parent != 0u) {
        const ONode& n = m.onodes[t];
        const uint32_t l = n.str_len & ~ON_SYS;
        end -= l;
        for (uint32_t k = 0; k < l; k++) A.S.topics[end + k] = m.opool[n.str_off + k];
        t = n.parent;
        if (m.onodes[t].parent != 0u) A.S.topics[--end] = '/';
    }
}

// ---- the output-ordered gather: item j of the output is the bytes [soff[sidx[j]], + doff[j + 1] - doff[j]) of src ----
template <class SO> struct RsGather {
    uint8_t* dst;               // 16-byte aligned
    const uint32_t* doff;       // [n + 1] where item j starts in dst
    uint32_t n;
    const uint8_t* src;
    const SO* soff;             // where source item s starts in src
    const uint32_t* sidx;       // [n] output item -> source item
    unsigned long long bytes;   // doff[n]
};
// the last item of [lo, hi) that starts at or before output byte o (doff[lo] <= o)
template <class SO> BMQ_HD uint32_t rs_item_at(const RsGather<SO>& G, unsigned long long o, uint32_t lo, uint32_t hi) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (G.doff[mid] <= o) lo = mid;
        else hi = mid;
    }
    return lo;
}
// output bytes [16 c, 16 c + 16) (the last chunk: up to G.bytes); the chunk's first byte belongs to an item of [lo, hi).  16 bytes at once
// where the chunk lies inside one item whose source is 16-byte aligned there; else byte loads, and one 16-byte store for a whole chunk.
template <class SO> BMQ_HD void rs_gather_chunk(const RsGather<SO>& G, unsigned long long c, uint32_t lo, uint32_t hi) {
    const unsigned long long o = 16ull * c, e = o + 16 < G.bytes ? o + 16 : G.bytes;
    uint32_t j = rs_item_at(G, o, lo, hi);
    const uint8_t* s = G.src + G.soff[G.sidx[j]] + (o - G.doff[j]);
    uint8_t* d = G.dst + o;
    if (e - o == 16 && G.doff[j + 1] >= e && (reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
        __builtin_memcpy(__builtin_assume_aligned(d, 16), __builtin_assume_aligned(s, 16), 16);
        return;
    }
    unsigned long long q[2] = {0ull, 0ull}; // the chunk's bytes, little-endian
    unsigned long long at = G.soff[G.sidx[j]] + (o - G.doff[j]), next = G.doff[j + 1]; // source position of byte p; where item j ends in dst
    const uint32_t nb = (uint32_t)(e - o);
    for (uint32_t k = 0; k < nb; k++, at++) {
        while (next <= o + k) { // (o + k < G.bytes = doff[n]: j stays below n)
            j++;
            at = G.soff[G.sidx[j]];
            next = G.doff[j + 1];
        }
        const unsigned long long v = (unsigned long long)G.src[at] << (8u * (k & 7u));
        if (k < 8) q[0] |= v;
        else q[1] |= v;
    }
    if (nb == 16) __builtin_memcpy(__builtin_assume_aligned(d, 16), q, 16);
    else
        for (uint32_t k = 0; k < nb; k++) d[k] = (uint8_t)((k < 8 ? q[0] : q[1]) >> (8u * (k & 7u)));
}

// ---- the builder's input from exec memory: which entries of the tenant table the items use, and their ranks ----
BMQ_HD void rs_used_one(const uint32_t* item_tenant, uint32_t* used, uint32_t i) { rs_mark(used + item_tenant[i]); }
BMQ_HD void rs_remap_one(const uint32_t* item_tenant, const uint32_t* rank_of, uint32_t* out, uint32_t i) { out[i] = rank_of[item_tenant[i]]; }

// ---- the next generation's per-id arrays, through the builder's permutation rank -> item of the snapshot ----
struct RsNext {
    const uint32_t* perm;            // [n_topics]
    uint32_t n_topics;
    const uint32_t* topic_off;       // the snapshot's
    const unsigned long long* ts;
    const uint32_t* expiry;
    uint32_t* klen;                  // [n_topics] topic length per rank
    uint32_t* koff;                  // [n_topics + 1] their exclusive sums
    unsigned long long *o_ts, *o_expire_at;
    uint32_t* o_expiry;
    unsigned long long* ks_topic_off; // [n_topics + 1] RetainKeyStore.topic_off of the next generation
};
BMQ_HD void rs_perm_len_one(const RsNext& N, uint32_t r) {
    const uint32_t it = N.perm[r];
    N.klen[r] = N.topic_off[it + 1] - N.topic_off[it];
}
BMQ_HD void rs_next_one(const RsNext& N, uint32_t r) {
    const uint32_t it = N.perm[r];
    const unsigned long long ts = N.ts[it];
    const uint32_t ex = N.expiry[it];
    N.o_ts[r] = ts;
    N.o_expiry[r] = ex;
    N.o_expire_at[r] = (ts == 0 && ex == 0xFFFFFFFFu) ? RETAIN_NEVER : retain_expire_at(ts, ex);
    if (r == 0) N.ks_topic_off[0] = 0ull;
    N.ks_topic_off[r + 1] = N.koff[r + 1];
}

} // namespace bmq
