// bmq_retain_build_core.h -- BULK LOAD of the retained-topic index where it lives: the per-item functions that turn the caller's
// (tenant, topic) items into the structures of bmq_retain.h (RNode[], the per-tenant REdge regions, the grandchild postings + RGp
// hash, the RTenantSlot directory, the level dictionary).  Every function is BMQ_HD: bmq_retain_build_kernels.h wraps them in gfx950
// kernels (k_rb_*), bmq_exec_host.h runs the very same code on host threads -- there is no second implementation.  The control
// (allocation, the order of the stages, what comes back to the host) is RetainBuild, bmq_retain_build.h.
//
// The pipeline works with flags, scans and sorts only -- no recursion, no per-tenant serial pass:
//   order      item indices sorted (stable) by (tenant rank, topic bytes with '/' below every other byte, shorter first): the order of
//              level lists, which makes every subtree one id range.  An item that equals its successor is dropped (the last add of a
//              topic wins); a scan of the survivors gives the ranks = topic ids.  Per rank: L = levels, lcp = leading levels shared
//              with the predecessor of the same tenant.
//   nodes      level-synchronously.  head_d(i) = L[i] >= d and lcp[i] < d; ord_d = its inclusive scan inside the tenant; the depth-d
//              node of item i is tenant-local node base_d + ord_d(i) - 1, base_1 = 1, base_{d+1} = base_d + count_d: breadth first,
//              children in label order, the children of a node range one node range.  sub_end of a node is the sub_begin of its next
//              sibling, else its parent's sub_end (the parent's depth was finished by the kernels of the iteration before).
//   dictionary every node label and tenant id is interned WITHOUT waiting for anybody: a lane claims a word of an owner table by CAS
//              (owner = a node index) or finds an owner there and compares its own label with the owner's -- both are input bytes,
//              complete before the kernel started.  The distinct labels (the owners) are numbered by a scan and placed into the
//              DictSlot table of bmq_dict.h's format by a second kernel: all distinct, so a claim (CAS on the tag) needs no compare.
//   edges      one lane per node claims a free entry of its tenant's region from the home bucket onwards with a 32-bit CAS on
//              `parent` and fills the rest with plain stores; RE_OVERFLOW is set on the home bucket's first entry by a SECOND kernel
//              (an atomic OR there cannot race the owner's plain store; readers come after a kernel boundary anyway).
//   postings   nodes whose grandparent has >= RPOST_MIN children, ordered by (grandparent, token, parent) with two stable radix
//              sorts; one RGp per (grandparent, token) run, inserted like the edges.
//   tenants    the run of the root's '$' children (children are in label order: a binary search by first byte), the directory entry.
#pragma once
#include <stdint.h>

#include "bmq_retain_core.h"

namespace bmq {

constexpr uint32_t RB_MAX_DEPTH = 128;          // a load that holds a topic of more levels is built by the host builder (reported: fallback)
constexpr uint32_t RB_LAB_TENANT = 0x80000000u; // lab_len flag: the label is a tenant id (bytes in the tenant table, not in the topics)
enum : uint32_t { RB_ERR_STUCK = 1u };          // a bounded probe loop ran out (cannot happen: every table has room for its entries)

struct RbCounters {
    uint32_t max_depth;      // levels of the deepest topic
    uint32_t edge_overflows; // edges that lie behind their home bucket
    uint32_t gp_overflows;   // ... (grandparent, token) runs
    uint32_t err;
};

struct RbTenant { // per tenant (rank in byte order of the ids): where its parts lie in the global arrays
    uint32_t node_base, n_nodes;
    uint32_t edge_base, edge_bucket_mask;
    uint32_t post_base, n_posts;
    uint32_t gp_base, gp_bucket_mask;
    uint32_t n_runs;
    uint32_t sys_node_lo, sys_node_hi, sys_id_lo, sys_id_hi;
    uint32_t pad[3];
};

// Everything the builder functions touch (exec memory: HBM under DevExec, host memory under HostExec).
struct RbArgs {
    // ---- input ----
    const uint8_t* tenants;      // the de-duplicated, byte-sorted tenant table, packed (readable 16 bytes past the end)
    const uint32_t* ten_off;     // [n_tenants + 1]
    uint32_t n_tenants;
    const uint8_t* topics;       // the caller's topics, packed (readable 16 bytes past the end)
    const uint32_t* topic_off;   // [n_items + 1]
    const uint32_t* item_tenant; // [n_items] rank of the item's tenant
    uint32_t n_items;
    // ---- order ----
    uint32_t* idx;    // [n_items] item indices in (tenant rank, topic) order
    uint32_t* flag;   // [max(n_items, owner slots, n_nodes)] scratch of the stage that runs
    uint32_t* scan;   // ... its inclusive scan
    uint32_t* perm;   // [n_topics] rank -> input item
    uint32_t n_topics;
    uint32_t* L;      // [n_topics] levels
    uint32_t* lcp;    // [n_topics] leading levels shared with the predecessor of the same tenant
    uint32_t* ten;    // [n_topics] tenant rank
    uint32_t* t_begin; // [n_tenants + 1] first rank of the tenant
    // ---- nodes ----
    RbTenant* plan;   // [n_tenants]
    uint32_t* tbase;  // [2 * n_tenants] base_d, base_{d-1} of the depth the loop is at
    uint32_t* S[3];   // [n_topics] inclusive scans of head_{d-1}, head_d, head_{d+1} over all ranks
    RNode* nodes;     // [n_nodes]
    uint32_t n_nodes;
    uint32_t* parent;   // [n_nodes] tenant-local id of the parent (NONE for a root)
    uint32_t* lab_off;  // [n_nodes] the label's bytes
    uint32_t* lab_len;  // [n_nodes] | RB_LAB_TENANT
    uint32_t* node_ten; // [n_nodes] tenant rank
    uint32_t* tok;      // [n_nodes] dictionary token of the label
    // ---- dictionary ----
    uint32_t* own;      // [own_mask + 1] owner table: 0 = free, else node index + 1
    uint32_t own_mask;
    uint32_t* slot_of;  // [n_nodes] the owner-table word that stands for the node's label
    uint32_t* own_rank; // [own_mask + 1] inclusive scan of "occupied": token = TOK_FIRST + rank - 1
    uint32_t* own_pool; // [own_mask + 1] inclusive scan of the pool bytes of the labels longer than 16 bytes
    DictSlot* dict;
    uint32_t dict_group_mask;
    uint8_t* pool;
    // ---- edges ----
    REdge* edges;
    uint32_t* ovf; // [n_nodes] home bucket (global entry index of its first entry) of an edge / a run that overflowed, else NONE
    // ---- postings ----
    uint32_t n_posts;
    unsigned long long* k64[2];   // [n_posts] (token << 32) | parent
    uint32_t* k32[2];             // [n_posts] global node index of the grandparent
    uint32_t* pv[3];              // [n_posts] the grandchildren (global node indices): as emitted, after the first sort, after the second
    REdge* posts;
    uint32_t n_runs;
    uint32_t* run_start; // [n_runs + 1]
    RGp* gps;
    // ---- tenants ----
    RTenantSlot* dir;
    uint32_t dir_mask;
    RbCounters* ctr;
};

// ------------------------------------------------------------------------------------------------------------
// order
// ------------------------------------------------------------------------------------------------------------
// order of level lists: '/' ranks below every other byte, a shorter topic first (cmp_topic of the host builder)
BMQ_HD int rb_cmp_topic(const uint8_t* p, uint32_t ab, uint32_t ae, uint32_t bb, uint32_t be) {
    const uint32_t la = ae - ab, lb = be - bb, n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; i++) {
        const int ca = p[ab + i] == '/' ? -1 : (int)p[ab + i], cb = p[bb + i] == '/' ? -1 : (int)p[bb + i];
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}
struct RbItemLess { // the comparator of the stable sort of item indices (std::stable_sort on the host, a device merge sort on the GPU)
    const uint8_t* topics;
    const uint32_t* topic_off;
    const uint32_t* item_tenant;
    BMQ_HD bool operator()(const uint32_t& a, const uint32_t& b) const {
        const uint32_t ta = item_tenant[a], tb = item_tenant[b];
        if (ta != tb) return ta < tb;
        return rb_cmp_topic(topics, topic_off[a], topic_off[a + 1], topic_off[b], topic_off[b + 1]) < 0;
    }
};
BMQ_HD bool rb_same_item(const RbArgs& B, uint32_t a, uint32_t b) {
    if (B.item_tenant[a] != B.item_tenant[b]) return false;
    const uint32_t ab = B.topic_off[a], la = B.topic_off[a + 1] - ab, bb = B.topic_off[b], lb = B.topic_off[b + 1] - bb;
    if (la != lb) return false;
    for (uint32_t i = 0; i < la; i++)
        if (B.topics[ab + i] != B.topics[bb + i]) return false;
    return true;
}
// flag[p] = the item at sorted position p survives (it does not equal its successor: the last add of a topic wins)
BMQ_HD void rb_keep_one(const RbArgs& B, uint32_t p) { B.flag[p] = (p + 1 < B.n_items && rb_same_item(B, B.idx[p], B.idx[p + 1])) ? 0u : 1u; }
// perm[rank] = input item (scan = inclusive scan of the flags)
BMQ_HD void rb_rank_one(const RbArgs& B, uint32_t p) {
    if (B.flag[p]) B.perm[B.scan[p] - 1] = B.idx[p];
}
// per rank: tenant, L, lcp; the first rank of every tenant; the deepest topic
BMQ_HD void rb_shape_one(const RbArgs& B, uint32_t r) {
    const uint32_t it = B.perm[r], t = B.item_tenant[it];
    const uint32_t b = B.topic_off[it], e = B.topic_off[it + 1];
    uint32_t L = 1;
    for (uint32_t i = b; i < e; i++) L += B.topics[i] == '/';
    uint32_t lcp = 0;
    const bool first = r == 0 || B.item_tenant[B.perm[r - 1]] != t;
    if (!first) {
        const uint32_t pit = B.perm[r - 1], pb = B.topic_off[pit], pe = B.topic_off[pit + 1];
        const uint32_t la = pe - pb, lb = e - b, n = la < lb ? la : lb;
        uint32_t m = 0;
        while (m < n && B.topics[pb + m] == B.topics[b + m]) {
            lcp += B.topics[b + m] == '/';
            m++;
        }
        if ((m == la || B.topics[pb + m] == '/') && (m == lb || B.topics[b + m] == '/')) lcp++; // the level that ends at m is shared too
    } else B.t_begin[t] = r;
    B.ten[r] = t;
    B.L[r] = L;
    B.lcp[r] = lcp;
    B.flag[r] = L - lcp; // nodes this topic adds to its tenant's trie
    if (L > atom_load(&B.ctr->max_depth)) atom_max(&B.ctr->max_depth, L); // (one hot word: asked first, raised a few times per load)
}

// ------------------------------------------------------------------------------------------------------------
// nodes
// ------------------------------------------------------------------------------------------------------------
BMQ_HD uint32_t rb_before(const uint32_t* S, uint32_t r) { return r ? S[r - 1] : 0u; } // the scan in front of rank r
// n_nodes of every tenant = 1 + sum of (L - lcp) over its ranks (scan = inclusive scan of rb_shape_one's flags)
BMQ_HD void rb_count_one(const RbArgs& B, uint32_t t) {
    const uint32_t tb = B.t_begin[t], te = B.t_begin[t + 1];
    B.plan[t].n_nodes = 1u + B.scan[te - 1] - rb_before(B.scan, tb);
}
BMQ_HD void rb_head_one(const RbArgs& B, uint32_t r, uint32_t d) { B.flag[r] = (B.L[r] >= d && B.lcp[r] < d) ? 1u : 0u; }
// the root of every tenant: (1, count_1, 0, n)
BMQ_HD void rb_root_one(const RbArgs& B, uint32_t t, const uint32_t* S1) {
    const uint32_t tb = B.t_begin[t], te = B.t_begin[t + 1], g = B.plan[t].node_base;
    B.nodes[g] = RNode{1u, S1[te - 1] - rb_before(S1, tb), 0u, te - tb};
    B.parent[g] = NONE;
    B.lab_off[g] = B.ten_off[t];
    B.lab_len[g] = (B.ten_off[t + 1] - B.ten_off[t]) | RB_LAB_TENANT;
    B.node_ten[g] = t;
    B.tbase[2 * t] = 1u;     // base_1
    B.tbase[2 * t + 1] = 0u; // base_0: the root
}
// [off, off + len) = level d (1-based) of the topic [b, e)
BMQ_HD void rb_level_at(const uint8_t* p, uint32_t b, uint32_t e, uint32_t d, uint32_t& off, uint32_t& len) {
    uint32_t s = b, lv = 1, i = b;
    for (; i < e; i++)
        if (p[i] == '/') {
            if (lv == d) break;
            lv++;
            s = i + 1;
        }
    off = s;
    len = i - s;
}
// depth d, one lane per rank: a head writes its node (all of it but sub_end and the child count) and what the later stages ask of a node
BMQ_HD void rb_emit_one(const RbArgs& B, uint32_t r, uint32_t d, const uint32_t* Sp, const uint32_t* Sc, const uint32_t* Sn) {
    if (!(B.L[r] >= d && B.lcp[r] < d)) return;
    const uint32_t t = B.ten[r], tb = B.t_begin[t], te = B.t_begin[t + 1];
    const uint32_t base_d = B.tbase[2 * t], base_p = B.tbase[2 * t + 1];
    const uint32_t base_n = base_d + (Sc[te - 1] - rb_before(Sc, tb));
    const uint32_t k = base_d + (Sc[r] - rb_before(Sc, tb)) - 1u;
    const uint32_t par = d == 1 ? 0u : base_p + (Sp[r] - rb_before(Sp, tb)) - 1u;
    const uint32_t g = B.plan[t].node_base + k;
    if (k >= B.plan[t].n_nodes) { // (cannot happen: the tenant's count is the sum of its heads)
        atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
        return;
    }
    RNode n;
    n.child_begin = base_n + (rb_before(Sn, r) - rb_before(Sn, tb));
    n.child_count = B.L[r] == d ? RN_TERM : 0u;
    n.sub_begin = r - tb;
    n.sub_end = 0u;
    B.nodes[g] = n;
    B.parent[g] = par;
    const uint32_t it = B.perm[r];
    uint32_t off, len;
    rb_level_at(B.topics, B.topic_off[it], B.topic_off[it + 1], d, off, len);
    B.lab_off[g] = off;
    B.lab_len[g] = len;
    B.node_ten[g] = t;
}
// ... then, behind a kernel boundary: sub_end = the next sibling's sub_begin, else the parent's sub_end; the child count from it
BMQ_HD void rb_close_one(const RbArgs& B, uint32_t r, uint32_t d, const uint32_t* Sc, const uint32_t* Sn) {
    if (!(B.L[r] >= d && B.lcp[r] < d)) return;
    const uint32_t t = B.ten[r], tb = B.t_begin[t], nb = B.plan[t].node_base;
    const uint32_t k = B.tbase[2 * t] + (Sc[r] - rb_before(Sc, tb)) - 1u;
    if (k >= B.plan[t].n_nodes) return;
    const RNode P = B.nodes[nb + B.parent[nb + k]];
    const uint32_t sub_end = (k + 1u < P.child_begin + (P.child_count & ~RN_TERM)) ? B.nodes[nb + k + 1u].sub_begin : P.sub_end;
    B.nodes[nb + k].sub_end = sub_end;
    B.nodes[nb + k].child_count |= Sn[tb + sub_end - 1u] - rb_before(Sn, r);
}
BMQ_HD void rb_advance_one(const RbArgs& B, uint32_t t, const uint32_t* Sc) { // base_d -> base_{d+1}
    const uint32_t tb = B.t_begin[t], te = B.t_begin[t + 1], base_d = B.tbase[2 * t];
    B.tbase[2 * t + 1] = base_d;
    B.tbase[2 * t] = base_d + (Sc[te - 1] - rb_before(Sc, tb));
}

// ------------------------------------------------------------------------------------------------------------
// dictionary
// ------------------------------------------------------------------------------------------------------------
BMQ_HD const uint8_t* rb_label(const RbArgs& B, uint32_t g, uint32_t& len) {
    const uint32_t ll = B.lab_len[g];
    len = ll & ~RB_LAB_TENANT;
    return ((ll & RB_LAB_TENANT) ? B.tenants : B.topics) + B.lab_off[g];
}
// hash_level of bmq_dict.h over s[0, len): every byte, as little-endian words
BMQ_HD void rb_hash_label(const uint8_t* s, uint32_t len, LevelHash& h, uint32_t inl[4]) {
    h = level_hash_init();
    inl[0] = inl[1] = inl[2] = inl[3] = 0;
    for (uint32_t i = 0; i < len; i += 4) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4 && i + k < len; k++) w |= (uint32_t)s[i + k] << (8 * k);
        level_hash_word(h, w);
        if (i < 16) inl[i >> 2] = w;
    }
}
BMQ_HD void rb_intern_one(const RbArgs& B, uint32_t g) {
    uint32_t len;
    const uint8_t* s = rb_label(B, g, len);
    LevelHash h;
    uint32_t inl[4];
    rb_hash_label(s, len, h, inl);
    uint32_t w = level_hash_slot(h, len) & B.own_mask;
    for (uint32_t probes = 0; probes <= B.own_mask; probes++) {
        uint32_t v = atom_load(&B.own[w]);
        if (v == 0) v = atom_cas(&B.own[w], 0u, g + 1u);
        if (v == 0 || v == g + 1u) { // claimed: this node's label stands for the string
            B.slot_of[g] = w;
            return;
        }
        uint32_t olen;
        const uint8_t* o = rb_label(B, v - 1u, olen); // the owner's label: input bytes, complete before the kernel started
        bool eq = olen == len;
        for (uint32_t i = 0; i < len && eq; i++) eq = o[i] == s[i];
        if (eq) {
            B.slot_of[g] = w;
            return;
        }
        w = (w + 1u) & B.own_mask;
    }
    B.slot_of[g] = 0;
    atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
}
// per owner-table word: occupied (-> flag), pool bytes of its string (-> scan, used as a second flag array)
BMQ_HD void rb_owner_one(const RbArgs& B, uint32_t w) {
    const uint32_t v = B.own[w];
    B.flag[w] = v ? 1u : 0u;
    uint32_t len = 0;
    if (v) (void)rb_label(B, v - 1u, len);
    B.scan[w] = len > 16 ? ((len + 3u) & ~3u) : 0u;
}
// the distinct strings into the DictSlot table (bmq_dict.h's format): claim by CAS on the tag, fill with plain stores
BMQ_HD void rb_place_one(const RbArgs& B, uint32_t w) {
    const uint32_t v = B.own[w];
    if (!v) return;
    uint32_t len;
    const uint8_t* s = rb_label(B, v - 1u, len);
    LevelHash h;
    uint32_t inl[4];
    rb_hash_label(s, len, h, inl);
    const uint32_t tag = level_hash_tag(h);
    uint32_t g = level_hash_slot(h, len) & B.dict_group_mask;
    for (uint32_t probes = 0; probes <= B.dict_group_mask; probes++) {
        for (uint32_t j = 0; j < DICT_GROUP; j++) {
            DictSlot* d = B.dict + DICT_GROUP * (size_t)g + j;
            if (atom_load(&d->tag) != 0u || atom_cas(&d->tag, 0u, tag) != 0u) continue;
            uint32_t off = 0;
            if (len > 16) {
                off = B.own_pool[w] - ((len + 3u) & ~3u);
                for (uint32_t i = 0; i < len; i++) B.pool[off + i] = s[i];
            }
            d->token = TOK_FIRST + B.own_rank[w] - 1u;
            d->len = len;
            d->pool_off = off;
            d->inl[0] = inl[0], d->inl[1] = inl[1], d->inl[2] = inl[2], d->inl[3] = inl[3];
            return;
        }
        g = (g + 1u) & B.dict_group_mask;
    }
    atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
}
BMQ_HD void rb_token_one(const RbArgs& B, uint32_t g) { B.tok[g] = TOK_FIRST + B.own_rank[B.slot_of[g]] - 1u; }

// ------------------------------------------------------------------------------------------------------------
// edges
// ------------------------------------------------------------------------------------------------------------
BMQ_HD void rb_edge_one(const RbArgs& B, uint32_t g) {
    B.ovf[g] = NONE;
    const uint32_t p = B.parent[g];
    if (p == NONE) return; // a root
    const RbTenant& T = B.plan[B.node_ten[g]];
    const uint32_t tok = B.tok[g], mask = T.edge_bucket_mask, home = redge_bucket(p, tok, mask);
    const RNode n = B.nodes[g];
    uint32_t bk = home;
    for (uint32_t probes = 0; probes <= mask; probes++) {
        for (uint32_t j = 0; j < 4; j++) {
            REdge* e = B.edges + T.edge_base + 4 * (size_t)bk + j;
            if (atom_load(&e->parent) != NONE || atom_cas(&e->parent, NONE, p) != NONE) continue;
            e->token = tok;
            e->child = g - T.node_base;
            e->child_topic = n.sub_begin | (n.child_count & RN_TERM);
            if (bk != home) {
                B.ovf[g] = T.edge_base + 4u * home;
                atom_add(&B.ctr->edge_overflows, 1u);
            }
            return;
        }
        bk = (bk + 1u) & mask;
    }
    atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
}
BMQ_HD void rb_edge_overflow_one(const RbArgs& B, uint32_t g) {
    if (B.ovf[g] != NONE) atom_or(&B.edges[B.ovf[g]].child, RE_OVERFLOW);
}

// ------------------------------------------------------------------------------------------------------------
// grandchild postings
// ------------------------------------------------------------------------------------------------------------
BMQ_HD void rb_post_flag_one(const RbArgs& B, uint32_t g) {
    uint32_t f = 0;
    const uint32_t p = B.parent[g];
    if (p != NONE && p != 0u) { // (a child of the root has no grandparent)
        const uint32_t nb = B.plan[B.node_ten[g]].node_base;
        const uint32_t gp = B.parent[nb + p];
        f = (B.nodes[nb + gp].child_count & ~RN_TERM) >= RPOST_MIN ? 1u : 0u;
    }
    B.flag[g] = f;
}
BMQ_HD void rb_post_emit_one(const RbArgs& B, uint32_t g) {
    if (!B.flag[g]) return;
    const uint32_t j = B.scan[g] - 1u;
    B.pv[0][j] = g;
    B.k64[0][j] = ((unsigned long long)B.tok[g] << 32) | B.parent[g];
}
BMQ_HD void rb_post_gp_one(const RbArgs& B, uint32_t i) { // key of the second sort: the grandparent's global node index
    const uint32_t g = B.pv[1][i], nb = B.plan[B.node_ten[g]].node_base;
    B.k32[0][i] = nb + B.parent[nb + B.parent[g]];
}
// posts[i] in its final order; flag[i] = a (grandparent, token) run starts here
BMQ_HD void rb_post_write_one(const RbArgs& B, uint32_t i) {
    const uint32_t g = B.pv[2][i];
    const RNode n = B.nodes[g];
    B.posts[i] = REdge{B.parent[g], B.tok[g], g - B.plan[B.node_ten[g]].node_base, n.sub_begin | (n.child_count & RN_TERM)};
    B.flag[i] = (i == 0 || B.k32[1][i] != B.k32[1][i - 1] || B.tok[B.pv[2][i - 1]] != B.tok[g]) ? 1u : 0u;
}
// per tenant: its slice of the postings (the sorted keys are global node indices: a binary search) and its runs
BMQ_HD void rb_post_tenant_one(const RbArgs& B, uint32_t t) {
    uint32_t lim[2];
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t key = B.plan[t].node_base + (k ? B.plan[t].n_nodes : 0u);
        uint32_t lo = 0, hi = B.n_posts;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (B.k32[1][mid] < key) lo = mid + 1;
            else hi = mid;
        }
        lim[k] = lo;
    }
    B.plan[t].post_base = lim[0];
    B.plan[t].n_posts = lim[1] - lim[0];
    B.plan[t].n_runs = lim[1] > lim[0] ? B.scan[lim[1] - 1] - rb_before(B.scan, lim[0]) : 0u;
}
BMQ_HD void rb_run_start_one(const RbArgs& B, uint32_t i) {
    if (B.flag[i]) B.run_start[B.scan[i] - 1u] = i;
    if (i == 0) B.run_start[B.n_runs] = B.n_posts;
}
BMQ_HD void rb_gp_one(const RbArgs& B, uint32_t run) {
    B.ovf[run] = NONE;
    const uint32_t i = B.run_start[run], cnt = B.run_start[run + 1] - i;
    const uint32_t g = B.pv[2][i];
    const RbTenant& T = B.plan[B.node_ten[g]];
    const uint32_t gp = B.k32[1][i] - T.node_base, tok = B.tok[g], mask = T.gp_bucket_mask, home = rgp_bucket(gp, tok, mask);
    uint32_t bk = home;
    for (uint32_t probes = 0; probes <= mask; probes++) {
        for (uint32_t j = 0; j < 4; j++) {
            RGp* e = B.gps + T.gp_base + 4 * (size_t)bk + j;
            if (atom_load(&e->gp) != NONE || atom_cas(&e->gp, NONE, gp) != NONE) continue;
            e->token = tok;
            e->begin = i - T.post_base;
            e->count = cnt;
            if (bk != home) {
                B.ovf[run] = T.gp_base + 4u * home;
                atom_add(&B.ctr->gp_overflows, 1u);
            }
            return;
        }
        bk = (bk + 1u) & mask;
    }
    atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
}
BMQ_HD void rb_gp_overflow_one(const RbArgs& B, uint32_t run) {
    if (B.ovf[run] != NONE) atom_or(&B.gps[B.ovf[run]].count, RE_OVERFLOW);
}

// ------------------------------------------------------------------------------------------------------------
// tenants
// ------------------------------------------------------------------------------------------------------------
BMQ_HD void rb_tenant_one(const RbArgs& B, uint32_t t) {
    RbTenant& T = B.plan[t];
    const RNode root = B.nodes[T.node_base];
    const uint32_t c0 = root.child_begin, c1 = c0 + (root.child_count & ~RN_TERM);
    // children are in label order: those that start with '$' are one run.  first byte of a label, -1 for the empty label
    uint32_t lim[2];
    for (uint32_t k = 0; k < 2; k++) {
        const int key = '$' + (int)k;
        uint32_t lo = c0, hi = c1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2, g = T.node_base + mid;
            const int fb = B.lab_len[g] ? (int)B.topics[B.lab_off[g]] : -1;
            if (fb < key) lo = mid + 1;
            else hi = mid;
        }
        lim[k] = lo;
    }
    T.sys_node_lo = T.sys_node_hi = T.sys_id_lo = T.sys_id_hi = 0;
    if (lim[1] > lim[0]) {
        T.sys_node_lo = lim[0];
        T.sys_node_hi = lim[1];
        T.sys_id_lo = B.nodes[T.node_base + lim[0]].sub_begin;
        T.sys_id_hi = B.nodes[T.node_base + lim[1] - 1u].sub_end;
    }
    const uint32_t token = B.tok[T.node_base];
    uint32_t d = tenant_hash(token) & B.dir_mask;
    for (uint32_t probes = 0; probes <= B.dir_mask; probes++) {
        RTenantSlot* s = B.dir + d;
        if (atom_load(&s->token) == 0u && atom_cas(&s->token, 0u, token) == 0u) {
            s->node_base = T.node_base;
            s->edge_base = T.edge_base;
            s->edge_bucket_mask = T.edge_bucket_mask;
            s->id_base = B.t_begin[t];
            s->sys_node_lo = T.sys_node_lo, s->sys_node_hi = T.sys_node_hi;
            s->sys_id_lo = T.sys_id_lo, s->sys_id_hi = T.sys_id_hi;
            s->post_base = T.post_base;
            s->gp_base = T.gp_base;
            s->gp_bucket_mask = T.gp_bucket_mask;
            return;
        }
        d = (d + 1u) & B.dir_mask;
    }
    atom_or(&B.ctr->err, (uint32_t)RB_ERR_STUCK);
}

} // namespace bmq
