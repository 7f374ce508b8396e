// bmq_order_core.h -- the per-item functions of the key-ordered window (DistIndex::window, bmq_routes_window): which live routes lie at
// or behind a cursor key, in which bin of a set of sorted pivot keys a route's key falls, and the rank of a key among the keys of a small
// bucket.  Keys are compared where they lie, in the key pool, as unsigned bytes with a proper prefix first (KV order, bytes_compare).
// The gfx950 kernels over them are bmq_order_kernels.h (k_o_*); HostExec loops over the same functions.  Nothing here writes to the index.
#pragma once
#include "bmq_build_core.h"

namespace bmq {

constexpr uint32_t ORDER_WINDOW_MAX = 65536; // BMQ_WINDOW_MAX
constexpr uint32_t ORDER_BUCKET_MAX = 512;   // keys of a bucket that is ranked by counting: every key against every other
constexpr uint32_t ORDER_PIVOTS = 255;       // pivots of one bucketing round
constexpr uint32_t ORDER_BINS = 2 * ORDER_PIVOTS + 1;
constexpr uint32_t ORDER_DROP = 0xFFFFFFFFu; // base[bin] of the scatter pass: the bin's ids go nowhere

// The lower bound of a window.  flags bit 0: there is one (else every live route passes); bit 1: exclusive (key > bound; else >=);
// bit 2: the bound is the key of route `id` (live; the pool holds its bytes, nothing is uploaded), else key[0, len) in exec memory
struct OrderCursor {
    const uint8_t* key;
    uint32_t len;
    uint32_t flags;
    uint32_t id;
    uint32_t pad0;
};
// where the cursor's bytes lie (a cursor by id is resolved through the key store)
BMQ_HD void order_cursor_resolve(const DistIndexMut& ix, OrderCursor& c) {
    if ((c.flags & 5u) != 5u) return;
    const unsigned long long r = ix.kref[c.id];
    c.key = ix.kpool + (r & KREF_OFF_MASK);
    c.len = (uint32_t)(r >> KREF_LEN_SHIFT);
}
// is route `id` live and at / behind the cursor?
BMQ_HD bool order_flag_one(const DistIndexMut& ix, uint32_t id, const OrderCursor& c) {
    const unsigned long long r = ix.kref[id];
    const unsigned long long len = r >> KREF_LEN_SHIFT;
    if (len == 0) return false;
    if ((c.flags & 1u) == 0) return true;
    const int d = key_compare(ix.kpool + (r & KREF_OFF_MASK), len, c.key, c.len);
    return (c.flags & 2u) ? d > 0 : d >= 0;
}
// Two keys of the pool, by reference: < 0, 0, > 0.  Sixteen bytes a step (bytes_chunk16: five aligned words requested together, the bytes
// past the shorter key read as zero in BOTH chunks, so they never decide); the first word that differs decides, compared as a big-endian
// number.  Route keys of one tenant share the whole header and often most of the filter: a byte loop would wait for every byte of it.
BMQ_HD int order_compare(const uint8_t* kp, unsigned long long ra, unsigned long long rb) {
    const unsigned long long ao = ra & KREF_OFF_MASK, an = ra >> KREF_LEN_SHIFT, bo = rb & KREF_OFF_MASK, bn = rb >> KREF_LEN_SHIFT;
    const unsigned long long m = an < bn ? an : bn;
    for (unsigned long long i = 0; i < m; i += 16) {
        uint32_t x[4], y[4];
        const uint32_t c = (uint32_t)(m - i < 16 ? m - i : 16);
        bytes_chunk16(kp, ao + i, c, x);
        bytes_chunk16(kp, bo + i, c, y);
        for (uint32_t w = 0; w < 4; w++)
            if (x[w] != y[w]) return __builtin_bswap32(x[w]) < __builtin_bswap32(y[w]) ? -1 : 1;
    }
    return an < bn ? -1 : (an > bn ? 1 : 0);
}
// The bin of route `id` among P pivots sorted by key (piv[0 .. P): route ids): 2 j + 1 is pivot j itself (keys are unique: the pivot's
// id), 2 j the keys strictly between pivot j - 1 and pivot j -- bins ascend in key order, and a bin of even number holds no pivot.
BMQ_HD uint32_t order_bin_one(const DistIndexMut& ix, uint32_t id, const uint32_t* piv, uint32_t P) {
    const unsigned long long r = ix.kref[id];
    uint32_t lo = 0, hi = P; // -> the number of pivots below the key
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (order_compare(ix.kpool, ix.kref[piv[mid]], r) < 0) lo = mid + 1;
        else hi = mid;
    }
    return 2 * lo + (lo < P && piv[lo] == id ? 1u : 0u);
}
// is key k of the list ids[0], ids[stride], ids[2 stride] ... below key j of it?  (never for k == j)
BMQ_HD bool order_below_one(const DistIndexMut& ix, const uint32_t* ids, uint32_t stride, uint32_t k, uint32_t j) {
    return k != j && order_compare(ix.kpool, ix.kref[ids[(size_t)k * stride]], ix.kref[ids[(size_t)j * stride]]) < 0;
}
// the rank of key j among the n keys of such a list: the keys below it (unique keys: the ranks are a permutation).  The device counts
// them 64 at a time, one wave per key (k_o_pivots, k_o_leaves)
BMQ_HD uint32_t order_rank_one(const DistIndexMut& ix, const uint32_t* ids, uint32_t n, uint32_t stride, uint32_t j) {
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n; k++) rank += order_below_one(ix, ids, stride, k, j) ? 1u : 0u;
    return rank;
}

// what the windows of an engine did so far (bmq_window_info): calls, candidates the flag pass left, bucketing rounds, pieces ranked, the
// largest of them, rounds that split a piece of an earlier round again
struct OrderStats {
    uint64_t n_calls = 0, n_candidates = 0, n_rounds = 0, n_bucket_sorts = 0, max_bucket = 0, n_rebucketed = 0;
};
// One bucket that is small enough to rank: n <= ORDER_BUCKET_MAX ids at src[off ..) of list `list` (0 / 1: the two id lists of the window
// scratch); the `keep` smallest go to out[out_off ..) in key order
struct OrderLeaf {
    uint32_t list, off, n, keep, out_off;
};
BMQ_HD void order_leaf_one(const DistIndexMut& ix, const uint32_t* src, const OrderLeaf& lf, uint32_t j, uint32_t* out) {
    const uint32_t rank = order_rank_one(ix, src + lf.off, lf.n, 1u, j);
    if (rank < lf.keep) out[lf.out_off + rank] = src[lf.off + j];
}

} // namespace bmq
