// bmq_caps_core.h -- the fan-out caps of MatchedRoutes (DW/cache/MatchedRoutes.java:87-141) over a whole match CSR: per-item functions,
// BMQ_HD like the other passes over device-resident state.  The gfx950 kernels over them are bmq_caps_kernels.h (k_caps_*), the control is
// bmq_caps.h; HostExec loops over the same functions.  Nothing here writes to the index.
//
// What it replaces.  DistWorkerCoProc.batchDist takes every topic's routes out of a MatchedRoutes, which admits persistent routes
// (subBrokerId == 1) and groups (flag 2 / 3) first-come in KV key order up to the tenant's MaxPersistentFanout / MaxGroupFanout and reports
// a throttle event for each route it turns away.  cap_rows (bmq_engine.hip) restates that on the host for one pair of caps per call; this is
// the same rule for a batch whose rows carry caps of their own (an index into a table: one entry per tenant), answered where the CSR lies:
//   a row no longer than min(pf, gf) cannot be throttled: copied through, never classified;
//   in every other row an id is classified from the tail of its key (caps_class_of); dead ids leave the row;
//   a class with more members than its cap keeps the `cap` members with the smallest KEYS (order_compare: unsigned bytes, a proper prefix
//   first) -- ids are key ranks only right after a bulk load --; each other member is one event;
//   the survivors stay in the input's order.
// Events: rows ascend; inside a row the persistent events in key order, then the group events in key order (the event of the member of
// key rank k >= cap lies at the class's base + k - cap), so no rank across the two classes is ever needed.
#pragma once
#include "bmq_fanout_core.h"
#include "bmq_order_core.h"

namespace bmq {

constexpr uint32_t CAPS_RANK_MAX = 4096; // members of a class that is ranked by counting: every key against every other of its row

// class of a pair
enum : uint8_t { CAPS_TRANSIENT = 0, CAPS_PERSISTENT = 1, CAPS_GROUP = 2, CAPS_DEAD = 3, CAPS_FREE = 4 /* its row was never classified */ };
// mode[row]: the low two bits say how the row is answered, the two above which of its classes exceed their cap
enum : uint8_t { CAPS_ROW_THROUGH = 0, CAPS_ROW_CLASSIFIED = 1, CAPS_ROW_RANKED = 2, CAPS_ROW_FALLBACK = 3, CAPS_OVER_P = 4, CAPS_OVER_G = 8 };
// ctr[]: rows classified, rows ranked on the device, rows left to the host, pairs to rank, error bits, events
enum : uint32_t { CAPS_C_CLASSIFIED = 0, CAPS_C_RANKED, CAPS_C_FALLBACK, CAPS_C_WORK, CAPS_C_ERR, CAPS_C_EVENTS, CAPS_CTRS = 8 };
enum : uint32_t { CAPS_ERR_INDEX = 1u, CAPS_ERR_KEY = 2u };

struct CapsBatch { // every pointer: exec memory
    const uint32_t* row_ptr; // [n_rows + 1], row_ptr[n_rows] == total
    const uint32_t* ids;     // [total]
    uint32_t n_rows, total;
    uint32_t id_end;          // ids handed out so far
    const uint32_t* row_caps; // [n_rows] index into the table, or null: entry 0
    const int32_t *max_pf, *max_gf; // [n_caps], none negative
    uint32_t n_caps;
    uint8_t* cls;        // [total]
    uint8_t* mode;       // [n_rows]
    uint32_t* row_cnt;   // [2 n_rows] members of class persistent / group (zeroed before the classify)
    uint32_t *ev_cnt, *ev_scan; // [2 n_rows] members over the cap, and their inclusive scan: the events in front of a class end at ev_scan - ev_cnt
    uint32_t *keep, *keep_scan; // [total] 1 = the pair survives, and its inclusive scan
    uint32_t* work;      // [total] the pairs to rank
    uint32_t* fb_rows;   // [n_rows] the rows left to the host
    uint32_t* ctr;       // [CAPS_CTRS] (zeroed)
    uint32_t *out_row_ptr, *out_ids, *out_class_counts; // out_class_counts may be null
    int32_t* out_events; // [4 events_cap], may be null
    uint32_t events_cap;
};

// the caps of row r; false: its index lies outside the table
BMQ_HD bool caps_of_row(const CapsBatch& b, uint32_t r, uint32_t& pf, uint32_t& gf) {
    const uint32_t t = b.row_caps ? b.row_caps[r] : 0u;
    if (t >= b.n_caps) return false;
    pf = (uint32_t)b.max_pf[t];
    gf = (uint32_t)b.max_gf[t];
    return true;
}
// is a row of n ids classified at all?  (not when neither cap can bind)
BMQ_HD bool caps_row_classified(uint32_t n, uint32_t pf, uint32_t gf) { return n > (pf < gf ? pf : gf); }

// The class of route `id`, from the tail of its key "... flag receiverUrl be16(len)" (fo_deliverer_span reads the same tail).  An id the
// index never handed out, or whose route is gone, has no key (gather_ref_one: DistIndex::route_keys gives it an empty key): dead.  Any flag but
// 1 is a group; flag 1 is persistent iff the decimal-digit prefix of the receiverUrl is not empty and equals 1 -- the rule of cap_rows,
// restated, not improved (the number wraps as that one's does).
BMQ_HD uint32_t caps_class_of(const DistIndexMut& ix, uint32_t id, uint32_t id_end, uint32_t* err) {
    const unsigned long long r = id < id_end && id < ix.id_cap ? ix.kref[id] : 0ull;
    if (r == 0) return CAPS_DEAD;
    const unsigned long long off = r & KREF_OFF_MASK, len = r >> KREF_LEN_SHIFT, end = off + len;
    const unsigned long long rlen = len >= 3 ? be16_at(ix.kpool, end - 2) : 0ull;
    if (len < 3 || rlen + 3 > len) { // not a route key: the call fails (cap_rows: "corrupt key store")
        *err |= CAPS_ERR_KEY;
        return CAPS_DEAD;
    }
    const unsigned long long rend = end - 2, recv = rend - rlen;
    if (ix.kpool[recv - 1] != 1) return CAPS_GROUP;
    unsigned long long broker = 0, p = recv;
    while (p < rend && ix.kpool[p] >= '0' && ix.kpool[p] <= '9') broker = broker * 10 + (unsigned long long)(ix.kpool[p++] - '0');
    return broker == 1 && p > recv ? CAPS_PERSISTENT : CAPS_TRANSIENT;
}
// pass 1, per pair i of row r: its class (CAPS_FREE in a row that is copied through)
BMQ_HD uint32_t caps_classify_one(const DistIndexMut& ix, const CapsBatch& b, uint32_t i, uint32_t r, uint32_t* err) {
    uint32_t pf = 0, gf = 0;
    if (!caps_of_row(b, r, pf, gf) || !caps_row_classified(b.row_ptr[r + 1] - b.row_ptr[r], pf, gf)) return CAPS_FREE; // (a bad index: reported by the row pass)
    return caps_class_of(ix, b.ids[i], b.id_end, err);
}
// pass 1b, per row (behind the counts of its classes): how it is answered, and its events per class.  -> mode[r], | CAPS_BAD_INDEX
constexpr uint32_t CAPS_BAD_INDEX = 16u;
BMQ_HD uint32_t caps_row_one(const CapsBatch& b, uint32_t r) {
    uint32_t pf = 0, gf = 0, m = CAPS_ROW_THROUGH, xp = 0, xg = 0;
    const bool known = caps_of_row(b, r, pf, gf);
    if (!known) m = CAPS_BAD_INDEX;
    else if (caps_row_classified(b.row_ptr[r + 1] - b.row_ptr[r], pf, gf)) {
        const uint32_t np = b.row_cnt[2 * r], ng = b.row_cnt[2 * r + 1];
        xp = np > pf ? np - pf : 0u;
        xg = ng > gf ? ng - gf : 0u;
        m = CAPS_ROW_CLASSIFIED;
        if (xp || xg) m = ((xp && np > CAPS_RANK_MAX) || (xg && ng > CAPS_RANK_MAX)) ? CAPS_ROW_FALLBACK : CAPS_ROW_RANKED;
        m |= (xp ? CAPS_OVER_P : 0u) | (xg ? CAPS_OVER_G : 0u);
    }
    b.ev_cnt[2 * r] = xp;
    b.ev_cnt[2 * r + 1] = xg;
    b.mode[r] = (uint8_t)m;
    return m;
}
// pass 1c, per pair i of row r: the pairs whose fate needs no rank are settled; true = the pair is to be ranked (on the device).  The
// members of a class over its cap in a fallback row get their flag from the host
BMQ_HD bool caps_list_one(const CapsBatch& b, uint32_t i, uint32_t r) {
    const uint32_t m = b.mode[r], c = b.cls[i];
    const bool over = (c == CAPS_PERSISTENT && (m & CAPS_OVER_P)) || (c == CAPS_GROUP && (m & CAPS_OVER_G));
    b.keep[i] = c != CAPS_DEAD && !over ? 1u : 0u;
    return over && (m & 3u) == CAPS_ROW_RANKED;
}
// is pair k of the row of pair p a member of p's class with a key below p's?  (never for k == p)
BMQ_HD bool caps_below_one(const DistIndexMut& ix, const CapsBatch& b, uint32_t k, uint32_t p) {
    return k != p && b.cls[k] == b.cls[p] && order_compare(ix.kpool, ix.kref[b.ids[k]], ix.kref[b.ids[p]]) < 0;
}
// the rank of pair p of row r among the members of its class in the row (unique keys: a permutation).  The device counts them 64 at a
// time, one wave per pair (k_caps_rank)
BMQ_HD uint32_t caps_rank_one(const DistIndexMut& ix, const CapsBatch& b, uint32_t p, uint32_t r) {
    uint32_t rank = 0;
    for (uint32_t k = b.row_ptr[r]; k < b.row_ptr[r + 1]; k++) rank += caps_below_one(ix, b, k, p) ? 1u : 0u;
    return rank;
}
// where the events of class c (CAPS_PERSISTENT / CAPS_GROUP) of row r begin
BMQ_HD uint32_t caps_event_base(const CapsBatch& b, uint32_t r, uint32_t c) {
    const uint32_t s = 2 * r + (c - CAPS_PERSISTENT);
    return b.ev_scan[s] - b.ev_cnt[s];
}
// pass 2, per ranked pair p of row r: the first `cap` of its class by key survive, every other is an event {type, row, route id, max count}
BMQ_HD void caps_settle_one(const CapsBatch& b, uint32_t p, uint32_t r, uint32_t rank) {
    uint32_t pf = 0, gf = 0;
    (void)caps_of_row(b, r, pf, gf);
    const uint32_t c = b.cls[p], cap = c == CAPS_PERSISTENT ? pf : gf;
    if (rank + 1 <= cap) {
        b.keep[p] = 1u;
        return;
    }
    b.keep[p] = 0u;
    const uint32_t slot = caps_event_base(b, r, c) + (rank - cap);
    if (b.out_events && slot < b.events_cap) {
        int32_t* o = b.out_events + 4 * (size_t)slot;
        o[0] = (int32_t)(c - CAPS_PERSISTENT), o[1] = (int32_t)r, o[2] = (int32_t)b.ids[p], o[3] = (int32_t)cap;
    }
}
// pass 3 (behind the inclusive scan of keep[]), per index i < max(total, n_rows + 1): a surviving pair moves to its place, the lanes in
// front write the row offsets and the class counts as well
BMQ_HD void caps_write_one(const CapsBatch& b, uint32_t i) {
    if (i < b.total && b.keep[i]) b.out_ids[b.keep_scan[i] - 1] = b.ids[i];
    if (i > b.n_rows) return;
    const uint32_t at = b.row_ptr[i]; // (row_ptr[n_rows] == total)
    b.out_row_ptr[i] = at < b.total ? b.keep_scan[at] - b.keep[at] : (b.total ? b.keep_scan[b.total - 1] : 0u);
    if (i == b.n_rows || !b.out_class_counts) return;
    uint32_t pf = 0, gf = 0, kp = 0xFFFFFFFFu, kg = 0xFFFFFFFFu;
    (void)caps_of_row(b, i, pf, gf);
    if ((b.mode[i] & 3u) != CAPS_ROW_THROUGH) {
        kp = b.row_cnt[2 * i] < pf ? b.row_cnt[2 * i] : pf;
        kg = b.row_cnt[2 * i + 1] < gf ? b.row_cnt[2 * i + 1] : gf;
    }
    b.out_class_counts[2 * i] = kp;
    b.out_class_counts[2 * i + 1] = kg;
}

} // namespace bmq
