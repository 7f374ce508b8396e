// bmq_delivery_core.h -- the delivery plan of a match batch: the step behind the fan-out grouping (bmq_fanout_core.h) and the resolve of
// shared subscriptions (bmq_share_core.h).  Per-item functions, BMQ_HD like those two: gfx950 kernels in bmq_delivery_kernels.h (wired
// through bmq_exec_dev.h), host threads in bmq_exec_host.h, control in bmq_delivery.h.
//
// What it replaces.  DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-278) sends a NormalMatching straight to its deliverer and
// a GroupMatching to the member it picks -- which is a NormalMatching again, filed by DeliverExecutor.send (DW/DeliverExecutor.java:85-90)
// under the member's OWN DelivererKey(subBrokerId, delivererKey), beside the normal routes of that key (BatchDeliveryCall.add,
// BatchDeliveryCall.java:71-76: tenant -> message pack -> set of MatchInfo).  So the two lists the steps before leave behind -- the pairs of
// the normal routes grouped by a group-table slot, the rows of the chosen members grouped by a share-deliverer number -- are ONE list per
// DelivererKey.  Both are ordered by (topic, route id[, sender]) inside a group and a route is never both normal and shared, so the merge
// of two groups of the same key is two sorted lists without ties: every row goes to base + own index + rank in the other list.
//
// Which groups are the same key.  A share-deliverer number's bytes "subBrokerId NUL delivererKey" are hashed as the fan-out grouping
// hashes a route's (fo_hash, the table's CURRENT seed), the group table is probed, the slot found is turned into this batch's group through
// slot_group[] (filled from dgroup[group_rep[g]] of the groups step 1 wrote) and the bytes are compared with those of that group's
// representative route: a route of this batch, alive as of the match (the slot's first route, gt_rep, may have been deleted since and could
// then not be compared; the representative was itself verified against it when it was mapped).  A hash that is found but whose bytes differ,
// a slot without a group in this batch and a hash that is not found all give a group of its own behind the normal ones.
#pragma once
#include "bmq_fanout_core.h"
#include "bmq_share_core.h"

namespace bmq {

constexpr uint32_t DL_NONE = 0xFFFFFFFFu;
constexpr uint32_t DL_UNRESOLVED = 0xFFFFFFFEu; // tgt[j] between map and assign: the share group of the rows without a member

struct DeliveryPlan {
    // ---- step 1: the pairs ordered by (group, topic, route id); groups [0, n_norm) are normal, then the shared slice [s0, s1), then
    // (has_dead) the group of dead route ids [s1, total)
    const uint32_t *g_topic, *g_route; // [total]
    const uint32_t *g_off, *g_rep;     // [n_fgroups + 1], [n_fgroups]
    uint32_t total, n_fgroups, n_norm, s0, s1, has_dead;
    // ---- step 2: the rows of the shared slice ordered by (share-deliverer number, pair, sender)
    const uint32_t *r_pair, *r_sender; // [n_srows] pair: index into the slice
    const uint32_t* r_off;             // [n_sgroups + 1]
    const uint32_t* r_key;             // [n_srows] share-deliverer number of the sorted row; n_sd: unresolved
    uint32_t n_srows, n_sgroups, n_sd;
    const uint8_t* sd_bytes;           // "subBrokerId NUL delivererKey" of number k: [sd_off[k], sd_off[k + 1])
    const uint32_t* sd_off;
    // ---- step 3
    uint32_t* slot_group;              // [gt_cap] group-table slot -> normal group of this batch, DL_NONE
    uint32_t *tgt, *is_new, *new_scan; // [n_sgroups] final group of share group j; 1 = a group of its own; inclusive scan
    uint32_t n_new;                    // (known after the scan)
    // ---- step 4: final groups [0, n_norm) normal (+ members), [n_norm, n_norm + n_new) members only, then unresolved, then dead
    uint32_t n_groups, n_rows;
    uint32_t* share_of;                // [n_groups] share group merged into final group g, DL_NONE
    uint32_t *cnt, *cnt_scan;          // [n_groups] rows of the group, inclusive scan
    uint32_t *out_topic, *out_route, *out_aux, *out_group_off;
};

// the spans of "subBrokerId NUL delivererKey" at kp[off, end): what fo_deliverer_span finds in a receiverUrl
BMQ_HD DelivererSpan dl_sd_span(const uint8_t* kp, unsigned long long off, unsigned long long end) {
    DelivererSpan s;
    unsigned long long p = off;
    s.b0 = off;
    while (p < end && kp[p] != 0) p++;
    s.e0 = p;
    s.b2 = p < end ? p + 1 : p;
    s.e2 = end;
    return s;
}
BMQ_HD bool dl_same_deliverer(const uint8_t* ka, const DelivererSpan& a, const uint8_t* kb, const DelivererSpan& b) {
    return a.e0 - a.b0 == b.e0 - b.b0 && a.e2 - a.b2 == b.e2 - b.b2 && bytes_equal(ka, a.b0, kb, b.b0, a.e0 - a.b0) &&
           bytes_equal(ka, a.b2, kb, b.b2, a.e2 - a.b2);
}

// step 3a, one lane per normal group of the batch: its slot of the group table names it
BMQ_HD void dl_scatter_one(const FanoutState& st, const DeliveryPlan& P, uint32_t g) {
    const uint32_t rep = P.g_rep[g];
    if (rep >= st.id_cap) return;
    const uint32_t slot = st.dgroup[rep] & ~FO_NEW;
    if (slot < st.gt_cap) P.slot_group[slot] = g;
}
// step 3b, one lane per share group: the normal group of the same DelivererKey, or a group of its own
BMQ_HD void dl_map_one(const DistIndexMut& ix, const FanoutState& st, const DeliveryPlan& P, uint32_t j) {
    const uint32_t sd = P.r_key[P.r_off[j]];
    if (sd >= P.n_sd) { // rows without a member
        P.tgt[j] = DL_UNRESOLVED;
        P.is_new[j] = 0;
        return;
    }
    uint32_t g = DL_NONE;
    const DelivererSpan a = dl_sd_span(P.sd_bytes, P.sd_off[sd], P.sd_off[sd + 1]);
    if (st.gt_cap != 0 && P.n_norm != 0) {
        const unsigned long long h = fo_hash(P.sd_bytes, a, st.seed);
        const uint32_t mask = st.gt_cap - 1;
        uint32_t slot = (uint32_t)(h >> 17) & mask;
        for (uint32_t probe = 0; probe < st.gt_cap; probe++, slot = (slot + 1) & mask) {
            const unsigned long long cur = st.gt_hash[slot];
            if (cur == 0) break;
            if (cur != h) continue;
            g = P.slot_group[slot];
            break;
        }
    }
    if (g != DL_NONE) { // a 64-bit hash alone merges nothing: the bytes of the group's representative route decide
        const uint32_t rep = P.g_rep[g];
        const unsigned long long r = rep < st.id_cap ? ix.kref[rep] : 0ull;
        DelivererSpan c;
        if (r == 0 || !fo_deliverer_span(ix.kpool, r & KREF_OFF_MASK, r >> KREF_LEN_SHIFT, c) || !dl_same_deliverer(P.sd_bytes, a, ix.kpool, c)) g = DL_NONE;
    }
    P.tgt[j] = g;
    P.is_new[j] = g == DL_NONE ? 1u : 0u;
}
// step 3c (after the inclusive scan of is_new[]), one lane per share group: its final group, and the way back
BMQ_HD void dl_assign_one(const DeliveryPlan& P, uint32_t j) {
    uint32_t g = P.tgt[j];
    if (g == DL_UNRESOLVED) g = P.n_norm + P.n_new;
    else if (g == DL_NONE) g = P.n_norm + P.new_scan[j] - 1;
    P.tgt[j] = g;
    P.share_of[g] = j;
}

// the normal pairs of final group g: positions [lo, hi) of g_topic / g_route
BMQ_HD void dl_norm_range(const DeliveryPlan& P, uint32_t g, uint32_t& lo, uint32_t& hi) {
    lo = hi = 0;
    if (g < P.n_norm) lo = P.g_off[g], hi = P.g_off[g + 1];
    else if (P.has_dead && g + 1 == P.n_groups) lo = P.s1, hi = P.total;
}
// step 4a, one lane per final group: its rows
BMQ_HD void dl_count_one(const DeliveryPlan& P, uint32_t g) {
    uint32_t lo, hi;
    dl_norm_range(P, g, lo, hi);
    const uint32_t j = P.share_of[g];
    P.cnt[g] = (hi - lo) + (j == DL_NONE ? 0u : P.r_off[j + 1] - P.r_off[j]);
}

// the last k < n with off[k] <= i (off[0] == 0 <= i < off[n]; groups are never empty)
BMQ_HD uint32_t dl_group_of(const uint32_t* off, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
BMQ_HD unsigned long long dl_key(uint32_t topic, uint32_t route) { return ((unsigned long long)topic << 32) | route; }
// normal pairs of [lo, hi) in front of (topic, route).  The sender takes no part: a route is normal or shared, never both, so a pair and
// a member row never agree in (topic, route), and rows that do are neighbours in ONE list already
BMQ_HD uint32_t dl_rank_in_pairs(const DeliveryPlan& P, uint32_t lo, uint32_t hi, unsigned long long key) {
    const uint32_t first = lo;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (dl_key(P.g_topic[mid], P.g_route[mid]) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo - first;
}
// member rows of [lo, hi) in front of (topic, route)
BMQ_HD uint32_t dl_rank_in_rows(const DeliveryPlan& P, uint32_t lo, uint32_t hi, unsigned long long key) {
    const uint32_t first = lo;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t p = P.s0 + P.r_pair[mid];
        if (dl_key(P.g_topic[p], P.g_route[p]) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo - first;
}
// position in g_topic / g_route of delivery row i < n_pairs: the shared slice is left out
BMQ_HD uint32_t dl_pair_pos(const DeliveryPlan& P, uint32_t i) { return i < P.s0 ? i : i + (P.s1 - P.s0); }
// What a wave knows from its first row: group k of that row's list (kind 1: g_topic / g_route, kind 2: the member rows) ends at position
// hi.  Good for the rows AT OR BEHIND the row it was taken from -- positions ascend with the row number --: lanes are consecutive rows and
// almost always of one group, so a lane whose position lies in front of hi skips its own search (the gfx950 kernel computes the hint
// from a wave-uniform row, so its loads are scalar; host threads pass none).
struct DeliveryHint {
    uint32_t kind, hi, k;
};
BMQ_HD DeliveryHint dl_hint(const DeliveryPlan& P, uint32_t i) {
    DeliveryHint h{0u, 0u, 0u};
    if (i >= P.n_rows) return h;
    const uint32_t n_pairs = P.total - (P.s1 - P.s0);
    if (i < n_pairs) {
        const uint32_t p = dl_pair_pos(P, i);
        h.kind = 1, h.k = dl_group_of(P.g_off, P.n_fgroups, p), h.hi = P.g_off[h.k + 1];
    } else {
        h.kind = 2, h.k = dl_group_of(P.r_off, P.n_sgroups, i - n_pairs), h.hi = P.r_off[h.k + 1];
    }
    return h;
}
// step 4b (after the inclusive scan of cnt[]), one lane per delivery row -- the normal pairs first (the shared slice left out), then the
// member rows --: the row goes to base of its group + own index + rank in the other list.  Lanes i <= n_groups write the offsets too.
BMQ_HD void dl_merge_one(const DeliveryPlan& P, uint32_t i, const DeliveryHint& hint) {
    if (i <= P.n_groups) P.out_group_off[i] = i ? P.cnt_scan[i - 1] : 0u;
    if (i >= P.n_rows) return;
    const uint32_t n_pairs = P.total - (P.s1 - P.s0);
    uint32_t g, dst, topic, route, aux = DL_NONE;
    if (i < n_pairs) {
        const uint32_t p = dl_pair_pos(P, i);
        const uint32_t fg = hint.kind == 1 && p < hint.hi ? hint.k : dl_group_of(P.g_off, P.n_fgroups, p);
        g = fg < P.n_norm ? fg : P.n_groups - 1;
        topic = P.g_topic[p];
        route = P.g_route[p];
        dst = p - P.g_off[fg];
        const uint32_t j = P.share_of[g];
        if (j != DL_NONE) dst += dl_rank_in_rows(P, P.r_off[j], P.r_off[j + 1], dl_key(topic, route));
    } else {
        const uint32_t r = i - n_pairs;
        const uint32_t j = hint.kind == 2 && r < hint.hi ? hint.k : dl_group_of(P.r_off, P.n_sgroups, r);
        g = P.tgt[j];
        const uint32_t p = P.s0 + P.r_pair[r];
        topic = P.g_topic[p];
        route = P.g_route[p];
        aux = r;
        dst = r - P.r_off[j];
        uint32_t lo, hi;
        dl_norm_range(P, g, lo, hi);
        if (hi > lo) dst += dl_rank_in_pairs(P, lo, hi, dl_key(topic, route));
    }
    dst += g ? P.cnt_scan[g - 1] : 0u;
    P.out_topic[dst] = topic;
    P.out_route[dst] = route;
    P.out_aux[dst] = aux;
}

} // namespace bmq
