// bmq_gate_core.h -- the submit-time fan-out gate of DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-231) over a whole match
// CSR: per-item functions, BMQ_HD like the other passes over device-resident state.  The gfx950 kernels over them are bmq_gate_kernels.h
// (k_gate_*), the control is bmq_gate.h; HostExec loops over the same functions.  Nothing here writes to the index.
//
// What it replaces.  Per message pack, submit() walks the pack's routes once: it admits persistent routes (subBrokerId == 1) while
// `count < MaxPersistentFanout && bytes < MaxPersistentFanoutBytes` (every admitted route adds the pack's estimated size) and the tenant has
// persistent fan-out bandwidth, transient routes while the tenant has transient fan-out bandwidth, groups up to MaxGroupFanout; it reports
// ONE event per kind and pack, meters MqttPersistentFanOutBytes per tenant, and bypasses all of it for a pack with exactly one route.
// `routes` is a concurrent hash set there, so WHICH routes fill the admitted places is unspecified; how many are admitted, which events are
// reported and what is metered depend only on the number of routes of each class (gate_row_rule).  Survivors are chosen as the caps choose
// them: the members of a class with the smallest KEYS (order_compare), in the input's order.
//
// The `break` at DeliverExecutorGroup.java:225 loses nothing: it leaves the loop once all three kinds are throttled, and a class that is
// throttled once stays throttled for the rest of the pack -- a persistent route behind it is admitted only if count < max && bytes < max
// AND bandwidth, none of which changes back; the transient bandwidth and the group count do not change back either -- so no route behind
// the break would have been sent, no event reported, and the metered bytes are those of the routes admitted before it.
//
// Unlike the caps EVERY pair is classified (caps_class_of, the same function): the meter needs the persistent count of every row.
#pragma once
#include "bmq_caps_core.h"

namespace bmq {

// out_row_flags bits (== BMQ_GATE_* of include/bmq.h)
enum : uint32_t { GATE_INLINE = 1u, GATE_P_COUNT = 2u, GATE_P_BYTES = 4u, GATE_NO_P_BANDWIDTH = 8u, GATE_NO_T_BANDWIDTH = 16u, GATE_GROUP = 32u };
// ctr[]: rows of one live route, rows of more, rows with any bit but INLINE, rows ranked on the device, rows left to the host, pairs to rank, error bits
enum : uint32_t { GATE_C_SINGLE = 0, GATE_C_GATED, GATE_C_FLAGGED, GATE_C_RANKED, GATE_C_FALLBACK, GATE_C_WORK, GATE_C_ERR, GATE_CTRS = 8 };
// where a class's count lies in row_cnt / row_keep / out_class_counts: persistent, transient, group
BMQ_HD uint32_t gate_slot_of(uint32_t c) { return c == CAPS_PERSISTENT ? 0u : (c == CAPS_TRANSIENT ? 1u : 2u); }

struct GateBatch { // every pointer: exec memory
    CapsBatch c;   // row_ptr, ids, n_rows, total, id_end, cls, mode, keep, keep_scan, work, fb_rows, ctr [GATE_CTRS], out_row_ptr, out_ids: as the caps use them
    const uint32_t* pack_bytes; // [n_rows]
    const uint32_t* row_gate;   // [n_rows] index into the table, or null: entry 0
    const int32_t *max_pf, *max_gf; // [n_gate], none negative
    const int64_t* max_pb;      // [n_gate], none negative
    const uint8_t* bw;          // [n_gate] bit 0: transient bandwidth, bit 1: persistent bandwidth
    uint32_t n_gate, inline_threshold;
    uint32_t* row_cnt;  // [3 n_rows] live members of class persistent / transient / group (zeroed before the classify)
    uint32_t* row_keep; // [3 n_rows] how many of them are kept
    uint32_t* flags;    // [n_rows]
    unsigned long long* meter_bytes; // [n_gate] (zeroed)
    uint32_t* meter_records;         // [n_gate] (zeroed)
    uint32_t *out_flags, *out_class_counts; // [n_rows], [3 n_rows] or null
    unsigned long long* out_meter_bytes;    // [n_gate]
    uint32_t* out_meter_records;            // [n_gate]
};

struct GateRow {
    uint32_t keep[3]; // persistent, transient, group routes kept
    uint32_t flags;
    unsigned long long meter; // bytes metered for the row's tenant
    uint32_t record;          // 1: the row is one summary sample of the meter (also with meter == 0)
};

// THE row rule: what submit() does to a pack of nP persistent, nT transient and nG group routes and an estimated size of s bytes under
// (pf, gf, pb, bw).  Both executors, the fallback and the emulator's mutants go through here; nothing else restates it.
BMQ_HD GateRow gate_row_rule(uint32_t nP, uint32_t nT, uint32_t nG, uint32_t s, uint32_t pf, uint32_t gf, unsigned long long pb, uint32_t bw, uint32_t inline_threshold) {
    GateRow o{};
    const unsigned long long n = (unsigned long long)nP + nT + nG;
    if (n == 0) return o;
    if (n == 1) { // routes.size() == 1: sent inline whatever the limits and the bandwidth say
        o.keep[0] = nP, o.keep[1] = nT, o.keep[2] = nG;
        o.flags = GATE_INLINE;
        o.meter = nP ? s : 0ull;
        o.record = nP;
        return o;
    }
    if (n < inline_threshold) o.flags |= GATE_INLINE;
    // persistent: admitted while count < pf && count * s < pb, so the first A = min(pf, ceil(pb / s)) of them
    unsigned long long A = pf;
    if (pb == 0) A = 0;
    else if (s != 0) {
        const unsigned long long lim = pb / s + (pb % s != 0 ? 1ull : 0ull);
        if (lim < A) A = lim;
    }
    if (bw & 2u) {
        o.keep[0] = nP < A ? nP : (uint32_t)A;
        if (nP > A) {
            if (A >= pf) o.flags |= GATE_P_COUNT;
            if (A * (unsigned long long)s >= pb) o.flags |= GATE_P_BYTES; // (A <= pf < 2^31, s < 2^32: 64 bits hold the product)
        }
    } else if (nP > 0) {
        if (pf > 0 && pb > 0) o.flags |= GATE_NO_P_BANDWIDTH;
        else o.flags |= (pf == 0 ? GATE_P_COUNT : 0u) | (pb == 0 ? GATE_P_BYTES : 0u);
    }
    if (bw & 1u) o.keep[1] = nT;
    else if (nT > 0) o.flags |= GATE_NO_T_BANDWIDTH;
    o.keep[2] = nG < gf ? nG : gf;
    if (nG > gf) o.flags |= GATE_GROUP;
    o.meter = (unsigned long long)o.keep[0] * s;
    o.record = 1;
    return o;
}

// the table entry of row r; false: its index lies outside the table
BMQ_HD bool gate_entry_of_row(const GateBatch& b, uint32_t r, uint32_t& t) {
    t = b.row_gate ? b.row_gate[r] : 0u;
    return t < b.n_gate;
}
// pass 1, per pair i: its class.  (the kernel counts the live classes per row)
BMQ_HD uint32_t gate_classify_one(const DistIndexMut& ix, const GateBatch& b, uint32_t i, uint32_t* err) { return caps_class_of(ix, b.c.ids[i], b.c.id_end, err); }

// pass 1b, per row (behind the counts of its classes): the rule, the kept counts, the flags, who ranks it.  -> mode[r] (| CAPS_BAD_INDEX);
// t / meter / record: what the row adds to the meter of its table entry
BMQ_HD uint32_t gate_row_one(const GateBatch& b, uint32_t r, uint32_t& t, unsigned long long& meter, uint32_t& record) {
    meter = 0, record = 0;
    uint32_t* cnt = b.row_cnt + 3 * (size_t)r;
    uint32_t* kp = b.row_keep + 3 * (size_t)r;
    if (!gate_entry_of_row(b, r, t)) {
        kp[0] = kp[1] = kp[2] = 0, b.flags[r] = 0, b.c.mode[r] = (uint8_t)CAPS_ROW_CLASSIFIED;
        return CAPS_BAD_INDEX;
    }
    const GateRow o = gate_row_rule(cnt[0], cnt[1], cnt[2], b.pack_bytes[r], (uint32_t)b.max_pf[t], (uint32_t)b.max_gf[t], (unsigned long long)b.max_pb[t], b.bw[t], b.inline_threshold);
    kp[0] = o.keep[0], kp[1] = o.keep[1], kp[2] = o.keep[2];
    b.flags[r] = o.flags;
    meter = o.meter, record = o.record;
    // a class is ranked when some but not all of its members stay (the transient class never: all or none)
    const bool xp = o.keep[0] > 0 && o.keep[0] < cnt[0], xg = o.keep[2] > 0 && o.keep[2] < cnt[2];
    uint32_t m = CAPS_ROW_CLASSIFIED;
    if (xp || xg) m = ((xp && cnt[0] > CAPS_RANK_MAX) || (xg && cnt[2] > CAPS_RANK_MAX)) ? CAPS_ROW_FALLBACK : CAPS_ROW_RANKED;
    m |= (xp ? CAPS_OVER_P : 0u) | (xg ? CAPS_OVER_G : 0u);
    b.c.mode[r] = (uint8_t)m;
    return m;
}
// pass 1c, per pair i of row r: the pairs whose fate needs no rank are settled; true = the pair is to be ranked (on the device).  The
// members of a ranked class in a fallback row get their flag from the host
BMQ_HD bool gate_list_one(const GateBatch& b, uint32_t i, uint32_t r) {
    const uint32_t m = b.c.mode[r], c = b.c.cls[i];
    if (c == CAPS_DEAD) {
        b.c.keep[i] = 0u;
        return false;
    }
    const bool over = (c == CAPS_PERSISTENT && (m & CAPS_OVER_P)) || (c == CAPS_GROUP && (m & CAPS_OVER_G));
    b.c.keep[i] = !over && b.row_keep[3 * (size_t)r + gate_slot_of(c)] > 0 ? 1u : 0u; // (not ranked: all of the class stay, or none)
    return over && (m & 3u) == CAPS_ROW_RANKED;
}
// the rank of pair p among the members of its class in row r: caps_rank_one / caps_rank_wave over b.c (caps_below_one compares the keys).
// pass 2, per ranked pair p of row r: the first `kept` of its class by key survive
BMQ_HD void gate_settle_one(const GateBatch& b, uint32_t p, uint32_t r, uint32_t rank) {
    b.c.keep[p] = rank + 1 <= b.row_keep[3 * (size_t)r + gate_slot_of(b.c.cls[p])] ? 1u : 0u;
}
// pass 3 (behind the inclusive scan of keep[]), per index i < max(total, n_rows + 1, n_gate): flags, kept counts and meters to the caller's
// arrays; with `rows` a surviving pair moves to its place and the lanes in front write the row offsets as well
BMQ_HD void gate_write_one(const GateBatch& b, uint32_t i, bool rows) {
    const CapsBatch& c = b.c;
    if (i < b.n_gate) {
        b.out_meter_bytes[i] = b.meter_bytes[i];
        b.out_meter_records[i] = b.meter_records[i];
    }
    if (i < c.n_rows) {
        b.out_flags[i] = b.flags[i];
        if (b.out_class_counts)
            for (uint32_t k = 0; k < 3; k++) b.out_class_counts[3 * (size_t)i + k] = b.row_keep[3 * (size_t)i + k];
    }
    if (!rows) return;
    if (i < c.total && c.keep[i]) c.out_ids[c.keep_scan[i] - 1] = c.ids[i];
    if (i > c.n_rows) return;
    const uint32_t at = c.row_ptr[i]; // (row_ptr[n_rows] == total)
    c.out_row_ptr[i] = at < c.total ? c.keep_scan[at] - c.keep[at] : (c.total ? c.keep_scan[c.total - 1] : 0u);
}

} // namespace bmq
