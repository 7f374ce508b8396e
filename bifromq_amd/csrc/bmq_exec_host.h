// bmq_exec_host.h -- HostExec: runs the builder functions of bmq_build_core.h on host threads over host memory.
// Used by host-only engines (bmq_config.device = -1: build / inspect an index without a GPU -- matching still requires
// the device) and by the sanitizer fuzzers (tools/host_fuzz.cpp runs the identical builder code under ASan/UBSan and,
// with several threads, TSan).  See bmq_dist_index.h for the Exec concept.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "bmq_build_core.h"
#include "bmq_caps_core.h"
#include "bmq_gate_core.h"
#include "bmq_delivery_core.h"
#include "bmq_fanout_core.h"
#include "bmq_order_core.h"
#include "bmq_prefix_core.h"
#include "bmq_retain_build_core.h"
#include "bmq_retain_core.h"
#include "bmq_retain_snap_core.h"
#include "bmq_rplan_core.h"
#include "bmq_share_core.h"

namespace bmq {

struct HostExec {
    std::string err;
    unsigned threads = 0; // 0 = hardware concurrency (capped)

    void* alloc(size_t bytes) { return malloc(bytes + 32); }
    void release(void* p) { free(p); }
    bool copy_in(void* d, const void* s, size_t n) {
        if (n) memcpy(d, s, n);
        return true;
    }
    bool copy_in_async(void* d, const void* s, size_t n) { return copy_in(d, s, n); }
    bool upload_async(void* d, const void* s, size_t n) { return copy_in(d, s, n); }
    bool uploads_done() { return true; }
    bool read_back_async(void*, const void*, size_t) { return true; } // (not gated: the stage-by-stage form reads after every stage)
    bool read_back_wait(void*, size_t) { return true; }
    bool copy_out(void* d, const void* s, size_t n) { return copy_in(d, s, n); }
    bool copy(void* d, const void* s, size_t n) { return copy_in(d, s, n); }
    bool zero(void* p, size_t n) {
        if (n) memset(p, 0, n);
        return true;
    }
    bool sync() { return true; }

    template <class F> void par(size_t n, F&& f) {
        unsigned hw = threads ? threads : std::min(std::thread::hardware_concurrency(), 16u);
        if (hw == 0) hw = 1;
        const size_t chunk = 256;
        const unsigned nth = (unsigned)std::min<size_t>(hw, (n + chunk - 1) / chunk);
        if (nth <= 1) {
            for (size_t i = 0; i < n; i++) f(i);
            return;
        }
        std::atomic<size_t> next{0};
        auto work = [&]() {
            for (;;) {
                const size_t b = next.fetch_add(chunk);
                if (b >= n) break;
                const size_t e = std::min(n, b + chunk);
                for (size_t i = b; i < e; i++) f(i);
            }
        };
        std::vector<std::thread> th;
        for (unsigned w = 1; w < nth; w++) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }

    bool fill_slots(TrieSlot* p, uint64_t n) {
        par(n, [&](size_t i) { p[i] = FREE_SLOT; });
        return true;
    }
    bool prepare(const DistIndexMut& ix, const OpBatch& ob) {
        par(ob.n, [&](size_t i) { prepare_one(ix, ob, (uint32_t)i); });
        return true;
    }
    static constexpr bool gated = false; // (host threads: every stage is followed by its read of the counters, there is nothing to save)
    bool gate(BuildCounters*, uint32_t) { return true; }
    bool prepare_check(const DistIndexMut& ix, const OpBatch& ob, uint32_t n_dir) {
        par(n_dir, [&](size_t d) { prepare_check_one(ix, ob, (uint32_t)d); });
        return true;
    }
    bool bulk_prepare(const DistIndexMut& ix, const OpBatch& ob) {
        par(ob.n, [&](size_t i) { bulk_prepare_one(ix, ob, (uint32_t)i); });
        return true;
    }
    bool scan_flags(const uint32_t* in, uint32_t* out, uint32_t n) { // inclusive
        uint32_t s = 0;
        for (uint32_t i = 0; i < n; i++) out[i] = (s += in[i]);
        return true;
    }
    bool bulk_tenants(const DistIndexMut& ix, const OpBatch& ob, const uint32_t* scan) {
        par(ob.n, [&](size_t i) { bulk_tenants_one(ix, ob, (uint32_t)i, scan); });
        return true;
    }
    bool bulk_counts(const OpBatch& ob, uint32_t n_ten, const uint32_t* nn_incl) {
        par(n_ten, [&](size_t t) { bulk_counts_one(ob, (uint32_t)t, n_ten, nn_incl); });
        return true;
    }
    bool locate(const DistIndexMut& ix, const OpBatch& ob) {
        if (!ob.op) {
            par(ob.n, [&](size_t i) { locate_one(ix, ob, (uint32_t)i, 2u); });
            return true;
        }
        par(ob.n, [&](size_t i) { locate_one(ix, ob, (uint32_t)i, 3u); }); // every op; a delete that finds no filter is marked
        par(ob.n, [&](size_t i) { locate_one(ix, ob, (uint32_t)i, 4u); }); // the marked deletes, behind every put of the batch
        return true;
    }
    bool sort_targets(const OpBatch& ob) {
        std::iota(ob.order, ob.order + ob.n, 0u);
        std::stable_sort(ob.order, ob.order + ob.n, [&](uint32_t a, uint32_t b) { return ob.target[a] < ob.target[b]; });
        for (uint32_t i = 0; i < ob.n; i++) ob.sorted_target[i] = ob.target[ob.order[i]];
        return true;
    }
    bool group(const DistIndexMut& ix, const OpBatch& ob) {
        par(ob.n, [&](size_t p) { group_one(ix, ob, (uint32_t)p); });
        return true;
    }
    bool rehash(const DistIndexMut& ix, uint32_t old_base, uint32_t old_slots, uint32_t new_base, uint32_t new_buckets, uint32_t d) {
        for (uint32_t pass = 0; pass < 2; pass++) par(old_slots, [&](size_t s) { rehash_one(ix, old_base, new_base, new_buckets, (uint32_t)s, pass, d); });
        return true;
    }
    bool tails(const DistIndexMut& ix, const TailPass& tp, uint32_t n_slots) {
        par(n_slots, [&](size_t g) { tail_count_one(ix, tp, (uint32_t)g); });
        par(n_slots, [&](size_t g) { tail_place_one(ix, tp, (uint32_t)g); });
        return true;
    }
    bool dict_rehash(const DictSlot* old, uint32_t old_slots, const DistIndexMut& ix) {
        par(old_slots, [&](size_t i) { dict_rehash_one(old, (uint32_t)i, ix); });
        return true;
    }
    bool find(const DistIndexMut& ix, const uint8_t* q, uint32_t tenant_len, uint32_t filter_len, uint32_t* out, uint32_t cap) {
        find_copy(ix, q, tenant_len, filter_len, out, cap);
        return true;
    }
    // out[i] = id of the live route whose key is key i of `ks`, NONE if there is none; *n_bad += malformed keys (k_b_find_keys on the device)
    bool find_keys(const DistIndexMut& ix, const KeySource& ks, uint32_t n, uint32_t* out, uint32_t* n_bad) {
        std::atomic<uint32_t> bad{0};
        par(n, [&](size_t i) {
            if (find_keys_one(ix, ks, (uint32_t)i, out)) bad.fetch_add(1, std::memory_order_relaxed);
        });
        *n_bad += bad.load();
        return true;
    }
    // ---- key-ordered window (bmq_order_core.h; k_o_* on the device): the same passes, one after the other ----
    bool o_flag(const DistIndexMut& ix, uint32_t n_ids, OrderCursor c, uint32_t* cand, uint32_t* n_cand) {
        order_cursor_resolve(ix, c);
        for (uint32_t i = 0; i < n_ids; i++)
            if (order_flag_one(ix, i, c)) cand[(*n_cand)++] = i;
        return true;
    }
    bool o_pivots(const DistIndexMut& ix, const uint32_t* list, uint32_t stride, uint32_t P, uint32_t* piv) {
        for (uint32_t j = 0; j < P; j++) piv[order_rank_one(ix, list, P, stride, j)] = list[(size_t)j * stride];
        return true;
    }
    bool o_bucket(const DistIndexMut& ix, const uint32_t* list, uint32_t n, const uint32_t* piv, uint32_t P, uint16_t* bins, uint32_t* hist) {
        par(n, [&](size_t i) { bins[i] = (uint16_t)order_bin_one(ix, list[i], piv, P); });
        for (uint32_t i = 0; i < n; i++) hist[bins[i]]++;
        return true;
    }
    bool o_scatter(const uint32_t* list, const uint16_t* bins, uint32_t n, const uint32_t* base, uint32_t* cursor, uint32_t* dst) {
        for (uint32_t i = 0; i < n; i++)
            if (base[bins[i]] != ORDER_DROP) dst[base[bins[i]] + cursor[bins[i]]++] = list[i];
        return true;
    }
    bool o_leaves(const DistIndexMut& ix, const uint32_t* list0, const uint32_t* list1, const OrderLeaf* leaves, uint32_t n_leaves, uint32_t* out) {
        par((size_t)n_leaves * ORDER_BUCKET_MAX, [&](size_t i) { // (one item per key slot of a piece: the ranking is the expensive pass)
            const OrderLeaf& lf = leaves[i / ORDER_BUCKET_MAX];
            const uint32_t j = (uint32_t)(i % ORDER_BUCKET_MAX);
            if (j < lf.n) order_leaf_one(ix, lf.list ? list1 : list0, lf, j, out);
        });
        return true;
    }
    // ---- fan-out grouping (bmq_fanout.h) ----
    static constexpr bool has_fanout_fast = false; // the counting-sort path is gfx950 kernels only; host engines take the generic passes
    bool fill_bytes(void* p, int byte, size_t n) {
        if (n) memset(p, byte, n);
        return true;
    }
    bool fo_fill(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        par(b.total, [&](size_t i) { fo_fill_one(ix, st, b, (uint32_t)i); });
        return true;
    }
    bool fo_verify(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        par(b.total, [&](size_t i) { fo_verify_one(ix, st, b, (uint32_t)i); });
        return true;
    }
    bool fo_keys(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        par(b.total, [&](size_t i) { fo_key_one(ix, st, b, (uint32_t)i); });
        return true;
    }
    bool sort_pairs32(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, int /*end_bit*/) {
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return keys_in[a] < keys_in[c]; });
        for (uint32_t i = 0; i < n; i++) {
            keys_out[i] = keys_in[order[i]];
            vals_out[i] = vals_in[order[i]];
        }
        return true;
    }
    bool fo_emit(const FanoutBatch& b) {
        par(b.total, [&](size_t j) { fo_emit_one(b, (uint32_t)j); });
        return true;
    }
    bool fo_groups(const FanoutState& st, const FanoutBatch& b) {
        par(b.total, [&](size_t j) { fo_group_one(st, b, (uint32_t)j); });
        return true;
    }
    bool gather_refs(const DistIndexMut& ix, const uint32_t* ids, uint32_t n, uint32_t id_end, unsigned long long* out) {
        par(n, [&](size_t i) { gather_ref_one(ix, ids, (uint32_t)i, id_end, out); });
        return true;
    }
    bool gather_bytes(const DistIndexMut& ix, const unsigned long long* refs, const uint64_t* offs, uint32_t n, uint8_t* out) {
        par(n, [&](size_t i) { gather_bytes_one(ix, refs, offs, (uint32_t)i, out); });
        return true;
    }
    // refs[0, n): references outside `b` lose their length bits; ctr[0] += keys inside, ctr[1] += their bytes (k_b_boundary on the device)
    bool boundary_filter(unsigned long long* refs, uint32_t n, const uint8_t* kpool, const KeyBoundary& b, unsigned long long* ctr) {
        std::atomic<unsigned long long> keys{0}, bytes{0};
        par(n, [&](size_t i) {
            if (const unsigned long long len = boundary_filter_one(kpool, refs, (uint32_t)i, b)) {
                keys.fetch_add(1, std::memory_order_relaxed);
                bytes.fetch_add(len, std::memory_order_relaxed);
            }
        });
        ctr[0] += keys.load();
        ctr[1] += bytes.load();
        return true;
    }
    // table[4 * directory slot ..] += live keys of kref[0, n) inside `b` per flag, and their bytes (k_b_census on the device)
    bool census(const DistIndexMut& ix, uint32_t n, const KeyBoundary& b, unsigned long long* table) {
        par(n, [&](size_t i) {
            uint32_t flag = 0, len = 0;
            const uint32_t d = census_key_one(ix, (uint32_t)i, b, flag, len);
            if (d == NONE) return;
            __atomic_fetch_add(table + 4 * (size_t)d + (flag - 1), 1ull, __ATOMIC_RELAXED);
            __atomic_fetch_add(table + 4 * (size_t)d + 3, (unsigned long long)len, __ATOMIC_RELAXED);
        });
        return true;
    }
    // table[4 * table slot ..] += live keys of kref[0, n) per flag, and their bytes, under the deepest prefix of T each has (k_b_prefix_census on the device)
    bool prefix_census(const DistIndexMut& ix, uint32_t n, const PrefixTable& T, unsigned long long* table) {
        par(n, [&](size_t i) {
            uint32_t flag = 0, len = 0;
            const uint32_t s = prefix_key_one(ix, (uint32_t)i, T, flag, len);
            if (s == NONE) return;
            __atomic_fetch_add(table + 4 * (size_t)s + (flag - 1), 1ull, __ATOMIC_RELAXED);
            __atomic_fetch_add(table + 4 * (size_t)s + 3, (unsigned long long)len, __ATOMIC_RELAXED);
        });
        return true;
    }
    // ---- receivers of shared subscriptions (bmq_share.h) ----
    // ---- the fan-out caps over a match CSR (bmq_caps.h): the per-item functions of bmq_caps_core.h; a row's counters belong to one thread ----
    bool caps_classify(const DistIndexMut& ix, const CapsBatch& b) { // row_cnt[] and ctr[] are zeroed before
        std::atomic<uint32_t> err{0};
        par(b.n_rows, [&](size_t r) {
            uint32_t e = 0;
            for (uint32_t i = b.row_ptr[r]; i < b.row_ptr[r + 1]; i++) {
                const uint32_t c = caps_classify_one(ix, b, i, (uint32_t)r, &e);
                b.cls[i] = (uint8_t)c;
                if (c == CAPS_PERSISTENT || c == CAPS_GROUP) b.row_cnt[2 * r + (c - CAPS_PERSISTENT)]++;
            }
            if (e) err.fetch_or(e);
        });
        b.ctr[CAPS_C_ERR] |= err.load();
        return true;
    }
    bool caps_rows(const CapsBatch& b) {
        for (uint32_t r = 0; r < b.n_rows; r++) {
            const uint32_t full = caps_row_one(b, r), m = full & 3u;
            if (full & CAPS_BAD_INDEX) b.ctr[CAPS_C_ERR] |= CAPS_ERR_INDEX;
            b.ctr[CAPS_C_CLASSIFIED] += m != CAPS_ROW_THROUGH;
            b.ctr[CAPS_C_RANKED] += m == CAPS_ROW_RANKED;
            if (m == CAPS_ROW_FALLBACK) b.fb_rows[b.ctr[CAPS_C_FALLBACK]++] = r;
        }
        return true;
    }
    bool caps_list(const CapsBatch& b) { // behind the inclusive scan of ev_cnt[]
        if (b.total == 0) return true;
        b.ctr[CAPS_C_EVENTS] = b.ev_scan[2 * (size_t)b.n_rows - 1];
        for (uint32_t r = 0; r < b.n_rows; r++)
            for (uint32_t i = b.row_ptr[r]; i < b.row_ptr[r + 1]; i++)
                if (caps_list_one(b, i, r)) b.work[b.ctr[CAPS_C_WORK]++] = i;
        return true;
    }
    bool caps_rank(const DistIndexMut& ix, const CapsBatch& b, uint32_t n_work) {
        par(n_work, [&](size_t item) {
            const uint32_t p = b.work[item], r = fo_row_of(b.row_ptr, b.n_rows, p);
            caps_settle_one(b, p, r, caps_rank_one(ix, b, p, r));
        });
        return true;
    }
    bool caps_write(const CapsBatch& b) { // behind the inclusive scan of keep[]
        par(std::max(b.total, b.n_rows + 1), [&](size_t i) { caps_write_one(b, (uint32_t)i); });
        return true;
    }
    // ---- the submit-time fan-out gate over a match CSR (bmq_gate.h): the per-item functions of bmq_gate_core.h; a row's counters belong to one thread ----
    bool gate_classify(const DistIndexMut& ix, const GateBatch& b) { // row_cnt[], ctr[] and the meters are zeroed before
        std::atomic<uint32_t> err{0};
        par(b.c.n_rows, [&](size_t r) {
            uint32_t e = 0;
            for (uint32_t i = b.c.row_ptr[r]; i < b.c.row_ptr[r + 1]; i++) {
                const uint32_t c = gate_classify_one(ix, b, i, &e);
                b.c.cls[i] = (uint8_t)c;
                if (c != CAPS_DEAD) b.row_cnt[3 * r + gate_slot_of(c)]++;
            }
            if (e) err.fetch_or(e);
        });
        b.c.ctr[GATE_C_ERR] |= err.load();
        return true;
    }
    bool gate_rows(const GateBatch& b) {
        for (uint32_t r = 0; r < b.c.n_rows; r++) {
            uint32_t t = 0, record = 0;
            unsigned long long meter = 0;
            const uint32_t full = gate_row_one(b, r, t, meter, record), m = full & 3u;
            if (full & CAPS_BAD_INDEX) {
                b.c.ctr[GATE_C_ERR] |= CAPS_ERR_INDEX;
                continue;
            }
            const uint64_t n = (uint64_t)b.row_cnt[3 * (size_t)r] + b.row_cnt[3 * (size_t)r + 1] + b.row_cnt[3 * (size_t)r + 2];
            b.c.ctr[GATE_C_SINGLE] += n == 1;
            b.c.ctr[GATE_C_GATED] += n > 1;
            b.c.ctr[GATE_C_FLAGGED] += (b.flags[r] & ~(uint32_t)GATE_INLINE) != 0;
            b.c.ctr[GATE_C_RANKED] += m == CAPS_ROW_RANKED;
            if (m == CAPS_ROW_FALLBACK) b.c.fb_rows[b.c.ctr[GATE_C_FALLBACK]++] = r;
            if (record) b.meter_bytes[t] += meter, b.meter_records[t] += record;
        }
        return true;
    }
    bool gate_list(const GateBatch& b) {
        for (uint32_t r = 0; r < b.c.n_rows; r++)
            for (uint32_t i = b.c.row_ptr[r]; i < b.c.row_ptr[r + 1]; i++)
                if (gate_list_one(b, i, r)) b.c.work[b.c.ctr[GATE_C_WORK]++] = i;
        return true;
    }
    bool gate_rank(const DistIndexMut& ix, const GateBatch& b, uint32_t n_work) {
        par(n_work, [&](size_t item) {
            const uint32_t p = b.c.work[item], r = fo_row_of(b.c.row_ptr, b.c.n_rows, p);
            gate_settle_one(b, p, r, caps_rank_one(ix, b.c, p, r));
        });
        return true;
    }
    bool gate_write(const GateBatch& b, bool rows) { // behind the inclusive scan of keep[]
        par(std::max(rows ? std::max(b.c.total, b.c.n_rows + 1) : b.c.n_rows, b.n_gate), [&](size_t i) { gate_write_one(b, (uint32_t)i, rows); });
        return true;
    }
    void mark(int) {} // (HIP-event marks of the device executor)
    float mark_ms(int, int) { return 0; }
    bool sh_count(const DistIndexMut& ix, const ShareTables& T, const ShareBatch& b) {
        par(b.n_pairs, [&](size_t i) {
            unsigned long long scores = 0;
            const unsigned long long rows = sh_count_one(ix, T, b, (uint32_t)i, scores);
            __atomic_fetch_add(b.totals, rows, __ATOMIC_RELAXED);
            __atomic_fetch_add(b.totals + 1, scores, __ATOMIC_RELAXED);
        });
        return true;
    }
    bool sh_rows(const ShareTables& T, const ShareBatch& b) {
        par(b.n_rows, [&](size_t r) { sh_row_one(T, b, (uint32_t)r); });
        return true;
    }
    bool sh_resolve(const ShareTables& T, const ShareBatch& b, uint32_t /*width*/) {
        par(b.n_rows, [&](size_t r) { sh_resolve_one(T, b, (uint32_t)r); });
        return true;
    }
    bool sh_heads(const ShareBatch& b, bool emit) {
        par(b.n_rows, [&](size_t j) {
            sh_head_one(b, (uint32_t)j);
            if (emit) sh_emit_one(b, (uint32_t)j);
        });
        return true;
    }
    bool sh_groups(const ShareTables& T, const ShareBatch& b) {
        par(b.n_rows, [&](size_t j) { sh_group_one(T, b, (uint32_t)j); });
        return true;
    }
    bool sh_rekey(uint32_t* slot_of, uint32_t id_cap, const uint32_t* new_id, const uint32_t* slot, uint32_t n) {
        par(n, [&](size_t i) { sh_rekey_one(slot_of, id_cap, new_id, slot, (uint32_t)i); });
        return true;
    }
    // ---- the delivery plan (bmq_delivery.h) ----
    bool dl_map(const DistIndexMut& ix, const FanoutState& st, const DeliveryPlan& P) { // slot_group[] is filled with DL_NONE before
        par(P.n_norm, [&](size_t g) { dl_scatter_one(st, P, (uint32_t)g); });
        par(P.n_sgroups, [&](size_t j) { dl_map_one(ix, st, P, (uint32_t)j); });
        return true;
    }
    bool dl_assign(const DeliveryPlan& P) {
        par(P.n_sgroups, [&](size_t j) { dl_assign_one(P, (uint32_t)j); });
        return true;
    }
    bool dl_count(const DeliveryPlan& P) {
        par(P.n_groups, [&](size_t g) { dl_count_one(P, (uint32_t)g); });
        return true;
    }
    bool dl_merge(const DeliveryPlan& P) {
        par(std::max(P.n_rows, P.n_groups + 1), [&](size_t i) { dl_merge_one(P, (uint32_t)i, DeliveryHint{0u, 0u, 0u}); });
        return true;
    }
    // ---- retain direction (bmq_retain_core.h) ----
    bool r_locate(const RetainMut& m, const RetainOps& ob) {
        par(ob.n, [&](size_t i) { rlocate_one(m, ob, (uint32_t)i, 0u); });
        par(ob.n, [&](size_t i) { rlocate_one(m, ob, (uint32_t)i, 1u); });
        return true;
    }
    bool r_commit(const RetainMut& m, const RetainOps& ob) {
        par(ob.n, [&](size_t i) { rcommit_one(m, ob, (uint32_t)i); });
        return true;
    }
    bool r_rank(const RetainMut& m, uint32_t n_words) {
        uint32_t run = 0;
        for (uint32_t w = 0; w < n_words; w++) {
            m.dead_rank[w] = run;
            run += (uint32_t)__builtin_popcountll(m.dead_bits[w]);
        }
        m.dead_rank[n_words] = run;
        return true;
    }
    bool r_rehash(const RetainMut& m, uint32_t n_nodes) {
        par(n_nodes, [&](size_t i) { ov_rehash_one(m, (uint32_t)i); });
        return true;
    }
    bool r_topic_lens(const RetainMut& m, const uint32_t* ids, uint32_t n, uint32_t* lens) {
        par(n, [&](size_t i) { ov_topic_len_one(m, ids, (uint32_t)i, lens); });
        return true;
    }
    bool r_topic_write(const RetainMut& m, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        par(n, [&](size_t i) { ov_topic_write_one(m, ids, (uint32_t)i, offs, out); });
        return true;
    }
    bool r_gc_select(const RetainMut& m, const GcQuery& q, uint8_t* /*flags*/, uint32_t* out_ids, uint32_t* out_count) {
        uint32_t n = 0;
        for (uint32_t id = 0; id < q.n_ids; id++)
            if (gc_flag_one(m, q, id)) out_ids[n++] = id;
        *out_count = n;
        return true;
    }
    bool r_flagged_ids(const uint8_t* flags, uint32_t n, uint32_t* out_ids, uint32_t* out_count) {
        uint32_t k = 0;
        for (uint32_t id = 0; id < n; id++)
            if (flags[id]) out_ids[k++] = id;
        *out_count = k;
        return true;
    }
    // ctr[0] += live ids of [0, n_ids) whose key lies inside `b`, ctr[1] += their key bytes if want_bytes; flags (may be null) [id] = inside
    // (k_r_boundary on the device)
    bool r_boundary(const RetainMut& m, const RetainKeyStore& ks, uint32_t n_ids, const KeyBoundary& b, uint8_t* flags, bool want_bytes, unsigned long long* ctr) {
        std::atomic<unsigned long long> topics{0}, bytes{0};
        par(n_ids, [&](size_t i) {
            if (const unsigned long long len = boundary_id_one(m, ks, (uint32_t)i, b, flags, want_bytes ? 1u : 0u)) {
                topics.fetch_add(1, std::memory_order_relaxed);
                if (want_bytes) bytes.fetch_add(len, std::memory_order_relaxed);
            }
        });
        ctr[0] += topics.load();
        ctr[1] += bytes.load();
        return true;
    }
    bool r_remove_ids(const RetainMut& m, const uint32_t* ids, uint32_t n, uint32_t n_ids) {
        par(n, [&](size_t i) { remove_id_one(m, ids, (uint32_t)i, n_ids); });
        return true;
    }
    bool r_census_bulk(const RetainMut& m, const uint32_t* ranges, uint32_t n_tenants, uint32_t* out) {
        par(n_tenants, [&](size_t t) { census_bulk_one(m, ranges, (uint32_t)t, out); });
        return true;
    }
    bool r_census(const RetainMut& m, uint32_t n_ids, unsigned long long* table) { // (k_r_census on the device)
        if (n_ids <= m.base_n) return true;
        par(n_ids - m.base_n, [&](size_t i) {
            const uint32_t tn = census_topic_one(m, m.base_n + (uint32_t)i);
            if (tn != NONE) __atomic_fetch_add(table + tn, 1ull, __ATOMIC_RELAXED);
        });
        return true;
    }
    bool r_census_pick(const unsigned long long* table, uint32_t n, unsigned long long* list, uint32_t* count) {
        par(n, [&](size_t i) { census_pick_one(table, (uint32_t)i, list, count); });
        return true;
    }
    bool r_node_lens(const RetainMut& m, const uint32_t* nodes, uint32_t n, uint32_t* lens) {
        par(n, [&](size_t i) { ov_node_len_one(m, nodes, (uint32_t)i, lens); });
        return true;
    }
    bool r_node_write(const RetainMut& m, const uint32_t* nodes, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        par(n, [&](size_t i) { ov_node_write_one(m, nodes, (uint32_t)i, offs, out); });
        return true;
    }
    bool r_key_offsets(const RetainMut& m, const RetainKeyStore& ks, const uint32_t* ids, uint32_t n, unsigned long long* lens, unsigned long long* offs) {
        par(n, [&](size_t i) { lens[i] = key_len_one(m, ks, ids[i]); });
        lens[n] = 0ull;
        unsigned long long run = 0;
        for (size_t i = 0; i <= n; i++) {
            offs[i] = run;
            run += lens[i];
        }
        return true;
    }
    bool r_key_write(const RetainMut& m, const RetainKeyStore& ks, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        par(n, [&](size_t i) { key_write_one(m, ks, ids[i], out + offs[i], offs[i + 1] - offs[i]); });
        return true;
    }
    // ---- the plan of a batch of retain ops (bmq_rplan_core.h): the passes of DevExec::rp_plan, one after the other ----
    bool rp_plan(const RetainMut& m, const RplanBatch& b, bool have_index, unsigned long long* offs) {
        par(b.n, [&](size_t i) { rp_find_one(m, b, (uint32_t)i, have_index); });
        par(b.n, [&](size_t i) { rp_group_one(b, (uint32_t)i, b.table_mask); });
        std::atomic<uint32_t> acts[4];
        for (auto& a : acts) a.store(0);
        par(b.n, [&](size_t i) {
            uint32_t dt = 0;
            int32_t dv = 0;
            const uint32_t a = rp_classify_one(b, (uint32_t)i, dt, dv);
            if (a <= RP_REMOVE) acts[a].fetch_add(1, std::memory_order_relaxed);
            if (dv) atom_add(&b.delta[dt], dv);
        });
        for (uint32_t a = 0; a < 4; a++) b.ctr[RP_C_ACTION + a] += acts[a].load();
        b.key_len[b.n] = 0ull;
        unsigned long long run = 0;
        for (size_t i = 0; i <= b.n; i++) {
            offs[i] = run;
            run += b.key_len[i];
        }
        return true;
    }
    bool rp_key_write(const RplanBatch& b, const unsigned long long* offs, uint8_t* out) {
        par(b.n, [&](size_t i) { rp_key_write_one(b, (uint32_t)i, offs, out); });
        return true;
    }
    // ---- bulk load of the retained-topic index (bmq_retain_build_core.h): one call per stage, in the order of RetainBuild::build ----
    bool rb_sort_items(const RbArgs& B) { // stable: of equal items the last one stays the last
        std::iota(B.idx, B.idx + B.n_items, 0u);
        std::stable_sort(B.idx, B.idx + B.n_items, RbItemLess{B.topics, B.topic_off, B.item_tenant});
        return true;
    }
    bool rb_fill16(void* p, uint64_t n) {
        uint32_t* q = (uint32_t*)p;
        par(n, [&](size_t i) { q[4 * i] = NONE, q[4 * i + 1] = q[4 * i + 2] = q[4 * i + 3] = 0u; });
        return true;
    }
    bool rb_iota(uint32_t* p, uint32_t n) {
        std::iota(p, p + n, 0u);
        return true;
    }
    bool sort_pairs64(const unsigned long long* keys_in, unsigned long long* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n) {
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return keys_in[a] < keys_in[c]; });
        for (uint32_t i = 0; i < n; i++) {
            keys_out[i] = keys_in[order[i]];
            vals_out[i] = vals_in[order[i]];
        }
        return true;
    }
    bool rb_keep(const RbArgs& B) {
        par(B.n_items, [&](size_t i) { rb_keep_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_rank(const RbArgs& B) {
        par(B.n_items, [&](size_t i) { rb_rank_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_shape(const RbArgs& B) {
        par(B.n_topics, [&](size_t i) { rb_shape_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_count(const RbArgs& B) {
        par(B.n_tenants, [&](size_t i) { rb_count_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_intern(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_intern_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_owner(const RbArgs& B) {
        par(B.own_mask + 1u, [&](size_t i) { rb_owner_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_place(const RbArgs& B) {
        par(B.own_mask + 1u, [&](size_t i) { rb_place_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_token(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_token_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_edge(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_edge_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_edge_overflow(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_edge_overflow_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_post_flag(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_post_flag_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_post_emit(const RbArgs& B) {
        par(B.n_nodes, [&](size_t i) { rb_post_emit_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_post_gp(const RbArgs& B) {
        par(B.n_posts, [&](size_t i) { rb_post_gp_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_post_write(const RbArgs& B) {
        par(B.n_posts, [&](size_t i) { rb_post_write_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_post_tenant(const RbArgs& B) {
        par(B.n_tenants, [&](size_t i) { rb_post_tenant_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_run_start(const RbArgs& B) {
        par(B.n_posts, [&](size_t i) { rb_run_start_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_gp(const RbArgs& B) {
        par(B.n_runs, [&](size_t i) { rb_gp_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_gp_overflow(const RbArgs& B) {
        par(B.n_runs, [&](size_t i) { rb_gp_overflow_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_tenant(const RbArgs& B) {
        par(B.n_tenants, [&](size_t i) { rb_tenant_one(B, (uint32_t)i); });
        return true;
    }
    bool rb_head(const RbArgs& B, uint32_t d) {
        par(B.n_topics, [&](size_t r) { rb_head_one(B, (uint32_t)r, d); });
        return true;
    }
    bool rb_root(const RbArgs& B, const uint32_t* S1) {
        par(B.n_tenants, [&](size_t t) { rb_root_one(B, (uint32_t)t, S1); });
        return true;
    }
    bool rb_emit(const RbArgs& B, uint32_t d, const uint32_t* Sp, const uint32_t* Sc, const uint32_t* Sn) {
        par(B.n_topics, [&](size_t r) { rb_emit_one(B, (uint32_t)r, d, Sp, Sc, Sn); });
        return true;
    }
    bool rb_close(const RbArgs& B, uint32_t d, const uint32_t* Sc, const uint32_t* Sn) {
        par(B.n_topics, [&](size_t r) { rb_close_one(B, (uint32_t)r, d, Sc, Sn); });
        return true;
    }
    bool rb_advance(const RbArgs& B, const uint32_t* Sc) {
        par(B.n_tenants, [&](size_t t) { rb_advance_one(B, (uint32_t)t, Sc); });
        return true;
    }
    bool r_find_tenant(const RetainMut& m, const uint8_t* name, uint32_t len, uint32_t* out) {
        LevelScan lv;
        unsigned long long pos = 0;
        lv.start = 0;
        scan_level_bytes<0u>(name, pos, len, lv.h, lv.inl, lv.len);
        out[0] = ov_find(m.onodes, m.oedges, m.oedge_mask, m.opool, 0u, lv.h.h1, lv.h.h2, lv.len, name, 0);
        return true;
    }
    // ---- snapshot of the retained-topic index and the next generation's per-id arrays (bmq_retain_snap_core.h) ----
    bool rs_lens(const RetainMut& m, const RetainKeyStore& ks, const RsArgs& A) { // A.totals[0] += topic bytes, [1] += bulk-loaded ids
        std::atomic<unsigned long long> bytes{0}, n_bulk{0};
        par(A.S.n, [&](size_t i) {
            bool bulk = false;
            bytes.fetch_add(rs_len_one(m, ks, A, (uint32_t)i, &bulk), std::memory_order_relaxed);
            if (bulk) n_bulk.fetch_add(1, std::memory_order_relaxed);
        });
        A.totals[0] += bytes.load();
        A.totals[1] += n_bulk.load();
        return true;
    }
    bool rs_tenant_lens(const RetainMut& m, const RsArgs& A) {
        par(A.ov_nodes, [&](size_t i) { rs_tenant_len_one(m, A, (uint32_t)i); });
        return true;
    }
    bool rs_totals(const RsArgs& A) {
        rs_totals_one(A);
        return true;
    }
    bool rs_tenants(const RetainMut& m, const RsArgs& A) {
        par(A.ov_nodes, [&](size_t i) { rs_tenant_write_one(m, A, (uint32_t)i); });
        return true;
    }
    bool rs_items(const RetainMut& m, const RsArgs& A) { // the overlay items [A.n_bulk, A.S.n)
        if (A.S.n > A.n_bulk) par(A.S.n - A.n_bulk, [&](size_t i) { rs_item_write_one(m, A, A.n_bulk + (uint32_t)i); });
        return true;
    }
    template <class SO> bool rs_gather(const RsGather<SO>& G) {
        if (G.n == 0 || G.bytes == 0) return true;
        par((size_t)((G.bytes + 15) / 16), [&](size_t c) { rs_gather_chunk(G, c, 0u, G.n); });
        return true;
    }
    bool rs_used(const uint32_t* item_tenant, uint32_t n, uint32_t* used) {
        par(n, [&](size_t i) { rs_used_one(item_tenant, used, (uint32_t)i); });
        return true;
    }
    bool rs_remap(const uint32_t* item_tenant, const uint32_t* rank_of, uint32_t* out, uint32_t n) {
        par(n, [&](size_t i) { rs_remap_one(item_tenant, rank_of, out, (uint32_t)i); });
        return true;
    }
    bool rs_perm_lens(const RsNext& N) {
        par(N.n_topics, [&](size_t r) { rs_perm_len_one(N, (uint32_t)r); });
        return true;
    }
    bool rs_next(const RsNext& N) {
        par(N.n_topics, [&](size_t r) { rs_next_one(N, (uint32_t)r); });
        return true;
    }
};

} // namespace bmq
