// bmq_gate.h -- control of the submit-time fan-out gate over a match CSR (bmq_gate_core.h) over an Exec (DevExec: the gfx950 kernels of
// bmq_gate_kernels.h on the engine stream; HostExec: host threads, for host-only engines and the CPU tests).  Besides the memory calls and
// scan_flags the Exec provides
//   bool gate_classify(ix, b), gate_rows(b), gate_list(b), gate_rank(ix, b, n_work), gate_write(b, rows)
// The control owns scratch only: nothing here outlives a call, so nothing is tied to a generation of the route index.  One read of eight
// counters separates the classify from the rank (how many pairs to rank, which rows are left to the host, whether a row names an entry
// outside the table), one word the rank from the write (how many ids survive).  Flags, kept counts and meters are made in scratch and reach
// the caller's arrays in the write pass only, so a refused call leaves them untouched.  A ranked class of more than CAPS_RANK_MAX members is
// not ranked by counting: the keys of its members come to the host, are sorted there, and the keep flags of that row go back in front of
// the write pass (as in bmq_caps.h).
#pragma once
#include <functional>
#include <string_view>

#include "bmq_dist_index.h"
#include "bmq_gate_core.h"

namespace bmq {

struct GateResult {
    uint64_t n_in = 0, n_kept = 0;
    uint32_t n_rows_single = 0, n_rows_gated = 0, n_rows_flagged = 0, n_rows_ranked = 0, n_rows_fallback = 0;
    bool overflow = false; // more ids survive than out_cap holds: flags, kept counts and meters are written, the rows are not
    float ms_classify = 0, ms_rank = 0, ms_write = 0; // when the executor's marks are on
};

struct GateTable { // every pointer: exec memory; none negative, no bw above 3 (the caller has checked)
    const int32_t *max_pf = nullptr, *max_gf = nullptr;
    const int64_t* max_pb = nullptr;
    const uint8_t* bw = nullptr;
    uint32_t n_gate = 0;
};

template <class Exec> class Gate {
public:
    explicit Gate(Exec& exec) : x(exec) {}
    ~Gate() { drop(); }
    Gate(const Gate&) = delete;
    Gate& operator=(const Gate&) = delete;

    std::string error;
    bool invalid = false;              // the last failure was the caller's input
    std::function<void()> before_free; // called before exec memory is released (a buffer that grows)

    // All pointers are exec memory.  row_ptr [n_rows + 1] with row_ptr[n_rows] == total < 2^31, ids [total]; pack_bytes [n_rows]; row_gate
    // [n_rows] or null; out_row_ptr [n_rows + 1], out_ids [out_cap], out_flags [n_rows], out_class_counts [3 n_rows] or null, out_meter_bytes /
    // out_meter_records [n_gate].
    bool run(DistIndex<Exec>& ix, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, const uint32_t* pack_bytes, const uint32_t* row_gate,
             const GateTable& T, uint32_t inline_threshold, uint32_t* out_row_ptr, uint32_t* out_ids, uint64_t out_cap, uint32_t* out_flags, uint32_t* out_class_counts,
             uint64_t* out_meter_bytes, uint32_t* out_meter_records, GateResult& res) {
        res = GateResult{};
        res.n_in = total;
        invalid = false;
        if (!ix.built) return fail("no index");
        if (!ensure(cls, cls_cap, total) || !ensure(mode, mode_cap, n_rows) || !ensure(row_cnt, cnt_cap, 3 * (size_t)n_rows) || !ensure(row_keep, rk_cap, 3 * (size_t)n_rows) ||
            !ensure(flags, fl_cap, n_rows) || !ensure(keep, keep_cap, total) || !ensure(keep_scan, ks_cap, total) || !ensure(work, work_cap, total) ||
            !ensure(fb_rows, fb_cap, n_rows) || !ensure(ctr, ctr_cap, GATE_CTRS) || !ensure(meter_bytes, mb_cap, T.n_gate) || !ensure(meter_records, mr_cap, T.n_gate))
            return false;
        GateBatch b{};
        b.c.row_ptr = row_ptr, b.c.ids = ids, b.c.n_rows = n_rows, b.c.total = total, b.c.id_end = ix.next_id;
        b.c.cls = cls, b.c.mode = mode, b.c.keep = keep, b.c.keep_scan = keep_scan, b.c.work = work, b.c.fb_rows = fb_rows, b.c.ctr = ctr;
        b.c.out_row_ptr = out_row_ptr, b.c.out_ids = out_ids;
        b.pack_bytes = pack_bytes, b.row_gate = row_gate, b.max_pf = T.max_pf, b.max_gf = T.max_gf, b.max_pb = T.max_pb, b.bw = T.bw, b.n_gate = T.n_gate;
        b.inline_threshold = inline_threshold;
        b.row_cnt = row_cnt, b.row_keep = row_keep, b.flags = flags, b.meter_bytes = meter_bytes, b.meter_records = meter_records;
        b.out_flags = out_flags, b.out_class_counts = out_class_counts, b.out_meter_bytes = (unsigned long long*)out_meter_bytes, b.out_meter_records = out_meter_records;
        const DistIndexMut im = ix.mut();
        // ---- 1. classes, per-row counts, the rule per row, the meter, who ranks what
        x.mark(17);
        uint32_t c[GATE_CTRS] = {};
        if (!x.zero(row_cnt, sizeof(uint32_t) * 3 * (size_t)n_rows) || !x.zero(ctr, sizeof(uint32_t) * GATE_CTRS) || !x.zero(meter_bytes, sizeof(unsigned long long) * (size_t)T.n_gate) ||
            !x.zero(meter_records, sizeof(uint32_t) * (size_t)T.n_gate) || !x.gate_classify(im, b) || !x.gate_rows(b) || !x.gate_list(b) || !x.copy_out(c, ctr, sizeof(c)))
            return xfail();
        if (c[GATE_C_ERR] & CAPS_ERR_INDEX) {
            invalid = true;
            return fail("row_gate: an index outside the gate table");
        }
        if (c[GATE_C_ERR] & CAPS_ERR_KEY) return fail("corrupt key store");
        res.n_rows_single = c[GATE_C_SINGLE], res.n_rows_gated = c[GATE_C_GATED], res.n_rows_flagged = c[GATE_C_FLAGGED], res.n_rows_ranked = c[GATE_C_RANKED];
        res.n_rows_fallback = c[GATE_C_FALLBACK];
        // ---- 2. the classes of which some members stay, by key
        x.mark(18);
        if (!x.gate_rank(im, b, c[GATE_C_WORK])) return xfail();
        if (c[GATE_C_FALLBACK] && !fallback(ix, b, c[GATE_C_FALLBACK])) return false;
        // ---- 3. the survivors to their places; flags, kept counts and meters to the caller
        x.mark(19);
        uint32_t n_kept = 0;
        if (total && (!x.scan_flags(keep, keep_scan, total) || !x.copy_out(&n_kept, keep_scan + (total - 1), sizeof(n_kept)))) return xfail();
        res.n_kept = n_kept;
        res.overflow = n_kept > out_cap;
        if (!x.gate_write(b, !res.overflow)) return xfail();
        x.mark(20);
        if (!x.sync()) return xfail();
        res.ms_classify = x.mark_ms(17, 18);
        res.ms_rank = x.mark_ms(18, 19);
        res.ms_write = x.mark_ms(19, 20);
        return true;
    }

    void drop() {
        rel(cls), rel(mode), rel(row_cnt), rel(row_keep), rel(flags), rel(keep), rel(keep_scan), rel(work), rel(fb_rows), rel(ctr), rel(meter_bytes), rel(meter_records);
        cls_cap = mode_cap = cnt_cap = rk_cap = fl_cap = keep_cap = ks_cap = work_cap = fb_cap = ctr_cap = mb_cap = mr_cap = 0;
    }

private:
    Exec& x;
    uint8_t *cls = nullptr, *mode = nullptr;
    uint32_t *row_cnt = nullptr, *row_keep = nullptr, *flags = nullptr, *keep = nullptr, *keep_scan = nullptr, *work = nullptr, *fb_rows = nullptr, *ctr = nullptr,
             *meter_records = nullptr;
    unsigned long long* meter_bytes = nullptr;
    size_t cls_cap = 0, mode_cap = 0, cnt_cap = 0, rk_cap = 0, fl_cap = 0, keep_cap = 0, ks_cap = 0, work_cap = 0, fb_cap = 0, ctr_cap = 0, mb_cap = 0, mr_cap = 0;

    // The rows with a ranked class of more than CAPS_RANK_MAX members: per ranked class of such a row the members' keys are sorted on the
    // host (unsigned bytes, a proper prefix first) and the first row_keep of them survive.  Classes and kept counts are the device's.
    bool fallback(DistIndex<Exec>& ix, const GateBatch& b, uint32_t n_fb) {
        std::vector<uint32_t> rows(n_fb);
        if (!x.copy_out(rows.data(), b.c.fb_rows, sizeof(uint32_t) * (size_t)n_fb)) return xfail();
        std::vector<uint32_t> r_ids, r_keep, m_at, m_ids, order;
        std::vector<uint8_t> r_cls, kb;
        std::vector<uint64_t> ko;
        for (const uint32_t r : rows) {
            uint32_t rp[2] = {0, 0}, cnt[3] = {0, 0, 0}, kp[3] = {0, 0, 0};
            if (!x.copy_out(rp, b.c.row_ptr + r, sizeof(rp)) || !x.copy_out(cnt, b.row_cnt + 3 * (size_t)r, sizeof(cnt)) || !x.copy_out(kp, b.row_keep + 3 * (size_t)r, sizeof(kp)))
                return xfail();
            const uint32_t n = rp[1] - rp[0];
            r_ids.resize(n), r_keep.resize(n), r_cls.resize(n);
            if (!x.copy_out(r_ids.data(), b.c.ids + rp[0], sizeof(uint32_t) * (size_t)n) || !x.copy_out(r_keep.data(), b.c.keep + rp[0], sizeof(uint32_t) * (size_t)n) ||
                !x.copy_out(r_cls.data(), b.c.cls + rp[0], n))
                return xfail();
            for (const uint32_t cl : {(uint32_t)CAPS_PERSISTENT, (uint32_t)CAPS_GROUP}) {
                const uint32_t s = gate_slot_of(cl);
                if (kp[s] == 0 || kp[s] >= cnt[s]) continue; // (all or none stay: settled by the list pass)
                m_at.clear(), m_ids.clear();
                for (uint32_t i = 0; i < n; i++)
                    if (r_cls[i] == cl) m_at.push_back(i), m_ids.push_back(r_ids[i]);
                if (!ix.route_keys(m_ids.data(), (uint32_t)m_ids.size(), kb, ko)) return fail(ix.error);
                auto key = [&](uint32_t j) { return std::string_view((const char*)kb.data() + ko[j], (size_t)(ko[j + 1] - ko[j])); };
                order.resize(m_ids.size());
                for (uint32_t j = 0; j < order.size(); j++) order[j] = j;
                std::sort(order.begin(), order.end(), [&](uint32_t u, uint32_t v) { return key(u) < key(v); });
                for (uint32_t rank = 0; rank < order.size(); rank++) r_keep[m_at[order[rank]]] = rank + 1 <= kp[s] ? 1u : 0u;
            }
            if (!x.copy_in(b.c.keep + rp[0], r_keep.data(), sizeof(uint32_t) * (size_t)n)) return xfail();
        }
        return true;
    }

    template <class T> void rel(T*& p) {
        if (p) x.release(p);
        p = nullptr;
    }
    bool fail(const std::string& m) {
        error = m;
        return false;
    }
    bool xfail() { return fail(x.err.empty() ? "exec failure" : x.err); }
    // grow-only scratch, contents dropped; a buffer in use by the stream is not freed under it, and the free goes through the hook
    template <class T> bool ensure(T*& p, size_t& cap, size_t need) {
        if (need <= cap && p) return true;
        if (!x.sync()) return xfail();
        if (p && before_free) before_free();
        rel(p);
        cap = 0;
        const size_t want = need + need / 4 + 64;
        p = (T*)x.alloc(want * sizeof(T) + 16);
        if (!p) return fail("out of memory");
        cap = want;
        return true;
    }
};

} // namespace bmq
