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
#include "bmq_filter.h"
#include "bmq_gate_core.h"

namespace bmq {

static_assert((uint32_t)GATE_CTRS == (uint32_t)CAPS_CTRS, "the filter frame holds one set of counters");

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

template <class Exec> class Gate : public CsrFilter<Exec> {
    using F = CsrFilter<Exec>;
    using F::x, F::fail, F::xfail, F::ensure;

public:
    using F::invalid;
    explicit Gate(Exec& exec) : F(exec) {}

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
        GateBatch b{};
        auto own_rows = [&] { return ensure(row_cnt, 3 * (size_t)n_rows) && ensure(row_keep, 3 * (size_t)n_rows) && ensure(flags, n_rows); };
        if (!this->frame(b.c, ix, row_ptr, ids, n_rows, total, out_row_ptr, out_ids, own_rows) || !ensure(meter_bytes, T.n_gate) || !ensure(meter_records, T.n_gate)) return false;
        b.pack_bytes = pack_bytes, b.row_gate = row_gate, b.max_pf = T.max_pf, b.max_gf = T.max_gf, b.max_pb = T.max_pb, b.bw = T.bw, b.n_gate = T.n_gate;
        b.inline_threshold = inline_threshold;
        b.row_cnt = row_cnt, b.row_keep = row_keep, b.flags = flags, b.meter_bytes = meter_bytes, b.meter_records = meter_records;
        b.out_flags = out_flags, b.out_class_counts = out_class_counts, b.out_meter_bytes = (unsigned long long*)out_meter_bytes, b.out_meter_records = out_meter_records;
        const DistIndexMut im = ix.mut();
        // ---- 1. classes, per-row counts, the rule per row, the meter, who ranks what
        x.mark(17);
        uint32_t c[GATE_CTRS] = {};
        if (!x.zero(row_cnt, sizeof(uint32_t) * 3 * (size_t)n_rows) || !x.zero(b.c.ctr, sizeof(uint32_t) * GATE_CTRS) || !x.zero(meter_bytes, sizeof(unsigned long long) * (size_t)T.n_gate) ||
            !x.zero(meter_records, sizeof(uint32_t) * (size_t)T.n_gate) || !x.gate_classify(im, b) || !x.gate_rows(b) || !x.gate_list(b) || !x.copy_out(c, b.c.ctr, sizeof(c)))
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
        if (!this->survivors(b.c, out_cap, res.n_kept, res.overflow)) return false;
        if (!x.gate_write(b, !res.overflow)) return xfail();
        x.mark(20);
        if (!x.sync()) return xfail();
        res.ms_classify = x.mark_ms(17, 18);
        res.ms_rank = x.mark_ms(18, 19);
        res.ms_write = x.mark_ms(19, 20);
        return true;
    }

private:
    typename F::template Scratch<uint32_t> row_cnt{*this}, row_keep{*this}, flags{*this}, meter_records{*this};
    typename F::template Scratch<unsigned long long> meter_bytes{*this};

    // The rows with a ranked class of more than CAPS_RANK_MAX members: per ranked class of such a row the members' keys are sorted on the
    // host (unsigned bytes, a proper prefix first) and the first row_keep of them survive.  Classes and kept counts are the device's.
    bool fallback(DistIndex<Exec>& ix, const GateBatch& b, uint32_t n_fb) {
        return this->host_rows(b.c, n_fb, [&](uint32_t r, typename F::HostRow& w) {
            uint32_t cnt[3] = {0, 0, 0}, kp[3] = {0, 0, 0};
            if (!x.copy_out(cnt, b.row_cnt + 3 * (size_t)r, sizeof(cnt)) || !x.copy_out(kp, b.row_keep + 3 * (size_t)r, sizeof(kp))) return xfail();
            for (const uint32_t cl : {(uint32_t)CAPS_PERSISTENT, (uint32_t)CAPS_GROUP}) {
                const uint32_t s = gate_slot_of(cl);
                if (kp[s] == 0 || kp[s] >= cnt[s]) continue; // (all or none stay: settled by the list pass)
                if (!this->rank_class(ix, w, cl, kp[s])) return false;
            }
            return true;
        });
    }
};

} // namespace bmq
