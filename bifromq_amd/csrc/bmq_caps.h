// bmq_caps.h -- control of the fan-out caps over a match CSR (bmq_caps_core.h) over an Exec (DevExec: the gfx950 kernels of
// bmq_caps_kernels.h on the engine stream; HostExec: host threads, for host-only engines and the CPU tests).  Besides the memory calls and
// scan_flags the Exec provides
//   bool caps_classify(ix, b), caps_rows(b), caps_list(b), caps_rank(ix, b, n_work), caps_write(b)
// The control owns scratch only: nothing here outlives a call, so nothing is tied to a generation of the route index.  One read of eight
// counters separates the classify from the rank (how many pairs to rank, which rows are left to the host), one word the rank from the write
// (how many ids survive).  A class of more than CAPS_RANK_MAX members over its cap is not ranked by counting: the keys of its members come
// to the host, are sorted there as cap_rows sorts a row, and the keep flags and events of that row go back in front of the write pass.
#pragma once
#include "bmq_filter.h"

namespace bmq {

struct CapsResult {
    uint64_t n_in = 0, n_kept = 0;
    uint32_t n_rows_classified = 0, n_rows_ranked = 0, n_rows_fallback = 0, n_events = 0;
    bool overflow = false; // more ids survive than out_cap holds: the events are written, the rows are not
    float ms_classify = 0, ms_rank = 0, ms_write = 0; // when the executor's marks are on
};

template <class Exec> class Caps : public CsrFilter<Exec> {
    using F = CsrFilter<Exec>;
    using F::x, F::fail, F::xfail, F::ensure;

public:
    using F::invalid;
    explicit Caps(Exec& exec) : F(exec) {}

    // All pointers but h_pf / h_gf are exec memory.  row_ptr [n_rows + 1] with row_ptr[n_rows] == total < 2^31, ids [total]; row_caps [n_rows] or
    // null; max_pf / max_gf [n_caps] and h_pf / h_gf their host copies, none negative (the caller has checked); out_row_ptr [n_rows + 1], out_ids
    // [out_cap], out_class_counts [2 n_rows] or null, out_events [4 events_cap] or null.
    bool run(DistIndex<Exec>& ix, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, const uint32_t* row_caps, const int32_t* max_pf,
             const int32_t* max_gf, uint32_t n_caps, const int32_t* h_pf, const int32_t* h_gf, uint32_t* out_row_ptr, uint32_t* out_ids, uint64_t out_cap,
             uint32_t* out_class_counts, int32_t* out_events, uint32_t events_cap, CapsResult& res) {
        res = CapsResult{};
        res.n_in = total;
        invalid = false;
        if (!ix.built) return fail("no index");
        CapsBatch b{};
        auto own_rows = [&] { return ensure(row_cnt, 2 * (size_t)n_rows) && ensure(ev_cnt, 2 * (size_t)n_rows) && ensure(ev_scan, 2 * (size_t)n_rows); };
        if (!this->frame(b, ix, row_ptr, ids, n_rows, total, out_row_ptr, out_ids, own_rows)) return false;
        b.row_caps = row_caps, b.max_pf = max_pf, b.max_gf = max_gf, b.n_caps = n_caps;
        b.row_cnt = row_cnt, b.ev_cnt = ev_cnt, b.ev_scan = ev_scan;
        b.out_class_counts = out_class_counts, b.out_events = out_events, b.events_cap = events_cap;
        const DistIndexMut im = ix.mut();
        // ---- 1. classes, per-row counts, who ranks what
        x.mark(13);
        uint32_t c[CAPS_CTRS] = {};
        if (!x.zero(row_cnt, sizeof(uint32_t) * 2 * (size_t)n_rows) || !x.zero(b.ctr, sizeof(uint32_t) * CAPS_CTRS) || !x.caps_classify(im, b) || !x.caps_rows(b) ||
            (n_rows && !x.scan_flags(ev_cnt, ev_scan, 2 * n_rows)) || !x.caps_list(b) || !x.copy_out(c, b.ctr, sizeof(c)))
            return xfail();
        if (c[CAPS_C_ERR] & CAPS_ERR_INDEX) {
            invalid = true;
            return fail("row_caps: an index outside the caps table");
        }
        if (c[CAPS_C_ERR] & CAPS_ERR_KEY) return fail("corrupt key store");
        res.n_rows_classified = c[CAPS_C_CLASSIFIED], res.n_rows_ranked = c[CAPS_C_RANKED], res.n_rows_fallback = c[CAPS_C_FALLBACK], res.n_events = c[CAPS_C_EVENTS];
        // ---- 2. the classes over their cap, by key
        x.mark(14);
        if (!x.caps_rank(im, b, c[CAPS_C_WORK])) return xfail();
        if (c[CAPS_C_FALLBACK] && !fallback(ix, b, c[CAPS_C_FALLBACK], h_pf, h_gf)) return false;
        // ---- 3. the survivors to their places
        x.mark(15);
        if (!this->survivors(b, out_cap, res.n_kept, res.overflow)) return false;
        if (!res.overflow && !x.caps_write(b)) return xfail();
        x.mark(16);
        if (!x.sync()) return xfail();
        res.ms_classify = x.mark_ms(13, 14);
        res.ms_rank = x.mark_ms(14, 15);
        res.ms_write = x.mark_ms(15, 16);
        return true;
    }

private:
    typename F::template Scratch<uint32_t> row_cnt{*this}, ev_cnt{*this}, ev_scan{*this};

    // The rows whose class over its cap has more than CAPS_RANK_MAX members: per such class the members' keys are sorted on the host (unsigned
    // bytes, a proper prefix first), the first `cap` survive, the others are its events in key order.  The classes are the device's (cls[]).
    bool fallback(DistIndex<Exec>& ix, const CapsBatch& b, uint32_t n_fb, const int32_t* h_pf, const int32_t* h_gf) {
        std::vector<int32_t> ev;
        return this->host_rows(b, n_fb, [&](uint32_t r, typename F::HostRow& w) {
            uint32_t t = 0, evc[2] = {0, 0}, evs[2] = {0, 0};
            if ((b.row_caps && !x.copy_out(&t, b.row_caps + r, sizeof(t))) || !x.copy_out(evc, b.ev_cnt + 2 * (size_t)r, sizeof(evc)) ||
                !x.copy_out(evs, b.ev_scan + 2 * (size_t)r, sizeof(evs)))
                return xfail();
            for (uint32_t k = 0; k < 2; k++) {
                if (evc[k] == 0) continue; // (within its cap: settled by the list pass)
                const uint32_t cap = (uint32_t)(k == 0 ? h_pf[t] : h_gf[t]), base = evs[k] - evc[k];
                if (!this->rank_class(ix, w, CAPS_PERSISTENT + k, cap)) return false;
                ev.clear();
                for (uint32_t rank = cap; rank < w.order.size() && b.out_events && base + (rank - cap) < b.events_cap; rank++)
                    ev.insert(ev.end(), {(int32_t)k, (int32_t)r, (int32_t)w.m_ids[w.order[rank]], (int32_t)cap});
                if (!ev.empty() && !x.copy_in(b.out_events + 4 * (size_t)base, ev.data(), sizeof(int32_t) * ev.size())) return xfail();
            }
            return true;
        });
    }
};

} // namespace bmq
