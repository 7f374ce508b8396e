// bmq_filter.h -- the frame of the two filters of a match CSR, the caps (bmq_caps.h) and the gate (bmq_gate.h): both classify every pair,
// settle most keep flags in a list pass, rank the members of some classes by key, and move the survivors to their places behind a scan of
// keep[].  Here: the scratch every such filter needs (the arrays of CapsBatch that are not the caps' own), the count of the survivors, and
// the ranking of a class of more than CAPS_RANK_MAX members on the host -- the keys of its members come to the host, are sorted there
// (unsigned bytes, a proper prefix first), and the keep flags of the row go back in front of the write pass.
#pragma once
#include <algorithm>
#include <string_view>
#include <vector>

#include "bmq_caps_core.h"
#include "bmq_control.h"
#include "bmq_dist_index.h"

namespace bmq {

template <class Exec> class CsrFilter : public Control<Exec> {
protected:
    using Control<Exec>::x;
    template <class T> using Scratch = typename Control<Exec>::template Scratch<T>;
    explicit CsrFilter(Exec& exec) : Control<Exec>(exec) {}

    Scratch<uint8_t> cls{*this}, mode{*this};
    Scratch<uint32_t> keep{*this}, keep_scan{*this}, work{*this}, fb_rows{*this}, ctr{*this};

    // The scratch of a batch, and the batch over it (ctr: CAPS_CTRS == GATE_CTRS words).  own_rows() ensures the filter's own per-row arrays; it
    // stays between mode[] and keep[], so that the arrays are allocated in the order they always were (profiles/post_match_refactor.json).
    template <class R>
    bool frame(CapsBatch& c, DistIndex<Exec>& ix, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, uint32_t* out_row_ptr, uint32_t* out_ids, R&& own_rows) {
        if (!this->ensure(cls, total) || !this->ensure(mode, n_rows) || !own_rows() || !this->ensure(keep, total) || !this->ensure(keep_scan, total) ||
            !this->ensure(work, total) || !this->ensure(fb_rows, n_rows) || !this->ensure(ctr, CAPS_CTRS))
            return false;
        c.row_ptr = row_ptr, c.ids = ids, c.n_rows = n_rows, c.total = total, c.id_end = ix.next_id;
        c.cls = cls, c.mode = mode, c.keep = keep, c.keep_scan = keep_scan, c.work = work, c.fb_rows = fb_rows, c.ctr = ctr;
        c.out_row_ptr = out_row_ptr, c.out_ids = out_ids;
        return true;
    }
    // behind the rank: how many ids survive, and whether out_cap holds them
    bool survivors(const CapsBatch& c, uint64_t out_cap, uint64_t& n_kept, bool& overflow) {
        uint32_t n = 0;
        if (c.total && (!x.scan_flags(c.keep, c.keep_scan, c.total) || !x.copy_out(&n, c.keep_scan + (c.total - 1), sizeof(n)))) return this->xfail();
        n_kept = n;
        overflow = n > out_cap;
        return true;
    }

    struct HostRow { // one row of the batch on the host, and the members of the class rank_class was last asked for
        std::vector<uint32_t> ids, keep, m_at, m_ids, order; // m_at / m_ids: the members' places in the row / ids; order: the members by key
        std::vector<uint8_t> cls, kb;
        std::vector<uint64_t> ko;
    };
    // The rows the list pass left to the host: f(r, row) settles the classes of row r with rank_class, then the row's keep flags go back.
    template <class F> bool host_rows(const CapsBatch& c, uint32_t n_fb, F&& f) {
        std::vector<uint32_t> rows(n_fb);
        if (!x.copy_out(rows.data(), c.fb_rows, sizeof(uint32_t) * (size_t)n_fb)) return this->xfail();
        HostRow w;
        for (const uint32_t r : rows) {
            uint32_t rp[2] = {0, 0};
            if (!x.copy_out(rp, c.row_ptr + r, sizeof(rp))) return this->xfail();
            const uint32_t n = rp[1] - rp[0];
            w.ids.resize(n), w.keep.resize(n), w.cls.resize(n);
            if (!x.copy_out(w.ids.data(), c.ids + rp[0], sizeof(uint32_t) * (size_t)n) || !x.copy_out(w.keep.data(), c.keep + rp[0], sizeof(uint32_t) * (size_t)n) ||
                !x.copy_out(w.cls.data(), c.cls + rp[0], n))
                return this->xfail();
            if (!f(r, w)) return false;
            if (!x.copy_in(c.keep + rp[0], w.keep.data(), sizeof(uint32_t) * (size_t)n)) return this->xfail();
        }
        return true;
    }
    // THE host rank: of the members of class cl in the row the first k by key survive.  w.order holds the members by key afterwards
    // (member w.order[rank] has id w.m_ids[w.order[rank]]), for what the caller reports about the others.  The classes are the device's.
    bool rank_class(DistIndex<Exec>& ix, HostRow& w, uint32_t cl, uint32_t k) {
        w.m_at.clear(), w.m_ids.clear();
        for (uint32_t i = 0; i < w.ids.size(); i++)
            if (w.cls[i] == cl) w.m_at.push_back(i), w.m_ids.push_back(w.ids[i]);
        if (!ix.route_keys(w.m_ids.data(), (uint32_t)w.m_ids.size(), w.kb, w.ko)) return this->fail(ix.error);
        auto key = [&](uint32_t j) { return std::string_view((const char*)w.kb.data() + w.ko[j], (size_t)(w.ko[j + 1] - w.ko[j])); };
        w.order.resize(w.m_ids.size());
        for (uint32_t j = 0; j < w.order.size(); j++) w.order[j] = j;
        std::sort(w.order.begin(), w.order.end(), [&](uint32_t u, uint32_t v) { return key(u) < key(v); });
        for (uint32_t rank = 0; rank < w.order.size(); rank++) w.keep[w.m_at[w.order[rank]]] = rank < k ? 1u : 0u;
        return true;
    }
};

} // namespace bmq
