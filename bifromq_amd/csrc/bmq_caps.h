// bmq_caps.h -- control of the fan-out caps over a match CSR (bmq_caps_core.h) over an Exec (DevExec: the gfx950 kernels of
// bmq_caps_kernels.h on the engine stream; HostExec: host threads, for host-only engines and the CPU tests).  Besides the memory calls and
// scan_flags the Exec provides
//   bool caps_classify(ix, b), caps_rows(b), caps_list(b), caps_rank(ix, b, n_work), caps_write(b)
// The control owns scratch only: nothing here outlives a call, so nothing is tied to a generation of the route index.  One read of eight
// counters separates the classify from the rank (how many pairs to rank, which rows are left to the host), one word the rank from the write
// (how many ids survive).  A class of more than CAPS_RANK_MAX members over its cap is not ranked by counting: the keys of its members come
// to the host, are sorted there as cap_rows sorts a row, and the keep flags and events of that row go back in front of the write pass.
#pragma once
#include <functional>
#include <string_view>

#include "bmq_caps_core.h"
#include "bmq_dist_index.h"

namespace bmq {

struct CapsResult {
    uint64_t n_in = 0, n_kept = 0;
    uint32_t n_rows_classified = 0, n_rows_ranked = 0, n_rows_fallback = 0, n_events = 0;
    bool overflow = false; // more ids survive than out_cap holds: the events are written, the rows are not
    float ms_classify = 0, ms_rank = 0, ms_write = 0; // when the executor's marks are on
};

template <class Exec> class Caps {
public:
    explicit Caps(Exec& exec) : x(exec) {}
    ~Caps() { drop(); }
    Caps(const Caps&) = delete;
    Caps& operator=(const Caps&) = delete;

    std::string error;
    bool invalid = false;              // the last failure was the caller's input
    std::function<void()> before_free; // called before exec memory is released (a buffer that grows)

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
        if (!ensure(cls, cls_cap, total) || !ensure(mode, mode_cap, n_rows) || !ensure(row_cnt, cnt_cap, 2 * (size_t)n_rows) || !ensure(ev_cnt, evc_cap, 2 * (size_t)n_rows) ||
            !ensure(ev_scan, evs_cap, 2 * (size_t)n_rows) || !ensure(keep, keep_cap, total) || !ensure(keep_scan, ks_cap, total) || !ensure(work, work_cap, total) ||
            !ensure(fb_rows, fb_cap, n_rows) || !ensure(ctr, ctr_cap, CAPS_CTRS))
            return false;
        CapsBatch b{};
        b.row_ptr = row_ptr, b.ids = ids, b.n_rows = n_rows, b.total = total, b.id_end = ix.next_id;
        b.row_caps = row_caps, b.max_pf = max_pf, b.max_gf = max_gf, b.n_caps = n_caps;
        b.cls = cls, b.mode = mode, b.row_cnt = row_cnt, b.ev_cnt = ev_cnt, b.ev_scan = ev_scan, b.keep = keep, b.keep_scan = keep_scan, b.work = work, b.fb_rows = fb_rows;
        b.ctr = ctr;
        b.out_row_ptr = out_row_ptr, b.out_ids = out_ids, b.out_class_counts = out_class_counts, b.out_events = out_events, b.events_cap = events_cap;
        const DistIndexMut im = ix.mut();
        // ---- 1. classes, per-row counts, who ranks what
        x.mark(13);
        uint32_t c[CAPS_CTRS] = {};
        if (!x.zero(row_cnt, sizeof(uint32_t) * 2 * (size_t)n_rows) || !x.zero(ctr, sizeof(uint32_t) * CAPS_CTRS) || !x.caps_classify(im, b) || !x.caps_rows(b) ||
            (n_rows && !x.scan_flags(ev_cnt, ev_scan, 2 * n_rows)) || !x.caps_list(b) || !x.copy_out(c, ctr, sizeof(c)))
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
        uint32_t n_kept = 0;
        if (total && (!x.scan_flags(keep, keep_scan, total) || !x.copy_out(&n_kept, keep_scan + (total - 1), sizeof(n_kept)))) return xfail();
        res.n_kept = n_kept;
        res.overflow = n_kept > out_cap;
        if (!res.overflow && !x.caps_write(b)) return xfail();
        x.mark(16);
        if (!x.sync()) return xfail();
        res.ms_classify = x.mark_ms(13, 14);
        res.ms_rank = x.mark_ms(14, 15);
        res.ms_write = x.mark_ms(15, 16);
        return true;
    }

    void drop() {
        rel(cls), rel(mode), rel(row_cnt), rel(ev_cnt), rel(ev_scan), rel(keep), rel(keep_scan), rel(work), rel(fb_rows), rel(ctr);
        cls_cap = mode_cap = cnt_cap = evc_cap = evs_cap = keep_cap = ks_cap = work_cap = fb_cap = ctr_cap = 0;
    }

private:
    Exec& x;
    uint8_t *cls = nullptr, *mode = nullptr;
    uint32_t *row_cnt = nullptr, *ev_cnt = nullptr, *ev_scan = nullptr, *keep = nullptr, *keep_scan = nullptr, *work = nullptr, *fb_rows = nullptr, *ctr = nullptr;
    size_t cls_cap = 0, mode_cap = 0, cnt_cap = 0, evc_cap = 0, evs_cap = 0, keep_cap = 0, ks_cap = 0, work_cap = 0, fb_cap = 0, ctr_cap = 0;

    // The rows whose class over its cap has more than CAPS_RANK_MAX members: per such class the members' keys are sorted on the host (unsigned
    // bytes, a proper prefix first), the first `cap` survive, the others are its events in key order.  The classes are the device's (cls[]).
    bool fallback(DistIndex<Exec>& ix, const CapsBatch& b, uint32_t n_fb, const int32_t* h_pf, const int32_t* h_gf) {
        std::vector<uint32_t> rows(n_fb);
        if (!x.copy_out(rows.data(), b.fb_rows, sizeof(uint32_t) * (size_t)n_fb)) return xfail();
        std::vector<uint32_t> r_ids, r_keep, m_at, m_ids, order;
        std::vector<uint8_t> r_cls, kb;
        std::vector<uint64_t> ko;
        std::vector<int32_t> ev;
        for (const uint32_t r : rows) {
            uint32_t rp[2] = {0, 0}, t = 0, evc[2] = {0, 0}, evs[2] = {0, 0};
            if (!x.copy_out(rp, b.row_ptr + r, sizeof(rp)) || (b.row_caps && !x.copy_out(&t, b.row_caps + r, sizeof(t))) ||
                !x.copy_out(evc, b.ev_cnt + 2 * (size_t)r, sizeof(evc)) || !x.copy_out(evs, b.ev_scan + 2 * (size_t)r, sizeof(evs)))
                return xfail();
            const uint32_t n = rp[1] - rp[0];
            r_ids.resize(n), r_keep.resize(n), r_cls.resize(n);
            if (!x.copy_out(r_ids.data(), b.ids + rp[0], sizeof(uint32_t) * (size_t)n) || !x.copy_out(r_keep.data(), b.keep + rp[0], sizeof(uint32_t) * (size_t)n) ||
                !x.copy_out(r_cls.data(), b.cls + rp[0], n))
                return xfail();
            for (uint32_t k = 0; k < 2; k++) {
                if (evc[k] == 0) continue; // (within its cap: settled by the list pass)
                const uint32_t cap = (uint32_t)(k == 0 ? h_pf[t] : h_gf[t]), base = evs[k] - evc[k];
                m_at.clear(), m_ids.clear();
                for (uint32_t i = 0; i < n; i++)
                    if (r_cls[i] == CAPS_PERSISTENT + k) m_at.push_back(i), m_ids.push_back(r_ids[i]);
                if (!ix.route_keys(m_ids.data(), (uint32_t)m_ids.size(), kb, ko)) return fail(ix.error);
                auto key = [&](uint32_t j) { return std::string_view((const char*)kb.data() + ko[j], (size_t)(ko[j + 1] - ko[j])); };
                order.resize(m_ids.size());
                for (uint32_t j = 0; j < order.size(); j++) order[j] = j;
                std::sort(order.begin(), order.end(), [&](uint32_t u, uint32_t v) { return key(u) < key(v); });
                ev.clear();
                for (uint32_t rank = 0; rank < order.size(); rank++) {
                    const uint32_t j = order[rank];
                    r_keep[m_at[j]] = rank + 1 <= cap ? 1u : 0u;
                    if (rank + 1 > cap && b.out_events && base + (rank - cap) < b.events_cap)
                        ev.insert(ev.end(), {(int32_t)k, (int32_t)r, (int32_t)m_ids[j], (int32_t)cap});
                }
                if (!ev.empty() && !x.copy_in(b.out_events + 4 * (size_t)base, ev.data(), sizeof(int32_t) * ev.size())) return xfail();
            }
            if (!x.copy_in(b.keep + rp[0], r_keep.data(), sizeof(uint32_t) * (size_t)n)) return xfail();
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
