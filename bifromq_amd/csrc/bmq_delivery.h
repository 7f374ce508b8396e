// bmq_delivery.h -- control of the delivery plan (bmq_delivery_core.h) over an Exec (DevExec: gfx950 kernels on the engine stream;
// HostExec: host threads, for host-only engines and the CPU tests).  It composes the two controls before it -- Fanout<Exec>::group and
// Share<Exec>::resolve are called as they are, on the engine's own objects -- and adds the map and the merge.  Besides what those two
// need the Exec provides
//   bool dl_map(ix, st, P), dl_assign(P), dl_count(P), dl_merge(P)
// The control owns scratch only: nothing here outlives a call, so nothing is tied to a generation of the route index (the slot -> group
// scatter is filled afresh from the groups of every batch; the share-deliverer bytes belong to Share and follow its rules).
#pragma once
#include "bmq_control.h"
#include "bmq_delivery_core.h"
#include "bmq_fanout.h"
#include "bmq_share.h"

namespace bmq {

struct DeliveryResult {
    uint32_t n_rows = 0, n_share_rows = 0, n_groups = 0; // written (or needed, when one exceeds the caller's capacity)
    uint32_t n_merged_groups = 0, n_share_only_groups = 0;
    uint32_t special = 0; // bit 0: the group of unresolved shared rows is present, bit 1: the group of dead route ids (the last ones, in this order)
    bool overflow = false;
    float ms_group = 0, ms_resolve = 0, ms_map = 0, ms_merge = 0; // when the executor's marks are on
};

template <class Exec> class Delivery : public Control<Exec> {
    using C = Control<Exec>;
    using C::x, C::fail, C::xfail, C::ensure;

public:
    using C::invalid; // (here: Share says so)
    explicit Delivery(Exec& exec) : C(exec) {}

    // All pointers are exec memory.  row_ptr [n_topics + 1] with row_ptr[n_topics] == total, ids [total]; sender_off [n_topics + 1],
    // sender_hash [n_senders]; out_topic / out_route / out_aux [row_cap]; out_share_sender / out_share_member [share_cap];
    // out_group_off [group_cap + 1].
    bool plan(Fanout<Exec>& fo, Share<Exec>& sh, DistIndex<Exec>& ix, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_topics, uint32_t total,
              const uint32_t* sender_off, const uint32_t* sender_hash, uint32_t n_senders, unsigned long long nonce, uint32_t* out_topic,
              uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap,
              uint32_t* out_group_off, uint32_t group_cap, DeliveryResult& res) {
        res = DeliveryResult{};
        invalid = false;
        const uint32_t z = 0;
        if (total == 0) {
            if (!ix.built) return fail("no index");
            return x.copy_in(out_group_off, &z, sizeof(z)) ? true : xfail();
        }
        // ---- 1. the pairs by group-table slot
        x.mark(8);
        FanoutResult fr;
        for (int attempt = 0;; attempt++) {
            if (!ensure(g_topic, total) || !ensure(g_route, total) || !ensure(g_off, (size_t)fgroup_cap + 1) || !ensure(g_rep, fgroup_cap))
                return false;
            if (!fo.group(row_ptr, ids, n_topics, total, g_topic, g_route, g_off, g_rep, fgroup_cap, fr)) return fail(fo.error);
            if (!fr.group_overflow) break;
            if (attempt == 2) return fail("delivery plan: the group scratch did not converge");
            fgroup_cap = fr.n_groups + fr.n_groups / 4 + 64;
        }
        x.mark(9);
        DeliveryPlan P{};
        P.g_topic = g_topic;
        P.g_route = g_route;
        P.g_off = g_off;
        P.g_rep = g_rep;
        P.total = total;
        P.n_fgroups = fr.n_groups;
        P.has_dead = (fr.special >> 1) & 1u;
        const uint32_t has_shared = fr.special & 1u;
        P.n_norm = fr.n_groups - has_shared - P.has_dead;
        P.s0 = P.s1 = total;
        if (has_shared || P.has_dead) { // the offsets of the trailing groups: [n_norm], [n_norm + 1], [n_norm + 2] as far as they exist
            uint32_t tail[3] = {total, total, total};
            if (!x.copy_out(tail, g_off + P.n_norm, sizeof(uint32_t) * (size_t)(has_shared + P.has_dead + 1))) return xfail();
            P.s0 = tail[0];
            P.s1 = has_shared ? tail[1] : tail[0];
        }
        // ---- 2. the members of the shared slice, where it lies
        const uint32_t n_shared = P.s1 - P.s0;
        ShareResult sr;
        if (n_shared) {
            for (int attempt = 0;; attempt++) {
                if (!ensure(r_off, (size_t)sgroup_cap + 1) || !ensure(r_pair, srow_cap)) return false;
                const uint32_t cap = std::min<uint32_t>(share_cap, srow_cap);
                if (!sh.resolve(ix, g_topic + P.s0, g_route + P.s0, n_shared, sender_off, sender_hash, n_topics, n_senders, nonce, r_pair, out_share_sender,
                                out_share_member, cap, r_off, sgroup_cap, sr)) {
                    invalid = sh.invalid;
                    return fail(sh.error);
                }
                const bool more_rows = sr.n_rows > srow_cap, more_groups = sr.n_groups > sgroup_cap;
                if (!more_rows && !more_groups) break;
                if (attempt == 2) return fail("delivery plan: the share scratch did not converge");
                if (more_rows) srow_cap = sr.n_rows + sr.n_rows / 4 + 64;
                if (more_groups) sgroup_cap = sr.n_groups + sr.n_groups / 4 + 64;
            }
        }
        x.mark(10);
        P.r_pair = r_pair;
        P.r_sender = out_share_sender;
        P.r_off = r_off;
        P.r_key = sh.last_keys();
        P.n_srows = sr.n_rows;
        P.n_sgroups = sr.n_rows ? sr.n_groups : 0;
        P.n_sd = sh.n_deliverers();
        P.sd_bytes = sh.deliverer_bytes();
        P.sd_off = sh.deliverer_off();
        // ---- 3. share groups -> normal groups of the same DelivererKey, or groups of their own
        const FanoutState st = fo.state(); // (as the call above left it: a grown table, another seed)
        const uint32_t has_unres = P.n_sgroups ? (sr.special & 1u) : 0u;
        if (P.n_sgroups) {
            if (!ensure(slot_group, st.gt_cap) || !ensure(tgt, P.n_sgroups) || !ensure(is_new, P.n_sgroups) || !ensure(new_scan, P.n_sgroups))
                return false;
            P.slot_group = slot_group;
            P.tgt = tgt;
            P.is_new = is_new;
            P.new_scan = new_scan;
            if (!x.fill_bytes(slot_group, 0xFF, sizeof(uint32_t) * (size_t)st.gt_cap) || !x.dl_map(ix.mut(), st, P) || !x.scan_flags(is_new, new_scan, P.n_sgroups) ||
                !x.copy_out(&P.n_new, new_scan + (P.n_sgroups - 1), sizeof(uint32_t)))
                return xfail();
        }
        x.mark(11);
        P.n_groups = P.n_norm + P.n_new + has_unres + P.has_dead;
        P.n_rows = (total - n_shared) + P.n_srows;
        res.n_rows = P.n_rows;
        res.n_share_rows = P.n_srows;
        res.n_groups = P.n_groups;
        res.n_share_only_groups = P.n_new;
        res.n_merged_groups = P.n_sgroups - has_unres - P.n_new;
        res.special = has_unres | (P.has_dead << 1);
        if ((uint64_t)(total - n_shared) + P.n_srows >= 0x7FFFFFF0ull) return fail("more than 2^31 delivery rows in one batch");
        res.overflow = P.n_rows > row_cap || P.n_srows > share_cap || P.n_groups > group_cap;
        if (res.overflow) return true;
        if (P.n_rows == 0) return x.copy_in(out_group_off, &z, sizeof(z)) ? true : xfail(); // (ordered shares only, and no topic has a sender)
        // ---- 4. sizes, offsets, rows
        if (!ensure(share_of, P.n_groups) || !ensure(cnt, P.n_groups) || !ensure(cnt_scan, P.n_groups)) return false;
        P.share_of = share_of;
        P.cnt = cnt;
        P.cnt_scan = cnt_scan;
        P.out_topic = out_topic;
        P.out_route = out_route;
        P.out_aux = out_aux;
        P.out_group_off = out_group_off;
        if (!x.fill_bytes(share_of, 0xFF, sizeof(uint32_t) * (size_t)P.n_groups) || (P.n_sgroups && !x.dl_assign(P)) || !x.dl_count(P) ||
            !x.scan_flags(cnt, cnt_scan, P.n_groups) || !x.dl_merge(P))
            return xfail();
        x.mark(12);
        if (!x.sync()) return xfail();
        res.ms_group = x.mark_ms(8, 9);
        res.ms_resolve = x.mark_ms(9, 10);
        res.ms_map = x.mark_ms(10, 11);
        res.ms_merge = x.mark_ms(11, 12);
        return true;
    }

private:
    uint32_t fgroup_cap = 1024, sgroup_cap = 1024, srow_cap = 4096; // what the two steps are offered; grown to what they report
    typename C::template Scratch<uint32_t> g_topic{*this}, g_route{*this}, g_off{*this}, g_rep{*this}, r_pair{*this}, r_off{*this}, slot_group{*this}, tgt{*this}, is_new{*this},
        new_scan{*this}, share_of{*this}, cnt{*this}, cnt_scan{*this};
};

} // namespace bmq
