// bmq_share.h -- control of the shared-subscription resolve (bmq_share_core.h) over an Exec (DevExec: gfx950 kernels + hipCUB sort / scan
// on the engine stream; HostExec: host threads, for host-only engines and the CPU tests): the member tables in exec memory with their
// host mirror (the mutation path: URLs are parsed, words mixed and share-deliverer numbers handed out on the host) and the passes of a
// resolve.  Besides what the fan-out grouping needs (bmq_fanout.h) the Exec provides
//   bool sh_count(ix, T, b), sh_rows(T, b), sh_resolve(T, b, width), sh_heads(b, emit), sh_groups(T, b), sh_rekey(slot_of, id_cap, new_id, slot, n),
//        find_keys(ix, key_source, n, out_ids, n_bad); void mark(i); float mark_ms(i, j)
// Tables are keyed by route id: they belong to ONE generation of the route index and are dropped when it changes -- unless the engine
// carries them along (bmq_config.share_carry: carry_prepare / carry_finish below move each table to the id its route KEY has next).
#pragma once
#include <unordered_map>

#include "bmq_control.h"
#include "bmq_dist_index.h"
#include "bmq_share_core.h"

namespace bmq {

struct ShareResult {
    uint32_t n_rows = 0, n_groups = 0; // written (or needed, when they exceed the caller's capacities)
    uint32_t special = 0;              // bit 0: the group of unresolved rows is present (the last one)
    bool overflow = false;
};
struct ShareInfo {
    uint64_t n_tables = 0, n_members = 0, n_deliverers = 0, bytes = 0, generation = 0;
    float ms[5] = {0, 0, 0, 0, 0}; // the last resolve, when the executor's marks are on: count + scan, rows, resolve, sort, heads + scan + groups
};

template <class Exec> class Share : public Control<Exec> {
    using C = Control<Exec>;
    using C::x, C::rel, C::fail, C::bad, C::xfail;

public:
    using C::error, C::invalid, C::before_free;
    explicit Share(Exec& exec) : C(exec) {}
    ~Share() { drop(); }

    // Replaces the member lists of route_ids[0 .. n): members member_off[i] .. member_off[i + 1] of (urls, url_off); an empty list removes
    // the table.  Everything is validated before anything changes.
    bool apply(DistIndex<Exec>& ix, const uint32_t* route_ids, uint32_t n, const uint32_t* member_off, const uint8_t* urls, const uint32_t* url_off) {
        invalid = false;
        if (!ix.built) return fail("no index");
        if (!sync_generation(ix)) return false;
        if (n == 0) return true;
        // ---- validation ----
        if (member_off[0] != 0 || url_off[0] != 0) return bad("member_off[0] / url_off[0] != 0");
        for (uint32_t i = 0; i < n; i++) {
            if (member_off[i + 1] < member_off[i]) return bad("member_off not ascending");
            if (member_off[i + 1] - member_off[i] > SH_MAX_MEMBERS) return bad("more than 65535 members in one group");
        }
        const uint32_t n_urls = member_off[n];
        for (uint32_t u = 0; u < n_urls; u++) {
            if (url_off[u + 1] < url_off[u]) return bad("url_off not ascending");
            uint32_t nul = 0;
            for (uint32_t p = url_off[u]; p < url_off[u + 1]; p++) nul += urls[p] == 0;
            if (nul != 2) return bad("a member's receiverUrl must be <subBrokerId> NUL <receiverId> NUL <delivererKey>");
        }
        std::vector<uint8_t> keys;
        std::vector<uint64_t> koff;
        if (!ix.route_keys(route_ids, n, keys, koff)) return fail(ix.error);
        std::vector<uint8_t> ordered(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t len = koff[i + 1] - koff[i];
            if (route_ids[i] >= ix.next_id || len < 4) return bad("route id " + std::to_string(route_ids[i]) + " is not a live route");
            const uint8_t* k = keys.data() + koff[i];
            const uint64_t rlen = ((uint64_t)k[len - 2] << 8) | k[len - 1];
            if (rlen + 3 > len) return bad("route id " + std::to_string(route_ids[i]) + ": malformed key");
            const uint8_t flag = k[len - 3 - rlen];
            if (flag != 2 && flag != 3) return bad("route id " + std::to_string(route_ids[i]) + " is not a route of a shared subscription");
            ordered[i] = flag == 3;
        }
        // ---- the host mirror ----
        std::vector<uint32_t> changed;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t id = route_ids[i], cnt = member_off[i + 1] - member_off[i];
            auto it = tabs.find(id);
            if (it != tabs.end()) {
                n_members -= it->second.urls.size();
                if (cnt == 0) {
                    free_slots.push_back(it->second.slot);
                    tabs.erase(it);
                }
            }
            if (cnt == 0) continue;
            const bool is_new = it == tabs.end(); // (taken before the insertion, which may rehash the map)
            HostTable& t = is_new ? tabs[id] : it->second;
            if (is_new) {
                if (free_slots.empty()) t.slot = n_slots++;
                else t.slot = free_slots.back(), free_slots.pop_back();
            }
            t.ordered = ordered[i];
            t.urls.clear();
            t.sd.clear();
            t.entries = 1;
            for (uint32_t u = member_off[i]; u < member_off[i + 1]; u++) {
                std::string url((const char*)urls + url_off[u], url_off[u + 1] - url_off[u]);
                const size_t a = url.find('\0'), c = url.find('\0', a + 1);
                const std::string dk = url.substr(0, a + 1) + url.substr(c + 1); // subBrokerId NUL delivererKey (neither part holds a NUL)
                auto ins = sd_num.emplace(dk, (uint32_t)sd_num.size());
                if (ins.second) { // a new number: its bytes go to exec memory as well (upload_deliverers)
                    h_sd_bytes.insert(h_sd_bytes.end(), dk.begin(), dk.end());
                    h_sd_off.push_back((uint32_t)h_sd_bytes.size());
                }
                t.sd.push_back(ins.first->second);
                t.entries = std::max<uint32_t>(t.entries, (uint32_t)((4 + url.size() + 15) / 16));
                t.urls.push_back(std::move(url));
            }
            n_members += t.urls.size();
            changed.push_back(id);
        }
        std::sort(changed.begin(), changed.end());
        changed.erase(std::unique(changed.begin(), changed.end()), changed.end());
        changed.erase(std::remove_if(changed.begin(), changed.end(), [&](uint32_t id) { return !tabs.count(id); }), changed.end());
        if (upload(ix, changed, route_ids, n) && upload_deliverers()) return true;
        // the executor failed half-way (out of memory, a copy error): mirror and device are out of step.  Every table goes -- rows come
        // back unresolved until the caller loads them again -- rather than a directory that names memory that is not there.
        const std::string why = error;
        rel(d_slot_of);
        rel(d_desc);
        rel(d_pool64);
        rel(d_pool32);
        slot_cap = 0;
        desc_cap = cap64 = cap32 = 0;
        h_slot_of.clear();
        clear_host();
        return fail(why + " (all member tables were dropped)");
    }

    // All pointers are exec memory.  pair_topic / pair_route [n_pairs]; sender_off [n_topics + 1]; sender_hash [n_senders];
    // out_pair / out_sender / out_member [row_cap]; group_off [group_cap + 1].
    bool resolve(DistIndex<Exec>& ix, const uint32_t* pair_topic, const uint32_t* pair_route, uint32_t n_pairs, const uint32_t* sender_off,
                 const uint32_t* sender_hash, uint32_t n_topics, uint32_t n_senders, unsigned long long nonce, uint32_t* out_pair, uint32_t* out_sender,
                 uint32_t* out_member, uint32_t row_cap, uint32_t* group_off, uint32_t group_cap, ShareResult& res) {
        res = ShareResult{};
        invalid = false;
        if (!ix.built) return fail("no index");
        if (!sync_generation(ix)) return false;
        const uint32_t z = 0;
        if (n_pairs == 0) return x.copy_in(group_off, &z, sizeof(z)) ? true : xfail();
        if (n_pairs >= 0x7FFFFFF0u) return fail("more than 2^31 pairs in one batch");
        if (!flags && !fresh(flags, 4)) return false;
        if (!totals && !fresh(totals, 2)) return false;
        if (n_pairs > p_cap) {
            if (!x.sync()) return xfail();
            const size_t want = (size_t)n_pairs + n_pairs / 4 + 64;
            p_cap = 0;
            if (!fresh(s_slot, want) || !fresh(s_cnt, want) || !fresh(s_cnt_scan, want)) return false;
            p_cap = want;
        }
        ShareBatch b{};
        b.pair_topic = pair_topic;
        b.pair_route = pair_route;
        b.sender_off = sender_off;
        b.sender_hash = sender_hash;
        b.n_pairs = n_pairs;
        b.n_topics = n_topics;
        b.n_senders = n_senders;
        b.id_end = ix.next_id;
        b.nonce = nonce;
        b.slot = s_slot;
        b.totals = totals;
        b.cnt = s_cnt;
        b.cnt_scan = s_cnt_scan;
        b.out_pair = out_pair;
        b.out_sender = out_sender;
        b.out_member = out_member;
        b.group_off = group_off;
        b.row_cap = row_cap;
        b.group_cap = group_cap;
        b.flags = flags;
        const ShareTables T = tables();
        const DistIndexMut m = ix.mut();
        uint32_t n_rows = 0;
        for (float& t : last_ms) t = 0;
        x.mark(0);
        if (!x.zero(totals, 2 * sizeof(unsigned long long)) || !x.sh_count(m, T, b) || !x.scan_flags(b.cnt, b.cnt_scan, n_pairs)) return xfail();
        x.mark(6);
        unsigned long long sums[2] = {0, 0}; // rows and scores of the batch, summed in 64 bits (the 32-bit scan could wrap unseen)
        if (!x.copy_out(sums, totals, sizeof(sums))) return xfail();
        if (sums[0] >= 0x7FFFFFF0ull) return fail("more than 2^31 delivery rows in one batch");
        n_rows = (uint32_t)sums[0];
        const float ms_count = x.mark_ms(0, 6);
        res.n_rows = n_rows;
        if (n_rows == 0) return x.copy_in(group_off, &z, sizeof(z)) ? true : xfail(); // (ordered shares only, and no topic has a sender)
        if (n_rows > r_cap) {
            if (!x.sync()) return xfail();
            const size_t want = (size_t)n_rows + n_rows / 4 + 64;
            r_cap = 0;
            for (uint32_t** p : {&s_row_pair, &s_row_sender, &s_row_member, &s_key, &s_key_sorted, &s_pos, &s_pos_sorted})
                if (!fresh(*p, want)) return false;
            r_cap = want;
        }
        b.n_rows = n_rows;
        b.row_pair = s_row_pair;
        b.row_sender = s_row_sender;
        b.row_member = s_row_member;
        b.key = s_key;
        b.key_sorted = s_key_sorted;
        b.pos = s_pos;
        b.pos_sorted = s_pos_sorted;
        b.head = s_key;      // the unsorted keys are dead after the sort
        b.head_scan = s_pos; // ... and so are the unsorted positions
        int end_bit = 1;
        while (end_bit < 32 && (1u << end_bit) <= T.n_sd) end_bit++; // sort keys are <= n_sd
        // lanes per row of the resolve kernel, from THIS batch: its mean scores per row (rows without a hash -- unordered, unresolved -- count
        // as 0: they keep one lane busy whatever the width).  Most tables are small: a wave then serves 8 or 4 rows.
        const uint64_t mean = sums[1] / sums[0];
        const uint32_t width = mean <= 8 ? 8u : (mean <= 32 ? 16u : 64u);
        const bool emit = n_rows <= row_cap;
        x.mark(1);
        if (!x.sh_rows(T, b)) return xfail();
        x.mark(2);
        if (!x.sh_resolve(T, b, width)) return xfail();
        x.mark(3);
        if (!x.sort_pairs32(b.key, b.key_sorted, b.pos, b.pos_sorted, n_rows, end_bit)) return xfail();
        x.mark(4);
        if (!x.sh_heads(b, emit) || !x.scan_flags(b.head, b.head_scan, n_rows) || !x.sh_groups(T, b)) return xfail();
        x.mark(5);
        uint32_t fl[4] = {0, 0, 0, 0};
        if (!x.copy_out(fl, flags, sizeof(fl))) return xfail();
        last_ms[0] = ms_count;
        for (int i = 1; i < 5; i++) last_ms[i] = x.mark_ms(i, i + 1);
        res.n_groups = fl[0];
        res.special = fl[1];
        res.overflow = !emit || res.n_groups > group_cap;
        return true;
    }

    // a member's receiverUrl; false: no such table / member
    bool member(DistIndex<Exec>& ix, uint32_t route_id, uint32_t index, std::string& out) {
        if (!sync_generation(ix)) return false;
        auto it = tabs.find(route_id);
        if (it == tabs.end() || index >= it->second.urls.size()) return bad("no such member");
        out = it->second.urls[index];
        return true;
    }
    bool info(DistIndex<Exec>& ix, ShareInfo& out) {
        if (!sync_generation(ix)) return false;
        out.n_tables = tabs.size();
        out.n_members = n_members;
        out.n_deliverers = sd_num.size();
        out.bytes = cap64 * 8 + cap32 * 4 + (size_t)slot_cap * 4 + desc_cap * sizeof(ShareDesc) + (p_cap * 3 + r_cap * 7) * 4;
        out.generation = generation;
        for (int i = 0; i < 5; i++) out.ms[i] = last_ms[i];
        return true;
    }

    // ---- what the delivery plan (bmq_delivery.h) reads behind a resolve ------------------------------------------------------------------
    // The share-deliverer number of every SORTED row of the last resolve (group g of its output is number last_keys()[group_off[g]];
    // n_deliverers() marks the unresolved rows), and the bytes "subBrokerId NUL delivererKey" of number k in exec memory:
    // deliverer_bytes()[deliverer_off()[k] .. deliverer_off()[k + 1]).  Uploaded where the numbers are handed out (apply), kept by the carry.
    const uint32_t* last_keys() const { return s_key_sorted; }
    uint32_t n_deliverers() const { return (uint32_t)sd_num.size(); }
    const uint8_t* deliverer_bytes() const { return d_sd_bytes; }
    const uint32_t* deliverer_off() const { return d_sd_off; }

    // ---- the carry through a generation change of the route index (bmq_config.share_carry) -------------------------------------------
    // The member data -- pools, descriptors, share-deliverer numbers -- does not depend on route ids; the directory slot_of[route id] and
    // the keys of the host mirror do.  A table follows its route KEY: old id -> key reference in the old generation (gather_refs) -> id in
    // the new generation (find_keys reads the key bytes where they lie: the old generation's key pool, or -- bmq_compact rebuilds inside
    // the same object -- a copy of those keys taken before) -> one uint32 per table comes back, the mirror is re-keyed and the directory
    // rewritten by k_sh_rekey.  A table whose route is dead or has no id in the new generation is dropped.
    //   carry_prepare(old, copy_bytes)   before the generation changes; copy_bytes: `old` itself is about to be rebuilt
    //   carry_finish(next)               `next` serves from here on (old, if it is another object, is still alive)
    //   carry_cancel()                   the generation change failed before anything changed
    // A failure of the executor half-way follows the rule of apply: every table goes, and the error string says so.
    struct CarryInfo {
        uint64_t from_generation = 0, to_generation = 0, n_carried = 0, n_dropped = 0, n_members_carried = 0;
        float ms_gather = 0, ms_find = 0, ms_rekey = 0;
        uint32_t status = 0; // 0 none, 1 carried, 2 failed: every table was dropped
    } carry_info;
    bool carry_prepare(DistIndex<Exec>& old, bool copy_bytes) {
        cy = Carry{};
        if (!old.built) return true;
        if (!sync_generation(old)) return carry_failed(old.generation, 0, error);
        cy.active = true;
        cy.from = old.generation;
        for (const auto& kv : tabs) cy.ids.push_back(kv.first);
        std::sort(cy.ids.begin(), cy.ids.end());
        const uint32_t n = (uint32_t)cy.ids.size();
        if (n == 0) return true;
        cy.src = old.kpool;
        x.mark(0);
        if (!carry_buf(c_ids, c_ids_cap, n) || !carry_buf(c_refs, c_refs_cap, n) || !carry_buf(c_new, c_new_cap, (size_t)n + 1) || !carry_buf(c_slot, c_slot_cap, n))
            return carry_failed(cy.from, 0, error);
        if (!x.copy_in(c_ids, cy.ids.data(), sizeof(uint32_t) * (size_t)n) || !x.gather_refs(old.mut(), c_ids, n, old.next_id, c_refs)) return carry_failed(cy.from, 0, xerr());
        if (copy_bytes) { // the key bytes of the tables' routes into a buffer of this object: the references (8 bytes per table) visit the host for the offsets
            std::vector<unsigned long long> refs(n), moved(n);
            std::vector<uint64_t> offs((size_t)n + 1, 0);
            if (!x.copy_out(refs.data(), c_refs, sizeof(unsigned long long) * (size_t)n)) return carry_failed(cy.from, 0, xerr());
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t len = refs[i] >> KREF_LEN_SHIFT;
                moved[i] = offs[i] | (len << KREF_LEN_SHIFT);
                offs[i + 1] = offs[i] + len;
            }
            if (!carry_buf(c_offs, c_offs_cap, (size_t)n + 1) || !carry_buf(c_bytes, c_bytes_cap, offs[n] + 32)) return carry_failed(cy.from, 0, error);
            if (!x.copy_in(c_offs, offs.data(), sizeof(uint64_t) * ((size_t)n + 1)) || !x.gather_bytes(old.mut(), c_refs, c_offs, n, c_bytes) ||
                !x.copy_in(c_refs, moved.data(), sizeof(unsigned long long) * (size_t)n))
                return carry_failed(cy.from, 0, xerr());
            cy.src = c_bytes;
        }
        x.mark(1);
        if (!x.sync()) return carry_failed(cy.from, 0, xerr());
        cy.ms_gather = x.mark_ms(0, 1);
        return true;
    }
    void carry_cancel() { cy = Carry{}; }
    bool carry_finish(DistIndex<Exec>& next) {
        if (cy.failed) { // carry_prepare dropped every table: nothing of the old generation is left to drop later
            carry_info.to_generation = generation = next.generation;
            cy = Carry{};
            return false;
        }
        if (!cy.active) return true;
        Carry c = std::move(cy);
        cy = Carry{};
        CarryInfo ci;
        ci.from_generation = c.from;
        ci.to_generation = next.generation;
        ci.ms_gather = c.ms_gather;
        ci.status = 1;
        const uint32_t n = (uint32_t)c.ids.size();
        if (n != 0) {
            std::vector<uint32_t> nid((size_t)n + 1, SH_NONE);
            x.mark(2);
            if (!x.fill_bytes(c_new, 0xFF, sizeof(uint32_t) * (size_t)n) || !x.zero(c_new + n, sizeof(uint32_t))) return carry_failed(c.from, next.generation, xerr());
            if (!next.find_keys_in(x, KeySource{c.src, c_refs}, n, c_new, c_new + n)) return carry_failed(c.from, next.generation, next.error);
            x.mark(3);
            if (!x.copy_out(nid.data(), c_new, sizeof(uint32_t) * ((size_t)n + 1))) return carry_failed(c.from, next.generation, xerr());
            ci.ms_find = x.mark_ms(2, 3);
            // (nid[n]: keys the new generation's parser refused -- none: they were parsed when they went into the old one)
            // ---- the host mirror ----
            std::unordered_map<uint32_t, HostTable> moved;
            for (uint32_t i = 0; i < n; i++) {
                auto it = tabs.find(c.ids[i]);
                if (it == tabs.end()) continue;
                if (nid[i] >= next.next_id || moved.count(nid[i])) { // dead, outside the boundary of a bounded swap, or not there
                    nid[i] = SH_NONE;
                    ci.n_dropped++;
                    n_members -= it->second.urls.size();
                    free_slots.push_back(it->second.slot);
                    continue;
                }
                ci.n_carried++;
                ci.n_members_carried += it->second.urls.size();
                moved.emplace(nid[i], std::move(it->second));
            }
            tabs.swap(moved);
        }
        // ---- the directory: the new generation's id capacity, all SH_NONE, then the (new id, slot) pairs ----
        x.mark(4);
        if (!tabs.empty() || d_slot_of) {
            if (next.id_cap > slot_cap) {
                const uint32_t cap = next.id_cap + next.id_cap / 4 + 64;
                if (!fresh(d_slot_of, cap)) return carry_failed(c.from, next.generation, error);
                slot_cap = cap;
            }
            if (!x.fill_bytes(d_slot_of, 0xFF, sizeof(uint32_t) * (size_t)slot_cap)) return carry_failed(c.from, next.generation, xerr());
            h_slot_of.assign(slot_cap, SH_NONE);
        }
        if (n != 0) {
            std::vector<uint32_t> nid(n), slots(n);
            uint32_t w = 0;
            for (const auto& kv : tabs) nid[w] = kv.first, slots[w] = kv.second.slot, h_slot_of[kv.first] = kv.second.slot, w++;
            if (w != 0 && (!x.copy_in(c_new, nid.data(), sizeof(uint32_t) * (size_t)w) || !x.copy_in(c_slot, slots.data(), sizeof(uint32_t) * (size_t)w) ||
                           !x.sh_rekey(d_slot_of, slot_cap, c_new, c_slot, w)))
                return carry_failed(c.from, next.generation, xerr());
        }
        x.mark(5);
        if (!x.sync()) return carry_failed(c.from, next.generation, xerr());
        ci.ms_rekey = x.mark_ms(4, 5);
        generation = next.generation;
        carry_info = ci;
        return true;
    }

    void drop() {
        for (uint32_t** p : {&c_ids, &c_new, &c_slot}) rel(*p);
        rel(c_refs);
        rel(c_offs);
        rel(c_bytes);
        c_ids_cap = c_refs_cap = c_new_cap = c_slot_cap = c_offs_cap = c_bytes_cap = 0;
        rel(totals);
        for (uint32_t** p : {&d_slot_of, &d_pool32, &flags, &s_slot, &s_cnt, &s_cnt_scan, &s_row_pair, &s_row_sender, &s_row_member, &s_key, &s_key_sorted, &s_pos, &s_pos_sorted})
            rel(*p);
        rel(d_desc);
        rel(d_pool64);
        rel(d_sd_bytes);
        rel(d_sd_off);
        sd_bytes_cap = sd_off_cap = 0;
        slot_cap = 0;
        desc_cap = cap64 = cap32 = p_cap = r_cap = 0;
        clear_host();
    }

private:
    struct HostTable {
        uint32_t slot = 0, entries = 1;
        bool ordered = false;
        std::vector<std::string> urls;
        std::vector<uint32_t> sd;
        uint64_t off64 = 0, off32 = 0;
        uint64_t size64() const { return (uint64_t)urls.size() * (2 * entries - 1); }
        uint64_t size32() const { return (uint64_t)urls.size() * 3; }
    };
    uint64_t generation = ~0ull;
    std::unordered_map<uint32_t, HostTable> tabs;    // by route id
    std::unordered_map<std::string, uint32_t> sd_num; // subBrokerId NUL delivererKey -> share-deliverer number
    std::vector<uint32_t> h_slot_of, free_slots;
    std::vector<uint8_t> h_sd_bytes;       // the keys of sd_num, in number order ...
    std::vector<uint32_t> h_sd_off{0u};    // ... number k: [h_sd_off[k], h_sd_off[k + 1])
    size_t sd_uploaded = 0;                // numbers whose bytes are in exec memory
    std::vector<ShareDesc> h_desc;
    uint32_t n_slots = 0;
    uint64_t n_members = 0, used64 = 0, used32 = 0;
    // exec memory
    uint32_t* d_slot_of = nullptr;
    uint32_t slot_cap = 0;
    ShareDesc* d_desc = nullptr;
    unsigned long long* d_pool64 = nullptr;
    uint32_t* d_pool32 = nullptr;
    size_t desc_cap = 0, cap64 = 0, cap32 = 0;
    uint8_t* d_sd_bytes = nullptr; // share-deliverer bytes and offsets (grow-only, freed through the before_free hook)
    uint32_t* d_sd_off = nullptr;
    size_t sd_bytes_cap = 0, sd_off_cap = 0;
    uint32_t *flags = nullptr, *s_slot = nullptr, *s_cnt = nullptr, *s_cnt_scan = nullptr;
    unsigned long long* totals = nullptr;
    uint32_t *s_row_pair = nullptr, *s_row_sender = nullptr, *s_row_member = nullptr, *s_key = nullptr, *s_key_sorted = nullptr, *s_pos = nullptr, *s_pos_sorted = nullptr;
    size_t p_cap = 0, r_cap = 0;
    float last_ms[5] = {0, 0, 0, 0, 0};
    // the carry: what carry_prepare notes for carry_finish, and its exec memory -- per table its old id, its key reference, its new id
    // (+ one word: malformed keys), its slot; for bmq_compact the offsets and the bytes of the copied keys
    struct Carry {
        bool active = false, failed = false;
        uint64_t from = 0;
        std::vector<uint32_t> ids; // ascending
        const uint8_t* src = nullptr; // where the key bytes lie
        float ms_gather = 0;
    } cy;
    uint32_t *c_ids = nullptr, *c_new = nullptr, *c_slot = nullptr;
    unsigned long long* c_refs = nullptr;
    uint64_t* c_offs = nullptr;
    uint8_t* c_bytes = nullptr;
    size_t c_ids_cap = 0, c_new_cap = 0, c_slot_cap = 0, c_refs_cap = 0, c_offs_cap = 0, c_bytes_cap = 0;
    template <class T> bool carry_buf(T*& p, size_t& cap, size_t need) { // grow-only, contents dropped; freed through the before_free hook
        if (need <= cap) return true;
        cap = 0;
        if (!fresh(p, need + need / 4 + 64)) return false;
        cap = need + need / 4 + 64;
        return true;
    }
    std::string xerr() const { return x.err.empty() ? "exec failure" : x.err; }
    // the rule of apply: mirror and device may be out of step, so every table goes rather than a directory that names the wrong members
    bool carry_failed(uint64_t from, uint64_t to, const std::string& why) {
        rel(d_slot_of);
        rel(d_desc);
        rel(d_pool64);
        rel(d_pool32);
        slot_cap = 0;
        desc_cap = cap64 = cap32 = 0;
        h_slot_of.clear();
        clear_host();
        cy = Carry{};
        cy.failed = to == 0; // (carry_prepare failed: carry_finish records the generation that follows)
        carry_info = CarryInfo{};
        carry_info.from_generation = from;
        carry_info.to_generation = to;
        carry_info.status = 2;
        if (to) generation = to;
        return fail(why + " (all member tables were dropped)");
    }

    ShareTables tables() const {
        ShareTables T{};
        T.slot_of = d_slot_of;
        T.id_cap = d_slot_of ? slot_cap : 0;
        T.desc = d_desc;
        T.pool64 = d_pool64;
        T.pool32 = d_pool32;
        T.n_sd = (uint32_t)sd_num.size();
        return T;
    }
    void clear_host() {
        tabs.clear();
        sd_num.clear();
        h_sd_bytes.clear();
        h_sd_off.assign(1, 0u);
        sd_uploaded = 0;
        free_slots.clear();
        h_desc.clear();
        std::fill(h_slot_of.begin(), h_slot_of.end(), SH_NONE);
        n_slots = 0;
        n_members = used64 = used32 = 0;
    }
    // route ids are renumbered by every rebuild / compact: the tables of another generation are dropped (the buffers stay)
    bool sync_generation(DistIndex<Exec>& ix) {
        if (generation == ix.generation) return true;
        if (!x.sync()) return xfail();
        clear_host();
        if (d_slot_of && !x.fill_bytes(d_slot_of, 0xFF, sizeof(uint32_t) * (size_t)slot_cap)) return xfail();
        generation = ix.generation;
        return true;
    }
    // pre-mixed words of one table at its place in the staging of the two pools
    void lay_out(const HostTable& t, unsigned long long* w64, uint32_t* w32) const {
        const size_t n = t.urls.size();
        std::fill(w64, w64 + t.size64(), 0ull);
        for (size_t m = 0; m < n; m++) {
            const std::string& url = t.urls[m];
            const uint32_t len = (uint32_t)(4 + url.size());
            auto word = [&](size_t at) { // 8 bytes of the message [sender | url] from offset `at` >= 4, little endian, zero padded
                unsigned long long v = 0;
                for (size_t k = 0; k < 8; k++)
                    if (at + k - 4 < url.size()) v |= (unsigned long long)(uint8_t)url[at + k - 4] << (8 * k);
                return v;
            };
            w32[m] = len;
            w32[n + m] = (uint32_t)word(4);
            w32[2 * n + m] = t.sd[m];
            w64[m] = sh_mix_k2(word(8));
            for (uint32_t j = 1; j < (len + 15) / 16; j++) {
                w64[(size_t)(2 * j - 1) * n + m] = sh_mix_k1(word(16 * (size_t)j));
                w64[(size_t)(2 * j) * n + m] = sh_mix_k2(word(16 * (size_t)j + 8));
            }
        }
    }
    bool upload(DistIndex<Exec>& ix, std::vector<uint32_t>& changed, const uint32_t* route_ids, uint32_t n) {
        uint64_t need64 = 0, need32 = 0;
        for (uint32_t id : changed) need64 += tabs[id].size64(), need32 += tabs[id].size32();
        bool all = used64 + need64 > cap64 || used32 + need32 > cap32 || n_slots > desc_cap;
        if (all || ix.id_cap > slot_cap) {
            if (!x.sync()) return xfail();
        }
        if (ix.id_cap > slot_cap) { // the id space grew: a new directory, refilled from the mirror
            const uint32_t cap = ix.id_cap + ix.id_cap / 4 + 64;
            if (!fresh(d_slot_of, cap)) return false;
            slot_cap = cap;
            h_slot_of.resize(cap, SH_NONE);
            if (!x.copy_in(d_slot_of, h_slot_of.data(), sizeof(uint32_t) * (size_t)cap)) return xfail();
        }
        if (all) { // the pools are full: every live table is laid out afresh (what replaced tables left behind goes), in pools twice the live size
            changed.clear();
            uint64_t live64 = 0, live32 = 0;
            for (auto& kv : tabs) {
                changed.push_back(kv.first);
                live64 += kv.second.size64();
                live32 += kv.second.size32();
            }
            std::sort(changed.begin(), changed.end());
            if (live64 * 2 > cap64 || live64 * 8 < cap64) {
                if (!fresh(d_pool64, (size_t)live64 * 2 + 1024)) return false;
                cap64 = (size_t)live64 * 2 + 1024;
            }
            if (live32 * 2 > cap32 || live32 * 8 < cap32) {
                if (!fresh(d_pool32, (size_t)live32 * 2 + 1024)) return false;
                cap32 = (size_t)live32 * 2 + 1024;
            }
            if (n_slots > desc_cap) {
                if (!fresh(d_desc, (size_t)n_slots * 2 + 64)) return false;
                desc_cap = (size_t)n_slots * 2 + 64;
            }
            used64 = used32 = 0;
        }
        const uint64_t base64 = used64, base32 = used32;
        for (uint32_t id : changed) {
            HostTable& t = tabs[id];
            t.off64 = used64;
            t.off32 = used32;
            used64 += t.size64();
            used32 += t.size32();
        }
        std::vector<unsigned long long> st64(used64 - base64);
        std::vector<uint32_t> st32(used32 - base32);
        h_desc.resize(std::max<size_t>(h_desc.size(), n_slots));
        uint32_t slot_lo = SH_NONE, slot_hi = 0;
        for (uint32_t id : changed) {
            const HostTable& t = tabs[id];
            lay_out(t, st64.data() + (t.off64 - base64), st32.data() + (t.off32 - base32));
            ShareDesc d{};
            d.off64 = t.off64;
            d.off32 = t.off32;
            d.n = (uint32_t)t.urls.size();
            d.entries = t.entries;
            d.ordered = t.ordered ? 1u : 0u;
            h_desc[t.slot] = d;
            slot_lo = std::min(slot_lo, t.slot);
            slot_hi = std::max(slot_hi, t.slot);
        }
        if (!x.copy_in(d_pool64 + base64, st64.data(), st64.size() * 8) || !x.copy_in(d_pool32 + base32, st32.data(), st32.size() * 4)) return xfail();
        if (!changed.empty() && !x.copy_in(d_desc + slot_lo, h_desc.data() + slot_lo, sizeof(ShareDesc) * ((size_t)slot_hi - slot_lo + 1))) return xfail();
        // the directory last: the ids of this call (a removed table: SH_NONE)
        uint32_t id_lo = SH_NONE, id_hi = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t id = route_ids[i];
            auto it = tabs.find(id);
            h_slot_of[id] = it == tabs.end() ? SH_NONE : it->second.slot;
            id_lo = std::min(id_lo, id);
            id_hi = std::max(id_hi, id);
        }
        if (!x.copy_in(d_slot_of + id_lo, h_slot_of.data() + id_lo, sizeof(uint32_t) * ((size_t)id_hi - id_lo + 1))) return xfail();
        return true;
    }

    // the bytes of the share-deliverer numbers handed out since the last upload, appended (a buffer that grows is written whole)
    bool upload_deliverers() {
        const size_t n = sd_num.size();
        if (n == sd_uploaded) return true;
        size_t first = sd_uploaded;
        if (h_sd_bytes.size() > sd_bytes_cap || n + 1 > sd_off_cap) {
            if (!x.sync()) return xfail();
            if (h_sd_bytes.size() > sd_bytes_cap) {
                sd_bytes_cap = 0;
                if (!fresh(d_sd_bytes, h_sd_bytes.size() * 2 + 256)) return false;
                sd_bytes_cap = h_sd_bytes.size() * 2 + 256;
            }
            if (n + 1 > sd_off_cap) {
                sd_off_cap = 0;
                if (!fresh(d_sd_off, (n + 1) * 2 + 64)) return false;
                sd_off_cap = (n + 1) * 2 + 64;
            }
            first = 0;
        }
        const size_t b0 = h_sd_off[first];
        if (!x.copy_in(d_sd_bytes + b0, h_sd_bytes.data() + b0, h_sd_bytes.size() - b0) ||
            !x.copy_in(d_sd_off + first, h_sd_off.data() + first, sizeof(uint32_t) * (n + 1 - first)))
            return xfail();
        sd_uploaded = n;
        return true;
    }

    template <class T> bool fresh(T*& p, size_t n) {
        if (p && before_free) before_free();
        rel(p);
        p = (T*)x.alloc(n * sizeof(T) + 16);
        return p ? true : fail("out of memory");
    }
};

} // namespace bmq
