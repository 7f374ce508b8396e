// bmq_retain_dyn.h -- control of the MUTABLE part of the retained-topic index (bmq_retain_core.h): owns the per-id arrays, the dead
// bitmap and the overlay trie in exec memory (HBM under DevExec, host memory under HostExec), sizes them ahead of every batch so that
// no lane can run out of room, and drives the locate / commit / rank kernels.  The bulk-loaded part (RetainIndexHost, bmq_retain.h)
// is handed in by the engine after every (re)build.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bmq_retain_core.h"
#include "bmq_retain_snap_core.h"
#include "bmq_rplan_core.h"

namespace bmq {

struct RetainDynInfo {
    uint64_t n_live = 0;      // retained topics now
    uint64_t id_bound = 0;    // ids handed out in this generation (live or not): every id is below
    uint64_t base_n = 0;      // ids below are ranks of the last bulk load
    uint64_t base_dead = 0;   // bulk-loaded ids whose topic has been removed
    uint64_t overlay_ids = 0; // ids handed out to topics added since the bulk load
    uint64_t overlay_nodes = 0;
    uint64_t batches = 0;
};

// A snapshot of the live retained topics in exec memory (RetainDyn::snapshot): owns the arrays of RsSnap
template <class Exec> struct RetainSnapshot {
    explicit RetainSnapshot(Exec& exec) : x(exec) {}
    ~RetainSnapshot() { drop(); }
    RetainSnapshot(const RetainSnapshot&) = delete;
    RetainSnapshot& operator=(const RetainSnapshot&) = delete;
    Exec& x;
    RsSnap s{};
    uint64_t topic_bytes = 0, bytes = 0; // bytes: everything the snapshot holds in exec memory
    void drop() {
        for (void* p : {(void*)s.tenants, (void*)s.tenant_off, (void*)s.item_tenant, (void*)s.topics, (void*)s.topic_off, (void*)s.ts, (void*)s.expiry}) x.release(p);
        s = RsSnap{};
        topic_bytes = bytes = 0;
    }
};

template <class Exec> class RetainDyn {
public:
    explicit RetainDyn(Exec& exec) : x(exec) {}
    ~RetainDyn() { drop(); }
    RetainDyn(const RetainDyn&) = delete;
    RetainDyn& operator=(const RetainDyn&) = delete;

    Exec& x;
    std::string error;
    bool tiny = false; // test knob: minimal capacities, every growth path runs all the time
    RetainDynInfo info;
    bool ready = false;
    uint64_t copied = 0; // bytes of host <-> exec copies issued so far, whatever the executor (what bmq_retain_compact_info.locked_copy_bytes is the difference of)

    // ---- after a bulk load: ids 0 .. n-1 are live ranks; everything dynamic starts empty ----
    bool reset(const RetainIndexView& base_view, const RetainIndexHost& h) {
        error.clear();
        drop();
        base = base_view;
        base_n = (uint32_t)h.n_topics;
        const uint32_t want_ids = base_n + (tiny ? 4u : std::max<uint32_t>(1024u, base_n / 8));
        if (!alloc_ids(want_ids)) return false;
        // per-id payload of the bulk load
        std::vector<unsigned long long> ts(base_n ? base_n : 1), ex_at(base_n ? base_n : 1);
        std::vector<uint32_t> ex(base_n ? base_n : 1);
        for (const RTenantState* t : h.order)
            for (size_t i = 0; i < t->topics.size(); i++) {
                ts[t->id_base + i] = t->ts[i];
                ex[t->id_base + i] = t->expiry[i];
                ex_at[t->id_base + i] = h.expire_at[t->id_base + i];
            }
        if (!cin(d_ts, ts.data(), sizeof(unsigned long long) * base_n) || !cin(d_expiry, ex.data(), sizeof(uint32_t) * base_n) ||
            !cin(d_expire_at, ex_at.data(), sizeof(unsigned long long) * base_n))
            return xfail();
        // dead bits: bulk-loaded ids live, everything behind them "not retained" until an add hands the id out
        {
            std::vector<unsigned long long> bits(n_words() + 1, ~0ull);
            for (uint32_t w = 0; w < base_n / 64; w++) bits[w] = 0ull;
            if (base_n & 63u) bits[base_n / 64] = ~0ull << (base_n & 63u);
            if (!cin(d_dead, bits.data(), sizeof(unsigned long long) * (n_words() + 1))) return xfail();
        }
        if (!alloc_overlay(tiny ? 4u : 4096u, tiny ? 16u : 1u << 16)) return false;
        RetainCounters c{};
        c.ov_nodes = 1; // the root
        c.next_id = base_n;
        ONode root{NONE, 0, 0, 0, 0, NONE, NONE, NONE};
        if (!cin(d_nodes, &root, sizeof(root)) || !cin(d_ctr, &c, sizeof(c))) return xfail();
        hc = c;
        if (!x.r_rank(mut(), n_words()) || !x.sync()) return xfail();
        info = RetainDynInfo{};
        info.n_live = base_n;
        info.id_bound = base_n;
        info.base_n = base_n;
        seq = 0;
        ready = true;
        return true;
    }

    RetainDynView view() const {
        RetainDynView v{};
        v.onodes = d_nodes;
        v.oedges = d_edges;
        v.oedge_mask = edge_slots - 1;
        v.opool = d_pool;
        v.dead_bits = d_dead;
        v.dead_rank = d_rank;
        v.base_n = base_n;
        v.use_dead = info.base_dead != 0;
        v.ov_live = (uint32_t)info.overlay_ids;
        return v;
    }
    const unsigned long long* expire_at() const { return d_expire_at; }
    RetainMut mut_view() const { return mut(); } // (the emulator harness of the plan kernels runs them on this instance's arrays)

    // ---- one batch of ops (host buffers).  out_ids (may be null): the id of every op's topic, NONE for a no-op / superseded op ----
    bool apply(const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant, const uint8_t* topics,
               const uint32_t* topic_off, const uint8_t* op, const unsigned long long* ts, const uint32_t* expiry, uint32_t n, uint32_t* out_ids) {
        error.clear();
        if (!ready) return fail("the retained-topic index has not been built");
        if (n == 0) return true;
        const size_t tb = tenant_off[n_tenants], pb = topic_off[n];
        // room for the worst case: every op adds a topic none of whose levels exists yet
        const size_t seps = (size_t)std::count(topics, topics + pb, (uint8_t)'/');
        uint64_t max_tenant_bytes = 0;
        for (uint32_t t = 0; t < n_tenants; t++) max_tenant_bytes = std::max<uint64_t>(max_tenant_bytes, tenant_off[t + 1] - tenant_off[t]);
        const uint64_t need_nodes = (uint64_t)hc.ov_nodes + seps + 2ull * n, need_pool = (uint64_t)hc.opool_used + pb + max_tenant_bytes * n;
        const uint64_t need_ids = (uint64_t)hc.next_id + n;
        if (need_nodes >= 0x7FFFFFF0ull || need_pool >= 0xFFFFFFF0ull || need_ids >= 0x7FFFFFF0ull) return fail("the retained-topic index is full: compact it");
        if (need_ids > id_cap && !grow_ids((uint32_t)std::min<uint64_t>(0x7FFFFFF0ull, need_ids + need_ids / 2))) return false;
        if ((need_nodes > ov_cap || need_pool > pool_cap || need_nodes * 2 > edge_slots) &&
            !grow_overlay((uint32_t)std::max<uint64_t>(need_nodes + need_nodes / 2, ov_cap), (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(need_pool + need_pool / 2, pool_cap))))
            return false;
        // staging
        const size_t off_t = 0, off_to = align16(off_t + tb + 16), off_ot = align16(off_to + 4 * ((size_t)n_tenants + 1)), off_p = align16(off_ot + 4 * (size_t)n),
                     off_po = align16(off_p + pb + 16), off_op = align16(off_po + 4 * ((size_t)n + 1)), off_ts = align16(off_op + n), off_ex = align16(off_ts + 8 * (size_t)n),
                     off_tg = align16(off_ex + 4 * (size_t)n), off_id = align16(off_tg + 4 * (size_t)n), total = align16(off_id + 4 * (size_t)n);
        if (total > stage_cap) {
            if (!x.sync()) return xfail();
            x.release(d_stage);
            d_stage = (uint8_t*)x.alloc(total + total / 4);
            stage_cap = d_stage ? total + total / 4 : 0;
            if (!d_stage) return fail("out of memory (retain op staging)");
        }
        if (!cin(d_stage + off_t, tenants, tb) || !cin(d_stage + off_to, tenant_off, 4 * ((size_t)n_tenants + 1)) ||
            (op_tenant && !cin(d_stage + off_ot, op_tenant, 4 * (size_t)n)) || !cin(d_stage + off_p, topics, pb) ||
            !cin(d_stage + off_po, topic_off, 4 * ((size_t)n + 1)) || !cin(d_stage + off_op, op, n) ||
            (ts && (!cin(d_stage + off_ts, ts, 8 * (size_t)n) || !cin(d_stage + off_ex, expiry, 4 * (size_t)n))))
            return xfail();
        RetainOps ob{};
        ob.tenants = d_stage + off_t;
        ob.tenant_off = (const uint32_t*)(d_stage + off_to);
        ob.n_tenants = n_tenants;
        ob.op_tenant = op_tenant ? (const uint32_t*)(d_stage + off_ot) : nullptr;
        ob.topics = d_stage + off_p;
        ob.topic_off = (const uint32_t*)(d_stage + off_po);
        ob.op = d_stage + off_op;
        ob.ts = ts ? (const unsigned long long*)(d_stage + off_ts) : nullptr;
        ob.expiry = ts ? (const uint32_t*)(d_stage + off_ex) : nullptr;
        ob.n = n;
        ob.seq = ++seq;
        ob.target = (uint32_t*)(d_stage + off_tg);
        ob.out_ids = (uint32_t*)(d_stage + off_id);
        // the per-batch counters start at zero (the persistent ones stay)
        if (!x.zero((uint8_t*)d_ctr + offsetof(RetainCounters, went_live), sizeof(RetainCounters) - offsetof(RetainCounters, went_live))) return xfail();
        const RetainMut m = mut();
        if (!x.r_locate(m, ob) || !x.r_commit(m, ob) || !x.r_rank(m, n_words())) return xfail();
        if (!cout(&hc, d_ctr, sizeof(hc))) return xfail(); // waits for the batch
        if (out_ids && !cout(out_ids, ob.out_ids, 4 * (size_t)n)) return xfail();
        if (hc.err) {
            const uint32_t err = hc.err;
            uint32_t zero32 = 0;
            (void)x.copy_in((uint8_t*)d_ctr + offsetof(RetainCounters, err), &zero32, 4);
            hc.err = 0;
            if (err & RERR_BAD_OP) return fail("malformed retain op (op code / tenant index)");
            return fail("retain overlay ran out of room despite the bound (" + std::to_string(err) + ")");
        }
        uint64_t live = 0, dead = 0, blive = 0, bdead = 0;
        for (uint32_t k = 0; k < N_CTR_LANES; k++) live += hc.went_live[k], dead += hc.went_dead[k], blive += hc.base_went_live[k], bdead += hc.base_went_dead[k];
        info.n_live += live;
        info.n_live -= dead;
        info.base_dead += bdead;
        info.base_dead -= blive;
        info.id_bound = hc.next_id;
        info.overlay_ids = hc.next_id - base_n;
        info.overlay_nodes = hc.ov_nodes - 1;
        info.batches++;
        return true;
    }

    // ---- removal by id (remove_id_one): the ids are the engine's own, every one below info.id_bound (the caller checked).  One kernel over
    // the ids and the rank directory, on the executor's stream behind whatever is in flight; removed = the topics that stopped being retained
    bool remove_ids(const uint32_t* ids, uint32_t n, uint64_t& removed) {
        error.clear();
        removed = 0;
        if (!ready) return fail("the retained-topic index has not been built");
        if (n == 0) return true;
        if (!ensure(q_buf, q_cap, 4 * (size_t)n)) return false;
        if (!cin(q_buf, ids, 4 * (size_t)n)) return xfail();
        if (!x.zero((uint8_t*)d_ctr + offsetof(RetainCounters, went_live), sizeof(RetainCounters) - offsetof(RetainCounters, went_live))) return xfail();
        const RetainMut m = mut();
        if (!x.r_remove_ids(m, (const uint32_t*)q_buf, n, (uint32_t)info.id_bound) || !x.r_rank(m, n_words())) return xfail();
        if (!cout(&hc, d_ctr, sizeof(hc))) return xfail(); // waits for the kernels
        uint64_t dead = 0, bdead = 0;
        for (uint32_t k = 0; k < N_CTR_LANES; k++) dead += hc.went_dead[k], bdead += hc.base_went_dead[k];
        info.n_live -= dead;
        info.base_dead += bdead;
        info.batches++;
        removed = dead;
        return true;
    }

    // the dead bitmap over the ids handed out: bit id set = not retained now
    bool dead_words(std::vector<unsigned long long>& w) {
        w.assign((size_t)(info.id_bound + 63) / 64 + 1, ~0ull);
        if (!ready) return fail("the retained-topic index has not been built");
        const size_t n = (size_t)(info.id_bound + 63) / 64;
        return (n == 0 || cout(w.data(), d_dead, 8 * n)) ? true : xfail();
    }

    // ---- retained topics per tenant.  bulk: the (id_base, id_base + topics) rank range of every bulk-loaded tenant, in the order of
    // bulk_live's entries; ov: (tenant id, live topics) of every tenant node of the overlay that has some
    bool tenant_counts(const std::vector<uint32_t>& bulk_ranges, std::vector<uint32_t>& bulk_live, std::vector<std::pair<std::string, uint64_t>>& ov) {
        error.clear();
        const uint32_t nt = (uint32_t)(bulk_ranges.size() / 2);
        bulk_live.assign(nt, 0);
        ov.clear();
        if (!ready) return fail("the retained-topic index has not been built");
        const RetainMut m = mut();
        if (nt) {
            const size_t off_out = align16(8 * (size_t)nt);
            if (!ensure(q_buf, q_cap, off_out + 4 * (size_t)nt)) return false;
            if (!cin(q_buf, bulk_ranges.data(), 8 * (size_t)nt) || !x.r_census_bulk(m, (const uint32_t*)q_buf, nt, (uint32_t*)(q_buf + off_out)) ||
                !cout(bulk_live.data(), q_buf + off_out, 4 * (size_t)nt))
                return xfail();
        }
        if (info.overlay_ids == 0) return true;
        // a counter per overlay node (zeroed and filled on the executor's side), then the non-zero entries as a list: the host reads the
        // list -- one entry per tenant -- and never the table, however many nodes the overlay has
        const uint32_t n_nodes = hc.ov_nodes;
        const size_t off_list = 8 * (size_t)n_nodes, off_cnt = 2 * off_list;
        if (!ensure(q_buf, q_cap, off_cnt + 16)) return false;
        unsigned long long* d_table = (unsigned long long*)q_buf;
        unsigned long long* d_list = (unsigned long long*)(q_buf + off_list);
        uint32_t* d_cnt = (uint32_t*)(q_buf + off_cnt);
        uint32_t n = 0;
        if (!x.zero(d_table, off_list) || !x.zero(d_cnt, 16) || !x.r_census(m, (uint32_t)info.id_bound, d_table) || !x.r_census_pick(d_table, n_nodes, d_list, d_cnt) ||
            !cout(&n, d_cnt, 4))
            return xfail();
        if (n == 0) return true;
        std::vector<unsigned long long> picked(n);
        if (!cout(picked.data(), d_list, 8 * (size_t)n)) return xfail();
        std::sort(picked.begin(), picked.end());
        std::vector<uint32_t> nodes(n);
        std::vector<unsigned long long> table_of(n);
        for (uint32_t i = 0; i < n; i++) nodes[i] = (uint32_t)(picked[i] >> 32), table_of[i] = picked[i] & 0xFFFFFFFFull;
        // the tenant ids: labels of the tenant nodes, from the overlay string pool
        const size_t off_len = align16(4 * (size_t)n), off_off = align16(off_len + 4 * (size_t)n);
        if (!ensure(q_buf, q_cap, off_off + 8 * ((size_t)n + 1))) return false;
        std::vector<uint32_t> lens(n);
        if (!cin(q_buf, nodes.data(), 4 * (size_t)n) || !x.r_node_lens(m, (const uint32_t*)q_buf, n, (uint32_t*)(q_buf + off_len)) ||
            !cout(lens.data(), q_buf + off_len, 4 * (size_t)n))
            return xfail();
        std::vector<unsigned long long> offs((size_t)n + 1, 0);
        for (uint32_t i = 0; i < n; i++) offs[i + 1] = offs[i] + lens[i];
        std::vector<uint8_t> bytes(offs[n] + 1);
        if (offs[n]) {
            if (!ensure(o_buf, o_cap, offs[n] + 16)) return false;
            if (!cin(q_buf + off_off, offs.data(), 8 * ((size_t)n + 1)) ||
                !x.r_node_write(m, (const uint32_t*)q_buf, n, (const unsigned long long*)(q_buf + off_off), o_buf) || !cout(bytes.data(), o_buf, offs[n]))
                return xfail();
        }
        for (uint32_t i = 0; i < n; i++) ov.emplace_back(std::string((const char*)bytes.data() + offs[i], lens[i]), table_of[i]);
        return true;
    }

    // ---- id -> tenant id + topic of overlay topics (bulk-loaded ids are the host's: RetainIndexHost::topic) ----
    // lens[2 i] = tenant length, lens[2 i + 1] = total length (0: no such overlay topic), bytes = the strings back to back
    bool overlay_topics(const uint32_t* ids, uint32_t n, std::vector<uint32_t>& lens, std::vector<uint8_t>& bytes) {
        lens.assign(2 * (size_t)n, 0);
        bytes.clear();
        if (n == 0) return true;
        if (!ready) return fail("the retained-topic index has not been built");
        const size_t off_len = align16(4 * (size_t)n), off_off = align16(off_len + 8 * (size_t)n);
        if (!ensure(q_buf, q_cap, off_off + 8 * ((size_t)n + 1))) return false;
        uint32_t* d_ids = (uint32_t*)q_buf;
        uint32_t* d_lens = (uint32_t*)(q_buf + off_len);
        unsigned long long* d_offs = (unsigned long long*)(q_buf + off_off);
        const RetainMut m = mut();
        if (!cin(d_ids, ids, 4 * (size_t)n) || !x.r_topic_lens(m, d_ids, n, d_lens) || !cout(lens.data(), d_lens, 8 * (size_t)n)) return xfail();
        std::vector<unsigned long long> offs((size_t)n + 1, 0);
        for (uint32_t i = 0; i < n; i++) offs[i + 1] = offs[i] + lens[2 * i + 1];
        bytes.resize(offs[n]);
        if (offs[n] == 0) return true;
        if (!ensure(o_buf, o_cap, offs[n] + 16)) return false;
        if (!cin(d_offs, offs.data(), 8 * ((size_t)n + 1)) || !x.r_topic_write(m, d_ids, n, d_offs, o_buf) || !cout(bytes.data(), o_buf, offs[n]))
            return xfail();
        return true;
    }
    // ---- id -> retainMessageKey (key_len_one / key_write_one).  The strings of the bulk-loaded ids come from a store in exec memory that is
    // built on first use in a generation (or by keys_prepare) from the host's copy of the load and dropped with the generation: reset() frees
    // it, so a bulk load that nobody asks keys of pays nothing for it.  bytes (may be null) = what the store holds in exec memory.
    bool keys_prepare(const RetainIndexHost& h, uint64_t* bytes) {
        error.clear();
        if (!ready) return fail("the retained-topic index has not been built");
        if (!ks_ready) {
            if (h.n_topics != base_n) return fail("the bulk load on the host is not the one this generation was built from");
            std::vector<uint8_t> topics, tenants;
            std::vector<unsigned long long> toff((size_t)base_n + 1, 0);
            std::vector<uint32_t> lo, tnoff{0};
            uint32_t rank = 0;
            for (const RTenantState* t : h.order) { // by id_base: a tenant is the rank range [id_base, id_base + topics)
                if (t->topics.empty()) continue;
                if (t->id_base != rank || (uint64_t)rank + t->topics.size() > base_n) return fail("the tenants of the bulk load do not tile its id range");
                lo.push_back(rank);
                tenants.insert(tenants.end(), t->name.begin(), t->name.end());
                tnoff.push_back((uint32_t)tenants.size());
                for (const std::string& p : t->topics) {
                    topics.insert(topics.end(), p.begin(), p.end());
                    toff[++rank] = topics.size();
                }
            }
            if (rank != base_n) return fail("the tenants of the bulk load do not tile its id range");
            lo.push_back(base_n);
            drop_key_store();
            ks_n_tenants = (uint32_t)lo.size() - 1;
            ks_topics = (uint8_t*)x.alloc(topics.size() + 16);
            ks_tenants = (uint8_t*)x.alloc(tenants.size() + 16);
            ks_topic_off = take<unsigned long long>(toff.size());
            ks_tenant_lo = take<uint32_t>(lo.size());
            ks_tenant_off = take<uint32_t>(tnoff.size());
            if (!ks_topics || !ks_tenants || !ks_topic_off || !ks_tenant_lo || !ks_tenant_off) {
                drop_key_store();
                return fail("out of memory (retain key store)");
            }
            if (!cin(ks_topics, topics.data(), topics.size()) || !cin(ks_tenants, tenants.data(), tenants.size()) ||
                !cin(ks_topic_off, toff.data(), 8 * toff.size()) || !cin(ks_tenant_lo, lo.data(), 4 * lo.size()) ||
                !cin(ks_tenant_off, tnoff.data(), 4 * tnoff.size()) || !x.sync()) {
                drop_key_store();
                return xfail();
            }
            ks_bytes = topics.size() + tenants.size() + 8 * toff.size() + 4 * lo.size() + 4 * tnoff.size();
            ks_ready = true;
        }
        if (bytes) *bytes = ks_bytes;
        return true;
    }
    bool keys_ready() const { return ks_ready; }
    // keys of ids[0, n) -- exec memory: the kept ids of a match never leave the device -- composed on the executor's stream behind whatever is
    // in flight: offs[0 .. n] (exec memory) = where every key starts, total = offs[n], bytes (exec memory) = the keys back to back.
    // Returns after the lengths are known (one read of `total`); the write kernel is in the stream.
    bool keys_compose(const RetainIndexHost& h, const uint32_t* ids, uint32_t n, const unsigned long long*& offs, const uint8_t*& bytes, uint64_t& total) {
        total = 0;
        if (!keys_prepare(h, nullptr)) return false;
        if (!ensure(k_off, k_off_cap, 16 * ((size_t)n + 1))) return false;
        unsigned long long* lens = (unsigned long long*)k_off;
        unsigned long long* o = lens + n + 1;
        const RetainMut m = mut();
        const RetainKeyStore ks = key_store();
        unsigned long long t = 0;
        if (!x.r_key_offsets(m, ks, ids, n, lens, o) || !cout(&t, o + n, 8)) return xfail();
        if (!ensure(k_out, k_out_cap, (size_t)t + 16)) return false;
        if (t && !x.r_key_write(m, ks, ids, n, o, k_out)) return xfail();
        offs = o;
        bytes = k_out;
        total = t;
        return true;
    }
    // ... for ids in host memory, with the buffer protocol of bmq_retain_message_keys: out_off[0 .. n] always, the bytes if they fit
    bool keys_by_id(const RetainIndexHost& h, const uint32_t* ids, uint32_t n, uint8_t* out, uint64_t cap, unsigned long long* out_off, bool& nospace) {
        nospace = false;
        if (!ensure(k_ids, k_ids_cap, 4 * (size_t)n + 16)) return false;
        if (!cin(k_ids, ids, 4 * (size_t)n)) return xfail();
        const unsigned long long* offs = nullptr;
        const uint8_t* bytes = nullptr;
        uint64_t total = 0;
        if (!keys_compose(h, (const uint32_t*)k_ids, n, offs, bytes, total)) return false;
        if (!cout(out_off, offs, 8 * ((size_t)n + 1))) return xfail();
        nospace = total > cap || (total && !out);
        if (!nospace && total && !cout(out, bytes, total)) return xfail();
        return true;
    }

    // ---- the plan of a batch of retain ops (bmq_rplan_core.h): the pre-commit half of RetainStoreCoProc.batchRetain for a whole batch, on
    // the executor's stream behind whatever is in flight.  Reads the index only (an instance that holds none answers "not retained" for
    // every topic).  The caller checked op_tenant[i] < n_tenants.  Two waits: one for everything but the key bytes -- the key offsets say how
    // many there are --, one for the bytes if they fit.
    struct PlanOut {               // host memory; every pointer may be null
        uint8_t *code, *action;    // [n]
        uint32_t *winner, *topic_id; // [n]
        int32_t* delta;            // [n_tenants]
        unsigned long long* key_off; // [n + 1]
        uint8_t* keys;
        uint64_t keys_cap;
        uint64_t by_action[4] = {0, 0, 0, 0}; // winners with RP_NONE .. RP_REMOVE
        uint64_t key_bytes = 0;
        bool nospace = false;      // keys_cap < key_bytes: everything but the key bytes was written
    };
    bool plan(const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant, const uint8_t* topics, const uint32_t* topic_off,
              const uint8_t* clear, uint32_t n, uint32_t min_table, PlanOut& o) {
        error.clear();
        const size_t tb = tenant_off[n_tenants], pb = topic_off[n];
        const uint32_t slots = min_table ? pow2_at_least((uint64_t)n) : std::max<uint32_t>(8u, pow2_at_least(2ull * n));
        // inputs | zeroed scratch and results (table, last, delta, ctr) | scratch (rep_of, key_len) | results, copied out in one piece
        const size_t off_t = 0, off_to = align16(off_t + tb + 16), off_ot = align16(off_to + 4 * ((size_t)n_tenants + 1)), off_p = align16(off_ot + 4 * (size_t)n),
                     off_po = align16(off_p + pb + 16), off_cl = align16(off_po + 4 * ((size_t)n + 1)), off_zero = align16(off_cl + n),
                     off_tab = off_zero, off_last = align16(off_tab + 4 * (size_t)slots), off_rep = align16(off_last + 4 * (size_t)n),
                     off_len = align16(off_rep + 4 * (size_t)n), off_res = align16(off_len + 8 * ((size_t)n + 1)),
                     off_koff = off_res, off_win = align16(off_koff + 8 * ((size_t)n + 1)), off_found = align16(off_win + 4 * (size_t)n),
                     off_delta = align16(off_found + 4 * (size_t)n), off_ctr = align16(off_delta + 4 * (size_t)n_tenants), off_code = align16(off_ctr + 4 * RP_C_N),
                     off_act = align16(off_code + n), total = align16(off_act + n);
        if (!ensure(p_buf, p_cap, total)) return false;
        if (!cin(p_buf + off_t, tenants, tb) || !cin(p_buf + off_to, tenant_off, 4 * ((size_t)n_tenants + 1)) || (op_tenant && !cin(p_buf + off_ot, op_tenant, 4 * (size_t)n)) ||
            !cin(p_buf + off_p, topics, pb) || !cin(p_buf + off_po, topic_off, 4 * ((size_t)n + 1)) || !cin(p_buf + off_cl, clear, n) ||
            !x.zero(p_buf + off_zero, off_rep - off_zero) || !x.zero(p_buf + off_delta, off_code - off_delta))
            return xfail();
        RplanBatch b{};
        b.tenants = p_buf + off_t;
        b.tenant_off = (const uint32_t*)(p_buf + off_to);
        b.n_tenants = n_tenants;
        b.op_tenant = op_tenant ? (const uint32_t*)(p_buf + off_ot) : nullptr;
        b.topics = p_buf + off_p;
        b.topic_off = (const uint32_t*)(p_buf + off_po);
        b.clear = p_buf + off_cl;
        b.n = n;
        b.table = (uint32_t*)(p_buf + off_tab);
        b.table_mask = slots - 1;
        b.rep_of = (uint32_t*)(p_buf + off_rep);
        b.last = (uint32_t*)(p_buf + off_last);
        b.found = (uint32_t*)(p_buf + off_found);
        b.code = p_buf + off_code;
        b.action = p_buf + off_act;
        b.winner = (uint32_t*)(p_buf + off_win);
        b.delta = (int32_t*)(p_buf + off_delta);
        b.key_len = (unsigned long long*)(p_buf + off_len);
        b.ctr = (uint32_t*)(p_buf + off_ctr);
        unsigned long long* d_koff = (unsigned long long*)(p_buf + off_koff);
        p_host.resize(total - off_res);
        if (!x.rp_plan(mut(), b, ready, d_koff) || !cout(p_host.data(), p_buf + off_res, total - off_res)) return xfail(); // waits for the passes
        const uint8_t* r = p_host.data() - off_res;
        uint32_t ctr[RP_C_N];
        memcpy(ctr, r + off_ctr, sizeof(ctr));
        if (ctr[RP_C_ERR] & RPERR_TENANT) return fail("malformed retain op (tenant index)");
        if (ctr[RP_C_ERR]) return fail("the group table of the retain plan ran full (" + std::to_string(ctr[RP_C_ERR]) + ")");
        unsigned long long kb = 0;
        memcpy(&kb, r + off_koff + 8 * (size_t)n, 8);
        o.key_bytes = kb;
        for (uint32_t a = 0; a < 4; a++) o.by_action[a] = ctr[RP_C_ACTION + a];
        if (o.code) memcpy(o.code, r + off_code, n);
        if (o.action) memcpy(o.action, r + off_act, n);
        if (o.winner) memcpy(o.winner, r + off_win, 4 * (size_t)n);
        if (o.topic_id) memcpy(o.topic_id, r + off_found, 4 * (size_t)n);
        if (o.delta) memcpy(o.delta, r + off_delta, 4 * (size_t)n_tenants);
        if (o.key_off) memcpy(o.key_off, r + off_koff, 8 * ((size_t)n + 1));
        o.nospace = kb > o.keys_cap || (kb && !o.keys);
        if (o.nospace || kb == 0) return true;
        if (!ensure(k_out, k_out_cap, (size_t)kb + 16)) return false;
        if (!x.rp_key_write(b, d_koff, k_out) || !cout(o.keys, k_out, kb)) return xfail();
        return true;
    }

    bool topic_info(uint32_t id, unsigned long long& ts, uint32_t& expiry, unsigned long long& expire_at_ms, bool& live) {
        if (!ready || id >= info.id_bound) return fail("no such retained topic");
        unsigned long long w = 0;
        if (!cout(&ts, d_ts + id, 8) || !cout(&expiry, d_expiry + id, 4) || !cout(&expire_at_ms, d_expire_at + id, 8) || !cout(&w, d_dead + (id >> 6), 8))
            return xfail();
        live = !((w >> (id & 63u)) & 1ull);
        return true;
    }
    // ids (ascending) the query accepts (GC scan / findAll); tenant_name: resolves GcQuery.t_node when q.has_tenant
    bool select(GcQuery q, const uint8_t* tenant_name, uint32_t tenant_len, std::vector<uint32_t>& out) {
        out.clear();
        const uint32_t* d_ids = nullptr;
        uint32_t cnt = 0;
        if (!select_exec(q, tenant_name, tenant_len, d_ids, cnt)) return false;
        out.resize(cnt);
        if (cnt && !cout(out.data(), d_ids, 4 * (size_t)cnt)) return xfail();
        return true;
    }
    // ... the ids stay in exec memory (q_buf: valid until the next call that uses it), only their number comes back
    bool select_exec(GcQuery q, const uint8_t* tenant_name, uint32_t tenant_len, const uint32_t*& d_ids, uint32_t& cnt) {
        d_ids = nullptr;
        cnt = 0;
        if (!ready) return fail("the retained-topic index has not been built");
        q.n_ids = (uint32_t)info.id_bound;
        if (q.n_ids == 0) return true;
        const size_t off_cnt = align16((size_t)q.n_ids), off_name = align16(off_cnt + 16), off_ids = align16(off_name + tenant_len + 32);
        if (!ensure(q_buf, q_cap, off_ids + 4 * (size_t)q.n_ids)) return false;
        uint32_t* d_cnt = (uint32_t*)(q_buf + off_cnt);
        const RetainMut m = mut();
        if (q.has_tenant) {
            std::vector<uint8_t> padded((size_t)tenant_len + 16, 0);
            if (tenant_len) memcpy(padded.data(), tenant_name, tenant_len);
            if (!cin(q_buf + off_name, padded.data(), padded.size()) || !x.r_find_tenant(m, q_buf + off_name, tenant_len, d_cnt + 1) ||
                !cout(&q.t_node, d_cnt + 1, 4))
                return xfail();
        }
        if (!x.r_gc_select(m, q, q_buf, (uint32_t*)(q_buf + off_ids), d_cnt) || !cout(&cnt, d_cnt, 4)) return xfail();
        d_ids = (const uint32_t*)(q_buf + off_ids);
        return true;
    }

    // ---- the ids whose retainMessageKey lies inside a KV boundary (retain_key_in_boundary): ONE pass of the boundary kernel over the ids
    // handed out, on the executor's stream behind whatever is in flight.  flags bit 0 / 1: start / end present (host memory; a present key
    // may be empty).  topics = live ids inside; key_bytes (may be null: the lengths are not computed) = the sum of their key lengths; ids (may
    // be null: no flag bytes are written, nothing is selected) = those ids, ascending.  Needs the key store: built here if the generation
    // has none, as keys_compose does.
    bool boundary_select(const RetainIndexHost& h, uint32_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len, uint64_t& topics,
                         uint64_t* key_bytes, std::vector<uint32_t>* ids) {
        if (ids) ids->clear();
        const uint32_t* d_ids = nullptr;
        uint32_t cnt = 0;
        if (!boundary_select_exec(h, flags, start, start_len, end, end_len, topics, key_bytes, ids != nullptr, d_ids, cnt)) return false;
        if (ids) {
            ids->resize(cnt);
            if (cnt && !cout(ids->data(), d_ids, 4 * (size_t)cnt)) return xfail();
        }
        return true;
    }
    // ... want_ids: the ids stay in exec memory (q_buf), their number comes back
    bool boundary_select_exec(const RetainIndexHost& h, uint32_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len, uint64_t& topics,
                              uint64_t* key_bytes, bool want_ids, const uint32_t*& d_ids, uint32_t& cnt) {
        topics = 0;
        if (key_bytes) *key_bytes = 0;
        d_ids = nullptr;
        cnt = 0;
        if (!keys_prepare(h, nullptr)) return false;
        const uint32_t n = (uint32_t)info.id_bound;
        if (n == 0) return true;
        if (!(flags & 1u)) start_len = 0;
        if (!(flags & 2u)) end_len = 0;
        const size_t off_ctr = align16((size_t)n), off_cnt = off_ctr + 16, off_start = off_cnt + 16, off_end = align16(off_start + start_len + 16),
                     off_ids = align16(off_end + end_len + 16);
        if (!ensure(q_buf, q_cap, off_ids + (want_ids ? 4 * (size_t)n : 0))) return false;
        unsigned long long* d_sums = (unsigned long long*)(q_buf + off_ctr);
        uint32_t* d_cnt = (uint32_t*)(q_buf + off_cnt);
        KeyBoundary kb{};
        kb.start = q_buf + off_start;
        kb.end = q_buf + off_end;
        kb.start_len = start_len;
        kb.end_len = end_len;
        kb.flags = flags & 3u;
        if (!x.zero(q_buf + off_ctr, 32) || !cin(q_buf + off_start, start, start_len) || !cin(q_buf + off_end, end, end_len)) return xfail();
        unsigned long long sums[2] = {0, 0};
        if (!x.r_boundary(mut(), key_store(), n, kb, want_ids ? q_buf : nullptr, key_bytes != nullptr, d_sums)) return xfail();
        if (want_ids && !x.r_flagged_ids(q_buf, n, (uint32_t*)(q_buf + off_ids), d_cnt)) return xfail();
        if (!cout(sums, d_sums, 16)) return xfail(); // waits for the pass
        topics = sums[0];
        if (key_bytes) *key_bytes = sums[1];
        if (want_ids) {
            if (!cout(&cnt, d_cnt, 4)) return xfail();
            d_ids = (const uint32_t*)(q_buf + off_ids);
        }
        return true;
    }

    // timestamp / expiry interval of every id handed out (compaction re-loads the live ones)
    bool payload(std::vector<unsigned long long>& ts, std::vector<uint32_t>& expiry) {
        ts.assign(info.id_bound ? info.id_bound : 1, 0);
        expiry.assign(info.id_bound ? info.id_bound : 1, 0);
        if (!ready) return fail("the retained-topic index has not been built");
        if (!cout(ts.data(), d_ts, 8 * (size_t)info.id_bound) || !cout(expiry.data(), d_expiry, 4 * (size_t)info.id_bound)) return xfail();
        return true;
    }

    // ---- the live topics (bflags = 0), or those whose retainMessageKey lies inside the boundary, as a private snapshot in exec memory, in the
    // layout the executor builder reads (bmq_retain_snap_core.h).  Runs on the executor's stream behind whatever is in flight and ends in a
    // synchronise; nothing of this generation is referenced by `out` afterwards.  What crosses to the host: the number of ids and four totals.
    // The strings of the bulk-loaded ids come from the key store, which is built here from the host's copy of the load if the generation has
    // none (keys_prepare ahead of the call takes that out of it).
    bool snapshot(const RetainIndexHost& h, uint32_t bflags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len, RetainSnapshot<Exec>& out) {
        error.clear();
        out.drop();
        if (!keys_prepare(h, nullptr)) return false;
        const uint32_t* d_ids = nullptr;
        uint32_t n = 0;
        if (bflags & 3u) {
            uint64_t topics = 0;
            if (!boundary_select_exec(h, bflags, start, start_len, end, end_len, topics, nullptr, true, d_ids, n)) return false;
        } else {
            GcQuery q{};
            q.live_only = 1;
            q.override_expiry = -1;
            if (!select_exec(q, nullptr, 0, d_ids, n)) return false;
        }
        std::vector<void*> tmp; // transient arrays: released behind the last synchronise
        struct Free {
            Exec& x;
            std::vector<void*>& v;
            ~Free() {
                (void)x.sync();
                for (void* p : v) x.release(p);
            }
        } free_tmp{x, tmp};
        auto get = [&](size_t bytes) {
            void* p = x.alloc(bytes + 16);
            if (p) tmp.push_back(p);
            return p;
        };
        const uint32_t nodes = hc.ov_nodes;
        RsArgs A{};
        RsSnap& S = out.s;
        S.n = n;
        S.item_tenant = take<uint32_t>((size_t)n + 4);
        S.topic_off = take<uint32_t>((size_t)n + 4);
        S.ts = take<unsigned long long>((size_t)n + 2);
        S.expiry = take<uint32_t>((size_t)n + 4);
        A.ids = d_ids;
        A.len = (uint32_t*)get(4 * ((size_t)n + 1));
        A.tn_flag = (uint32_t*)get(4 * (size_t)nodes);
        A.tn_len = (uint32_t*)get(4 * (size_t)nodes);
        A.tn_rank = (uint32_t*)get(4 * (size_t)nodes);
        A.tn_end = (uint32_t*)get(4 * (size_t)nodes);
        A.totals = (unsigned long long*)get(32);
        A.ov_nodes = nodes;
        if (!S.item_tenant || !S.topic_off || !S.ts || !S.expiry || !A.len || !A.tn_flag || !A.tn_len || !A.tn_rank || !A.tn_end || !A.totals)
            return fail("out of memory (retain snapshot)");
        A.S = S;
        const RetainMut m = mut();
        const RetainKeyStore ks = key_store();
        uint32_t ks_tb = 0; // bytes of the key store's tenant ids: its last offset (4 bytes, once per snapshot)
        if (ks.n_tenants && !cout(&ks_tb, ks.tenant_off + ks.n_tenants, 4)) return xfail();
        A.ks_tenants = ks.n_tenants;
        A.ks_tenant_bytes = ks_tb;
        // lengths and tenants per id, their sums; the overlay tenants that own one
        unsigned long long totals[4] = {0, 0, 0, 0};
        if (!x.zero(A.totals, 32) || !x.zero(A.tn_flag, 4 * (size_t)nodes) || !x.zero(S.topic_off, 4) || !x.rs_lens(m, ks, A) || (n && !x.scan_flags(A.len, S.topic_off + 1, n)) ||
            !x.rs_tenant_lens(m, A) || (nodes && (!x.scan_flags(A.tn_flag, A.tn_rank, nodes) || !x.scan_flags(A.tn_len, A.tn_end, nodes))) || !x.rs_totals(A) ||
            !cout(totals, A.totals, 32))
            return xfail();
        if (totals[0] >= 0xFFFFFFF0ull) return fail("the topics of the snapshot exceed 4 GiB");
        const uint32_t n_ov_t = (uint32_t)totals[2], ov_tb = (uint32_t)totals[3];
        A.n_bulk = (uint32_t)totals[1];
        out.topic_bytes = totals[0];
        S.n_tenants = ks.n_tenants + n_ov_t;
        S.topics = (uint8_t*)x.alloc((size_t)totals[0] + 32);
        S.tenants = (uint8_t*)x.alloc((size_t)ks_tb + ov_tb + 32);
        S.tenant_off = take<uint32_t>((size_t)S.n_tenants + 4);
        if (!S.topics || !S.tenants || !S.tenant_off) return fail("out of memory (retain snapshot)");
        A.S = S;
        // the tenant table: the key store's entries, then the overlay's; the topics: the bulk-loaded ids' runs of the key store, then the overlay chains
        RsGather<unsigned long long> G{S.topics, S.topic_off, A.n_bulk, ks.topics, ks.topic_off, d_ids, 0ull};
        uint32_t bulk_bytes = 0;
        if (A.n_bulk && !cout(&bulk_bytes, S.topic_off + A.n_bulk, 4)) return xfail();
        G.bytes = bulk_bytes;
        if (!x.zero(S.tenant_off, 4) || (ks.n_tenants && (!x.copy(S.tenant_off, ks.tenant_off, 4 * ((size_t)ks.n_tenants + 1)) || !x.copy(S.tenants, ks.tenants, ks_tb))) ||
            !x.zero(S.tenants + ks_tb + ov_tb, 16) || !x.rs_tenants(m, A) || !x.zero(S.topics + totals[0], 16) || !x.rs_gather(G) || !x.rs_items(m, A) || !x.sync())
            return xfail();
        out.bytes = totals[0] + ks_tb + ov_tb + 4 * ((size_t)S.n_tenants + 1) + 24 * (size_t)n + 4;
        return true;
    }

    // ---- the mutable part of a generation that RetainBuild<Exec> has just built from a snapshot, made ready AHEAD of the swap on this
    // instance's executor (the build stream): per-id payload and key store through the builder's permutation (d_perm: exec memory, rank ->
    // item of `s`), dead bitmap and empty overlay by fills.  No host loop over the topics.  adopt() of the serving instance takes it over.
    bool reset_exec(const RsSnap& s, const uint32_t* d_perm, uint32_t n_topics, const std::vector<std::string>& names, const std::vector<uint32_t>& t_begin) {
        error.clear();
        drop();
        base = RetainIndexView{};
        base_n = n_topics;
        const uint32_t want_ids = base_n + (tiny ? 4u : std::max<uint32_t>(1024u, base_n / 8));
        if (!alloc_ids(want_ids)) return false;
        const uint32_t live_words = base_n / 64;
        unsigned long long edge_word = ~0ull << (base_n & 63u); // the word the bulk-loaded ids end in
        if (!x.zero(d_dead, 8 * (size_t)live_words) || !x.fill_bytes(d_dead + live_words, 0xFF, 8 * ((size_t)n_words() + 1 - live_words)) ||
            ((base_n & 63u) && !cin(d_dead + live_words, &edge_word, 8)))
            return xfail();
        if (!alloc_overlay(tiny ? 4u : 4096u, tiny ? 16u : 1u << 16)) return false;
        RetainCounters c{};
        c.ov_nodes = 1; // the root
        c.next_id = base_n;
        ONode root{NONE, 0, 0, 0, 0, NONE, NONE, NONE};
        if (!cin(d_nodes, &root, sizeof(root)) || !cin(d_ctr, &c, sizeof(c)) || !x.sync()) return xfail();
        hc = c;
        // the key store: the builder's tenants are the ranges t_begin[t] .. t_begin[t + 1] of the ranks, every one with topics
        std::vector<uint8_t> tbytes;
        std::vector<uint32_t> tnoff{0};
        for (const std::string& nm : names) {
            tbytes.insert(tbytes.end(), nm.begin(), nm.end());
            tnoff.push_back((uint32_t)tbytes.size());
        }
        std::vector<uint32_t> lo(t_begin.begin(), t_begin.end());
        if (lo.empty()) lo.push_back(0u);
        lo.back() = base_n;
        ks_n_tenants = (uint32_t)lo.size() - 1;
        uint32_t* klen = take<uint32_t>((size_t)base_n + 4);
        uint32_t* koff = take<uint32_t>((size_t)base_n + 4);
        ks_topic_off = take<unsigned long long>((size_t)base_n + 2);
        ks_tenants = (uint8_t*)x.alloc(tbytes.size() + 16);
        ks_tenant_lo = take<uint32_t>(lo.size());
        ks_tenant_off = take<uint32_t>(tnoff.size());
        bool ok = klen && koff && ks_topic_off && ks_tenants && ks_tenant_lo && ks_tenant_off;
        uint32_t key_bytes = 0;
        RsNext N{d_perm, base_n, s.topic_off, s.ts, s.expiry, klen, koff, d_ts, d_expire_at, d_expiry, ks_topic_off};
        if (ok)
            ok = x.zero(koff, 4) && x.zero(ks_topic_off, 8) && x.rs_perm_lens(N) && (base_n == 0 || x.scan_flags(klen, koff + 1, base_n)) && x.rs_next(N) &&
                 cout(&key_bytes, koff + base_n, 4);
        if (ok) ks_topics = (uint8_t*)x.alloc((size_t)key_bytes + 32);
        ok = ok && ks_topics;
        if (ok) {
            const RsGather<uint32_t> G{ks_topics, koff, base_n, s.topics, s.topic_off, d_perm, key_bytes};
            ok = x.rs_gather(G) && x.zero(ks_topics + key_bytes, 16) && cin(ks_tenants, tbytes.data(), tbytes.size()) && cin(ks_tenant_lo, lo.data(), 4 * lo.size()) &&
                 cin(ks_tenant_off, tnoff.data(), 4 * tnoff.size()) && x.r_rank(mut(), n_words());
        }
        ok = x.sync() && ok;
        x.release(klen);
        x.release(koff);
        if (!ok) {
            const std::string why = x.err.empty() ? std::string("out of memory (next retain generation)") : x.err;
            drop();
            return fail(why);
        }
        ks_bytes = (uint64_t)key_bytes + tbytes.size() + 8 * ((size_t)base_n + 1) + 4 * lo.size() + 4 * tnoff.size();
        ks_ready = true;
        info = RetainDynInfo{};
        info.n_live = base_n;
        info.id_bound = base_n;
        info.base_n = base_n;
        seq = 0;
        ready = true;
        return true;
    }
    // the arrays `o` prepared (reset_exec) become this instance's: pointers change hands, nothing is copied; `o` is left empty
    void adopt(RetainDyn& o, const RetainIndexView& base_view) {
        drop();
        base = base_view;
        base_n = o.base_n;
        d_expire_at = o.d_expire_at, d_ts = o.d_ts, d_expiry = o.d_expiry, d_id_node = o.d_id_node, d_id_tnode = o.d_id_tnode;
        d_dead = o.d_dead, d_rank = o.d_rank, d_last = o.d_last, d_nodes = o.d_nodes, d_edges = o.d_edges, d_pool = o.d_pool, d_ctr = o.d_ctr;
        hc = o.hc;
        id_cap = o.id_cap, ov_cap = o.ov_cap, pool_cap = o.pool_cap, edge_slots = o.edge_slots;
        ks_topics = o.ks_topics, ks_tenants = o.ks_tenants, ks_topic_off = o.ks_topic_off, ks_tenant_lo = o.ks_tenant_lo, ks_tenant_off = o.ks_tenant_off;
        ks_n_tenants = o.ks_n_tenants, ks_bytes = o.ks_bytes, ks_ready = o.ks_ready;
        info = o.info;
        seq = 0;
        ready = o.ready;
        o.d_expire_at = o.d_ts = nullptr;
        o.d_expiry = o.d_id_node = o.d_id_tnode = nullptr;
        o.d_dead = nullptr, o.d_rank = nullptr, o.d_last = nullptr, o.d_nodes = nullptr, o.d_edges = nullptr, o.d_pool = nullptr, o.d_ctr = nullptr;
        o.ks_topics = o.ks_tenants = nullptr;
        o.ks_topic_off = nullptr;
        o.ks_tenant_lo = o.ks_tenant_off = nullptr;
        o.drop();
    }

    void drop() {
        for (void* p : {(void*)d_expire_at, (void*)d_ts, (void*)d_expiry, (void*)d_id_node, (void*)d_id_tnode, (void*)d_dead, (void*)d_rank, (void*)d_last,
                        (void*)d_nodes, (void*)d_edges, (void*)d_pool, (void*)d_ctr, (void*)d_stage, (void*)q_buf, (void*)o_buf, (void*)k_ids, (void*)k_off,
                        (void*)k_out, (void*)p_buf})
            if (p) x.release(p);
        drop_key_store(); // (its ids are the ranks of the generation that ends here)
        d_expire_at = d_ts = nullptr;
        d_expiry = d_id_node = d_id_tnode = nullptr;
        d_dead = nullptr;
        d_rank = nullptr;
        d_last = nullptr;
        d_nodes = nullptr;
        d_edges = nullptr;
        d_pool = nullptr;
        d_ctr = nullptr;
        d_stage = q_buf = o_buf = k_ids = k_off = k_out = p_buf = nullptr;
        id_cap = ov_cap = pool_cap = edge_slots = 0;
        stage_cap = q_cap = o_cap = k_ids_cap = k_off_cap = k_out_cap = p_cap = 0;
        ready = false;
    }

private:
    RetainIndexView base{};
    uint32_t base_n = 0;
    unsigned long long *d_expire_at = nullptr, *d_ts = nullptr;
    uint32_t *d_expiry = nullptr, *d_id_node = nullptr, *d_id_tnode = nullptr;
    unsigned long long* d_dead = nullptr;
    uint32_t* d_rank = nullptr;
    unsigned long long* d_last = nullptr;
    ONode* d_nodes = nullptr;
    uint32_t* d_edges = nullptr;
    uint8_t* d_pool = nullptr;
    RetainCounters* d_ctr = nullptr;
    RetainCounters hc{};
    uint32_t id_cap = 0, ov_cap = 0, pool_cap = 0, edge_slots = 0;
    uint8_t *d_stage = nullptr, *q_buf = nullptr, *o_buf = nullptr;
    size_t stage_cap = 0, q_cap = 0, o_cap = 0;
    unsigned long long seq = 0;
    // the key store (RetainKeyStore) and the scratch of the key calls
    uint8_t *ks_topics = nullptr, *ks_tenants = nullptr;
    unsigned long long* ks_topic_off = nullptr;
    uint32_t *ks_tenant_lo = nullptr, *ks_tenant_off = nullptr;
    uint32_t ks_n_tenants = 0;
    uint64_t ks_bytes = 0;
    bool ks_ready = false;
    uint8_t *k_ids = nullptr, *k_off = nullptr, *k_out = nullptr;
    size_t k_ids_cap = 0, k_off_cap = 0, k_out_cap = 0;
    uint8_t* p_buf = nullptr; // staging, scratch and results of plan()
    size_t p_cap = 0;
    std::vector<uint8_t> p_host;

    void drop_key_store() {
        for (void* p : {(void*)ks_topics, (void*)ks_tenants, (void*)ks_topic_off, (void*)ks_tenant_lo, (void*)ks_tenant_off})
            if (p) x.release(p);
        ks_topics = ks_tenants = nullptr;
        ks_topic_off = nullptr;
        ks_tenant_lo = ks_tenant_off = nullptr;
        ks_n_tenants = 0;
        ks_bytes = 0;
        ks_ready = false;
    }
    RetainKeyStore key_store() const {
        RetainKeyStore ks{};
        ks.topics = ks_topics;
        ks.topic_off = ks_topic_off;
        ks.tenant_lo = ks_tenant_lo;
        ks.tenants = ks_tenants;
        ks.tenant_off = ks_tenant_off;
        ks.n_tenants = ks_n_tenants;
        ks.n_ids = ks_ready ? base_n : 0u;
        return ks;
    }

    static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
    // every host <-> exec copy of this class is issued here and counted (`copied`)
    bool cin(void* d, const void* s, size_t n) {
        copied += n;
        return x.copy_in_async(d, s, n);
    }
    bool cout(void* d, const void* s, size_t n) {
        copied += n;
        return x.copy_out(d, s, n);
    }
    uint32_t n_words() const { return (id_cap + 63) / 64; }
    bool fail(const std::string& m) {
        error = m;
        return false;
    }
    bool xfail() { return fail(x.err.empty() ? std::string("exec failure") : x.err); }
    bool ensure(uint8_t*& p, size_t& cap, size_t need) {
        if (need <= cap) return true;
        if (!x.sync()) return xfail();
        x.release(p);
        p = (uint8_t*)x.alloc(need + need / 4);
        cap = p ? need + need / 4 : 0;
        return p ? true : fail("out of memory (retain scratch)");
    }
    RetainMut mut() const {
        RetainMut m{};
        m.base = base;
        m.base_n = base_n;
        m.onodes = d_nodes;
        m.ov_cap = ov_cap;
        m.oedges = d_edges;
        m.oedge_mask = edge_slots - 1;
        m.opool = d_pool;
        m.opool_cap = pool_cap;
        m.expire_at = d_expire_at;
        m.ts = d_ts;
        m.expiry = d_expiry;
        m.id_node = d_id_node;
        m.id_tnode = d_id_tnode;
        m.id_cap = id_cap;
        m.dead_bits = d_dead;
        m.dead_rank = d_rank;
        m.last_op = d_last;
        m.ctr = d_ctr;
        return m;
    }
    template <class T> T* take(size_t n) { return (T*)x.alloc(sizeof(T) * (n ? n : 1)); }
    bool alloc_ids(uint32_t cap) {
        id_cap = cap;
        const size_t w = n_words() + 1;
        d_expire_at = take<unsigned long long>(cap);
        d_ts = take<unsigned long long>(cap);
        d_expiry = take<uint32_t>(cap);
        d_id_node = take<uint32_t>(cap);
        d_id_tnode = take<uint32_t>(cap);
        d_dead = take<unsigned long long>(w);
        d_rank = take<uint32_t>(w + 1);
        d_ctr = take<RetainCounters>(1);
        if (!d_expire_at || !d_ts || !d_expiry || !d_id_node || !d_id_tnode || !d_dead || !d_rank || !d_ctr) return fail("out of memory (retain ids)");
        if (!x.zero(d_expire_at, 8 * (size_t)cap) || !x.zero(d_ts, 8 * (size_t)cap) || !x.zero(d_expiry, 4 * (size_t)cap) ||
            !x.fill_bytes(d_id_node, 0xFF, 4 * (size_t)cap) || !x.fill_bytes(d_id_tnode, 0xFF, 4 * (size_t)cap))
            return xfail();
        return true;
    }
    bool alloc_last() { // bids: one per id and per overlay node
        if (d_last) {
            if (!x.sync()) return xfail();
            x.release(d_last);
        }
        d_last = take<unsigned long long>((size_t)id_cap + ov_cap);
        if (!d_last) return fail("out of memory (retain bids)");
        return x.zero(d_last, 8 * ((size_t)id_cap + ov_cap)) ? true : xfail();
    }
    bool alloc_overlay(uint32_t nodes, uint32_t pool) {
        ov_cap = nodes;
        pool_cap = pool;
        edge_slots = pow2_at_least((uint64_t)nodes * 2);
        if (edge_slots < 8) edge_slots = 8;
        d_nodes = take<ONode>(nodes);
        d_edges = take<uint32_t>(edge_slots);
        d_pool = (uint8_t*)x.alloc((size_t)pool + 16);
        if (!d_nodes || !d_edges || !d_pool) return fail("out of memory (retain overlay)");
        if (!x.zero(d_edges, 4 * (size_t)edge_slots)) return xfail();
        return alloc_last();
    }
    template <class T> bool regrow(T*& p, size_t old_n, size_t new_n, int fill) {
        T* np = take<T>(new_n);
        if (!np) return fail("out of memory (retain growth)");
        if (!x.copy(np, p, sizeof(T) * old_n) || !x.fill_bytes((uint8_t*)(np + old_n), fill, sizeof(T) * (new_n - old_n)) || !x.sync()) return xfail();
        x.release(p);
        p = np;
        return true;
    }
    bool grow_ids(uint32_t cap) {
        const uint32_t old = id_cap, old_w = n_words() + 1;
        id_cap = cap;
        const uint32_t new_w = n_words() + 1;
        if (!regrow(d_expire_at, old, cap, 0) || !regrow(d_ts, old, cap, 0) || !regrow(d_expiry, old, cap, 0) || !regrow(d_id_node, old, cap, 0xFF) ||
            !regrow(d_id_tnode, old, cap, 0xFF) || !regrow(d_dead, old_w, new_w, 0xFF))
            return false;
        if (!x.sync()) return xfail();
        x.release(d_rank);
        d_rank = take<uint32_t>((size_t)new_w + 1);
        if (!d_rank) return fail("out of memory (retain growth)");
        // (the old last word was allocated all-ones beyond id_cap: ids in it that are now in range are "not retained", as they must be)
        return alloc_last();
    }
    bool grow_overlay(uint32_t nodes, uint32_t pool) {
        if (nodes > ov_cap && !regrow(d_nodes, ov_cap, nodes, 0)) return false;
        if (pool > pool_cap) {
            uint8_t* np = (uint8_t*)x.alloc((size_t)pool + 16);
            if (!np) return fail("out of memory (retain growth)");
            if (!x.copy(np, d_pool, pool_cap) || !x.sync()) return xfail();
            x.release(d_pool);
            d_pool = np;
            pool_cap = pool;
        }
        ov_cap = std::max(ov_cap, nodes);
        const uint32_t want = pow2_at_least((uint64_t)ov_cap * 2);
        if (want > edge_slots) { // re-insert every node into the larger table
            if (!x.sync()) return xfail();
            x.release(d_edges);
            d_edges = take<uint32_t>(want);
            if (!d_edges) return fail("out of memory (retain growth)");
            edge_slots = want;
            if (!x.zero(d_edges, 4 * (size_t)edge_slots) || !x.r_rehash(mut(), hc.ov_nodes)) return xfail();
        }
        return alloc_last();
    }
};

} // namespace bmq
