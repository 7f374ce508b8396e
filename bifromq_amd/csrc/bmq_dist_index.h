// bmq_dist_index.h -- owner of the dist index: the arrays of bmq_layout.h in "exec memory" (HBM under DevExec, host memory
// under HostExec) and the host-side control of the builder pipeline of bmq_build_core.h.  The host side only moves bytes,
// sizes buffers and reads back counters; every key is parsed, every node inserted and every id set edited by the builder
// functions on the exec side.
//
//   rebuild(keys)  <- IKVRangeCoProc.reset(Boundary)           (KVAPI/IKVRangeCoProc.java:64, DW/DistWorkerCoProc.java:283-291)
//   apply(ops)     <- ISubscriptionCache.refresh(add/remove)   (DW/DistWorkerCoProc.java:188-209, DW/cache/SubscriptionCache.java:127-134)
//   route_key(id)  -> key bytes, so the Java side can materialise Matching objects (SCHEMA/KVSchemaUtil.java:73-89)
//
// Exec concept (bmq_exec_host.h: HostExec; bmq_engine.hip: DevExec):
//   void* alloc(size_t); void release(void*);
//   bool copy_in(dst, src, n)  [blocking]   bool copy_in_async(dst, src, n) [src valid until sync()]
//   bool copy_out(dst, src, n) [blocking, after everything queued before]   bool copy(dst, src, n)   bool zero(p, n)   bool sync()
//   bool fill_slots(TrieSlot*, n), iota(uint32_t*, n)
//   bool prepare(ix, ob), prepare_check(ix, ob, n_dir), bulk_prepare(ix, ob), scan_flags(in, out, n), bulk_tenants(ix, ob, scan),
//        locate(ix, ob), sort_targets(ob), group(ix, ob), rehash(ix, old_base, old_slots, new_base, new_buckets), tails(ix, tail_pass, n_slots),
//        dict_rehash(old, old_slots, ix), find(ix, query, tenant_len, filter_len, out, cap), gather_refs(ix, ids, n, out_refs),
//        gather_bytes(ix, refs, offs, n, out), find_keys(ix, key_source, n, out_ids, n_bad)
//   std::string err;
#pragma once
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "bmq_build_core.h"
#include "bmq_order_core.h"
#include "bmq_prefix_core.h"

// A tenant's region holds nodes * (1 + slack / 4) two-slot buckets (DistIndex::slack_num, bmq_config.region_slack): 1 -> load factor 0.4
// (rounds 2-5), 3 -> 0.29, 6 -> 0.2 (the default since round 6).  What the slack buys is fewer SECOND probes: at 0.4 a publish of the survey's
// workload pays 1.24 line fetches beyond the home buckets of its 10.2 probes (a home bucket full of other edges; a Bloom false positive walks on
// to the first bucket with a free slot), at 0.29 0.55, at 0.2 0.28, at 0.125 0.12 -- and k_walk, which is bound by the rate of its line requests,
// takes 0.212 / 0.198 / 0.195 / 0.194 ms (profiles/r06/extras/ab_region_slack.txt).  The price is memory: 64 bytes x (1 + slack / 4) per node.
#ifndef BMQ_REGION_SLACK_NUM
#define BMQ_REGION_SLACK_NUM 6
#endif

namespace bmq {

struct DistIndexStats {
    uint64_t n_routes = 0, n_tenants = 0, n_nodes = 0, n_tokens = 0;
    uint64_t trie_slots = 0, dict_slots = 0, bytes = 0;
    uint64_t id_list_words = 0, id_list_garbage = 0, trie_garbage_slots = 0, key_bytes = 0;
    uint32_t next_id = 0;
};
struct ApplyResult {
    uint32_t added = 0, removed = 0, dups = 0;
};
// A KV boundary as the host holds it (IKVRangeCoProc.reset(Boundary), DW/DistWorkerCoProc.java:283-291).  flags bit 0: `start` is present,
// bit 1: `end` is present; a present key may be empty.  Order: key_compare (unsigned bytes, a proper prefix first).
struct Boundary {
    uint8_t flags = 0;
    std::string start, end;
    static int cmp(std::string_view a, std::string_view b) {
        return key_compare((const uint8_t*)a.data(), a.size(), (const uint8_t*)b.data(), b.size());
    }
    bool bounded() const { return (flags & 3u) != 0; }
    bool valid() const { return (flags & 3u) != 3u || cmp(start, end) < 0; } // (no start, end = "": NULL_BOUNDARY, valid and empty)
    // BoundaryUtil.inRange (base-kv/.../utils/BoundaryUtil.java:241-252)
    bool contains(std::string_view k) const { return (!(flags & 1u) || cmp(k, start) >= 0) && (!(flags & 2u) || cmp(k, end) < 0); }
    // no key that begins with `prefix` is inside: end <= prefix, or start >= upperBound(prefix) (the prefix with its last byte below 0xFF
    // incremented and what follows it cut off; a prefix of 0xFF bytes only has no upper bound)
    bool excludes_prefix(std::string_view prefix) const {
        if ((flags & 2u) && cmp(end, prefix) <= 0) return true;
        if (!(flags & 1u)) return false;
        std::string ub(prefix);
        while (!ub.empty() && (uint8_t)ub.back() == 0xFF) ub.pop_back();
        if (ub.empty()) return false;
        ub.back() = (char)((uint8_t)ub.back() + 1);
        return cmp(start, ub) >= 0;
    }
};

template <class Exec> class DistIndex {
    // BMQ_TIMING=1: phase times on stderr (each lap synchronises the exec first, so the numbers include the kernels)
    struct PhaseTimer {
        Exec& x;
        bool on;
        std::chrono::steady_clock::time_point t0;
        explicit PhaseTimer(Exec& ex) : x(ex), on(bmq_env("BMQ_TIMING") != nullptr), t0(std::chrono::steady_clock::now()) {}
        void lap(const char* what) {
            if (!on) return;
            (void)x.sync();
            const auto t1 = std::chrono::steady_clock::now();
            fprintf(stderr, "[bmq index] %-34s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
        }
    };

public:
    explicit DistIndex(Exec& exec) : x(exec) {}
    ~DistIndex() { drop(); }
    DistIndex(const DistIndex&) = delete;
    DistIndex& operator=(const DistIndex&) = delete;

    Exec& x;
    std::string error;
    bool built = false, broken = false;
    uint64_t generation = 0; // bumped by every rebuild: ids of different generations are unrelated
    uint32_t slack_num = BMQ_REGION_SLACK_NUM; // region size = nodes * (1 + slack_num / 4) buckets (bmq_config.region_slack)
    bool tail_records = true; // the tail pass after a bulk load / before a compacted generation serves (bmq_config.tail_records)
    bool child_filters = true; // the walk reads the child filter words of the nodes (bmq_config.child_filters); the builder keeps them either way
    bool tiny = false;       // test knob (tools/host_fuzz.cpp): minimal initial capacities, so that every growth path runs all the time

    // ---- arrays in exec memory ----
    TrieSlot* trie = nullptr;
    uint64_t trie_cap = 0, trie_used = 0;
    TenantSlot* dir = nullptr;
    uint32_t dir_slots = 0;
    uint8_t* names = nullptr;
    uint32_t names_cap = 0, names_used = 0;
    DictSlot* dict = nullptr;
    uint32_t dict_slots = 0;
    uint8_t* dpool = nullptr;
    uint32_t dpool_cap = 0;
    uint32_t* route_pos = nullptr;
    uint64_t rp_cap = 0;
    unsigned long long* kref = nullptr;
    uint32_t* khash = nullptr;
    uint32_t id_cap = 0, next_id = 0;
    uint64_t n_routes = 0; // live routes (host count: rebuild sets it, every apply adds what the groups report)
    uint8_t* kpool = nullptr;
    uint64_t kpool_cap = 0, kpool_used = 0;
    BuildCounters* bc = nullptr;
    BuildCounters hbc{}; // last read-back
    uint32_t* fo_dgroup = nullptr; // registered by the fan-out grouping (bmq_fanout.h): deletes mark their ids dead in its per-id cache
    uint32_t fo_cap = 0;

    // ---- host bookkeeping ----
    std::unordered_map<std::string, uint32_t> tenant_slot; // tenant id -> directory slot
    std::vector<std::pair<uint64_t, uint64_t>> free_regions; // (base, slots) abandoned by region growth
    uint64_t trie_garbage = 0;

    DistIndexView view() const {
        DistIndexView v{};
        v.trie = trie;
        v.tenants = dir;
        v.tenant_mask = dir_slots - 1;
        v.filter_off = child_filters ? 0u : 0xFFFFFFFFu;
        v.tenant_names = names;
        v.dict = dict;
        v.dict_group_mask = dict_slots / DICT_GROUP - 1;
        v.pool = dpool;
        v.route_pos = route_pos;
        return v;
    }
    DistIndexMut mut() const {
        DistIndexMut m{};
        m.trie = trie;
        m.tenants = dir;
        m.tenant_mask = dir_slots - 1;
        m.tenant_names = names;
        m.dict = dict;
        m.dict_group_mask = dict_slots / DICT_GROUP - 1;
        m.dpool = dpool;
        m.dpool_cap = dpool_cap;
        m.route_pos = route_pos;
        m.rp_cap = rp_cap;
        m.kref = kref;
        m.khash = khash;
        m.id_cap = id_cap;
        m.kpool = kpool;
        m.bc = bc;
        m.fo_dgroup = fo_dgroup;
        m.fo_cap = fo_cap;
        return m;
    }

    // ---- full (re)load.  keys: packed route keys, any order (a KV scan yields them sorted: that is the fast path) ----
    bool rebuild(const uint8_t* keys, const uint32_t* key_off, uint32_t n) {
        error.clear();
        std::vector<uint8_t> sorted_bytes; // only used when the input was not strictly ascending
        std::vector<uint32_t> sorted_off;
        for (int attempt = 0; attempt < 2; attempt++) {
            uint32_t err = 0;
            if (!rebuild_sorted(keys, key_off, n, err)) {
                if (err & ERR_BAD_KEY) return false;
                if ((err & ERR_UNSORTED) && attempt == 0) { // not a KV scan: order + de-duplicate on the host, once
                    sort_unique(keys, key_off, n, sorted_bytes, sorted_off);
                    keys = sorted_bytes.data();
                    key_off = sorted_off.data();
                    n = (uint32_t)sorted_off.size() - 1;
                    continue;
                }
                return false;
            }
            built = true;
            broken = false;
            generation++;
            return true;
        }
        return fail("rebuild: input could not be ordered");
    }

    // ---- post-commit mutations, applied in order.  op[i]: 0 = put, 1 = delete ----
    // apply = apply_begin + apply_end.  On the device apply_begin only ENQUEUES: the ops are uploaded on the executor's upload stream (beside
    // whatever the engine stream still runs), the stages follow on the engine stream behind the gate, the counters travel back into
    // page-locked memory; apply_end waits for them, lets the stage-by-stage loops finish what the gate stopped and does the bookkeeping.
    // The caller's buffers must stay valid in between; at most one batch is open.
    struct OpenApply {
        bool open = false;
        const uint8_t* keys = nullptr;
        const uint32_t* key_off = nullptr;
        const uint8_t* op = nullptr;
        uint32_t n = 0, n_put = 0;
        uint64_t kb = 0;
        OpBatch ob{};
        std::vector<uint32_t> put_rank;
    } open_apply;
    bool apply(const uint8_t* keys, const uint32_t* key_off, const uint8_t* op, uint32_t n, ApplyResult* res = nullptr) {
        return apply_begin(keys, key_off, op, n) && apply_end(res);
    }
    // sized: a batch of the carry-over behind reserve_like(old) (import_apply) -- all puts of keys `old` holds, `keys` is device memory
    bool apply_begin(const uint8_t* keys, const uint32_t* key_off, const uint8_t* op, uint32_t n, bool sized = false) {
        error.clear();
        OpenApply& oa = open_apply;
        if (oa.open) return fail("an apply batch is open: apply_end first");
        if (n == 0) return true;
        if (broken) return fail("the index is inconsistent after a failed batch: bmq_rebuild is required");
        if (!built && !reset_empty()) return false;
        const uint64_t kb = key_off[n];
        oa.put_rank.resize(n);
        uint32_t n_put = 0;
        for (uint32_t i = 0; i < n; i++) {
            oa.put_rank[i] = n_put;
            n_put += op[i] == 0;
        }
        if ((uint64_t)next_id + n_put >= 0xFFFFFFF0ull) return fail("route id space exhausted: bmq_rebuild re-numbers the routes");
        if (!ensure_keys(kb) || !ensure_ids(next_id + n_put) || !ensure_scratch(n, true)) return false;
        OpBatch ob = batch(n);
        ob.key_base = kpool_used;
        ob.id_base = next_id;
        ob.put_rank = s_put_rank;
        ob.op = s_op;
        ob.bulk = 0;
        ob.sized = sized ? 1 : 0;
        if (!x.upload_async(kpool + kpool_used, keys, kb) || !x.upload_async(s_key_off, key_off, sizeof(uint32_t) * ((size_t)n + 1)) ||
            !x.upload_async(s_op, op, n) || !x.upload_async(s_put_rank, oa.put_rank.data(), sizeof(uint32_t) * (size_t)n) || !x.uploads_done())
            return xfail();
        oa.keys = keys, oa.key_off = key_off, oa.op = op, oa.n = n, oa.n_put = n_put, oa.kb = kb, oa.ob = ob;
        if (Exec::gated) { // the stages back to back behind the gate, the counters on their way back: nothing waits here
            DistIndexMut ix = mut();
            // (the gate word and the per-batch counters are one memset; nothing is zeroed BETWEEN the stages any more: a stage that leaves a
            // counter non-zero closes the gate, and behind an open gate the counters are still zero -- round 5 spent three fill kernels on it)
            static_assert(offsetof(BuildCounters, err) == offsetof(BuildCounters, gate) + 8, "gate, its pad and the per-batch block are contiguous");
            if (!x.zero(&bc->gate, sizeof(BuildCounters) - offsetof(BuildCounters, gate)) || !x.prepare(ix, ob) || !x.prepare_check(ix, ob, dir_slots) || !x.gate(bc, 1) ||
                !x.locate(ix, ob) || !x.prepare_check(ix, ob, dir_slots) || !x.gate(bc, 2) || !x.zero(ob.group_done, n) ||
                !x.sort_targets(ob) || !x.group(ix, ob) || !x.gate(bc, 3) || !x.read_back_async(&hbc, bc, sizeof(BuildCounters)))
                return xfail();
        }
        oa.open = true;
        return true;
    }
    bool apply_end(ApplyResult* res = nullptr) {
        OpenApply& oa = open_apply;
        if (!oa.open) return true;
        oa.open = false;
        const uint32_t* const key_off = oa.key_off;
        const uint32_t n = oa.n, n_put = oa.n_put;
        const uint64_t kb = oa.kb;
        OpBatch ob = oa.ob;
        PhaseTimer pt(x);
        auto count_groups = [&]() { // what the group step of this round did (the counters are zeroed in front of every round)
            uint64_t a = 0, r = 0, du = 0;
            for (uint32_t c = 0; c < N_CTR_LANES; c++) a += hbc.n_added[c], r += hbc.n_removed[c], du += hbc.n_dups[c];
            n_routes += a;
            n_routes -= r;
            if (res) {
                res->added += (uint32_t)a;
                res->removed += (uint32_t)r;
                res->dups += (uint32_t)du;
            }
        };
        // ---- the stages back to back, ONE read-back (round 5; rounds 1-4: a read-back behind each of the three stages).  A stage that
        // leaves work for the host closes the gate (BuildCounters.gate): the stages behind it do nothing and the loops below -- the
        // stage-by-stage form, idempotent -- take over from that stage.  The common batch needs nothing from the host.
        uint32_t from = 1; // the stage the stage-by-stage form starts at; 4: nothing left to do
        bool groups_pending = false;
        if (Exec::gated) {
            if (!x.read_back_wait(&hbc, sizeof(BuildCounters))) return xfail();
            pt.lap("apply: prepare, locate, sort, groups (one read-back)");
            from = hbc.gate ? hbc.gate : 4;
            if (from >= 3) { // the group step ran (to the end, or up to the groups that found the id-list pool full)
                if (hbc.err) return broke("apply: group step failed");
                count_groups();
                groups_pending = hbc.n_deferred != 0;
                if (groups_pending && !grow_route_pos(hbc.rp_used + 2 * hbc.rp_need + 1024)) return false;
            }
            if (hbc.gate && !x.zero(&bc->gate, sizeof(uint32_t))) return xfail();
        }
        // ---- prepare: validate + tenants + growth bounds (re-run once if tenants had to be created) ----
        for (int round = 0; from <= 1; round++) {
            if (!zero_batch_counters()) return false;
            DistIndexMut ix = mut();
            if (!x.prepare(ix, ob) || !x.prepare_check(ix, ob, dir_slots) || !read_counters()) return xfail();
            if (hbc.err & ERR_BAD_KEY) return fail("malformed route key or op in apply batch"); // nothing was changed
            if (hbc.n_unknown == 0) break;
            if (round == 1) return fail("apply: tenant creation did not converge");
            std::vector<uint32_t> unk(hbc.n_unknown);
            if (!x.copy_out(unk.data(), ob.unknown_list, sizeof(uint32_t) * unk.size())) return xfail();
            std::unordered_map<std::string, uint64_t> need; // new tenant -> nodes its puts may add
            // (from this index's key pool, where apply_begin put the batch: the caller's pointer may be device memory -- the builder of the
            // next generation hands the keys over where they live.  A few keys one by one, many with one copy of the batch.)
            std::vector<uint8_t> kbuf;
            const bool whole = unk.size() > 8;
            if (whole) {
                kbuf.resize(kb);
                if (!x.copy_out(kbuf.data(), kpool + ob.key_base, kb)) return xfail();
            }
            for (uint32_t i : unk) {
                const size_t klen = key_off[i + 1] - key_off[i];
                if (!whole) {
                    kbuf.resize(klen);
                    if (!x.copy_out(kbuf.data(), kpool + ob.key_base + key_off[i], klen)) return xfail();
                }
                const std::string_view k((const char*)kbuf.data() + (whole ? key_off[i] : 0u), klen);
                const size_t tlen = ((size_t)(uint8_t)k[1] << 8) | (uint8_t)k[2]; // validated by prepare
                uint64_t levels = 1;
                for (size_t q = 3 + tlen; q < k.size(); q++) levels += k[q] == 0;
                need[std::string(k.substr(3, tlen))] += levels;
            }
            for (auto& e : need)
                if (!create_tenant(e.first, e.second, 0)) return false;
            if (!flush_directory()) return false;
            ob.grow_list = s_grow; // the directory may have grown, and its scratch with it
        }
        if (from <= 1) {
            pt.lap("apply: prepare (+ tenants)");
            if (!grow_flagged_regions(ob)) return false;
            pt.lap("apply: region growth");
        }
        // ---- locate (idempotent: re-run after growing what it ran out of) ----
        for (int attempt = 0; from <= 2; attempt++) {
            if (attempt == 8) return broke("apply: growth did not converge");
            if (!zero_batch_counters()) return false;
            DistIndexMut ix = mut();
            if (!x.locate(ix, ob) || !x.prepare_check(ix, ob, dir_slots) || !read_counters()) return xfail();
            if (hbc.err & ERR_STUCK) return broke("apply: a probe loop did not terminate");
            if (!(hbc.err & (ERR_DICT_FULL | ERR_REGION_FULL)) && hbc.n_grow == 0) break;
            if ((hbc.err & ERR_DICT_FULL) && !grow_dict(std::max<uint64_t>((uint64_t)dict_slots * 4, 4096), (uint64_t)dpool_cap * 2 + kb)) return false;
            if (!grow_flagged_regions(ob)) return false;
        }
        // ---- sort by filter node, apply the groups ----
        if (from <= 2) {
            pt.lap("apply: locate");
            if (!x.zero(ob.group_done, n) || !x.sort_targets(ob)) return xfail();
            pt.lap("apply: sort by filter node");
        }
        for (int attempt = 0; from <= 2 || groups_pending; attempt++) {
            if (attempt == 8) return broke("apply: id-list pool growth did not converge");
            if (!zero_batch_counters()) return false;
            DistIndexMut ix = mut();
            if (!x.group(ix, ob) || !read_counters()) return xfail();
            if (hbc.err) return broke("apply: group step failed");
            count_groups();
            if (hbc.n_deferred == 0) break;
            if (!grow_route_pos(hbc.rp_used + 2 * hbc.rp_need + 1024)) return false;
        }
        pt.lap("apply: groups");
        kpool_used += (kb + 15) & ~15ull;
        next_id += n_put;
        if ((uint64_t)hbc.n_tokens * 4 > dict_slots && !grow_dict((uint64_t)dict_slots * 4, dpool_cap)) return false;
        return true;
    }

    // ---- maintenance: re-build the index from its own live routes.  Drops abandoned regions and id lists, dead trie nodes and
    // dictionary tokens nobody uses any more; the key store shrinks to the live keys.  Route ids are re-numbered (ranks again):
    // a new generation, exactly like a bmq_rebuild with the current key set.
    bool compact() {
        error.clear();
        if (!built) return true;
        std::vector<uint32_t> ids(next_id);
        for (uint32_t i = 0; i < next_id; i++) ids[i] = i;
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off;
        if (!route_keys(ids.data(), next_id, bytes, off)) return false;
        if (off[next_id] >= 0xFFFFFFF0ull) return fail("compact: more than 4 GB of route keys");
        std::vector<uint8_t> kb;
        std::vector<uint32_t> ko{0};
        kb.reserve(bytes.size() + 16);
        for (uint32_t i = 0; i < next_id; i++)
            if (off[i + 1] > off[i]) { // live
                kb.insert(kb.end(), bytes.begin() + (long)off[i], bytes.begin() + (long)off[i + 1]);
                ko.push_back((uint32_t)kb.size());
            }
        kb.resize(kb.size() + 16, 0);
        return rebuild(kb.data(), ko.data(), (uint32_t)ko.size() - 1); // not ascending any more after churn: sorted on the host
    }

    // ---- tail records (bmq_layout.h): two passes over the slot table with per-node scratch (8 bytes per node, released at once) ----
    bool form_tails() {
        if (!tail_records || !built_regions()) return true;
        std::vector<TenantSlot> d(dir_slots);
        if (!x.copy_out(d.data(), dir, sizeof(TenantSlot) * (size_t)dir_slots)) return xfail();
        std::vector<TailRegion> regs;
        uint64_t ids = 0;
        for (const TenantSlot& t : d) {
            if (!(t.hash_lo | t.hash_hi) || t.buckets == 0) continue;
            regs.push_back({t.base, 2u * t.buckets, (uint32_t)ids, t.n_nodes + 1u});
            ids += (uint64_t)t.n_nodes + 1u;
        }
        if (regs.empty()) return true;
        if (ids >= 0xFFFFFFF0ull) return true; // (no records: the index still answers every lookup)
        std::sort(regs.begin(), regs.end(), [](const TailRegion& a, const TailRegion& b) { return a.base < b.base; });
        TailRegion* d_regs = (TailRegion*)x.alloc(sizeof(TailRegion) * regs.size());
        uint32_t* scratch = (uint32_t*)x.alloc(sizeof(uint32_t) * 2 * (size_t)ids);
        bool ok = d_regs && scratch;
        if (ok) {
            TailPass tp{d_regs, (uint32_t)regs.size(), scratch, scratch + ids};
            ok = x.copy_in(d_regs, regs.data(), sizeof(TailRegion) * regs.size()) && x.zero(scratch, sizeof(uint32_t) * (size_t)ids) &&
                 x.tails(mut(), tp, (uint32_t)trie_used) && x.sync();
        }
        if (d_regs) x.release(d_regs);
        if (scratch) x.release(scratch);
        return ok ? true : (d_regs && scratch ? xfail() : fail("out of memory (tail records)"));
    }
    bool built_regions() const { return trie != nullptr && trie_used != 0 && trie_used < 0xFFFFFFFFull; }

    // ---- id -> key ----
    // false + empty error: no such route (never existed or deleted)
    bool route_key(uint32_t id, std::string& out) {
        out.clear();
        if (!built || id >= next_id) return false;
        unsigned long long r = 0;
        if (!x.copy_out(&r, kref + id, sizeof(r))) return xfail();
        if (r == 0) return false;
        out.resize((size_t)(r >> KREF_LEN_SHIFT));
        if (!x.copy_out(out.data(), kpool + (r & KREF_OFF_MASK), out.size())) return xfail();
        return true;
    }
    // keys of many ids at once: out_off[n + 1], bytes appended to out (a dead id gives an empty key)
    bool route_keys(const uint32_t* ids, uint32_t n, std::vector<uint8_t>& out, std::vector<uint64_t>& out_off) {
        out.clear();
        out_off.assign((size_t)n + 1, 0);
        if (n == 0) return true;
        if (!built) return fail("no index");
        if (!ensure_buf(g_ids, g_ids_cap, n) || !ensure_buf(g_refs, g_refs_cap, n) || !ensure_buf(g_offs, g_offs_cap, (size_t)n + 1)) return false;
        std::vector<unsigned long long> refs(n);
        if (!x.copy_in(g_ids, ids, sizeof(uint32_t) * (size_t)n) || !x.gather_refs(mut(), g_ids, n, next_id, g_refs) ||
            !x.copy_out(refs.data(), g_refs, sizeof(unsigned long long) * (size_t)n))
            return xfail();
        for (uint32_t i = 0; i < n; i++) out_off[i + 1] = out_off[i] + (refs[i] >> KREF_LEN_SHIFT);
        const uint64_t total = out_off[n];
        out.resize(total);
        if (total == 0) return true;
        if (!ensure_buf(g_bytes, g_bytes_cap, total)) return false;
        if (!x.copy_in(g_offs, out_off.data(), sizeof(uint64_t) * ((size_t)n + 1)) || !x.gather_bytes(mut(), g_refs, g_offs, n, g_bytes) ||
            !x.copy_out(out.data(), g_bytes, total))
            return xfail();
        return true;
    }
    // ---- key -> id (bmq_routes_find): out_ids[i] = id of the live route whose key is keys[key_off[i] .. key_off[i + 1]), NONE if there is
    // none.  Read-only: the batch is uploaded into buffers of its own (not the key pool) and every key walks the index as a delete would,
    // without its side effects (find_key_one).  n_bad = malformed keys (an empty key, descending offsets, what key_parse refuses): the
    // ids mean nothing then.  find_fits: the buffers hold such a batch already (nothing is allocated or freed by the call).
    bool find_fits(uint32_t n, uint64_t key_bytes) const { return (size_t)n + 1 <= f_ids_cap && n <= f_refs_cap && key_bytes + 32 <= f_bytes_cap; }
    bool find_keys(const uint8_t* keys, const uint32_t* key_off, uint32_t n, uint32_t* out_ids, uint32_t& n_bad) {
        error.clear();
        n_bad = 0;
        if (n == 0) return true;
        std::vector<unsigned long long> refs(n);
        const uint32_t k0 = key_off[0];
        for (uint32_t i = 0; i < n; i++) {
            if (key_off[i + 1] <= key_off[i] || key_off[i + 1] - key_off[i] >= (1u << (64 - KREF_LEN_SHIFT))) { // (a reference holds 24 bits of length)
                n_bad++;
                continue;
            }
            refs[i] = (unsigned long long)(key_off[i] - k0) | ((unsigned long long)(key_off[i + 1] - key_off[i]) << KREF_LEN_SHIFT);
        }
        if (n_bad) return true;
        if (!built) { // no index: nothing is live, and a malformed key is still the caller's error (the parser the lookup runs, on the host)
            for (uint32_t i = 0; i < n; i++) {
                KeyView k;
                n_bad += key_parse(keys, key_off[i], key_off[i + 1], k) ? 0u : 1u;
            }
            std::fill(out_ids, out_ids + n, NONE);
            return true;
        }
        const uint64_t kb = key_off[n] - k0;
        if (dir_dirty && !flush_directory()) return false;
        if (!ensure_buf(f_bytes, f_bytes_cap, kb + 32) || !ensure_buf(f_refs, f_refs_cap, n) || !ensure_buf(f_ids, f_ids_cap, (size_t)n + 1)) return false;
        std::vector<uint32_t> got((size_t)n + 1);
        if (!x.copy_in_async(f_bytes, keys + k0, kb) || !x.copy_in_async(f_refs, refs.data(), sizeof(unsigned long long) * (size_t)n) ||
            !x.zero(f_ids + n, sizeof(uint32_t)) || !x.find_keys(mut(), KeySource{f_bytes, f_refs}, n, f_ids, f_ids + n) ||
            !x.copy_out(got.data(), f_ids, sizeof(uint32_t) * ((size_t)n + 1)))
            return xfail();
        n_bad = got[n];
        memcpy(out_ids, got.data(), sizeof(uint32_t) * (size_t)n);
        return true;
    }
    // the same for keys that lie in exec memory already (the carry of the member tables of shared subscriptions, bmq_share.h: the keys are
    // another generation's, read through its own references), on the executor `on`; *n_bad (exec memory, zeroed by the caller) += malformed keys
    template <class X> bool find_keys_in(X& on, const KeySource& ks, uint32_t n, uint32_t* out_ids, uint32_t* n_bad) {
        error.clear();
        if (n == 0 || !built) return true;
        if (dir_dirty && !flush_directory()) return false;
        return on.find_keys(mut(), ks, n, out_ids, n_bad) ? true : fail(on.err.empty() ? "exec failure" : on.err);
    }
    // ---- generation change: THIS index (the generation being built, behind reserve_like(old)) takes the live keys among old's ids [lo, hi).
    // Two steps, so that the caller needs to keep `old` still only for the first.  import_snapshot ENQUEUES a copy of old's key references
    // kref[lo, hi) on this index's executor (the caller ordered it behind whatever old was told so far) and notes where old's key bytes
    // lie -- the key pool is append-only, and while a generation change runs old keeps the blocks it outgrows (defer_release), so the
    // pointer stays good whatever old is told meanwhile.  import_apply does the rest on this index's executor alone: the references come
    // back (8 bytes per id: length + liveness), the live keys are gathered -- HBM to HBM, the bytes never visit the host -- and go through
    // the apply path as puts (no order required, so no sort) into regions that are already sized.
    struct Import {
        uint32_t n = 0;
        const uint8_t* old_kpool = nullptr;
    } imp;
    bool import_snapshot(DistIndex& old, uint32_t lo, uint32_t hi) {
        error.clear();
        imp = Import{};
        if (!old.built) return true;
        if (hi > old.next_id) hi = old.next_id;
        if (hi <= lo) return true;
        const uint32_t n = hi - lo;
        if (!ensure_buf(g_refs, g_refs_cap, n)) return false;
        if (!x.copy(g_refs, old.kref + lo, sizeof(unsigned long long) * (size_t)n)) return xfail();
        imp.n = n;
        imp.old_kpool = old.kpool;
        return true;
    }
    // sized = false: the batch of a bmq_routes_import -- keys of ANOTHER index, so tenants may be unknown and regions may grow; res counts
    // what the puts did (keys this index already held: dups).  Behind set_import_boundary the chunk's references go through the boundary
    // predicate first (on the device: k_b_boundary): a key outside is a dead id to everything below.
    bool import_apply(uint32_t& n_live, bool sized = true, ApplyResult* res = nullptr) {
        n_live = 0;
        const uint32_t n = imp.n;
        if (n == 0) return true;
        imp.n = 0;
        if (imp_bounded && !x.boundary_filter(g_refs, n, imp.old_kpool, imp_bnd.kb, imp_bnd.ctr())) return xfail();
        std::vector<unsigned long long> refs(n);
        if (!x.copy_out(refs.data(), g_refs, sizeof(unsigned long long) * (size_t)n)) return xfail();
        std::vector<uint64_t> offs((size_t)n + 1, 0);
        std::vector<uint32_t> live_off(1, 0u);
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t len = refs[i] >> KREF_LEN_SHIFT; // 0: no such route (never existed / deleted)
            offs[i + 1] = offs[i] + len;
            if (len) live_off.push_back((uint32_t)offs[i + 1]);
        }
        const uint64_t total = offs[n];
        if (total == 0) return true;
        if (total >= 0xFFFFFFF0ull) return fail("generation change: more than 4 GB of route keys in one chunk");
        if (!ensure_buf(g_offs, g_offs_cap, (size_t)n + 1) || !ensure_buf(g_bytes, g_bytes_cap, total + 16)) return false;
        DistIndexMut m = mut();
        m.kpool = const_cast<uint8_t*>(imp.old_kpool); // (gather_bytes reads the key pool and nothing else)
        if (!x.copy_in_async(g_offs, offs.data(), sizeof(uint64_t) * ((size_t)n + 1)) || !x.gather_bytes(m, g_refs, g_offs, n, g_bytes) || !x.sync()) return xfail();
        n_live = (uint32_t)live_off.size() - 1;
        const std::vector<uint8_t> puts(n_live, 0);
        return apply_begin(g_bytes, live_off.data(), puts.data(), n_live, sized) && apply_end(res);
    }
    // The generation being built takes only the keys inside `b` from here on (bmq_compact_begin_in); bmq_routes_import sets it per call.
    bool set_import_boundary(const Boundary& b) {
        if (b.bounded() && !built && !reset_empty()) return false; // (an index that never held a route: its first reset drops every buffer)
        imp_bounded = b.bounded();
        return !imp_bounded || stage_boundary(imp_bnd, b);
    }
    // bmq_routes_import: `snap` holds n key references of ANOTHER index of the same executor kind (a copy in exec memory), src_kpool its
    // key pool (kept readable by that index's defer_release).  The live keys inside the import boundary go through the ordinary apply path.
    bool import_refs(const unsigned long long* snap, uint32_t n, const uint8_t* src_kpool, ApplyResult& res) {
        error.clear();
        imp = Import{};
        if (n == 0) return true;
        if (!built && !reset_empty()) return false; // (before the chunk is staged: the first reset of an index drops every buffer)
        if (!ensure_buf(g_refs, g_refs_cap, n)) return false;
        if (!x.copy(g_refs, snap, sizeof(unsigned long long) * (size_t)n)) return xfail();
        imp.n = n;
        imp.old_kpool = src_kpool;
        uint32_t n_live = 0;
        return import_apply(n_live, false, &res);
    }
    // live routes inside `b` and the sum of their key lengths (reader.size(boundary), DW/hinter/FanoutSplitHinter.java:175-178): one pass
    // of the predicate over a scratch copy of kref[0, next_id); the index is not changed
    bool count_in(const Boundary& b, uint64_t& routes, uint64_t& bytes) {
        error.clear();
        routes = bytes = 0;
        if (!built || next_id == 0) return true;
        if (!ensure_buf(g_refs, g_refs_cap, next_id) || !stage_boundary(q_bnd, b)) return false;
        unsigned long long c[2] = {0, 0};
        if (!x.copy(g_refs, kref, sizeof(unsigned long long) * (size_t)next_id) || !x.boundary_filter(g_refs, next_id, kpool, q_bnd.kb, q_bnd.ctr()) ||
            !x.copy_out(c, q_bnd.ctr(), sizeof(c)))
            return xfail();
        routes = c[0];
        bytes = c[1];
        return true;
    }
    // ---- key-ordered window (bmq_routes_window; bmq_order_core.h): the ids of the first min(max_routes, C) of the C live routes whose key
    // is >= the cursor (> if exclusive; all live routes without a cursor), ascending in KV order; more = a further live key follows.
    // The cursor is key bytes (lo) or, by_id, the key of the live route lo_id (nothing is uploaded then: the sweep's next window begins
    // behind the last key of the one before).  Read-only.  One pass flags and compacts the candidates (o_flag); then a list of ids is
    // split by <= 255 pivot keys taken at a fixed stride of it (o_pivots ranks them, o_bucket bins every id and counts, the host reads
    // the counters and decides per bin: kept or dropped, o_scatter moves the kept bins, in bin order, into the other list) until every
    // piece holds <= ORDER_BUCKET_MAX ids; neighbouring small bins make one piece.  Bins behind the one where the running count reaches
    // `keep` are dropped, so the same round narrows C candidates to max_routes and orders what it keeps.  The pieces are ranked by
    // counting in one launch (o_leaves).  A piece that is split again lies inside ONE bin of even number, which holds none of the
    // round's pivots (order_bin_one) while its list held 255: every round shortens what it splits, so the loop ends.
    // A piece at [off, off + n) of one list owns that range of both lists: its children are written there.
    // the scratch holds such a call already (nothing is allocated or freed by it)
    bool window_fits(uint32_t lo_len) const {
        return !built || next_id == 0 ||
               (o_list_cap[0] >= next_id && o_list_cap[1] >= next_id && o_bins_cap >= next_id && o_ctr_cap >= O_CTR_WORDS && o_out_cap >= ORDER_WINDOW_MAX &&
                o_leaves_cap >= O_LEAVES_MAX && o_key_cap >= (size_t)lo_len + 32);
    }
    uint64_t window_scratch_bytes() const {
        return 4 * (uint64_t)(o_list_cap[0] + o_list_cap[1] + o_ctr_cap + o_out_cap) + 2 * (uint64_t)o_bins_cap + sizeof(OrderLeaf) * (uint64_t)o_leaves_cap + o_key_cap;
    }
    bool window(const uint8_t* lo, uint32_t lo_len, bool has_lo, bool exclusive, bool by_id, uint32_t lo_id, uint32_t max_routes, uint32_t* out_ids,
                uint32_t& out_n, uint32_t& more, OrderStats& st) {
        error.clear();
        out_n = more = 0;
        st.n_calls++;
        if (max_routes > ORDER_WINDOW_MAX) return fail("window: more than BMQ_WINDOW_MAX routes asked for");
        if (!built || next_id == 0) return true;
        if (by_id && (lo_id >= next_id || !has_lo)) return fail("window: no such route to begin behind");
        if (!ensure_buf(o_list[0], o_list_cap[0], next_id) || !ensure_buf(o_list[1], o_list_cap[1], next_id) || !ensure_buf(o_bins, o_bins_cap, next_id) ||
            !ensure_buf(o_ctr, o_ctr_cap, O_CTR_WORDS) || !ensure_buf(o_out, o_out_cap, ORDER_WINDOW_MAX) || !ensure_buf(o_leaves, o_leaves_cap, O_LEAVES_MAX) ||
            !ensure_buf(o_key, o_key_cap, (size_t)lo_len + 32))
            return false;
        OrderCursor cur{};
        cur.key = o_key;
        cur.len = by_id ? 0u : lo_len;
        cur.flags = (has_lo ? 1u : 0u) | (exclusive ? 2u : 0u) | (by_id ? 4u : 0u);
        cur.id = lo_id;
        uint32_t* hist = o_ctr + 16;
        uint32_t* cursor = hist + ORDER_BINS;
        uint32_t* base = cursor + ORDER_BINS;
        uint32_t* piv = base + ORDER_BINS;
        uint32_t C = 0;
        if ((has_lo && !by_id && lo_len && !x.copy_in_async(o_key, lo, lo_len)) || !x.zero(o_ctr, sizeof(uint32_t)) ||
            !x.o_flag(mut(), next_id, cur, o_list[0], o_ctr) || !x.copy_out(&C, o_ctr, sizeof(C)))
            return xfail();
        if (C > next_id) return fail("window: more candidates than ids");
        st.n_candidates += C;
        const uint32_t take = std::min(C, max_routes);
        more = C > max_routes ? 1u : 0u;
        if (take == 0) return true;
        struct Piece {
            uint32_t list, off, n, keep, out, depth;
        };
        std::vector<Piece> work{Piece{0u, 0u, C, take, 0u, 0u}};
        std::vector<OrderLeaf> leaves;
        std::vector<uint32_t> h(ORDER_BINS), b(ORDER_BINS);
        while (!work.empty()) {
            const Piece s = work.back();
            work.pop_back();
            if (s.n <= ORDER_BUCKET_MAX) {
                leaves.push_back(OrderLeaf{s.list, s.off, s.n, s.keep, s.out});
                st.max_bucket = std::max<uint64_t>(st.max_bucket, s.n);
                continue;
            }
            st.n_rounds++;
            if (s.depth) st.n_rebucketed++;
            const uint32_t* src = o_list[s.list] + s.off;
            if (!x.zero(hist, sizeof(uint32_t) * 2 * ORDER_BINS) || !x.o_pivots(mut(), src, s.n / ORDER_PIVOTS, ORDER_PIVOTS, piv) ||
                !x.o_bucket(mut(), src, s.n, piv, ORDER_PIVOTS, o_bins, hist) || !x.copy_out(h.data(), hist, sizeof(uint32_t) * ORDER_BINS))
                return xfail();
            uint32_t acc = 0, c_at = 0, c_n = 0, seen = 0; // kept so far; the piece being gathered from small neighbouring bins
            auto flush = [&]() {
                if (c_n) work.push_back(Piece{s.list ^ 1u, s.off + c_at, c_n, std::min(c_n, s.keep - c_at), s.out + c_at, s.depth + 1});
                c_n = 0;
            };
            for (uint32_t k = 0; k < ORDER_BINS; k++) {
                const uint32_t cnt = h[k];
                seen += cnt;
                b[k] = ORDER_DROP;
                if (cnt == 0 || acc >= s.keep) continue;
                if (cnt >= s.n) return fail("window: a bin holds its whole list");
                b[k] = s.off + acc;
                if (c_n + cnt > ORDER_BUCKET_MAX) flush();
                if (c_n == 0) c_at = acc;
                c_n += cnt;
                acc += cnt;
                if (cnt > ORDER_BUCKET_MAX) flush(); // (a piece of its own: it is split again)
            }
            flush();
            if (seen != s.n || acc < s.keep) return fail("window: the bins do not add up");
            if (!x.copy_in_async(base, b.data(), sizeof(uint32_t) * ORDER_BINS) || !x.o_scatter(src, o_bins, s.n, base, cursor, o_list[s.list ^ 1u]) || !x.sync())
                return xfail();
        }
        if (leaves.size() > O_LEAVES_MAX) return fail("window: more pieces than ids");
        st.n_bucket_sorts += leaves.size();
        if (!x.copy_in_async(o_leaves, leaves.data(), sizeof(OrderLeaf) * leaves.size()) ||
            !x.o_leaves(mut(), o_list[0], o_list[1], o_leaves, (uint32_t)leaves.size(), o_out) || !x.copy_out(out_ids, o_out, sizeof(uint32_t) * (size_t)take))
            return xfail();
        out_n = take;
        return true;
    }
    // ---- the dist worker's GC sweep (DW/DistWorkerCoProc.java:554-701) over positions of the key order, the keys fetched window by window
    // as the loop reaches them: the first window of a phase from its cursor, every further one behind the last key of the one before
    // (by id: nothing is uploaded).  include/bmq.h, bmq_routes_gc_sweep, says what the loop does; out_ids[0 .. min(inspected, cap)).
    struct SweepResult {
        uint64_t inspected = 0;
        bool wrapped = false, has_next = false;
        uint32_t next_id = 0;
    };
    static uint64_t sweep_keys_needed(uint32_t step_hint, uint32_t scan_quota) { // of one phase: the last inspected position, and the one the cursor ends on
        const uint64_t step = std::max<uint32_t>(step_hint, 1u), quota = scan_quota > 0 ? (uint64_t)scan_quota : 256 * step;
        return (quota - 1) * step + 2;
    }
    bool gc_sweep(const uint8_t* start, uint32_t start_len, bool has_start, uint32_t step_hint, uint32_t scan_quota, uint32_t* out_ids, uint32_t cap, SweepResult& res,
                  OrderStats& st) {
        res = SweepResult{};
        const uint64_t step = std::max<uint32_t>(step_hint, 1u), quota = scan_quota > 0 ? (uint64_t)scan_quota : 256 * step;
        const uint64_t need = sweep_keys_needed(step_hint, scan_quota);
        if (need > 16ull * ORDER_WINDOW_MAX) return fail("a sweep of more than 16 windows per phase");
        struct Stream { // the live keys from a cursor on, in key order
            std::vector<uint32_t> ids;
            uint64_t budget;  // keys the sweep can still ask for
            bool more = true; // keys may follow ids.back()
        } a{{}, need}, b{{}, need}; // from the start key; from the first key
        bool failed = false;
        auto at = [&](Stream& sm, bool from_start, uint64_t i) -> uint32_t { // the id at position i of a stream, NONE behind its last key
            while (i >= sm.ids.size()) {
                if (!sm.more || sm.budget == 0) return NONE;
                const uint32_t want = (uint32_t)std::min<uint64_t>(sm.budget, ORDER_WINDOW_MAX);
                const size_t have = sm.ids.size();
                sm.ids.resize(have + want);
                uint32_t n = 0, m = 0;
                const bool ok = have ? window(nullptr, 0, true, true, true, sm.ids[have - 1], want, sm.ids.data() + have, n, m, st)
                                     : window(from_start ? start : nullptr, from_start ? start_len : 0u, from_start && has_start, false, false, 0, want, sm.ids.data() + have, n, m, st);
                if (!ok) {
                    failed = true;
                    return NONE;
                }
                sm.ids.resize(have + n);
                sm.budget -= n;
                sm.more = m != 0;
                if (n == 0) return NONE;
            }
            return sm.ids[i];
        };
        const uint32_t first = at(a, true, 0); // K[p0]: the session's start key
        if (failed) return false;
        if (first == NONE) { // (:584-591: nothing at or behind the cursor, whatever lies in front of it)
            res.wrapped = true;
            return true;
        }
        uint64_t pos = 0; // a position of the stream in use
        uint32_t next = NONE;
        for (;;) {
            uint32_t id = res.wrapped ? at(b, false, pos) : at(a, true, pos);
            if (id == NONE && !res.wrapped && !failed) { // the tail, the first time: on from the first key
                res.wrapped = true;
                pos = 0;
                id = at(b, false, 0);
            }
            if (failed) return false;
            if (id == NONE) break;            // the tail again
            if (res.wrapped && id == first) { // the start key after the wrap: the cursor stays on it
                next = id;
                break;
            }
            if (res.inspected < cap) out_ids[res.inspected] = id;
            res.inspected++;
            if (res.inspected >= quota) { // one position on, whatever the step
                next = res.wrapped ? at(b, false, pos + 1) : at(a, true, pos + 1);
                if (failed) return false;
                break;
            }
            pos += step;
        }
        res.has_next = next != NONE;
        res.next_id = next != NONE ? next : 0u;
        return true;
    }
    // The per-tenant census of the live keys inside `b` (TenantsStats.doReset, DW/TenantsStats.java:229-246: normal and shared routes per
    // tenant from the key's flag; :140-162: the tenant's space): one READ-ONLY pass over kref[0, next_id) (on the device: k_b_census,
    // bmq_census_kernels.h) into a table of four 64-bit counters per directory slot, zeroed per call.  Tenants with nothing inside are
    // left out; the result is in byte order of the tenant ids.
    struct TenantStat {
        std::string tenant;
        uint64_t n_normal = 0, n_unordered_share = 0, n_ordered_share = 0, key_bytes = 0;
    };
    bool tenant_stats(const Boundary& b, std::vector<TenantStat>& out) {
        error.clear();
        out.clear();
        if (!built || next_id == 0 || dir_slots == 0) return true;
        if (dir_dirty && !flush_directory()) return false;
        const size_t words = 4 * (size_t)dir_slots;
        if (!ensure_buf(g_census, g_census_cap, words) || !stage_boundary(q_bnd, b)) return false;
        std::vector<unsigned long long> t(words);
        if (!x.zero(g_census, sizeof(unsigned long long) * words) || !x.census(mut(), next_id, q_bnd.kb, g_census) ||
            !x.copy_out(t.data(), g_census, sizeof(unsigned long long) * words))
            return xfail();
        for (const auto& [name, d] : tenant_slot) {
            const unsigned long long* c = t.data() + 4 * (size_t)d;
            if ((c[0] | c[1] | c[2]) == 0) continue;
            out.push_back(TenantStat{name, c[0], c[1], c[2], c[3]});
        }
        std::sort(out.begin(), out.end(), [](const TenantStat& a, const TenantStat& c) { // unsigned byte order, a proper prefix first
            const size_t m = std::min(a.tenant.size(), c.tenant.size());
            const int r = m ? memcmp(a.tenant.data(), c.tenant.data(), m) : 0;
            return r ? r < 0 : a.tenant.size() < c.tenant.size();
        });
        return true;
    }
    // ---- per-prefix census (bmq_routes_prefix_census; bmq_prefix_core.h): for each of n byte prefixes (prefix i = bytes[off[i], off[i + 1]),
    // any order, repeats and nesting allowed) the live keys that start with it, per flag, and the sum of their lengths -- what
    // reader.size([prefix, upperBound(prefix))) tells the split hinter per prefix (DW/hinter/FanoutSplitHinter.java:175-178), for a whole
    // mutation batch in ONE READ-ONLY pass over kref[0, next_id) (on the device: k_b_prefix_census, bmq_prefix_kernels.h).  The host sorts
    // and de-duplicates the prefixes (at most PREFIX_MAX strings) and links every distinct one to its parent; the pass adds every key to
    // the deepest prefix it has; the sums are carried to the parents here and copied out through the input-to-slot map.
    // before_grow() runs before the scratch of the call is allocated anew (a free waits for every stream of the device).
    static size_t prefix_need(size_t m, size_t bytes) { return 32 * m + 4 * (m + 1) + 4 * m + bytes + 16; }
    template <class F> bool prefix_census(const uint8_t* bytes, const uint32_t* off, uint32_t n, uint64_t* out, PrefixStats& stats, F&& before_grow) {
        error.clear();
        for (size_t i = 0; i < 4 * (size_t)n; i++) out[i] = 0;
        stats.n_calls++;
        stats.n_prefixes += n;
        if (n == 0) return true;
        auto at = [&](uint32_t i) { return bytes + off[i]; };
        auto len = [&](uint32_t i) { return (unsigned long long)(off[i + 1] - off[i]); };
        std::vector<uint32_t> order(n);
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return key_compare(at(a), len(a), at(c), len(c)) < 0; });
        std::vector<uint32_t> slot_of(n), rep; // input -> table slot; table slot -> one input that holds its bytes
        for (uint32_t j = 0; j < n; j++) {
            if (j == 0 || key_compare(at(order[j - 1]), len(order[j - 1]), at(order[j]), len(order[j])) != 0) rep.push_back(order[j]);
            slot_of[order[j]] = (uint32_t)rep.size() - 1;
        }
        const uint32_t m = (uint32_t)rep.size();
        // the parents: sorted with a proper prefix first, the table is the preorder of the prefixes' trie -- a stack holds the chain of
        // the entry before, and the nearest entry of it that is a proper prefix of this one is the parent
        std::vector<uint32_t> parent(m, NONE), depth(m, 0), stack;
        uint64_t nested = 0, chain = 0, total = 0;
        for (uint32_t s = 0; s < m; s++) {
            while (!stack.empty() && !prefix_is_of(at(rep[stack.back()]), len(rep[stack.back()]), at(rep[s]), len(rep[s]))) stack.pop_back();
            if (!stack.empty()) {
                parent[s] = stack.back();
                depth[s] = depth[stack.back()] + 1;
                nested++;
                chain = std::max<uint64_t>(chain, depth[s]);
            }
            stack.push_back(s);
            total += len(rep[s]);
        }
        stats.n_distinct += m;
        stats.n_nested += nested;
        stats.max_chain = std::max(stats.max_chain, chain);
        if (!built || next_id == 0) return true;
        stats.n_keys_scanned += next_id;
        // exec memory: [4 m counters][m + 1 offsets][m parents][the prefixes' bytes]
        const size_t o_off = 32 * (size_t)m, o_par = o_off + 4 * ((size_t)m + 1), o_bytes = o_par + 4 * (size_t)m, need = prefix_need(m, total);
        if (need > g_prefix_cap) before_grow();
        if (!ensure_buf(g_prefix, g_prefix_cap, need)) return false;
        std::vector<uint8_t> h(need - o_off, 0);
        uint32_t* h_off = reinterpret_cast<uint32_t*>(h.data());
        uint32_t* h_par = reinterpret_cast<uint32_t*>(h.data() + (o_par - o_off));
        uint8_t* h_bytes = h.data() + (o_bytes - o_off);
        uint32_t pos = 0;
        for (uint32_t s = 0; s < m; s++) {
            h_off[s] = pos;
            h_par[s] = parent[s];
            if (len(rep[s])) memcpy(h_bytes + pos, at(rep[s]), len(rep[s]));
            pos += (uint32_t)len(rep[s]);
        }
        h_off[m] = pos;
        PrefixTable T{};
        T.bytes = g_prefix + o_bytes;
        T.off = reinterpret_cast<const uint32_t*>(g_prefix + o_off);
        T.parent = reinterpret_cast<const uint32_t*>(g_prefix + o_par);
        T.n = m;
        unsigned long long* table = reinterpret_cast<unsigned long long*>(g_prefix);
        std::vector<unsigned long long> t(4 * (size_t)m);
        if (!x.zero(g_prefix, o_off) || !x.copy_in_async(g_prefix + o_off, h.data(), h.size()) || !x.prefix_census(mut(), next_id, T, table) ||
            !x.copy_out(t.data(), g_prefix, o_off))
            return xfail();
        for (uint32_t s = m; s-- > 0;) { // a child sorts behind its parent: its sums are complete when its turn comes
            if (parent[s] == NONE) continue;
            for (uint32_t w = 0; w < 4; w++) t[4 * (size_t)parent[s] + w] += t[4 * (size_t)s + w];
        }
        for (uint32_t i = 0; i < n; i++) // (repeated inputs share a slot)
            for (uint32_t w = 0; w < 4; w++) out[4 * (size_t)i + w] = t[4 * (size_t)slot_of[i] + w];
        return true;
    }
    // The buffers a chunk of `n` ids / `bytes` key bytes of a generation change goes through, taken NOW: the first bmq_compact_poll used to
    // allocate them -- a dozen device allocations beside a saturated matcher, the one batch of a compaction that took 10 ms instead of 0.35.
    bool reserve_import(uint32_t n, uint64_t bytes) {
        return ensure_buf(g_refs, g_refs_cap, n) && ensure_buf(g_offs, g_offs_cap, (size_t)n + 1) && ensure_buf(g_bytes, g_bytes_cap, bytes + 16) &&
               ensure_scratch(n, true);
    }
    // blocks this index outgrew while another generation was being built from it
    bool defer_release = false;
    std::vector<void*> graveyard;
    void release_deferred() {
        for (void* q : graveyard) x.release(q);
        graveyard.clear();
    }
    uint32_t id_bound() const { return next_id; } // ids handed out so far (live or not)
    // Room for everything a generation change is about to hand over, taken once: every tenant of `old` that has routes gets its region at
    // the size its trie had there (dead nodes included: an upper bound), the trie pool, the dictionary, the id-list pool, the key store
    // and the id tables likewise.  The batches that carry the keys over then meet no unknown tenant and grow nothing.
    // bound: the next generation keeps the keys inside it only (bmq_compact_begin_in).  A tenant whose key prefix `00 | u16be(len) | tenant`
    // lies wholly outside gets no region and no directory entry; the key store and the id tables take what is inside.
    bool reserve_like(DistIndex& old, const Boundary* bound = nullptr) {
        error.clear();
        if (!built && !reset_empty()) return false;
        if (!old.built) return true;
        if (!old.read_counters()) return fail(old.x.err);
        const bool bounded = bound && bound->bounded();
        uint64_t in_routes = 0, in_bytes = 0;
        if (bounded && !old.count_in(*bound, in_routes, in_bytes)) return fail(old.error);
        auto leaves = [&](const TenantSlot& t) {
            if (!bounded) return false;
            std::string prefix(3, '\0');
            prefix[1] = (char)(t.name_len >> 8), prefix[2] = (char)(t.name_len & 0xFF);
            prefix.append((const char*)old.names_h.data() + t.name_off, t.name_len);
            return bound->excludes_prefix(prefix);
        };
        std::vector<TenantSlot> d(old.dir_slots);
        if (old.dir_slots && !old.x.copy_out(d.data(), old.dir, sizeof(TenantSlot) * (size_t)old.dir_slots)) return fail(old.x.err);
        uint64_t slots = 0, n_ten = 0;
        for (auto& t : d)
            if ((t.hash_lo | t.hash_hi) && t.n_routes && !leaves(t)) slots += 2ull * buckets_for((uint64_t)t.n_nodes + 1), n_ten++;
        if (trie_used + slots > trie_cap) {
            if (trie_used + slots >= 0xFFFFFFF0ull) return fail("trie too large (2^32 slots)");
            const uint64_t cap = std::min<uint64_t>(trie_used + slots + (tiny ? 0 : slots / 8 + (1u << 16)), 0xFFFFFFF0ull);
            if (!regrow(trie, trie_used, cap)) return false;
            if (!x.fill_slots(trie + trie_used, cap - trie_used)) return xfail();
            trie_cap = cap;
        }
        if (!ensure_directory(tenant_slot.size() + n_ten)) return false;
        for (auto& t : d)
            if ((t.hash_lo | t.hash_hi) && t.n_routes && !leaves(t) &&
                !create_tenant(std::string((const char*)old.names_h.data() + t.name_off, t.name_len), (uint64_t)t.n_nodes + 1, 0))
                return false;
        if (!flush_directory()) return false;
        if (old.dict_slots > dict_slots && !grow_dict(old.dict_slots, old.dpool_cap)) return false;
        if (!grow_route_pos(old.hbc.rp_used + 1024)) return false; // (lists are handed out in blocks: the old pool's size, not the live words)
        // (bounded: every chunk of the carry-over pads its keys to 16 bytes, a chunk may be one key; what the log replays grows the store)
        const uint64_t key_room = bounded ? std::min<uint64_t>(old.kpool_used, in_bytes + 16 * in_routes + 16) : old.kpool_used;
        return ensure_keys(key_room) && ensure_ids(std::min<uint64_t>((uint64_t)next_id + (bounded ? in_routes : old.next_id) + 64, 0xFFFFFFF0ull));
    }
    // exact lookup (inspection only -- never used for matching): ids stored under (tenant, MQTT filter)
    bool find(std::string_view tenant, std::string_view filter, std::vector<uint32_t>& ids) {
        ids.clear();
        if (!built) return true;
        const size_t qn = tenant.size() + filter.size();
        std::vector<uint8_t> q(qn + 32, 0);
        if (!tenant.empty()) memcpy(q.data(), tenant.data(), tenant.size());
        if (!filter.empty()) memcpy(q.data() + tenant.size(), filter.data(), filter.size());
        if (!ensure_buf(g_bytes, g_bytes_cap, q.size())) return false;
        uint32_t cap = 1024;
        for (;;) {
            if (!ensure_buf(g_ids, g_ids_cap, (size_t)cap + 1)) return false;
            if (!x.copy_in(g_bytes, q.data(), q.size()) ||
                !x.find(mut(), g_bytes, (uint32_t)tenant.size(), (uint32_t)filter.size(), g_ids, cap))
                return xfail();
            uint32_t cnt = 0;
            if (!x.copy_out(&cnt, g_ids, sizeof(cnt))) return xfail();
            if (cnt > cap) {
                cap = cnt;
                continue;
            }
            ids.resize(cnt);
            if (cnt && !x.copy_out(ids.data(), g_ids + 1, sizeof(uint32_t) * (size_t)cnt)) return xfail();
            return true;
        }
    }
    bool stats(DistIndexStats& st) {
        st = DistIndexStats{};
        if (!built) return true;
        if (!read_counters()) return xfail();
        std::vector<TenantSlot> d(dir_slots);
        if (!x.copy_out(d.data(), dir, sizeof(TenantSlot) * (size_t)dir_slots)) return xfail();
        for (auto& t : d)
            if (t.hash_lo | t.hash_hi) {
                st.n_tenants += t.n_routes != 0 ? 1 : 0;
                st.n_nodes += t.n_nodes;
            }
        st.n_routes = n_routes;
        st.n_tokens = hbc.n_tokens;
        st.trie_slots = trie_used;
        st.dict_slots = dict_slots;
        st.id_list_words = hbc.rp_used;
        st.id_list_garbage = hbc.rp_garbage;
        st.trie_garbage_slots = trie_garbage;
        st.key_bytes = kpool_used;
        st.next_id = next_id;
        st.bytes = trie_cap * sizeof(TrieSlot) + (uint64_t)dir_slots * sizeof(TenantSlot) + names_cap + (uint64_t)dict_slots * sizeof(DictSlot) +
                   dpool_cap + rp_cap * 4 + (uint64_t)id_cap * 12 + kpool_cap;
        return true;
    }

    void drop() {
        auto rel = [&](auto*& p) {
            if (p) x.release((void*)p);
            p = nullptr;
        };
        release_deferred();
        rel(trie); rel(dir); rel(names); rel(dict); rel(dpool); rel(route_pos); rel(kref); rel(khash); rel(kpool); rel(bc);
        rel(s_key_off); rel(s_op); rel(s_put_rank); rel(s_dir_slot); rel(s_nn); rel(s_flag); rel(s_target); rel(s_order);
        rel(s_sorted_target); rel(s_group_done); rel(s_unknown); rel(s_grow); rel(s_bt_first); rel(s_bt_nodes); rel(s_bt_keys); rel(s_bt_dir);
        rel(g_ids); rel(g_refs); rel(g_offs); rel(g_bytes); rel(g_census); rel(g_prefix); rel(q_bnd.buf); rel(imp_bnd.buf);
        rel(f_bytes); rel(f_refs); rel(f_ids);
        f_bytes_cap = f_refs_cap = f_ids_cap = 0;
        rel(o_list[0]); rel(o_list[1]); rel(o_bins); rel(o_ctr); rel(o_out); rel(o_leaves); rel(o_key);
        o_list_cap[0] = o_list_cap[1] = o_bins_cap = o_ctr_cap = o_out_cap = o_leaves_cap = o_key_cap = 0;
        q_bnd = imp_bnd = StagedBoundary{};
        imp_bounded = false;
        trie_cap = trie_used = 0; dir_slots = 0; names_cap = names_used = 0; dict_slots = 0; dpool_cap = 0; rp_cap = 0; id_cap = next_id = 0;
        kpool_cap = kpool_used = 0; s_cap = 0; s_bt_cap = 0; s_grow_cap = 0; g_ids_cap = g_refs_cap = g_offs_cap = g_bytes_cap = g_census_cap = g_prefix_cap = 0;
        tenant_slot.clear(); free_regions.clear(); dir_h.clear(); names_h.clear(); trie_garbage = 0;
        built = false;
    }

private:
    // ---- scratch in exec memory ----
    uint32_t *s_key_off = nullptr, *s_put_rank = nullptr, *s_dir_slot = nullptr, *s_nn = nullptr, *s_flag = nullptr, *s_order = nullptr,
             *s_unknown = nullptr, *s_grow = nullptr, *s_bt_first = nullptr, *s_bt_nodes = nullptr, *s_bt_keys = nullptr, *s_bt_dir = nullptr;
    uint8_t *s_op = nullptr, *s_group_done = nullptr;
    unsigned long long *s_target = nullptr, *s_sorted_target = nullptr;
    size_t s_cap = 0, s_bt_cap = 0, s_grow_cap = 0;
    uint32_t* g_ids = nullptr;
    unsigned long long* g_refs = nullptr;
    uint64_t* g_offs = nullptr;
    uint8_t* g_bytes = nullptr;
    size_t g_ids_cap = 0, g_refs_cap = 0, g_offs_cap = 0, g_bytes_cap = 0;
    unsigned long long* g_census = nullptr; // tenant_stats: four counters per directory slot
    size_t g_census_cap = 0;
    uint8_t* g_prefix = nullptr; // prefix_census: [four counters per distinct prefix][offsets][parents][prefix bytes]
    size_t g_prefix_cap = 0;
    uint8_t* f_bytes = nullptr; // find_keys: the batch's key bytes, references and ids (+ the count of malformed keys)
    unsigned long long* f_refs = nullptr;
    uint32_t* f_ids = nullptr;
    size_t f_bytes_cap = 0, f_refs_cap = 0, f_ids_cap = 0;
    // window: the two id lists, the bin of every id of the list being split, [candidates | 16 .. : counters per bin, places taken per
    // bin, the bins' places, the sorted pivots], the window, the pieces to rank, the cursor key
    static constexpr size_t O_CTR_WORDS = 16 + 3 * ORDER_BINS + 256, O_LEAVES_MAX = ORDER_WINDOW_MAX + 1;
    uint32_t* o_list[2] = {nullptr, nullptr};
    uint16_t* o_bins = nullptr;
    uint32_t *o_ctr = nullptr, *o_out = nullptr;
    OrderLeaf* o_leaves = nullptr;
    uint8_t* o_key = nullptr;
    size_t o_list_cap[2] = {0, 0}, o_bins_cap = 0, o_ctr_cap = 0, o_out_cap = 0, o_leaves_cap = 0, o_key_cap = 0;
    // a boundary in exec memory: [inside keys, their bytes: two 64-bit counters][start key][end key]
    struct StagedBoundary {
        uint8_t* buf = nullptr;
        size_t cap = 0;
        KeyBoundary kb{};
        unsigned long long* ctr() const { return reinterpret_cast<unsigned long long*>(buf); }
    } q_bnd, imp_bnd; // of count_in / of the import path: a count between two chunks of an import must not replace the import's
    bool imp_bounded = false;
    bool stage_boundary(StagedBoundary& s, const Boundary& b) { // (counters zeroed)
        const size_t need = 16 + b.start.size() + b.end.size();
        if (!ensure_buf(s.buf, s.cap, need)) return false;
        std::vector<uint8_t> h(need, 0);
        if (!b.start.empty()) memcpy(h.data() + 16, b.start.data(), b.start.size());
        if (!b.end.empty()) memcpy(h.data() + 16 + b.start.size(), b.end.data(), b.end.size());
        if (!x.copy_in(s.buf, h.data(), need)) return xfail();
        s.kb.start = s.buf + 16;
        s.kb.end = s.buf + 16 + b.start.size();
        s.kb.start_len = (uint32_t)b.start.size();
        s.kb.end_len = (uint32_t)b.end.size();
        s.kb.flags = b.flags & 3u;
        return true;
    }
    // host mirror of the directory (placement only; live counters stay on the exec side) and of the tenant names
    std::vector<TenantSlot> dir_h;
    std::vector<uint8_t> names_h;
    bool dir_dirty = false;

    bool fail(const std::string& m) {
        error = m;
        return false;
    }
    bool xfail() { return fail(x.err.empty() ? "exec failure" : x.err); }
    bool broke(const std::string& m) {
        broken = true;
        return fail(m);
    }
    template <class T> bool ensure_buf(T*& p, size_t& cap, size_t need) { // grow-only, contents dropped
        if (need <= cap) return true;
        if (p) x.release(p);
        const size_t want = need + need / 4 + 64;
        p = (T*)x.alloc(want * sizeof(T));
        cap = p ? want : 0;
        return p ? true : fail("out of memory");
    }
    template <class T> bool regrow(T*& p, uint64_t old_n, uint64_t new_n) { // contents [0, old_n) survive
        T* q = (T*)x.alloc(new_n * sizeof(T) + 16);
        if (!q) return fail("out of memory");
        if (p && old_n && !x.copy(q, p, old_n * sizeof(T))) return xfail();
        if (p && defer_release) graveyard.push_back((void*)p); // (somebody may still read it: see import_snapshot)
        else if (p) {
            if (!x.sync()) return xfail();
            x.release(p);
        }
        p = q;
        return true;
    }
    bool read_counters() { return x.copy_out(&hbc, bc, sizeof(BuildCounters)); }
    bool zero_batch_counters() {
        const size_t off = offsetof(BuildCounters, err);
        return x.zero((uint8_t*)bc + off, sizeof(BuildCounters) - off) ? true : xfail();
    }
    OpBatch batch(uint32_t n) {
        OpBatch ob{};
        ob.key_off = s_key_off;
        ob.n = n;
        ob.dir_slot = s_dir_slot;
        ob.nn = s_nn;
        ob.flag = s_flag;
        ob.target = s_target;
        ob.order = s_order;
        ob.sorted_target = s_sorted_target;
        ob.group_done = s_group_done;
        ob.unknown_list = s_unknown;
        ob.grow_list = s_grow;
        ob.bt_first = s_bt_first;
        ob.bt_nodes = s_bt_nodes;
        ob.bt_keys = s_bt_keys;
        ob.bt_dir = s_bt_dir;
        return ob;
    }
    bool ensure_scratch(uint32_t n, bool incremental) {
        const size_t need = (size_t)n + 1;
        if (need > s_cap) {
            auto rel = [&](auto*& p) {
                if (p) x.release((void*)p);
                p = nullptr;
            };
            rel(s_key_off); rel(s_op); rel(s_put_rank); rel(s_dir_slot); rel(s_nn); rel(s_flag); rel(s_target); rel(s_order);
            rel(s_sorted_target); rel(s_group_done); rel(s_unknown);
            const size_t want = need + need / 4 + 64;
            s_key_off = (uint32_t*)x.alloc(4 * want);
            s_op = (uint8_t*)x.alloc(want);
            s_put_rank = (uint32_t*)x.alloc(4 * want);
            s_dir_slot = (uint32_t*)x.alloc(4 * want);
            s_nn = (uint32_t*)x.alloc(4 * want);
            s_flag = (uint32_t*)x.alloc(4 * want);
            s_target = (unsigned long long*)x.alloc(8 * want);
            s_order = (uint32_t*)x.alloc(4 * want);
            s_sorted_target = (unsigned long long*)x.alloc(8 * want);
            s_group_done = (uint8_t*)x.alloc(want);
            s_unknown = (uint32_t*)x.alloc(4 * want);
            if (!s_key_off || !s_op || !s_put_rank || !s_dir_slot || !s_nn || !s_flag || !s_target || !s_order || !s_sorted_target ||
                !s_group_done || !s_unknown) {
                s_cap = 0;
                return fail("out of memory (builder scratch)");
            }
            s_cap = want;
        }
        (void)incremental;
        const size_t gneed = 2 * (size_t)std::max<uint32_t>(dir_slots, 64);
        if (gneed > s_grow_cap) {
            if (s_grow) x.release(s_grow);
            s_grow = (uint32_t*)x.alloc(4 * gneed);
            s_grow_cap = s_grow ? gneed : 0;
            if (!s_grow) return fail("out of memory (builder scratch)");
        }
        return true;
    }
    void release_scratch() { // after a bulk load: 10M-key scratch is not worth keeping
        auto rel = [&](auto*& p) {
            if (p) x.release((void*)p);
            p = nullptr;
        };
        rel(s_key_off); rel(s_op); rel(s_put_rank); rel(s_dir_slot); rel(s_nn); rel(s_flag); rel(s_target); rel(s_order);
        rel(s_sorted_target); rel(s_group_done); rel(s_unknown); rel(s_bt_first); rel(s_bt_nodes); rel(s_bt_keys); rel(s_bt_dir);
        s_cap = 0;
        s_bt_cap = 0;
    }
    bool ensure_keys(uint64_t more) {
        const uint64_t need = kpool_used + more + 32;
        if (need <= kpool_cap) return true;
        if (need >= (1ull << KREF_LEN_SHIFT)) return fail("key store exceeds 1 TB");
        const uint64_t cap = tiny ? need : std::max<uint64_t>(need + need / 2, 1u << 20);
        if (!regrow(kpool, kpool_used, cap)) return false;
        kpool_cap = cap;
        return true;
    }
    bool ensure_ids(uint64_t need) {
        if (need <= id_cap) return true;
        const uint64_t cap = tiny ? need : std::min<uint64_t>(std::max<uint64_t>(need + need / 2, 1u << 16), 0xFFFFFFF0ull);
        if (!regrow(kref, id_cap, cap) || !regrow(khash, id_cap, cap)) return false;
        if (!x.zero(kref + id_cap, (cap - id_cap) * sizeof(unsigned long long))) return xfail();
        id_cap = (uint32_t)cap;
        return true;
    }
    bool grow_route_pos(uint64_t need) {
        if (need <= rp_cap) return true;
        if (need >= 0x7FFFFFF0ull) return fail("id-list pool exceeds 2^31 words: bmq_rebuild compacts it");
        const uint64_t cap = tiny ? need : std::min<uint64_t>(std::max<uint64_t>(need + need / 2, 1u << 16), 0x7FFFFFF0ull);
        if (!regrow(route_pos, std::min<uint64_t>(rp_cap, hbc.rp_used ? hbc.rp_used : rp_cap), cap)) return false;
        rp_cap = cap;
        return true;
    }
    // dictionary of `slots` slots (power of two) + string pool of `pool` bytes; existing entries are re-inserted
    bool grow_dict(uint64_t slots, uint64_t pool) {
        if (slots > (1ull << 30)) return fail("level dictionary exceeds 2^30 slots");
        uint32_t ns = tiny ? 4 : 64;
        while (ns < slots) ns <<= 1;
        DictSlot* nd = (DictSlot*)x.alloc((size_t)ns * sizeof(DictSlot));
        if (!nd) return fail("out of memory (dictionary)");
        if (!x.zero(nd, (size_t)ns * sizeof(DictSlot))) return xfail();
        const uint32_t np = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pool, dpool_cap), 0xFFFFFF00ull);
        if (np > dpool_cap) {
            if (!read_counters()) return xfail();
            if (!regrow(dpool, std::min<uint32_t>(hbc.dpool_used, dpool_cap), np)) return false;
            dpool_cap = np;
        }
        DictSlot* old = dict;
        const uint32_t old_slots = dict_slots;
        dict = nd;
        dict_slots = ns;
        if (old) {
            if (!x.dict_rehash(old, old_slots, mut()) || !x.sync()) return xfail();
            x.release(old);
        }
        return true;
    }
    // ---- tenants ----
    static uint64_t hash_name(std::string_view s) {
        uint64_t h = TENANT_HASH_INIT;
        for (unsigned char c : s) h = tenant_hash_step(h, c);
        return tenant_hash_final(h);
    }
    bool ensure_directory(size_t n_tenants) { // load factor <= 1/2; growing re-places every entry (live counters come back first)
        if (dir_slots && n_tenants * 2 <= dir_slots) return true;
        if (dir_dirty && !flush_directory()) return false; // entries created but not uploaded yet must survive the re-placement
        uint32_t ns = tiny ? 2 : 64;
        while ((size_t)ns < n_tenants * 2 + 2) ns <<= 1;
        std::vector<TenantSlot> old;
        if (dir) {
            old.resize(dir_slots);
            if (!x.copy_out(old.data(), dir, sizeof(TenantSlot) * (size_t)dir_slots)) return xfail();
            x.release(dir);
            dir = nullptr;
        }
        dir_h.assign(ns, TenantSlot{});
        for (auto& t : old)
            if (t.hash_lo | t.hash_hi) place(t, ns);
        dir = (TenantSlot*)x.alloc(sizeof(TenantSlot) * (size_t)ns);
        if (!dir) return fail("out of memory (tenant directory)");
        dir_slots = ns;
        tenant_slot.clear();
        for (uint32_t d = 0; d < ns; d++)
            if (dir_h[d].hash_lo | dir_h[d].hash_hi)
                tenant_slot[std::string((const char*)names_h.data() + dir_h[d].name_off, dir_h[d].name_len)] = d;
        if (!x.copy_in(dir, dir_h.data(), sizeof(TenantSlot) * (size_t)ns)) return xfail();
        dir_dirty = false;
        if (s_grow_cap < 2 * (size_t)ns) {
            if (s_grow) x.release(s_grow);
            s_grow = (uint32_t*)x.alloc(8 * (size_t)ns);
            s_grow_cap = s_grow ? 2 * (size_t)ns : 0;
            if (!s_grow) return fail("out of memory (builder scratch)");
        }
        return true;
    }
    uint32_t place(const TenantSlot& t, uint32_t ns) {
        uint32_t d = (t.hash_lo ^ t.hash_hi) & (ns - 1);
        while (dir_h[d].hash_lo | dir_h[d].hash_hi) d = (d + 1) & (ns - 1);
        dir_h[d] = t;
        return d;
    }
    // a region of `slots` free (FREE_SLOT-filled) slots; NONE64 on failure
    bool alloc_region(uint64_t slots, uint64_t& base) {
        for (size_t i = 0; i < free_regions.size(); i++)
            if (free_regions[i].second >= slots && free_regions[i].second <= slots + slots / 2) { // reuse a region of similar size
                base = free_regions[i].first;
                const uint64_t got = free_regions[i].second;
                free_regions.erase(free_regions.begin() + (long)i);
                trie_garbage -= got;
                if (!x.fill_slots(trie + base, got)) return xfail();
                return true;
            }
        if (trie_used + slots > trie_cap) {
            if (trie_used + slots >= 0xFFFFFFF0ull) return fail("trie too large (2^32 slots): bmq_rebuild compacts it");
            const uint64_t cap = tiny ? trie_used + slots : std::min<uint64_t>(std::max<uint64_t>((trie_used + slots) * 2, 1u << 16), 0xFFFFFFF0ull);
            if (!regrow(trie, trie_used, cap)) return false;
            if (!x.fill_slots(trie + trie_used, cap - trie_used)) return xfail();
            trie_cap = cap;
        }
        base = trie_used;
        trie_used += slots;
        return true;
    }
    uint32_t buckets_for(uint64_t nodes) const { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(nodes + (tiny ? 0 : nodes * slack_num / 4 + 2), tiny ? 1 : 8), 0x7FFFFFF0ull); }
    // new tenant with room for `nodes` nodes; written to the host mirror (flush_directory uploads)
    bool create_tenant(const std::string& name, uint64_t nodes, uint32_t n_routes) {
        if (tenant_slot.count(name)) return true;
        if (!ensure_directory(tenant_slot.size() + 1)) return false;
        const uint32_t buckets = buckets_for(nodes);
        uint64_t base;
        if (!alloc_region(2ull * buckets, base)) return false;
        const uint64_t h = hash_name(name);
        TenantSlot t{};
        t.hash_lo = (uint32_t)h;
        t.hash_hi = (uint32_t)(h >> 32);
        t.name_off = (uint32_t)names_h.size();
        t.name_len = (uint32_t)name.size();
        memcpy(t.name12, name.data(), std::min<size_t>(name.size(), 12));
        t.root_plus = NONE;
        t.base = (uint32_t)base;
        t.buckets = buckets;
        t.n_routes = n_routes;
        names_h.insert(names_h.end(), name.begin(), name.end());
        const uint32_t d = place(t, dir_slots);
        tenant_slot[name] = d;
        new_dir_slots.push_back(d);
        dir_dirty = true;
        return true;
    }
    std::vector<uint32_t> new_dir_slots;
    bool flush_directory() { // upload the entries created since the last flush + the name pool
        if (names_h.size() + 16 > names_cap) {
            const uint32_t cap = (uint32_t)std::max<size_t>(names_h.size() * 2 + 64, 4096);
            if (names) {
                if (!x.sync()) return xfail();
                x.release(names);
            }
            names = (uint8_t*)x.alloc(cap);
            if (!names) return fail("out of memory (tenant names)");
            names_cap = cap;
            names_used = 0;
        }
        if (names_h.size() > names_used) {
            if (!x.copy_in(names + names_used, names_h.data() + names_used, names_h.size() - names_used)) return xfail();
            names_used = (uint32_t)names_h.size();
        }
        if (new_dir_slots.size() == tenant_slot.size()) { // bulk load: every entry is new, one copy (no live counters to preserve yet)
            if (!x.copy_in(dir, dir_h.data(), sizeof(TenantSlot) * (size_t)dir_slots)) return xfail();
        } else {
            for (uint32_t d : new_dir_slots)
                if (!x.copy_in(dir + d, &dir_h[d], sizeof(TenantSlot))) return xfail();
        }
        new_dir_slots.clear();
        dir_dirty = false;
        return true;
    }
    // regions listed by prepare_check (hbc.n_grow entries in ob.grow_list): move each into a larger region
    bool grow_flagged_regions(const OpBatch& ob) {
        if (hbc.n_grow == 0) return true;
        std::vector<uint32_t> gl(2 * (size_t)hbc.n_grow);
        if (!x.copy_out(gl.data(), ob.grow_list, sizeof(uint32_t) * gl.size())) return xfail();
        for (uint32_t g = 0; g < hbc.n_grow; g++) {
            const uint32_t d = gl[2 * g];
            TenantSlot t;
            if (!x.copy_out(&t, dir + d, sizeof(TenantSlot))) return xfail();
            const uint64_t need = std::max<uint64_t>(gl[2 * g + 1], (uint64_t)t.n_nodes + 1);
            const uint32_t nb = std::max<uint32_t>(buckets_for(need + need / 2), t.buckets < 0x3FFFFFFFu ? t.buckets * 2 : t.buckets);
            uint64_t base;
            if (!alloc_region(2ull * nb, base)) return false;
            if (!x.rehash(mut(), t.base, 2 * t.buckets, (uint32_t)base, nb, d)) return xfail();
            const uint32_t upd[2] = {(uint32_t)base, nb};
            if (!x.copy_in(&dir[d].base, upd, sizeof(upd))) return xfail(); // base and buckets are adjacent
            dir_h[d].base = (uint32_t)base;
            dir_h[d].buckets = nb;
            free_regions.push_back({t.base, 2ull * t.buckets});
            trie_garbage += 2ull * t.buckets;
        }
        if (!read_counters()) return xfail();
        if (hbc.err & ERR_REGION_FULL) return broke("region growth failed");
        hbc.n_grow = 0;
        return true;
    }
    bool reset_empty() { // an index with no routes (apply on a fresh engine)
        uint32_t err = 0;
        static const uint32_t zero_off[1] = {0};
        if (!rebuild_sorted(nullptr, zero_off, 0, err)) return false;
        built = true;
        generation++;
        return true;
    }
    static void sort_unique(const uint8_t* keys, const uint32_t* key_off, uint32_t n, std::vector<uint8_t>& bytes, std::vector<uint32_t>& off) {
        std::vector<std::string_view> v(n);
        for (uint32_t i = 0; i < n; i++) v[i] = std::string_view((const char*)keys + key_off[i], key_off[i + 1] - key_off[i]);
        auto less = [](std::string_view a, std::string_view b) {
            const size_t m = std::min(a.size(), b.size());
            const int c = m ? memcmp(a.data(), b.data(), m) : 0;
            return c < 0 || (c == 0 && a.size() < b.size());
        };
        std::sort(v.begin(), v.end(), less);
        v.erase(std::unique(v.begin(), v.end()), v.end());
        bytes.clear();
        off.assign(1, 0);
        for (auto& k : v) {
            bytes.insert(bytes.end(), k.begin(), k.end());
            off.push_back((uint32_t)bytes.size());
        }
        bytes.resize(bytes.size() + 16, 0);
    }

    // the bulk pipeline on strictly ascending keys; err receives the builder's error flags
    bool rebuild_sorted(const uint8_t* keys, const uint32_t* key_off, uint32_t n, uint32_t& err) {
        PhaseTimer pt(x);
        drop();
        pt.lap("rebuild: drop old index");
        const uint64_t kb = n ? key_off[n] : 0;
        bc = (BuildCounters*)x.alloc(sizeof(BuildCounters));
        if (!bc) return fail("out of memory");
        BuildCounters init{};
        init.rp_used = 1; // word 0 is never handed out: 0 means "no list"
        if (!x.copy_in(bc, &init, sizeof(init))) return xfail();
        kpool_used = 16; // offset 0 is never a key: kref == 0 means "no such route"
        if (!ensure_keys(tiny ? kb : kb + kb / 2 + (1u << 20)) || !ensure_ids(tiny ? n : (uint64_t)n + n / 2 + (1u << 16))) return false;
        if (!x.zero(kpool, 16)) return xfail();
        if (!grow_dict(tiny ? 64 : 1u << 16, tiny ? 64 : 1u << 20)) return false;
        if (!grow_route_pos(tiny ? 8 : 1u << 16)) return false;
        if (!ensure_directory(tiny ? 1 : 64)) return false;
        next_id = 0;
        n_routes = 0;
        if (n == 0) {
            if (!x.sync()) return xfail();
            return true;
        }
        if (!ensure_scratch(n, false)) return false;
        OpBatch ob = batch(n);
        ob.key_base = kpool_used;
        ob.id_base = 0;
        ob.put_rank = nullptr;
        ob.op = nullptr;
        ob.bulk = 1;
        if (!x.copy_in_async(kpool + kpool_used, keys, kb) || !x.copy_in_async(s_key_off, key_off, sizeof(uint32_t) * ((size_t)n + 1)))
            return xfail();
        pt.lap("rebuild: alloc + upload keys");
        // ---- sizes: tenants (runs of the sorted scan) and their exact node counts ----
        if (!zero_batch_counters()) return false;
        DistIndexMut ix = mut();
        if (!x.bulk_prepare(ix, ob) || !x.scan_flags(ob.flag, ob.order, n) || !read_counters()) return xfail();
        err = hbc.err;
        if (hbc.err & ERR_BAD_KEY) return fail("malformed route key");
        if (hbc.err & ERR_UNSORTED) return fail("keys are not strictly ascending");
        uint32_t n_ten = 0;
        if (!x.copy_out(&n_ten, ob.order + (n - 1), sizeof(uint32_t))) return xfail();
        if (n_ten > s_bt_cap) {
            auto rel = [&](auto*& p) {
                if (p) x.release((void*)p);
                p = nullptr;
            };
            rel(s_bt_first); rel(s_bt_nodes); rel(s_bt_keys); rel(s_bt_dir);
            const size_t want = (size_t)n_ten + 64;
            s_bt_first = (uint32_t*)x.alloc(4 * want);
            s_bt_nodes = (uint32_t*)x.alloc(4 * want);
            s_bt_keys = (uint32_t*)x.alloc(4 * want);
            s_bt_dir = (uint32_t*)x.alloc(4 * want);
            if (!s_bt_first || !s_bt_nodes || !s_bt_keys || !s_bt_dir) return fail("out of memory (builder scratch)");
            s_bt_cap = want;
            ob = batch(n);
            ob.key_base = kpool_used;
            ob.bulk = 1;
        }
        // run starts, then per-run key / node counts from a second scan (of nn[]; its output borrows the unknown-tenant list)
        if (!x.bulk_tenants(ix, ob, ob.order) || !x.scan_flags(ob.nn, ob.unknown_list, n) || !x.bulk_counts(ob, n_ten, ob.unknown_list))
            return xfail();
        std::vector<uint32_t> bt_first(n_ten), bt_nodes(n_ten), bt_keys(n_ten), bt_dir(n_ten);
        if (!x.copy_out(bt_first.data(), s_bt_first, 4 * (size_t)n_ten) || !x.copy_out(bt_nodes.data(), s_bt_nodes, 4 * (size_t)n_ten) ||
            !x.copy_out(bt_keys.data(), s_bt_keys, 4 * (size_t)n_ten))
            return xfail();
        pt.lap("rebuild: bulk prepare + tenant runs");
        // ---- tenants + regions ----
        if (!ensure_directory(n_ten)) return false;
        uint64_t total_slots = 0;
        for (uint32_t t = 0; t < n_ten; t++) total_slots += 2ull * buckets_for(bt_nodes[t]);
        {
            if (total_slots >= 0xFFFFFFF0ull) return fail("trie too large (2^32 slots)");
            const uint64_t cap = tiny ? total_slots + 2 : std::min<uint64_t>(total_slots + total_slots / 4 + (1u << 16), 0xFFFFFFF0ull); // head-room: new tenants, growth
            trie = (TrieSlot*)x.alloc(cap * sizeof(TrieSlot));
            if (!trie) return fail("out of device memory (trie)");
            trie_cap = cap;
            trie_used = 0;
            if (!x.fill_slots(trie, cap)) return xfail();
        }
        for (uint32_t t = 0; t < n_ten; t++) {
            const uint32_t ko = key_off[bt_first[t]];
            const size_t tlen = ((size_t)keys[ko + 1] << 8) | keys[ko + 2];
            const std::string name((const char*)keys + ko + 3, tlen);
            if (tenant_slot.count(name)) return fail("keys are not strictly ascending"); // cannot happen after the order check
            if (!create_tenant(name, bt_nodes[t], bt_keys[t])) return false;
            bt_dir[t] = tenant_slot[name];
        }
        if (!flush_directory()) return false;
        if (!x.copy_in(s_bt_dir, bt_dir.data(), 4 * (size_t)n_ten)) return xfail();
        pt.lap("rebuild: directory + regions");
        // ---- locate (re-run with a larger dictionary if it filled up), sort, groups ----
        for (int attempt = 0;; attempt++) {
            if (attempt == 10) return fail("rebuild: dictionary growth did not converge");
            if (!zero_batch_counters()) return false;
            ix = mut();
            if (!x.locate(ix, ob) || !read_counters()) return xfail();
            if (hbc.err & (ERR_STUCK | ERR_REGION_FULL)) return fail("rebuild: trie construction failed");
            if (!(hbc.err & ERR_DICT_FULL)) break;
            if (!grow_dict((uint64_t)dict_slots * 4, (uint64_t)dpool_cap * 4)) return false;
        }
        pt.lap("rebuild: locate");
        if (!x.zero(ob.group_done, n) || !x.sort_targets(ob)) return xfail();
        pt.lap("rebuild: sort by filter node");
        for (int attempt = 0;; attempt++) {
            if (attempt == 8) return fail("rebuild: id-list pool growth did not converge");
            if (!zero_batch_counters()) return false;
            ix = mut();
            if (!x.group(ix, ob) || !read_counters()) return xfail();
            if (hbc.err) return fail("rebuild: group step failed");
            if (hbc.n_deferred == 0) break;
            if (!grow_route_pos(hbc.rp_used + 2 * hbc.rp_need + 1024)) return false;
        }
        pt.lap("rebuild: groups");
        n_routes = n;
        kpool_used += (kb + 15) & ~15ull;
        next_id = n;
        // right-size the dictionary: load factor 1/4 keeps a lookup at one line, a small table stays cache resident
        {
            uint64_t want = 4096;
            while (want < (uint64_t)hbc.n_tokens * 4) want <<= 1;
            if (want != dict_slots && !grow_dict(want, dpool_cap)) return false;
        }
        if (!form_tails()) return false;
        pt.lap("rebuild: tail records");
        if (!x.sync()) return xfail();
        release_scratch();
        pt.lap("rebuild: dictionary resize, cleanup");
        return true;
    }
};

} // namespace bmq
