// bmq_retain_build.h -- control of the executor-side BULK LOAD of the retained-topic index (bmq_retain_build_core.h): owns the image
// of a generation in exec memory (HBM under DevExec, host memory under HostExec), allocates the transient arrays of a build, runs the
// stages in order and hands the host what its catalogue needs -- the permutation rank -> input item and the per-tenant counts.
// Selected by bmq_config.retain_builder = 1; the host builder (bmq_retain.cpp) stays the default and the fallback for a load that
// holds a topic of more than RB_MAX_DEPTH levels.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "bmq_retain_build_core.h"

namespace bmq {

struct RbInput { // the caller's items: host memory, or (in_exec) a snapshot that lies in exec memory already -- the tenant table is host memory always
    const uint8_t* tenants;
    const uint32_t* tenant_off;
    uint32_t n_tenants;
    const uint32_t* item_tenant; // [n] index into the tenant table (may hold an id twice, and ids no item refers to)
    const uint8_t* topics;
    const uint32_t* topic_off; // [n + 1]
    uint32_t n;
    const uint64_t* ts;        // [n] or null: no stamps (ts 0, expiry 0xFFFFFFFF: never expires)
    const uint32_t* expiry;    // [n] or null (together with ts)
    bool in_exec = false;      // item_tenant, topics (zero-filled 16 bytes past the end) and topic_off are exec memory: used where they lie (ts / expiry are not read)
    uint64_t topic_bytes = 0;  // in_exec: topic_off[n]
};

struct RetainBuildInfo {
    uint32_t builder = 0, fallback = 0;
    uint64_t n_items = 0, n_topics = 0, n_tenants = 0, n_nodes = 0, n_edges = 0, n_edge_overflows = 0, n_gp_overflows = 0, n_posts = 0, n_gp_runs = 0, n_tokens = 0;
    uint32_t max_depth = 0;
    float ms_total = 0, ms_sort = 0;
};

struct RbImage { // what RetainIndexView points at
    void *nodes = nullptr, *edges = nullptr, *posts = nullptr, *gps = nullptr, *dir = nullptr, *dict = nullptr, *pool = nullptr;
    uint32_t dir_slots = 0, dict_slots = 0;
};

template <class Exec> class RetainBuild {
public:
    explicit RetainBuild(Exec& exec) : x(exec) {}
    ~RetainBuild() {
        drop(img);
        drop_perm();
    }
    RetainBuild(const RetainBuild&) = delete;
    RetainBuild& operator=(const RetainBuild&) = delete;

    Exec& x;
    std::string error;
    bool too_deep = false; // the last build stopped at a topic of more than RB_MAX_DEPTH levels: nothing was changed, the host builder takes the load
    RbImage img;           // the generation built last (the serving one once the engine has published it)
    RetainBuildInfo info;
    // ---- what the host's catalogue is filled from ----
    std::vector<std::string> names; // tenant ids, de-duplicated, in byte order
    std::vector<uint32_t> perm;     // rank (= topic id) -> input item
    std::vector<uint32_t> t_begin;  // [tenants + 1] first rank of every tenant
    std::vector<RbTenant> plan;
    // keep_perm: the permutation also stays in exec memory after a build (d_perm[info.n_topics]) until drop_perm / the next build: what lays the
    // next generation's per-id arrays out in rank order reads it there (RetainDyn::reset_exec)
    bool keep_perm = false;
    uint32_t* d_perm = nullptr;
    void drop_perm() {
        x.release(d_perm);
        d_perm = nullptr;
    }
    // the image `o` built becomes this one's (exec memory is the executors' common ground: alloc / release do not depend on the instance)
    void take_image(RetainBuild& o) {
        drop(img);
        img = o.img;
        o.img = RbImage{};
        info = o.info;
    }

    void view(RetainIndexView& v) const {
        v = RetainIndexView{};
        v.nodes = (const RNode*)img.nodes;
        v.edges = (const REdge*)img.edges;
        v.posts = (const REdge*)img.posts;
        v.gps = (const RGp*)img.gps;
        v.tenants = (const RTenantSlot*)img.dir;
        v.tenant_mask = img.dir_slots - 1;
        v.dict = (const DictSlot*)img.dict;
        v.dict_group_mask = img.dict_slots / DICT_GROUP - 1;
        v.pool = (const uint8_t*)img.pool;
    }
    void release_image() { drop(img); }

    // The image of the items in exec memory.  false: `error` says why, or too_deep is set; the image built before stays as it is.
    bool build(const RbInput& in) {
        using clk = std::chrono::steady_clock;
        const auto t0 = clk::now();
        error.clear();
        too_deep = false;
        drop_perm();
        Scratch sc{x, {}};
        RbImage ni;
        const bool ok = run(in, sc, ni);
        if (!x.sync()) { // (transient arrays are released behind everything that reads them)
            drop(ni);
            drop_perm();
            return xfail();
        }
        if (!ok) {
            drop(ni);
            drop_perm();
            return false;
        }
        drop(img);
        img = ni;
        info.builder = 1;
        info.fallback = 0;
        info.ms_total = std::chrono::duration<float, std::milli>(clk::now() - t0).count();
        return true;
    }

private:
    struct Scratch {
        Exec& x;
        std::vector<void*> blocks;
        ~Scratch() {
            for (void* p : blocks) x.release(p);
        }
    };
    bool fail(const char* msg) {
        error = msg;
        return false;
    }
    bool xfail() {
        error = x.err.empty() ? "executor failure (retain bulk load)" : x.err;
        return false;
    }
    void drop(RbImage& i) {
        for (void* p : {i.nodes, i.edges, i.posts, i.gps, i.dir, i.dict, i.pool}) x.release(p);
        i = RbImage{};
    }
    template <class T> T* get(Scratch& sc, size_t n) {
        T* p = (T*)x.alloc(sizeof(T) * std::max<size_t>(n, 1) + 16);
        if (p) sc.blocks.push_back(p);
        else error = "out of memory (retain bulk load)";
        return p;
    }
    template <class T> bool part(void*& slot, size_t n) { // an array of the image
        slot = x.alloc(sizeof(T) * std::max<size_t>(n, 16) + 16);
        if (!slot) error = "out of memory (retain bulk load)";
        return slot != nullptr;
    }
    bool last_of(const uint32_t* scan, uint32_t n, uint32_t& out) { return x.copy_out(&out, scan + n - 1, sizeof(uint32_t)); }

    // an empty load: tables nobody finds anything in
    bool empty_image(RbImage& ni) {
        if (!part<RNode>(ni.nodes, 16) || !part<REdge>(ni.edges, 16) || !part<REdge>(ni.posts, 16) || !part<RGp>(ni.gps, 16) || !part<RTenantSlot>(ni.dir, 64) ||
            !part<DictSlot>(ni.dict, 64) || !part<uint8_t>(ni.pool, 16))
            return false;
        ni.dir_slots = 64, ni.dict_slots = 64;
        if (!x.zero(ni.nodes, sizeof(RNode) * 16) || !x.rb_fill16(ni.edges, 16) || !x.rb_fill16(ni.posts, 16) || !x.rb_fill16(ni.gps, 16) ||
            !x.zero(ni.dir, sizeof(RTenantSlot) * 64) || !x.zero(ni.dict, sizeof(DictSlot) * 64) || !x.zero(ni.pool, 16))
            return xfail();
        return true;
    }

    bool run(const RbInput& in, Scratch& sc, RbImage& ni) {
        using clk = std::chrono::steady_clock;
        info = RetainBuildInfo{};
        info.n_items = in.n;
        names.clear(), perm.clear(), t_begin.assign(1, 0u), plan.clear();
        const uint32_t n = in.n;
        if ((uint64_t)n >= 0x7FFFFFF0ull) return fail("too many retained topics");
        if (n == 0) return empty_image(ni);
        // ---- the tenant table: small, so the host de-duplicates and byte-sorts it and hands every item its tenant's rank ----
        std::vector<uint32_t> rank_of(in.n_tenants, NONE), item_rank(in.in_exec ? 0 : n);
        uint32_t* d_rank_of = nullptr; // in_exec: which table entries the items use, then the entries' ranks
        {
            std::vector<uint32_t> used(in.n_tenants, 0);
            if (in.in_exec) {
                d_rank_of = get<uint32_t>(sc, in.n_tenants);
                if (!d_rank_of) return false;
                if (!x.zero(d_rank_of, sizeof(uint32_t) * in.n_tenants) || !x.rs_used(in.item_tenant, n, d_rank_of) || !x.copy_out(used.data(), d_rank_of, sizeof(uint32_t) * in.n_tenants))
                    return xfail();
            } else
                for (uint32_t i = 0; i < n; i++) used[in.item_tenant[i]] = 1;
            std::vector<uint32_t> ord;
            for (uint32_t t = 0; t < in.n_tenants; t++)
                if (used[t]) ord.push_back(t);
            auto name = [&](uint32_t t) { return std::string_view((const char*)in.tenants + in.tenant_off[t], in.tenant_off[t + 1] - in.tenant_off[t]); };
            std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return name(a) < name(b); });
            for (size_t k = 0; k < ord.size(); k++) {
                if (k == 0 || name(ord[k]) != name(ord[k - 1])) names.emplace_back(name(ord[k]));
                rank_of[ord[k]] = (uint32_t)names.size() - 1;
            }
            if (!in.in_exec)
                for (uint32_t i = 0; i < n; i++) item_rank[i] = rank_of[in.item_tenant[i]];
        }
        const uint32_t nt = (uint32_t)names.size();
        std::vector<uint8_t> tbytes;
        std::vector<uint32_t> toff{0};
        for (auto& s : names) {
            tbytes.insert(tbytes.end(), s.begin(), s.end());
            toff.push_back((uint32_t)tbytes.size());
        }
        tbytes.resize(tbytes.size() + 16, 0);
        const size_t topic_bytes = in.in_exec ? (size_t)in.topic_bytes : in.topic_off[n];

        RbArgs B{};
        uint8_t* d_tenants = get<uint8_t>(sc, tbytes.size());
        uint32_t* d_toff = get<uint32_t>(sc, nt + 1);
        const uint8_t* d_topics = in.in_exec ? in.topics : get<uint8_t>(sc, topic_bytes + 16);
        const uint32_t* d_poff = in.in_exec ? in.topic_off : get<uint32_t>(sc, (size_t)n + 1);
        uint32_t* d_item = get<uint32_t>(sc, n);
        B.idx = get<uint32_t>(sc, n);
        B.flag = get<uint32_t>(sc, n);
        B.scan = get<uint32_t>(sc, n);
        B.ctr = get<RbCounters>(sc, 1);
        if (!d_tenants || !d_toff || !d_topics || !d_poff || !d_item || !B.idx || !B.flag || !B.scan || !B.ctr) return false;
        if (!x.copy_in_async(d_tenants, tbytes.data(), tbytes.size()) || !x.copy_in_async(d_toff, toff.data(), sizeof(uint32_t) * (nt + 1)) || !x.zero(B.ctr, sizeof(RbCounters)))
            return xfail();
        if (in.in_exec) {
            if (!x.copy_in_async(d_rank_of, rank_of.data(), sizeof(uint32_t) * in.n_tenants) || !x.rs_remap(in.item_tenant, d_rank_of, d_item, n)) return xfail();
        } else if (!x.copy_in_async((uint8_t*)d_topics, in.topics, topic_bytes) || !x.zero((uint8_t*)d_topics + topic_bytes, 16) ||
                   !x.copy_in_async((uint32_t*)d_poff, in.topic_off, sizeof(uint32_t) * ((size_t)n + 1)) || !x.copy_in_async(d_item, item_rank.data(), sizeof(uint32_t) * n))
            return xfail();
        B.tenants = d_tenants, B.ten_off = d_toff, B.n_tenants = nt;
        B.topics = d_topics, B.topic_off = d_poff, B.item_tenant = d_item, B.n_items = n;

        // ---- order ----
        if (!x.sync()) return xfail();
        const auto ts0 = clk::now();
        if (!x.rb_sort_items(B) || !x.sync()) return xfail();
        info.ms_sort = std::chrono::duration<float, std::milli>(clk::now() - ts0).count();
        uint32_t n_topics = 0;
        if (!x.rb_keep(B) || !x.scan_flags(B.flag, B.scan, n) || !last_of(B.scan, n, n_topics)) return xfail();
        B.n_topics = n_topics;
        if (keep_perm) {
            d_perm = (uint32_t*)x.alloc(sizeof(uint32_t) * std::max<size_t>(n_topics, 1) + 16);
            if (!d_perm) error = "out of memory (retain bulk load)";
        }
        B.perm = keep_perm ? d_perm : get<uint32_t>(sc, n_topics);
        B.L = get<uint32_t>(sc, n_topics);
        B.lcp = get<uint32_t>(sc, n_topics);
        B.ten = get<uint32_t>(sc, n_topics);
        B.t_begin = get<uint32_t>(sc, nt + 1);
        B.plan = get<RbTenant>(sc, nt);
        B.tbase = get<uint32_t>(sc, 2 * (size_t)nt);
        if (!B.perm || !B.L || !B.lcp || !B.ten || !B.t_begin || !B.plan || !B.tbase) return false;
        if (!x.rb_rank(B) || !x.copy_in(B.t_begin + nt, &n_topics, sizeof(uint32_t)) || !x.zero(B.plan, sizeof(RbTenant) * nt) || !x.rb_shape(B) ||
            !x.scan_flags(B.flag, B.scan, n_topics) || !x.rb_count(B))
            return xfail();
        plan.resize(nt);
        RbCounters c{};
        if (!x.copy_out(plan.data(), B.plan, sizeof(RbTenant) * nt) || !x.copy_out(&c, B.ctr, sizeof(c))) return xfail();
        info.max_depth = c.max_depth;
        if (c.max_depth > RB_MAX_DEPTH) {
            too_deep = true;
            return fail("a topic has more levels than the executor builder takes");
        }
        // ---- where every tenant's parts lie ----
        uint64_t n_nodes = 0, n_eslots = 0;
        for (RbTenant& T : plan) {
            T.node_base = (uint32_t)n_nodes;
            n_nodes += T.n_nodes;
            const uint32_t eslots = pow2_at_least(std::max<uint64_t>(8, (uint64_t)T.n_nodes * 2));
            T.edge_base = (uint32_t)n_eslots;
            T.edge_bucket_mask = eslots / 4 - 1;
            n_eslots += eslots;
            if (n_nodes >= 0x7FFFFFF0ull || n_eslots >= 0xFFFFFFF0ull) return fail("too many retained topics");
        }
        const uint32_t N = (uint32_t)n_nodes;
        B.n_nodes = N;
        const uint32_t own_slots = pow2_at_least((uint64_t)N * 2);
        const size_t wide = std::max<size_t>(std::max<size_t>(n, N), own_slots);
        if (!part<RNode>(ni.nodes, N) || !part<REdge>(ni.edges, n_eslots)) return false;
        B.nodes = (RNode*)ni.nodes, B.edges = (REdge*)ni.edges;
        B.flag = get<uint32_t>(sc, wide);
        B.scan = get<uint32_t>(sc, wide);
        for (auto& S : B.S) S = get<uint32_t>(sc, n_topics);
        B.parent = get<uint32_t>(sc, N);
        B.lab_off = get<uint32_t>(sc, N);
        B.lab_len = get<uint32_t>(sc, N);
        B.node_ten = get<uint32_t>(sc, N);
        B.tok = get<uint32_t>(sc, N);
        B.slot_of = get<uint32_t>(sc, N);
        B.ovf = get<uint32_t>(sc, N);
        B.own = get<uint32_t>(sc, own_slots);
        B.own_rank = get<uint32_t>(sc, own_slots);
        B.own_pool = get<uint32_t>(sc, own_slots);
        B.own_mask = own_slots - 1;
        if (!B.flag || !B.scan || !B.S[0] || !B.S[1] || !B.S[2] || !B.parent || !B.lab_off || !B.lab_len || !B.node_ten || !B.tok || !B.slot_of || !B.ovf || !B.own ||
            !B.own_rank || !B.own_pool)
            return false;
        if (!x.copy_in(B.plan, plan.data(), sizeof(RbTenant) * nt) || !x.rb_fill16(ni.edges, std::max<uint64_t>(n_eslots, 16)) || !x.zero(B.own, sizeof(uint32_t) * own_slots) ||
            !x.zero(B.S[0], sizeof(uint32_t) * n_topics))
            return xfail();
        // ---- nodes, one depth at a time ----
        if (!x.rb_head(B, 1) || !x.scan_flags(B.flag, B.S[1], n_topics) || !x.rb_root(B, B.S[1])) return xfail();
        for (uint32_t d = 1; d <= c.max_depth; d++) {
            const uint32_t *Sp = B.S[(d + 2) % 3], *Sc = B.S[d % 3];
            uint32_t* Sn = B.S[(d + 1) % 3];
            if (!x.rb_head(B, d + 1) || !x.scan_flags(B.flag, Sn, n_topics) || !x.rb_emit(B, d, Sp, Sc, Sn) || !x.rb_close(B, d, Sc, Sn) || !x.rb_advance(B, Sc)) return xfail();
        }
        // ---- dictionary ----
        uint32_t n_tokens = 0, pool_bytes = 0;
        if (!x.rb_intern(B) || !x.rb_owner(B) || !x.scan_flags(B.flag, B.own_rank, own_slots) || !x.scan_flags(B.scan, B.own_pool, own_slots) ||
            !last_of(B.own_rank, own_slots, n_tokens) || !last_of(B.own_pool, own_slots, pool_bytes))
            return xfail();
        const uint32_t dslots = pow2_at_least(std::max<uint64_t>(8, (uint64_t)n_tokens * 4));
        const size_t pool_cap = std::max<size_t>(16, ((size_t)pool_bytes + 15) & ~(size_t)15);
        if (!part<DictSlot>(ni.dict, dslots) || !part<uint8_t>(ni.pool, pool_cap)) return false;
        ni.dict_slots = dslots;
        B.dict = (DictSlot*)ni.dict, B.dict_group_mask = dslots / DICT_GROUP - 1, B.pool = (uint8_t*)ni.pool;
        if (!x.zero(ni.dict, sizeof(DictSlot) * dslots) || !x.zero(ni.pool, pool_cap) || !x.rb_place(B) || !x.rb_token(B)) return xfail();
        // ---- edges ----
        if (!x.rb_edge(B) || !x.rb_edge_overflow(B)) return xfail();
        // ---- grandchild postings ----
        uint32_t n_posts = 0, n_runs = 0;
        if (!x.rb_post_flag(B) || !x.scan_flags(B.flag, B.scan, N) || !last_of(B.scan, N, n_posts)) return xfail();
        B.n_posts = n_posts;
        if (!part<REdge>(ni.posts, n_posts)) return false;
        B.posts = (REdge*)ni.posts;
        if (n_posts) {
            for (auto& k : B.k64) k = get<unsigned long long>(sc, n_posts);
            for (auto& k : B.k32) k = get<uint32_t>(sc, n_posts);
            for (auto& v : B.pv) v = get<uint32_t>(sc, n_posts);
            if (!B.k64[0] || !B.k64[1] || !B.k32[0] || !B.k32[1] || !B.pv[0] || !B.pv[1] || !B.pv[2]) return false;
            if (!x.rb_post_emit(B) || !x.sort_pairs64(B.k64[0], B.k64[1], B.pv[0], B.pv[1], n_posts) || !x.rb_post_gp(B) ||
                !x.sort_pairs32(B.k32[0], B.k32[1], B.pv[1], B.pv[2], n_posts, 32) || !x.rb_post_write(B) || !x.scan_flags(B.flag, B.scan, n_posts) ||
                !last_of(B.scan, n_posts, n_runs) || !x.rb_post_tenant(B) || !x.copy_out(plan.data(), B.plan, sizeof(RbTenant) * nt))
                return xfail();
        } else if (!x.rb_fill16(ni.posts, 16)) return xfail();
        B.n_runs = n_runs;
        uint64_t n_gslots = 0;
        for (RbTenant& T : plan) {
            const uint32_t gslots = pow2_at_least(std::max<uint64_t>(4, (uint64_t)T.n_runs * 2));
            T.gp_base = (uint32_t)n_gslots;
            T.gp_bucket_mask = gslots / 4 - 1;
            n_gslots += gslots;
            if (n_gslots >= 0xFFFFFFF0ull) return fail("too many retained topics");
        }
        if (!part<RGp>(ni.gps, n_gslots)) return false;
        B.gps = (RGp*)ni.gps;
        if (!x.copy_in(B.plan, plan.data(), sizeof(RbTenant) * nt) || !x.rb_fill16(ni.gps, std::max<uint64_t>(n_gslots, 16))) return xfail();
        if (n_runs) {
            B.run_start = get<uint32_t>(sc, (size_t)n_runs + 1);
            if (!B.run_start) return false;
            if (!x.rb_run_start(B) || !x.rb_gp(B) || !x.rb_gp_overflow(B)) return xfail();
        }
        // ---- tenant directory ----
        const uint32_t tslots = pow2_at_least((uint64_t)nt * 2);
        if (!part<RTenantSlot>(ni.dir, tslots)) return false;
        ni.dir_slots = tslots;
        B.dir = (RTenantSlot*)ni.dir, B.dir_mask = tslots - 1;
        if (!x.zero(ni.dir, sizeof(RTenantSlot) * tslots) || !x.rb_tenant(B)) return xfail();
        // ---- what comes back ----
        perm.resize(n_topics);
        t_begin.resize((size_t)nt + 1);
        if (!x.copy_out(plan.data(), B.plan, sizeof(RbTenant) * nt) || !x.copy_out(perm.data(), B.perm, sizeof(uint32_t) * n_topics) ||
            !x.copy_out(t_begin.data(), B.t_begin, sizeof(uint32_t) * ((size_t)nt + 1)) || !x.copy_out(&c, B.ctr, sizeof(c)))
            return xfail();
        if (c.err) return fail("the retain bulk load ran out of a table it had sized itself (damaged input?)");
        info.n_topics = n_topics;
        info.n_tenants = nt;
        info.n_nodes = N;
        info.n_edges = N - nt;
        info.n_edge_overflows = c.edge_overflows;
        info.n_gp_overflows = c.gp_overflows;
        info.n_posts = n_posts;
        info.n_gp_runs = n_runs;
        info.n_tokens = n_tokens;
        return true;
    }
};

// The host's catalogue of a generation the executor built: O(n) copies in rank order, no sort.  The image vectors of RetainIndexHost stay
// empty -- the arrays lie in the executor's buffers (RetainBuild::view).
template <class Exec> inline bool retain_catalogue(RetainIndexHost& h, const RbInput& in, const RetainBuild<Exec>& rb) {
    h.error.clear();
    h.by_name.clear();
    h.order.clear();
    h.nodes = {}, h.edges = {}, h.posts = {}, h.gps = {}, h.tenants = {}, h.dict = {}, h.pool = {};
    h.dict_h = HostDict();
    h.strings.clear();
    h.node_free = h.edge_free = h.post_free = h.gp_free = 0;
    h.full_upload = h.dict_changed = false;
    h.dirty.clear();
    const size_t nt = rb.names.size();
    h.n_topics = rb.perm.size();
    h.expire_at.assign(h.n_topics ? h.n_topics : 1, RETAIN_NEVER);
    for (size_t t = 0; t < nt; t++) {
        auto st = std::make_unique<RTenantState>();
        st->name = rb.names[t];
        const uint32_t b = rb.t_begin[t], e = rb.t_begin[t + 1];
        st->id_base = b;
        st->topics.reserve(e - b), st->ts.reserve(e - b), st->expiry.reserve(e - b);
        for (uint32_t r = b; r < e; r++) {
            const uint32_t it = rb.perm[r];
            st->topics.emplace_back((const char*)in.topics + in.topic_off[it], in.topic_off[it + 1] - in.topic_off[it]);
            const uint64_t ts = in.ts ? in.ts[it] : 0ull;
            const uint32_t ex = in.ts ? in.expiry[it] : 0xFFFFFFFFu;
            st->ts.push_back(ts);
            st->expiry.push_back(ex);
            h.expire_at[r] = (ts == 0 && ex == 0xFFFFFFFFu) ? RETAIN_NEVER : retain_expire_at(ts, ex);
        }
        const RbTenant& T = rb.plan[t];
        st->sys_node_lo = T.sys_node_lo, st->sys_node_hi = T.sys_node_hi, st->sys_id_lo = T.sys_id_lo, st->sys_id_hi = T.sys_id_hi;
        h.order.push_back(st.get());
        h.by_name.emplace_hint(h.by_name.end(), rb.names[t], std::move(st));
    }
    return true;
}

} // namespace bmq
