// retain_snapshot_check.cpp -- test tool, not product: the snapshot of the retained-topic index and what bmq_retain_compact_build makes of it
// (bmq_config.retain_builder = 3), without a GPU, over HostExec -- the very functions the k_rs_* kernels wrap (bmq_retain_snap_core.h) -- under
// AddressSanitizer/UBSan and under ThreadSanitizer.  Per seeded round:
//   * a random load (0 / 1 / 64 / 65 items among the sizes, zero-length topics, empty levels, a tenant id twice) becomes a serving generation,
//     built by the host builder or by the executor builder in turn; a churn batch adds below loaded tenants and under new ones and removes
//     loaded topics, a few ids are removed by id;
//   * RetainDyn::snapshot (all live topics, then those inside a KV boundary) is compared item for item with the strings and stamps the
//     existing host path gives for the same ids (select / boundary_select, payload, RetainIndexHost::topic, overlay_topics);
//   * retain_build_next (bmq_retain_next.h: the very function bmq_retain_compact_build runs) builds from the snapshot where it lies -- the
//     permutation, tenants, counts and RNode array equal those of a build of the same items handed in from host memory; with a topic of 129
//     levels in the load it falls back to the host builder, whose catalogue holds exactly the snapshot's items; 128 levels do not fall back;
//   * its RetainDyn (reset_exec), adopted, is the mutable part the next generation serves with: live ids are the ranks, stamps and expire_at those
//     of the catalogue, every key of keys_by_id (the key store the gather laid out) equals retain_message_key of the catalogue's strings;
//   * PackedTopics (the engine's one packer) round-trips hostile tenants, topics and stamps, once, before the rounds;
//   * with more than one thread (the TSan form) a second thread applies batches to the serving generation while the build runs.
// Build + run: make -C bifromq_amd/csrc rscheck   (tests/test_retain_generation.py builds and runs both forms)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../bifromq_amd/csrc/bmq_codec.h"
#include "../bifromq_amd/csrc/bmq_exec_host.h"
#include "../bifromq_amd/csrc/bmq_retain.h"
#include "../bifromq_amd/csrc/bmq_retain_build.h"
#include "../bifromq_amd/csrc/bmq_retain_dyn.h"
#include "../bifromq_amd/csrc/bmq_retain_next.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

struct Packed {
    std::string tb, pb;
    std::vector<uint32_t> toff{0}, poff{0}, it;
    std::vector<uint64_t> ts;
    std::vector<uint32_t> ex;
    std::vector<uint8_t> op;
    void tenant(const std::string& t) { tb += t, toff.push_back((uint32_t)tb.size()); }
    void item(uint32_t t, const std::string& p, uint64_t s, uint32_t e, uint8_t o = 0) {
        it.push_back(t), pb += p, poff.push_back((uint32_t)pb.size()), ts.push_back(s), ex.push_back(e), op.push_back(o);
    }
    void pad() { tb.append(16, '\0'), pb.append(16, '\0'); }
    RbInput input() const {
        return RbInput{(const uint8_t*)tb.data(), toff.data(), (uint32_t)toff.size() - 1, it.data(), (const uint8_t*)pb.data(), poff.data(), (uint32_t)it.size(), ts.data(), ex.data()};
    }
};

struct Item {
    std::string tenant, topic;
    uint64_t ts;
    uint32_t ex;
    bool operator==(const Item& o) const { return tenant == o.tenant && topic == o.topic && ts == o.ts && ex == o.ex; }
};

static RetainIndexView view_of(const RetainIndexHost& h) {
    RetainIndexView v{};
    v.nodes = h.nodes.data(), v.edges = h.edges.data(), v.posts = h.posts.data(), v.gps = h.gps.data(), v.tenants = h.tenants.data();
    v.tenant_mask = (uint32_t)h.tenants.size() - 1;
    v.dict = h.dict.data(), v.dict_group_mask = (uint32_t)h.dict.size() / DICT_GROUP - 1, v.pool = h.pool.data();
    return v;
}

// the items of `ids` through the existing host path
static bool items_of(RetainDyn<HostExec>& rt, const RetainIndexHost& h, const std::vector<uint32_t>& ids, std::vector<Item>& out) {
    std::vector<unsigned long long> ts;
    std::vector<uint32_t> ex, ov, lens;
    std::vector<uint8_t> bytes;
    if (!rt.payload(ts, ex)) return false;
    for (uint32_t id : ids)
        if (id >= rt.info.base_n) ov.push_back(id);
    if (!rt.overlay_topics(ov.data(), (uint32_t)ov.size(), lens, bytes)) return false;
    size_t off = 0, k = 0;
    out.clear();
    for (uint32_t id : ids) {
        Item x;
        if (id < rt.info.base_n) {
            std::string_view tn, tp;
            if (!h.topic(id, tn, tp)) return false;
            x.tenant = std::string(tn), x.topic = std::string(tp);
        } else {
            x.tenant.assign((const char*)bytes.data() + off, lens[2 * k]);
            x.topic.assign((const char*)bytes.data() + off + lens[2 * k], lens[2 * k + 1] - lens[2 * k]);
            off += lens[2 * k + 1];
            k++;
        }
        x.ts = ts[id], x.ex = ex[id];
        out.push_back(std::move(x));
    }
    return true;
}

static int compare_snapshot(const RetainSnapshot<HostExec>& snap, const std::vector<Item>& want, int round, const char* what) {
    const RsSnap& S = snap.s;
    if (S.n != want.size()) FAIL("round %d (%s): the snapshot holds %u items, the host path %zu\n", round, what, S.n, want.size());
    if (S.topic_off[0] != 0 || S.topic_off[S.n] != snap.topic_bytes) FAIL("round %d (%s): topic offsets do not span the bytes\n", round, what);
    for (uint32_t k = 0; k < 16; k++)
        if (S.topics[snap.topic_bytes + k]) FAIL("round %d (%s): the 16 bytes behind the topics are not zero\n", round, what);
    for (uint32_t i = 0; i < S.n; i++) {
        const uint32_t t = S.item_tenant[i];
        if (t >= S.n_tenants) FAIL("round %d (%s): item %u has tenant entry %u of %u\n", round, what, i, t, S.n_tenants);
        const Item got{std::string((const char*)S.tenants + S.tenant_off[t], S.tenant_off[t + 1] - S.tenant_off[t]),
                       std::string((const char*)S.topics + S.topic_off[i], S.topic_off[i + 1] - S.topic_off[i]), S.ts[i], S.expiry[i]};
        if (!(got == want[i]))
            FAIL("round %d (%s): item %u is ('%s', '%s', %llu, %u), the host path gives ('%s', '%s', %llu, %u)\n", round, what, i, got.tenant.c_str(), got.topic.c_str(),
                 (unsigned long long)got.ts, got.ex, want[i].tenant.c_str(), want[i].topic.c_str(), (unsigned long long)want[i].ts, want[i].ex);
    }
    return 0;
}

// PackedTopics: pack -> pad -> rb_input -> items gives the input back (an item stamped (0, 0xFFFFFFFF) as one without stamps)
static int packed_round_trip() {
    using It = RetainIndexHost::Item;
    const std::string big(200, 'T'), t255 = "x/" + std::string(253, 'y');
    auto item = [](const std::string& tn, const std::string& tp, bool has, uint64_t ts, uint32_t ex) {
        It it;
        it.tenant = tn, it.topic = tp, it.has_ts = has, it.ts = ts, it.expiry = ex;
        return it;
    };
    const std::vector<It> in = {item("", "", true, 5, 10),          item(big, "a//b", true, 1ull << 40, 0), item("t", "/", true, 7, 0xFFFFFFFFu), item("", "$SYS/x", true, 0, 3),
                                item(big, "$share", false, 99, 99), item("t", t255, true, 9, 9),            item("", "a/", true, 0, 0xFFFFFFFFu), item(big, "", true, 1, 1),
                                item("t", "//", false, 0, 0),       item("", "a//b", true, 2, 2)};
    PackedTopics P;
    for (const It& it : in)
        if (!P.add(it.tenant, it.topic, it.has_ts, it.ts, it.expiry)) FAIL("PackedTopics: add refused a small item\n");
    const size_t tenant_bytes = P.tenants.size(), topic_bytes = P.topics.size();
    P.pad();
    const RbInput r = P.rb_input();
    if (r.n != in.size() || r.n_tenants != 3 || P.n() != r.n || r.tenant_off[3] != tenant_bytes || tenant_bytes != 201 || r.topic_off[r.n] != topic_bytes || !P.any_ts)
        FAIL("PackedTopics: %u items over %u tenants, %zu / %zu bytes\n", r.n, r.n_tenants, tenant_bytes, topic_bytes);
    if (P.tenants.size() != tenant_bytes + 16 || P.topics.size() != topic_bytes + 16) FAIL("PackedTopics: pad did not add 16 bytes\n");
    for (size_t k = 0; k < 16; k++)
        if (r.tenants[tenant_bytes + k] || r.topics[topic_bytes + k]) FAIL("PackedTopics: the 16 bytes behind the tenants / topics are not zero\n");
    const std::vector<It> own = P.items(), cut = PackedTopics::items(r.n, PackedTopics::by_table(r.tenants, r.tenant_off, r.item_tenant, r.topics, r.topic_off), r.ts, r.expiry),
                          bare = PackedTopics::items(r.n, PackedTopics::by_table(r.tenants, r.tenant_off, r.item_tenant, r.topics, r.topic_off), nullptr, nullptr);
    for (size_t i = 0; i < in.size(); i++) {
        const bool has = in[i].has_ts && !(in[i].ts == 0 && in[i].expiry == 0xFFFFFFFFu); // the sentinel rule
        const uint64_t ts = has ? in[i].ts : 0;
        const uint32_t ex = has ? in[i].expiry : 0xFFFFFFFFu;
        for (const std::vector<It>* got : {&own, &cut})
            if ((*got)[i].tenant != in[i].tenant || (*got)[i].topic != in[i].topic || (*got)[i].has_ts != has || (*got)[i].ts != ts || (*got)[i].expiry != ex)
                FAIL("PackedTopics: item %zu comes back as ('%s', '%s', %d, %llu, %u)\n", i, (*got)[i].tenant.c_str(), (*got)[i].topic.c_str(), (int)(*got)[i].has_ts,
                     (unsigned long long)(*got)[i].ts, (*got)[i].expiry);
        if (bare[i].tenant != in[i].tenant || bare[i].topic != in[i].topic || bare[i].has_ts) FAIL("PackedTopics: item %zu without stamp arrays\n", i);
    }
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 24;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const unsigned threads = argc > 3 ? (unsigned)atoi(argv[3]) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    const std::vector<std::string> alpha = {"a", "a!", "", " ", "$x", "b", "0", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0", "w"};
    auto topic = [&]() {
        std::string p;
        const size_t depth = rnd(8) == 0 ? 0 : 1 + rnd(4); // depth 0: the zero-length topic
        for (size_t k = 0; k < depth; k++) p += (k ? "/" : "") + alpha[rnd(alpha.size())] + (rnd(3) ? std::to_string(rnd(40)) : "");
        return p;
    };
    uint64_t n_items = 0, n_overlay = 0, n_bounded = 0, n_fallback = 0, n_deep128 = 0;
    if (packed_round_trip()) return 1;
    const size_t sizes[] = {0, 1, 64, 65, 63, 257};
    for (int round = 0; round < rounds; round++) {
        HostExec hx, bx;
        hx.threads = bx.threads = threads;
        // ---- the serving generation ----
        Packed L;
        const std::vector<std::string> tenants = {"t", "tt", "T", "a-much-longer-tenant-identifier", "", "t"};
        for (auto& t : tenants) L.tenant(t);
        const size_t n = round < 6 ? sizes[round] : 1 + rnd(900);
        for (size_t i = 0; i < n; i++) L.item((uint32_t)rnd(tenants.size()), topic(), ((uint64_t)(1 + i)) << 16, rnd(5) ? (uint32_t)rnd(1000) : 0xFFFFFFFFu);
        // one topic at the executor builder's limit (every 8th round from 7 on) or a level past it (from 6 on): the generation change falls back
        const size_t deep = round % 8 == 6 ? 129 : (round % 8 == 7 ? 128 : 0);
        if (deep) {
            std::string p = "d";
            for (size_t k = 1; k < deep; k++) p += "/d";
            L.item(2, p, 77ull << 16, 1000);
        }
        L.pad();
        RetainIndexHost h;
        RetainBuild<HostExec> rb(hx);
        RetainIndexView v{};
        if (round % 2) {
            if (!rb.build(L.input())) FAIL("round %d: executor builder: %s\n", round, rb.error.c_str());
            retain_catalogue(h, L.input(), rb);
            rb.view(v);
        } else {
            std::vector<RetainIndexHost::Item> items(L.it.size());
            for (size_t i = 0; i < items.size(); i++) {
                items[i].tenant = tenants[L.it[i]];
                items[i].topic.assign(L.pb.data() + L.poff[i], L.poff[i + 1] - L.poff[i]);
                items[i].has_ts = true, items[i].ts = L.ts[i], items[i].expiry = L.ex[i];
            }
            if (!h.rebuild(std::move(items))) FAIL("round %d: host builder: %s\n", round, h.error.c_str());
            v = view_of(h);
        }
        RetainDyn<HostExec> rt(hx);
        rt.tiny = round % 3 != 0;
        if (!rt.reset(v, h)) FAIL("round %d: reset: %s\n", round, rt.error.c_str());
        // ---- churn: adds under loaded and new tenants, removals of loaded topics, removal by id ----
        auto churn = [&](RetainDyn<HostExec>& r, size_t n_ops, uint64_t stamp0) {
            Packed C;
            for (auto& t : {"t", "tt", "brand-new", "", "another-new-tenant-of-some-length"}) C.tenant(t);
            for (size_t i = 0; i < n_ops; i++) {
                const bool remove = rnd(4) == 0 && h.n_topics;
                std::string_view tn, tp;
                if (remove && h.topic((uint32_t)rnd(h.n_topics), tn, tp) && (tn == "t" || tn == "tt" || tn == "")) C.item(tn == "t" ? 0 : (tn == "tt" ? 1 : 3), std::string(tp), 0, 0xFFFFFFFFu, 1);
                else C.item((uint32_t)rnd(5), topic(), (stamp0 + i) << 16, rnd(4) ? (uint32_t)rnd(500) : 0xFFFFFFFFu, 0);
            }
            C.pad();
            return r.apply((const uint8_t*)C.tb.data(), C.toff.data(), 5, C.it.data(), (const uint8_t*)C.pb.data(), C.poff.data(), C.op.data(), (const unsigned long long*)C.ts.data(),
                           C.ex.data(), (uint32_t)C.it.size(), nullptr);
        };
        if (round != 2 && !churn(rt, round < 6 ? 3 + (size_t)round : 1 + rnd(200), 5000)) FAIL("round %d: apply: %s\n", round, rt.error.c_str());
        if (rt.info.id_bound) {
            std::vector<uint32_t> gone;
            for (int k = 0; k < 4; k++) {
                const uint32_t id = (uint32_t)rnd(rt.info.id_bound);
                std::string_view tn, tp;
                if (deep && h.topic(id, tn, tp) && (size_t)std::count(tp.begin(), tp.end(), '/') + 1 == deep) continue; // (the deep topic stays: the round is about it)
                gone.push_back(id);
            }
            uint64_t removed = 0;
            if (!rt.remove_ids(gone.data(), (uint32_t)gone.size(), removed)) FAIL("round %d: remove_ids: %s\n", round, rt.error.c_str());
        }
        if (round % 4 == 1 && !rt.keys_prepare(h, nullptr)) FAIL("round %d: keys_prepare: %s\n", round, rt.error.c_str()); // (else the snapshot builds the store)
        // ---- the snapshot against the host path ----
        std::vector<uint32_t> ids;
        std::vector<Item> want;
        GcQuery q{};
        q.live_only = 1, q.override_expiry = -1;
        RetainNext<HostExec> nx;
        nx.snap = std::make_unique<RetainSnapshot<HostExec>>(hx);
        RetainSnapshot<HostExec>& snap = *nx.snap;
        const RsSnap& S = snap.s;
        if (!rt.select(q, nullptr, 0, ids) || !items_of(rt, h, ids, want)) FAIL("round %d: the host path failed: %s\n", round, rt.error.c_str());
        if (!rt.snapshot(h, 0, nullptr, 0, nullptr, 0, snap)) FAIL("round %d: snapshot: %s\n", round, rt.error.c_str());
        if (compare_snapshot(snap, want, round, "all")) return 1;
        n_items += want.size();
        for (uint32_t id : ids) n_overlay += id >= rt.info.base_n;
        if (!want.empty()) { // ... and bounded: from some live topic's key on
            const Item& m = want[rnd(want.size())];
            const std::string key = retain_message_key(m.tenant, m.topic);
            RetainSnapshot<HostExec> part(hx);
            std::vector<uint32_t> in_ids;
            std::vector<Item> in_want;
            uint64_t topics = 0;
            if (!rt.boundary_select(h, 1u, (const uint8_t*)key.data(), (uint32_t)key.size(), nullptr, 0, topics, nullptr, &in_ids) || !items_of(rt, h, in_ids, in_want))
                FAIL("round %d: boundary_select: %s\n", round, rt.error.c_str());
            if (!rt.snapshot(h, 1u, (const uint8_t*)key.data(), (uint32_t)key.size(), nullptr, 0, part)) FAIL("round %d: bounded snapshot: %s\n", round, rt.error.c_str());
            if (compare_snapshot(part, in_want, round, "bounded")) return 1;
            n_bounded += in_want.size();
        }
        // ---- the product's build step (retain_build_next) from the snapshot, on an executor of its own; meanwhile (threads > 1) the serving
        // generation is mutated ----
        bool churn_ok = true;
        std::thread mutator;
        if (threads > 1) mutator = std::thread([&] { for (int k = 0; k < 3 && churn_ok; k++) churn_ok = churn(rt, 50, 9000 + 100 * (uint64_t)k); });
        RetainIndexHost h2;
        std::string msg;
        const int rc = retain_build_next(nx, bx, h2, rt.tiny, msg);
        if (mutator.joinable()) mutator.join();
        if (!churn_ok) FAIL("round %d: apply beside the build: %s\n", round, rt.error.c_str());
        if (rc != BMQ_OK) FAIL("round %d: retain_build_next: %d, %s\n", round, rc, msg.c_str());
        if (nx.n_items != want.size()) FAIL("round %d: retain_build_next counts %llu items of %zu\n", round, (unsigned long long)nx.n_items, want.size());
        size_t max_levels = 0;
        for (const Item& w : want) max_levels = std::max<size_t>(max_levels, 1 + (size_t)std::count(w.topic.begin(), w.topic.end(), '/'));
        if (deep == 129 && max_levels != 129) FAIL("round %d: the topic of 129 levels is not in the snapshot\n", round);
        if (deep == 128 && max_levels != 128) FAIL("round %d: the topic of 128 levels is not in the snapshot\n", round);
        if (max_levels > RB_MAX_DEPTH) { // declined by the executor builder: the host builder has loaded the snapshot's items, the swap would upload
            if (nx.fallback != 1 || nx.exec_built || nx.rb || nx.rt) FAIL("round %d: a topic of %zu levels, but no fallback to the host builder\n", round, max_levels);
            if (h2.nodes.empty() || h2.n_topics != want.size()) FAIL("round %d: the fallback catalogue holds %llu topics of %zu\n", round, (unsigned long long)h2.n_topics, want.size());
            std::vector<Item> got, sorted = want;
            for (uint32_t id = 0; id < h2.n_topics; id++) {
                std::string_view tn, tp;
                uint64_t s0 = 0;
                uint32_t e0 = 0;
                if (!h2.topic(id, tn, tp, &s0, &e0)) FAIL("round %d: the fallback catalogue has no id %u\n", round, id);
                got.push_back(Item{std::string(tn), std::string(tp), s0, e0});
            }
            auto by_name = [](const Item& a, const Item& b) { return a.tenant != b.tenant ? a.tenant < b.tenant : a.topic < b.topic; };
            std::sort(got.begin(), got.end(), by_name), std::sort(sorted.begin(), sorted.end(), by_name);
            if (!(got == sorted)) FAIL("round %d: the fallback catalogue's items are not the snapshot's\n", round);
            RetainDyn<HostExec> frt(hx); // ... and serves like any host-built generation
            if (!frt.reset(view_of(h2), h2) || frt.info.n_live != want.size() || !churn(frt, 20, 12000)) FAIL("round %d: the fallback generation does not serve: %s\n", round, frt.error.c_str());
            n_fallback++;
            continue;
        }
        if (nx.fallback != 0 || !nx.exec_built || !nx.rb || !nx.rt) FAIL("round %d: no topic of more than %u levels, but a fallback\n", round, RB_MAX_DEPTH);
        n_deep128 += max_levels == 128;
        RetainBuild<HostExec>& nb = *nx.rb;
        RetainDyn<HostExec>& nrt = *nx.rt;
        RetainBuild<HostExec> ref(bx);
        // the same items from host memory (copies: nothing shared with the snapshot)
        std::vector<uint8_t> tb(S.tenants, S.tenants + S.tenant_off[S.n_tenants] + 16);
        std::vector<uint32_t> toff(S.tenant_off, S.tenant_off + S.n_tenants + 1);
        std::vector<uint8_t> pb(S.topics, S.topics + snap.topic_bytes + 16);
        std::vector<uint32_t> poff(S.topic_off, S.topic_off + S.n + 1), itn(S.item_tenant, S.item_tenant + S.n), ex(S.expiry, S.expiry + S.n);
        std::vector<uint64_t> ts(S.ts, S.ts + S.n);
        const RbInput hin{tb.data(), toff.data(), S.n_tenants, itn.data(), pb.data(), poff.data(), S.n, ts.data(), ex.data()};
        if (!ref.build(hin)) FAIL("round %d: build from host memory: %s\n", round, ref.error.c_str());
        if (nb.perm != ref.perm || nb.t_begin != ref.t_begin || nb.names != ref.names || nb.info.n_topics != ref.info.n_topics || nb.info.n_nodes != ref.info.n_nodes ||
            nb.info.n_tokens != ref.info.n_tokens || nb.info.n_posts != ref.info.n_posts || nb.info.n_gp_runs != ref.info.n_gp_runs || nb.info.max_depth != ref.info.max_depth ||
            nb.info.n_items != ref.info.n_items)
            FAIL("round %d: the build from the snapshot and the build from host memory differ (%llu / %llu topics)\n", round, (unsigned long long)nb.info.n_topics,
                 (unsigned long long)ref.info.n_topics);
        if (nb.info.n_nodes && memcmp(nb.img.nodes, ref.img.nodes, sizeof(RNode) * nb.info.n_nodes) != 0) FAIL("round %d: the RNode arrays differ\n", round);
        if (threads == 1 && nb.info.n_nodes) { // one thread: every claim falls the same way, the tables are equal bit for bit
            uint64_t eslots = 0;
            for (const RbTenant& T : nb.plan) eslots = std::max<uint64_t>(eslots, (uint64_t)T.edge_base + 4ull * (T.edge_bucket_mask + 1));
            if (memcmp(nb.img.edges, ref.img.edges, sizeof(REdge) * eslots) != 0 || memcmp(nb.img.posts, ref.img.posts, sizeof(REdge) * nb.info.n_posts) != 0)
                FAIL("round %d: the edge / posting arrays differ\n", round);
        }
        // ---- the next generation's mutable part, adopted by a serving instance ----
        RetainIndexView v2{};
        nb.view(v2);
        RetainDyn<HostExec> rt2(hx);
        rt2.adopt(nrt, v2);
        const uint32_t nt = (uint32_t)h2.n_topics;
        std::vector<uint32_t> live2;
        if (!rt2.select(q, nullptr, 0, live2)) FAIL("round %d: select on the adopted generation: %s\n", round, rt2.error.c_str());
        if (live2.size() != nt || rt2.info.n_live != nt || rt2.info.id_bound != nt) FAIL("round %d: the adopted generation has %zu live ids of %u\n", round, live2.size(), nt);
        for (uint32_t i = 0; i < nt; i++)
            if (live2[i] != i) FAIL("round %d: live ids of the adopted generation are not the ranks\n", round);
        std::vector<unsigned long long> dead;
        if (!rt2.dead_words(dead)) FAIL("round %d: dead_words\n", round);
        std::vector<uint64_t> koff((size_t)nt + 1, 0);
        std::vector<uint8_t> keys((size_t)nt * 400 + 64);
        bool nospace = false;
        if (nt && (!rt2.keys_by_id(h2, live2.data(), nt, keys.data(), keys.size(), (unsigned long long*)koff.data(), nospace) || nospace)) FAIL("round %d: keys_by_id: %s\n", round, rt2.error.c_str());
        for (uint32_t id = 0; id < nt; id++) {
            std::string_view tn, tp;
            uint64_t s0 = 0;
            uint32_t e0 = 0;
            unsigned long long s1 = 0, at = 0;
            uint32_t e1 = 0;
            bool live = false;
            if (!h2.topic(id, tn, tp, &s0, &e0) || !rt2.topic_info(id, s1, e1, at, live) || !live || s0 != s1 || e0 != e1 || at != h2.expire_at[id])
                FAIL("round %d: id %u of the adopted generation: stamps (%llu, %u, %llu), the catalogue has (%llu, %u, %llu)\n", round, id, s1, e1, at, (unsigned long long)s0, e0,
                     (unsigned long long)h2.expire_at[id]);
            const std::string key = retain_message_key(tn, tp);
            if (key != std::string((const char*)keys.data() + koff[id], koff[id + 1] - koff[id])) FAIL("round %d: the key of id %u differs from retain_message_key\n", round, id);
        }
        // ... it takes ops like any other
        if (!churn(rt2, 20, 12000)) FAIL("round %d: apply on the adopted generation: %s\n", round, rt2.error.c_str());
    }
    if (rounds >= 8 && (n_overlay == 0 || n_bounded == 0 || n_fallback == 0 || n_deep128 == 0))
        FAIL("no round reached an overlay topic / a bounded snapshot / a fallback / a topic of 128 levels: the check proves nothing\n");
    printf("retain_snapshot_check ok: %d rounds, %llu items (%llu from the overlay), %llu in bounded snapshots, %llu fallbacks to the host builder, %llu builds of a 128-level topic, packed round trip, %u threads\n",
           rounds, (unsigned long long)n_items, (unsigned long long)n_overlay, (unsigned long long)n_bounded, (unsigned long long)n_fallback, (unsigned long long)n_deep128, threads);
    return 0;
}
