// retain_build_check.cpp -- test tool, not product: the two bulk builders of the retained-topic index side by side, without a GPU, under
// AddressSanitizer/UBSan and (several host threads: the CAS inserts) ThreadSanitizer.  Per seeded round one load is built by the host builder
// (bmq_retain.cpp) and by the executor builder (bmq_retain_build_core.h through RetainBuild<HostExec>: the very functions the k_rb_* kernels
// wrap), and the IMAGE is compared:
//   * the catalogue: the same ids for the same (tenant, topic), the stamps of the LAST add of a duplicate;
//   * RNode slices bitwise equal per tenant (the child_begin of childless nodes included);
//   * edge sets equal as (parent, label bytes, child, child_topic); every edge reachable from its home bucket the way redge_find and the walk
//     go (every bucket in front of it full, RE_OVERFLOW on the home bucket's first entry exactly when an edge of that home lies elsewhere);
//   * the grandchild postings: every (grandparent, label) run found through the RGp hash under the same overflow rule, its slice ordered by
//     parent and equal to the host builder's;
//   * the '$' runs and the directory entries; every label and tenant id resolves through rdict_find to the token the edges carry; tokens are
//     injective and >= TOK_FIRST;
//   * a load with a topic of more than RB_MAX_DEPTH levels is declined (too_deep), one of exactly RB_MAX_DEPTH is built.
// Build + run: make -C bifromq_amd/csrc rbcheck   (tests/test_retain_build.py builds and runs both forms)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../bifromq_amd/csrc/bmq_exec_host.h"
#include "../bifromq_amd/csrc/bmq_retain.h"
#include "../bifromq_amd/csrc/bmq_retain_build.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

struct Load {
    std::vector<std::string> tenants;
    std::vector<uint32_t> item_tenant;
    std::vector<std::string> topics;
    std::vector<uint64_t> ts;
    std::vector<uint32_t> ex;
};

static uint32_t find_token(const RetainIndexView& v, std::string_view s) { // the read side's look-up, hashed the host dictionary's way
    const LevelHash h = hash_level(s);
    uint32_t inl[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < s.size() && i < 16; i++) inl[i >> 2] |= (uint32_t)(uint8_t)s[i] << (8 * (i & 3));
    return rdict_find(v, h, (uint32_t)s.size(), inl, (const uint8_t*)s.data(), 0);
}

using EdgeKey = std::tuple<uint32_t, std::string, uint32_t, uint32_t>; // parent, label, child, child_topic

// edges of a region as a set + the reachability rule
static int edge_region(const REdge* e, uint32_t mask, const std::map<uint32_t, std::string>& label, std::set<EdgeKey>& out, uint64_t& overflows, const char* who) {
    std::set<uint32_t> need_flag;
    const uint32_t slots = 4 * (mask + 1);
    for (uint32_t s = 0; s < slots; s++) {
        if (e[s].parent == NONE) continue;
        auto l = label.find(e[s].token);
        if (l == label.end()) FAIL("%s: edge with a token nobody interned\n", who);
        if (!out.insert({e[s].parent, l->second, e[s].child & ~RE_OVERFLOW, e[s].child_topic}).second) FAIL("%s: an edge twice\n", who);
        const uint32_t home = redge_bucket(e[s].parent, e[s].token, mask);
        for (uint32_t bk = home; bk != s / 4; bk = (bk + 1) & mask)
            for (uint32_t j = 0; j < 4; j++)
                if (e[4 * bk + j].parent == NONE) FAIL("%s: a free entry in front of an edge (home %u, entry %u)\n", who, home, s);
        if (s / 4 != home) need_flag.insert(home), overflows++;
    }
    for (uint32_t bk = 0; bk <= mask; bk++)
        if (((e[4 * bk].child & RE_OVERFLOW) != 0) != (need_flag.count(bk) != 0)) FAIL("%s: RE_OVERFLOW of bucket %u is %s\n", who, bk, need_flag.count(bk) ? "missing" : "spurious");
    return 0;
}

using Run = std::vector<std::tuple<uint32_t, uint32_t, uint32_t>>; // parent, child, child_topic
static int gp_table(const RGp* g, uint32_t mask, const REdge* posts, size_t n_posts, const std::map<uint32_t, std::string>& label,
                    std::map<std::pair<uint32_t, std::string>, Run>& out, uint64_t& overflows, const char* who) {
    std::set<uint32_t> need_flag;
    const uint32_t slots = 4 * (mask + 1);
    size_t covered = 0;
    for (uint32_t s = 0; s < slots; s++) {
        if (g[s].gp == NONE) continue;
        auto l = label.find(g[s].token);
        if (l == label.end()) FAIL("%s: run with a token nobody interned\n", who);
        const uint32_t cnt = g[s].count & ~RE_OVERFLOW;
        if (cnt == 0 || (uint64_t)g[s].begin + cnt > n_posts) FAIL("%s: run outside the postings\n", who);
        Run r;
        for (uint32_t k = 0; k < cnt; k++) {
            const REdge& p = posts[g[s].begin + k];
            if (p.token != g[s].token) FAIL("%s: a posting with another token inside a run\n", who);
            if (k && p.parent <= std::get<0>(r.back())) FAIL("%s: a run not ordered by parent\n", who);
            r.push_back({p.parent, p.child, p.child_topic});
        }
        covered += cnt;
        if (!out.emplace(std::make_pair(g[s].gp, l->second), std::move(r)).second) FAIL("%s: a run twice\n", who);
        const uint32_t home = rgp_bucket(g[s].gp, g[s].token, mask);
        for (uint32_t bk = home; bk != s / 4; bk = (bk + 1) & mask)
            for (uint32_t j = 0; j < 4; j++)
                if (g[4 * bk + j].gp == NONE) FAIL("%s: a free entry in front of a run\n", who);
        if (s / 4 != home) need_flag.insert(home), overflows++;
    }
    if (covered != n_posts) FAIL("%s: the runs cover %zu of %zu postings\n", who, covered, n_posts);
    for (uint32_t bk = 0; bk <= mask; bk++)
        if (((g[4 * bk].count & RE_OVERFLOW) != 0) != (need_flag.count(bk) != 0)) FAIL("%s: RE_OVERFLOW of gp bucket %u is %s\n", who, bk, need_flag.count(bk) ? "missing" : "spurious");
    return 0;
}

static RbInput pack(const Load& L, std::string& tb, std::vector<uint32_t>& toff, std::string& pb, std::vector<uint32_t>& poff) {
    tb.clear(), pb.clear(), toff.assign(1, 0), poff.assign(1, 0);
    for (auto& t : L.tenants) tb += t, toff.push_back((uint32_t)tb.size());
    for (auto& p : L.topics) pb += p, poff.push_back((uint32_t)pb.size());
    tb.append(16, '\0'), pb.append(16, '\0');
    return RbInput{(const uint8_t*)tb.data(), toff.data(), (uint32_t)L.tenants.size(), L.item_tenant.data(), (const uint8_t*)pb.data(), poff.data(), (uint32_t)L.topics.size(),
                   L.ts.data(), L.ex.data()};
}

static int compare(const Load& L, unsigned threads, int round, uint64_t& n_nodes, uint64_t& n_edge_ovf, uint64_t& n_gp_ovf, uint64_t& n_posts) {
    std::vector<RetainIndexHost::Item> items(L.topics.size());
    for (size_t i = 0; i < items.size(); i++) {
        items[i].tenant = L.tenants[L.item_tenant[i]];
        items[i].topic = L.topics[i];
        items[i].has_ts = true, items[i].ts = L.ts[i], items[i].expiry = L.ex[i];
    }
    RetainIndexHost h0;
    if (!h0.rebuild(std::move(items))) FAIL("round %d: host builder: %s\n", round, h0.error.c_str());
    std::string tb, pb;
    std::vector<uint32_t> toff, poff;
    const RbInput in = pack(L, tb, toff, pb, poff);
    HostExec hx;
    hx.threads = threads;
    RetainBuild<HostExec> rb(hx);
    if (!rb.build(in)) FAIL("round %d: executor builder: %s\n", round, rb.error.c_str());
    RetainIndexHost h1;
    retain_catalogue(h1, in, rb);
    RetainIndexView v{};
    rb.view(v);
    // ---- catalogue ----
    if (h0.n_topics != h1.n_topics || h0.order.size() != h1.order.size() || rb.info.n_topics != h0.n_topics) FAIL("round %d: %llu topics / %zu tenants, host builder %llu / %zu\n", round,
                                                                                                                  (unsigned long long)h1.n_topics, h1.order.size(), (unsigned long long)h0.n_topics, h0.order.size());
    for (uint32_t id = 0; id < h0.n_topics; id++) {
        std::string_view t0, p0, t1, p1;
        uint64_t s0 = 0, s1 = 0;
        uint32_t e0 = 0, e1 = 0;
        if (!h0.topic(id, t0, p0, &s0, &e0) || !h1.topic(id, t1, p1, &s1, &e1) || t0 != t1 || p0 != p1 || s0 != s1 || e0 != e1 || h0.expire_at[id] != h1.expire_at[id])
            FAIL("round %d: id %u is ('%.*s', '%.*s') stamp %llu, host builder ('%.*s', '%.*s') stamp %llu\n", round, id, (int)t1.size(), t1.data(), (int)p1.size(), p1.data(),
                 (unsigned long long)s1, (int)t0.size(), t0.data(), (int)p0.size(), p0.data(), (unsigned long long)s0);
    }
    // ---- dictionary: token -> string, injective both ways ----
    std::map<uint32_t, std::string> lab1, lab0;
    {
        std::set<std::string> seen;
        const uint32_t slots = (v.dict_group_mask + 1) * DICT_GROUP;
        for (uint32_t s = 0; s < slots; s++) {
            const DictSlot& d = v.dict[s];
            if (!d.tag) continue;
            std::string str;
            for (uint32_t i = 0; i < d.len && i < 16; i++) str.push_back((char)((d.inl[i >> 2] >> (8 * (i & 3))) & 0xFF));
            if (d.len > 16) str.assign((const char*)v.pool + d.pool_off, d.len);
            if (d.token < TOK_FIRST || !lab1.emplace(d.token, str).second || !seen.insert(str).second) FAIL("round %d: dictionary token %u / string '%s' twice or out of range\n", round, d.token, str.c_str());
            if (find_token(v, str) != d.token) FAIL("round %d: '%s' does not resolve to its token\n", round, str.c_str());
        }
        if (lab1.size() != rb.info.n_tokens || lab1.size() != h0.dict_h.entries.size()) FAIL("round %d: %zu tokens, info says %llu, host builder %zu\n", round, lab1.size(),
                                                                                             (unsigned long long)rb.info.n_tokens, h0.dict_h.entries.size());
        if (slots < 4 * lab1.size()) FAIL("round %d: dictionary load above 1/4\n", round);
        for (size_t t = 0; t < h0.dict_h.entries.size(); t++) lab0[(uint32_t)t + TOK_FIRST] = std::string(h0.dict_h.entries[t].s);
    }
    // ---- per tenant ----
    uint64_t eo = 0, go = 0;
    for (size_t t = 0; t < h0.order.size(); t++) {
        const RTenantState& a = *h0.order[t];
        const RbTenant& P = rb.plan[t];
        const std::string who = "round " + std::to_string(round) + " tenant '" + a.name + "'";
        if (a.name != rb.names[t]) FAIL("%s: is '%s' here\n", who.c_str(), rb.names[t].c_str());
        if (a.nodes.size() != P.n_nodes || memcmp(a.nodes.data(), v.nodes + P.node_base, sizeof(RNode) * P.n_nodes) != 0) {
            for (size_t k = 0; k < std::min<size_t>(a.nodes.size(), P.n_nodes); k++) {
                const RNode &x = a.nodes[k], &y = v.nodes[P.node_base + k];
                if (memcmp(&x, &y, sizeof(RNode))) FAIL("%s: node %zu is (%u, %#x, %u, %u), host builder (%u, %#x, %u, %u)\n", who.c_str(), k, y.child_begin, y.child_count, y.sub_begin, y.sub_end,
                                                        x.child_begin, x.child_count, x.sub_begin, x.sub_end);
            }
            FAIL("%s: %u nodes, host builder %zu\n", who.c_str(), P.n_nodes, a.nodes.size());
        }
        n_nodes += P.n_nodes;
        const uint32_t ttok = find_token(v, a.name);
        const RTenantSlot* slot = ttok == TOK_UNKNOWN ? nullptr : rtenant_find(v, ttok);
        if (!slot) FAIL("%s: not in the directory\n", who.c_str());
        if (slot->node_base != P.node_base || slot->edge_base != P.edge_base || slot->edge_bucket_mask != P.edge_bucket_mask || slot->id_base != a.id_base || slot->post_base != P.post_base ||
            slot->gp_base != P.gp_base || slot->gp_bucket_mask != P.gp_bucket_mask)
            FAIL("%s: directory entry and plan differ\n", who.c_str());
        if (slot->sys_node_lo != a.sys_node_lo || slot->sys_node_hi != a.sys_node_hi || slot->sys_id_lo != a.sys_id_lo || slot->sys_id_hi != a.sys_id_hi || P.sys_id_lo != a.sys_id_lo ||
            P.sys_id_hi != a.sys_id_hi)
            FAIL("%s: '$' run nodes [%u, %u) ids [%u, %u), host builder [%u, %u) [%u, %u)\n", who.c_str(), slot->sys_node_lo, slot->sys_node_hi, slot->sys_id_lo, slot->sys_id_hi, a.sys_node_lo,
                 a.sys_node_hi, a.sys_id_lo, a.sys_id_hi);
        if (P.edge_bucket_mask != (uint32_t)a.edges.size() / 4 - 1 || P.gp_bucket_mask != (uint32_t)a.gps.size() / 4 - 1) FAIL("%s: table sizes differ from the host builder's\n", who.c_str());
        std::set<EdgeKey> e0, e1;
        uint64_t x = 0;
        if (edge_region(a.edges.data(), (uint32_t)a.edges.size() / 4 - 1, lab0, e0, x, (who + " (host builder)").c_str())) return 1;
        if (edge_region(v.edges + P.edge_base, P.edge_bucket_mask, lab1, e1, eo, who.c_str())) return 1;
        if (e0 != e1) FAIL("%s: edge sets differ (%zu, host builder %zu)\n", who.c_str(), e1.size(), e0.size());
        for (auto& e : e1) // every label resolves through the read side to the token of its edge
            if (redge_find(v, P.edge_base, P.edge_bucket_mask, std::get<0>(e), find_token(v, std::get<1>(e))) != std::get<2>(e)) FAIL("%s: redge_find misses an edge\n", who.c_str());
        if (a.posts.size() != P.n_posts) FAIL("%s: %u postings, host builder %zu\n", who.c_str(), P.n_posts, a.posts.size());
        std::map<std::pair<uint32_t, std::string>, Run> r0, r1;
        if (gp_table(a.gps.data(), (uint32_t)a.gps.size() / 4 - 1, a.posts.data(), a.posts.size(), lab0, r0, x, (who + " (host builder)").c_str())) return 1;
        if (gp_table(v.gps + P.gp_base, P.gp_bucket_mask, v.posts + P.post_base, P.n_posts, lab1, r1, go, who.c_str())) return 1;
        if (r0 != r1) FAIL("%s: postings differ (%zu runs, host builder %zu)\n", who.c_str(), r1.size(), r0.size());
        if (r1.size() != P.n_runs) FAIL("%s: %zu runs, plan says %u\n", who.c_str(), r1.size(), P.n_runs);
        n_posts += P.n_posts;
    }
    if (eo != rb.info.n_edge_overflows || go != rb.info.n_gp_overflows) FAIL("round %d: %llu / %llu overflows counted, the image holds %llu / %llu\n", round, (unsigned long long)rb.info.n_edge_overflows,
                                                                             (unsigned long long)rb.info.n_gp_overflows, (unsigned long long)eo, (unsigned long long)go);
    n_edge_ovf += eo, n_gp_ovf += go;
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const unsigned threads = argc > 3 ? (unsigned)atoi(argv[3]) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    uint64_t n_nodes = 0, n_edge_ovf = 0, n_gp_ovf = 0, n_posts = 0, n_items = 0;
    for (int round = 0; round < rounds; round++) {
        Load L;
        const int kind = round % 4;
        // labels that sort around '/' (0x2F), empty levels, '$', one longer than the inline 16 bytes
        std::vector<std::string> alpha = {"a", "a!", "a-", "a.", "a0", "", " ", "$x", "$", "b", "!", "0", "a-level-longer-than-sixteen-bytes", "a-level-longer-than-sixteen-bytez", "\xE4\xBD\xA0"};
        if (kind == 1)
            for (int i = 0; i < 300; i++) alpha.push_back("w" + std::to_string(i));
        L.tenants = {"t", "tt", "T", "a-much-longer-tenant-identifier", "", "t"}; // (one id twice)
        if (kind == 2)
            for (int i = 0; i < 300; i++) L.tenants.push_back("ten" + std::to_string(rnd(1000)));
        const size_t n = round == 0 ? 0 : (round == 1 ? 1 : 1 + rnd(kind == 1 ? 6000 : 1200));
        for (size_t i = 0; i < n; i++) {
            std::string p;
            const size_t depth = 1 + rnd(kind == 3 && rnd(50) == 0 ? RB_MAX_DEPTH : 5);
            for (size_t k = 0; k < depth; k++) p += (k ? "/" : "") + alpha[rnd(rnd(3) ? std::min<size_t>(alpha.size(), 15) : alpha.size())];
            if (kind == 1 && rnd(3) == 0) p = "a/" + alpha[15 + rnd(300)] + "/" + alpha[rnd(rnd(2) ? 3 : alpha.size())] + (rnd(2) ? "/b" : "");
            if (kind == 3 && i && rnd(4) == 0) p = L.topics[rnd(i)]; // duplicates: the last add wins
            L.topics.push_back(p);
            L.item_tenant.push_back((uint32_t)rnd(kind == 3 ? 2 : L.tenants.size()));
            L.ts.push_back(((uint64_t)(1 + i)) << 16);
            L.ex.push_back((uint32_t)rnd(5) ? (uint32_t)rnd(1000) : 0xFFFFFFFFu);
        }
        n_items += n;
        if (compare(L, threads, round, n_nodes, n_edge_ovf, n_gp_ovf, n_posts)) return 1;
    }
    { // depth: RB_MAX_DEPTH levels are built, one more is declined and nothing changes
        Load L;
        L.tenants = {"t"};
        std::string p = "x";
        for (uint32_t k = 1; k < RB_MAX_DEPTH; k++) p += "/x";
        L.topics = {"a", p, p + "/y"};
        L.item_tenant = {0, 0, 0};
        L.ts = {1 << 16, 2 << 16, 3 << 16};
        L.ex = {1, 2, 3};
        std::string tb, pb;
        std::vector<uint32_t> toff, poff;
        HostExec hx;
        hx.threads = threads;
        RetainBuild<HostExec> rb(hx);
        RbInput in = pack(L, tb, toff, pb, poff);
        if (rb.build(in) || !rb.too_deep || rb.img.nodes) FAIL("a topic of %u levels was not declined\n", RB_MAX_DEPTH + 1);
        L.topics.pop_back(), L.item_tenant.pop_back(), L.ts.pop_back(), L.ex.pop_back();
        if (compare(L, threads, -1, n_nodes, n_edge_ovf, n_gp_ovf, n_posts)) return 1;
    }
    if (rounds >= 8 && (n_edge_ovf == 0 || n_gp_ovf == 0 || n_posts == 0)) FAIL("no round reached an overflowing edge bucket / gp bucket / a posting: the check proves nothing\n");
    printf("retain_build_check ok: %d rounds, %llu items, %llu nodes, %llu postings, %llu + %llu overflows, %u threads\n", rounds, (unsigned long long)n_items, (unsigned long long)n_nodes,
           (unsigned long long)n_posts, (unsigned long long)n_edge_ovf, (unsigned long long)n_gp_ovf, threads);
    return 0;
}
