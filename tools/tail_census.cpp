// tools/tail_census.cpp -- planning tool for tail records (CPU only): builds the route index of a few tenants of bench.py's C3 population with the
// product's own builder on the host executor, finds every node X whose subtree is a unary chain X -> c1 -> ... -> ck (one child per level, routes only at
// ck) and whose line has its other slot free, and replays a batch of the workload's publishes over the image by the layout's reading rule twice: as the
// walk reads it today, and with a record for each such X (the walk that resolves X compares the topic's next tokens with the record's and fetches none of
// c1..ck).  Per record format (K = 4 tokens + one payload range, K = 2 + both ranges, and a mixed format: 4 tokens when ck holds one kind of route, 2 when
// both): heads, line fetches per publish with and without records.  The walk below follows tools/plus_census.cpp.
//     g++ -O2 -std=c++17 -pthread -I bifromq_amd/csrc tools/tail_census.cpp bifromq_amd/csrc/bmq_gen.cpp bifromq_amd/csrc/bmq_codec.cpp -o /tmp/tail_census && /tmp/tail_census [tenants=32] [topics=200000] [region_slack=6]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "bmq_dist_index.h"
#include "bmq_exec_host.h"

extern "C" {
void* bmqgen_create(uint64_t seed, uint32_t tenant_base, uint32_t n_tenants, uint32_t routes_per_tenant, int mode);
uint32_t bmqgen_n_keys(void* h);
const uint8_t* bmqgen_key_bytes(void* h);
const uint32_t* bmqgen_key_off(void* h);
const uint8_t* bmqgen_tenant_bytes(void* h);
const uint32_t* bmqgen_tenant_off(void* h);
uint32_t bmqgen_topics(void* h, uint64_t seed, uint32_t n_topics, uint32_t tenant_lo, uint32_t tenant_hi, uint32_t hit_permille, int grouped);
const uint8_t* bmqgen_topic_bytes(void* h);
const uint32_t* bmqgen_topic_off(void* h);
const uint32_t* bmqgen_topic_tenant(void* h);
}
using namespace bmq;

int main(int argc, char** argv) {
    const uint32_t n_ten = argc > 1 ? (uint32_t)atoi(argv[1]) : 32, n_topics = argc > 2 ? (uint32_t)atoi(argv[2]) : 200000;
    const uint32_t slack = argc > 3 ? (uint32_t)atoi(argv[3]) : 6;
    void* g = bmqgen_create(0xB1F20003ull, 0, n_ten, 10000, 1 /* MODE_MIXED */);
    HostExec x;
    x.threads = 8;
    DistIndex<HostExec> h(x);
    h.slack_num = slack;
    h.tail_records = false; // (the records are what this tool models: it starts from the layout without them)
    if (!h.rebuild(bmqgen_key_bytes(g), bmqgen_key_off(g), bmqgen_n_keys(g))) {
        fprintf(stderr, "rebuild: %s\n", h.error.c_str());
        return 1;
    }
    // per tenant: node id -> slot, child count, only child's slot
    struct NodeInfo {
        uint64_t slot;
        uint32_t n_kids;
        uint64_t kid;
    };
    std::vector<std::unordered_map<uint32_t, NodeInfo>> info(h.dir_slots);
    for (uint32_t d = 0; d < h.dir_slots; d++) {
        const TenantSlot& t = h.dir[d];
        if (!(t.hash_lo | t.hash_hi)) continue;
        auto& m = info[d];
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& e = h.trie[t.base + s];
            if (e.parent == NONE) continue;
            m[e.node].slot = s;
        }
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& e = h.trie[t.base + s];
            if (e.parent == NONE || e.parent == 0) continue;
            auto& p = m[e.parent];
            p.n_kids++;
            p.kid = s;
        }
    }
    // chain length below X (0: X is not a head); fmt: 0 = K 4 one range, 1 = K 2 both ranges, 2 = mixed
    auto chain = [&](uint32_t d, const NodeInfo& xi, int fmt) -> uint32_t {
        const TenantSlot& t = h.dir[d];
        if (xi.n_kids != 1) return 0;
        if (h.trie[t.base + (xi.slot ^ 1ull)].parent != NONE) return 0;
        uint64_t s = xi.kid;
        for (uint32_t k = 1; k <= 4; k++) {
            const TrieSlot& c = h.trie[t.base + s];
            const NodeInfo& ci = info[d].at(c.node);
            const bool own = c.own_count != 0, hash = c.hash_count != 0;
            if (ci.n_kids == 0) {
                const uint32_t kmax = fmt == 0 ? (own && hash ? 0 : 4) : fmt == 1 ? 2 : (own && hash ? 2 : 4);
                return k <= kmax ? k : 0;
            }
            if (ci.n_kids != 1 || own || hash) return 0;
            s = ci.kid;
        }
        return 0;
    };
    const uint32_t n = bmqgen_topics(g, 11, n_topics, 0, n_ten, 900, 1);
    const uint8_t* tb = bmqgen_topic_bytes(g);
    const uint32_t* to = bmqgen_topic_off(g);
    const uint32_t* tt = bmqgen_topic_tenant(g);
    const uint8_t* nb = bmqgen_tenant_bytes(g);
    const uint32_t* no = bmqgen_tenant_off(g);
    const DistIndexMut ix = h.mut();
    for (int fmt = -1; fmt < 3; fmt++) {
        uint64_t heads = 0, nodes = 0;
        std::vector<std::unordered_map<uint32_t, uint32_t>> rec(h.dir_slots); // node -> k
        if (fmt >= 0)
            for (uint32_t d = 0; d < h.dir_slots; d++)
                for (const auto& [node, xi] : info[d]) {
                    nodes++;
                    const uint32_t k = chain(d, xi, fmt);
                    if (k) rec[d][node] = k, heads++;
                }
        uint64_t visits = 0, fetches = 0, tail_hits = 0;
        struct Item {
            uint32_t node, level;
            bool is_plus;
            uint64_t pslot;
        };
        constexpr uint64_t AT_ROOT = ~0ull;
        std::vector<Item> st;
        std::vector<uint32_t> toks;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t d = tenant_find(ix.tenants, ix.tenant_mask, ix.tenant_names, nb, no[tt[i]], no[tt[i] + 1]);
            if (d == NONE) continue;
            const TenantSlot& rg = h.dir[d];
            toks.clear();
            unsigned long long pos = to[i];
            const unsigned long long end = to[i + 1];
            for (;;) {
                LevelHash lh;
                uint32_t inl[4], len;
                const unsigned long long start = pos;
                scan_level_bytes<0x2F2F2F2Fu>(tb, pos, end, lh, inl, len);
                toks.push_back(dict_intern(ix, lh, len, inl, tb, start, false));
                if (pos >= end) break;
                pos++;
            }
            const bool sys = end > to[i] && tb[to[i]] == '$';
            st.clear();
            auto visit = [&](uint32_t node, uint64_t slot, uint32_t dl, uint32_t bloom) {
                if (dl >= toks.size()) return;
                if (slot != AT_ROOT) {
                    auto r = rec[d].find(node);
                    if (r != rec[d].end()) { // the record: compare the tokens of the chain
                        tail_hits++;
                        uint64_t s = info[d].at(node).kid;
                        for (uint32_t k = 0; k < r->second && dl + k < toks.size(); k++) {
                            const TrieSlot& c = h.trie[rg.base + s];
                            if (c.token != TOK_PLUS && c.token != toks[dl + k]) break;
                            visits++;
                            if (k + 1 < r->second) s = info[d].at(c.node).kid;
                        }
                        return;
                    }
                }
                const uint32_t t = toks[dl];
                if (t != TOK_UNKNOWN && ((bloom >> bloom_bit(t)) & 1u)) st.push_back({node, dl, false, slot});
                if ((bloom & BLOOM_PLUS) && !(dl == 0 && sys)) st.push_back({node, dl, true, slot});
            };
            visit(0, AT_ROOT, 0, rg.root_lit_bloom);
            while (!st.empty()) {
                const Item it = st.back();
                st.pop_back();
                const uint32_t tok = it.is_plus ? TOK_PLUS : toks[it.level];
                if (it.is_plus && it.pslot == AT_ROOT && rg.root_plus != NONE) {
                    const TrieSlot& p0 = h.trie[rg.base + rg.root_plus];
                    visits++;
                    visit(p0.node, rg.root_plus, it.level + 1, p0.lit_bloom);
                    continue;
                }
                if (it.is_plus && it.pslot != AT_ROOT) {
                    const TrieSlot& o = h.trie[rg.base + (it.pslot ^ 1ull)];
                    if (o.parent == it.node && o.token == TOK_PLUS) {
                        visits++;
                        visit(o.node, it.pslot ^ 1ull, it.level + 1, o.lit_bloom);
                        continue;
                    }
                }
                uint32_t bk = edge_bucket(it.node, tok, rg.buckets);
                for (uint32_t probes = 0; probes < rg.buckets; probes++) {
                    fetches++;
                    const TrieSlot* hit = nullptr;
                    uint64_t slot = 0;
                    for (uint32_t j = 0; j < 2 && !hit; j++) {
                        const TrieSlot& e = h.trie[rg.base + 2 * bk + j];
                        if (e.parent == it.node && e.token == tok) hit = &e, slot = 2ull * bk + j;
                    }
                    if (hit) {
                        visits++;
                        visit(hit->node, slot, it.level + 1, hit->lit_bloom);
                        break;
                    }
                    // (a record fills its bucket: a probe that ends here today would go on to the next bucket)
                    const bool free0 = h.trie[rg.base + 2 * bk].parent == NONE && !(fmt >= 0 && rec[d].count(h.trie[rg.base + 2 * bk + 1].node));
                    const bool free1 = h.trie[rg.base + 2 * bk + 1].parent == NONE && !(fmt >= 0 && rec[d].count(h.trie[rg.base + 2 * bk].node));
                    if (free0 || free1) break;
                    bk = bk + 1 == rg.buckets ? 0 : bk + 1;
                }
            }
        }
        static const char* names[] = {"no records", "K=4, one range", "K=2, both ranges", "mixed (4 | 2)"};
        printf("slack %u  %-17s heads %8llu of %8llu nodes  per publish: %.3f nodes discovered, %.3f line fetches, %.3f records read\n", slack, names[fmt + 1],
               (unsigned long long)heads, (unsigned long long)nodes, (double)visits / n, (double)fetches / n, (double)tail_hits / n);
    }
    return 0;
}
