// tools/bloom_census.cpp -- planning tool for the child filter words (CPU only): builds the route index of a few tenants of bench.py's C3 population with
// the product's own builder on the host executor and replays a batch of the workload's publishes over the image by the layout's reading rule (tail records
// modelled in their shipped format, K = 4 tokens + one range, as tools/tail_census.cpp does) twice: with the 31-bit Bloom word alone deciding which literal
// child is probed for, and with the shipped rule -- the Bloom word AND the child filter words the builder left in the begin words of the parent's empty
// ranges (bmq_layout.h: filter_bit_own / filter_bit_hash).  Per publish: nodes discovered, line fetches, literal probes, probes that found their child,
// FALSE POSITIVES (a probe for a child that does not exist: one line fetched for nothing -- more where the home bucket is full).  Then the false positives
// by the parent's number of literal children and by how many of its range words are free, and, for the record, what 62 bits per empty range (the begin
// word + 30 bits of the count word behind a flag: not built) would leave.
//     g++ -O2 -std=c++17 -pthread -I bifromq_amd/csrc tools/bloom_census.cpp bifromq_amd/csrc/bmq_gen.cpp bifromq_amd/csrc/bmq_codec.cpp -o /tmp/bloom_census && /tmp/bloom_census [tenants=32] [topics=200000] [region_slack=6]
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
    h.tail_records = false; // (the records are modelled below, as in tools/tail_census.cpp; the filter words do not depend on them)
    if (!h.rebuild(bmqgen_key_bytes(g), bmqgen_key_off(g), bmqgen_n_keys(g))) {
        fprintf(stderr, "rebuild: %s\n", h.error.c_str());
        return 1;
    }
    // per tenant: node id -> slot, child count, only child's slot, literal children's tokens
    struct NodeInfo {
        uint64_t slot = 0;
        uint32_t n_kids = 0;
        uint64_t kid = 0;
        std::vector<uint32_t> lit;
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
            if (e.token != TOK_PLUS) p.lit.push_back(e.token);
        }
    }
    // tail records, K = 4 + one range: chain length below X (0: X is not a head)
    auto chain = [&](uint32_t d, const NodeInfo& xi) -> uint32_t {
        const TenantSlot& t = h.dir[d];
        if (xi.n_kids != 1) return 0;
        if (h.trie[t.base + (xi.slot ^ 1ull)].parent != NONE) return 0;
        uint64_t s = xi.kid;
        for (uint32_t k = 1; k <= 4; k++) {
            const TrieSlot& c = h.trie[t.base + s];
            const NodeInfo& ci = info[d].at(c.node);
            const bool own = c.own_count != 0, hash = c.hash_count != 0;
            if (ci.n_kids == 0) return own && hash ? 0 : k;
            if (ci.n_kids != 1 || own || hash) return 0;
            s = ci.kid;
        }
        return 0;
    };
    std::vector<std::unordered_map<uint32_t, uint32_t>> rec(h.dir_slots); // node -> k
    for (uint32_t d = 0; d < h.dir_slots; d++)
        for (const auto& [node, xi] : info[d]) {
            const uint32_t k = chain(d, xi);
            if (k) rec[d][node] = k;
        }
    const uint32_t n = bmqgen_topics(g, 11, n_topics, 0, n_ten, 900, 1);
    const uint8_t* tb = bmqgen_topic_bytes(g);
    const uint32_t* to = bmqgen_topic_off(g);
    const uint32_t* tt = bmqgen_topic_tenant(g);
    const uint8_t* nb = bmqgen_tenant_bytes(g);
    const uint32_t* no = bmqgen_tenant_off(g);
    const DistIndexMut ix = h.mut();
    // what 62 bits per empty range would say (one more mix of the token per range; not built)
    auto bit62 = [](uint32_t tok, uint32_t which) { return (uint32_t)(((uint64_t)(tok * (which ? 0x85EBCA77u : 0x9E3779B1u)) * 62u) >> 32); };
    constexpr int N_CLASS = 6;
    static const char* class_name[N_CLASS] = {"< 4", "4-7", "8-15", "16-31", "32-63", ">= 64"};
    auto kid_class = [](size_t k) { return k < 4 ? 0 : k < 8 ? 1 : k < 16 ? 2 : k < 32 ? 3 : k < 64 ? 4 : 5; };
    double fetches_mode[2] = {0, 0}, visits_mode[2] = {0, 0};
    for (int mode = 0; mode < 2; mode++) { // 0: the Bloom word alone; 1: the shipped rule
        uint64_t visits = 0, fetches = 0, lit_probes = 0, lit_found = 0, fp = 0, fp_root = 0;
        uint64_t fp_class[N_CLASS] = {}, fp_free[3] = {}, fp_left_shipped = 0, fp_left_62 = 0;
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
                bool lit = t != TOK_UNKNOWN && ((bloom >> bloom_bit(t)) & 1u);
                if (lit && mode == 1 && slot != AT_ROOT) { // the shipped rule: the words the builder left in the node's slot
                    const TrieSlot& e = h.trie[rg.base + slot];
                    lit = ((filter_word(e.own_begin, e.own_count) >> filter_bit_own(t)) & (filter_word(e.hash_begin, e.hash_count) >> filter_bit_hash(t)) & 1u) != 0;
                }
                if (lit) st.push_back({node, dl, false, slot});
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
                if (!it.is_plus) lit_probes++;
                bool found = false;
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
                        found = true;
                        visit(hit->node, slot, it.level + 1, hit->lit_bloom);
                        break;
                    }
                    // (a record fills its bucket: a probe that ends here without records goes on to the next bucket)
                    const bool free0 = h.trie[rg.base + 2 * bk].parent == NONE && !rec[d].count(h.trie[rg.base + 2 * bk + 1].node);
                    const bool free1 = h.trie[rg.base + 2 * bk + 1].parent == NONE && !rec[d].count(h.trie[rg.base + 2 * bk].node);
                    if (free0 || free1) break;
                    bk = bk + 1 == rg.buckets ? 0 : bk + 1;
                }
                if (it.is_plus) continue;
                if (found) {
                    lit_found++;
                    continue;
                }
                fp++;
                if (it.pslot == AT_ROOT) {
                    fp_root++;
                    fp_left_shipped++, fp_left_62++;
                    continue;
                }
                const TrieSlot& e = h.trie[rg.base + it.pslot];
                const NodeInfo& pi = info[d].at(it.node);
                fp_class[kid_class(pi.lit.size())]++;
                fp_free[(e.own_count == 0) + (e.hash_count == 0)]++;
                if ((filter_word(e.own_begin, e.own_count) >> filter_bit_own(tok)) & (filter_word(e.hash_begin, e.hash_count) >> filter_bit_hash(tok)) & 1u) fp_left_shipped++;
                bool pass62 = true;
                for (uint32_t which = 0; which < 2 && pass62; which++) {
                    if ((which ? e.hash_count : e.own_count) != 0) continue;
                    unsigned long long w = 0;
                    for (uint32_t c : pi.lit) w |= 1ull << bit62(c, which);
                    pass62 = (w >> bit62(tok, which)) & 1ull;
                }
                fp_left_62 += pass62;
            }
        }
        fetches_mode[mode] = (double)fetches / n, visits_mode[mode] = (double)visits / n;
        printf("slack %u  %-17s per publish: %.3f nodes discovered, %.3f line fetches, %.3f literal probes, %.3f found, %.3f false positives (%.3f at the tenant root)\n", slack,
               mode == 0 ? "Bloom word alone" : "child filters", (double)visits / n, (double)fetches / n, (double)lit_probes / n, (double)lit_found / n, (double)fp / n,
               (double)fp_root / n);
        if (mode == 0) {
            printf("  false positives per publish by the parent's literal children:");
            for (int c = 0; c < N_CLASS; c++) printf("  %s: %.3f", class_name[c], (double)fp_class[c] / n);
            printf("\n  ... by the parent's free range words:  neither: %.3f  one: %.3f  both: %.3f\n", (double)fp_free[0] / n, (double)fp_free[1] / n, (double)fp_free[2] / n);
            printf("  ... left by the shipped rule (32 bits per empty range): %.3f;  by 62 bits per empty range (not built): %.3f\n", (double)fp_left_shipped / n,
                   (double)fp_left_62 / n);
        }
    }
    printf("child filters: %.3f line fetches per publish fewer, nodes discovered %s\n", fetches_mode[0] - fetches_mode[1], visits_mode[0] == visits_mode[1] ? "equal" : "DIFFERENT");
    return visits_mode[0] == visits_mode[1] ? 0 : 1;
}
