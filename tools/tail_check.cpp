// tools/tail_check.cpp -- checks the tail records of the filter trie (bmq_layout.h) on indexes the product's own builder makes on the host executor:
// every record equals the chain it stands for (tokens, payload, one route kind at the leaf, at most TAIL_K levels, free slot beside its head -- never
// beside a '+' child that lies beside its parent), through rebuilds, apply batches (puts inside tails, deletes and puts on their leaves, id lists),
// region growth (minimal capacities: every growth path runs) and compaction; apply batches must leave tombstones; with the records switched off there
// are none.  Prints "tail check ok: ..." (tests/test_tail_records.py).
//     g++ -O1 -std=c++17 -pthread -I bifromq_amd/csrc tools/tail_check.cpp bifromq_amd/csrc/bmq_codec.cpp -o /tmp/tail_check && /tmp/tail_check [rounds] [seed]
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "bmq_codec.h"
#include "bmq_dist_index.h"
#include "bmq_exec_host.h"

using namespace bmq;

struct Census {
    uint64_t records = 0, tombs = 0, heads = 0;
};
// false + message: a record that does not stand for its chain
static bool check_image(DistIndex<HostExec>& h, Census& c, std::string& why) {
    for (uint32_t d = 0; d < h.dir_slots; d++) {
        const TenantSlot& t = h.dir[d];
        if (!(t.hash_lo | t.hash_hi)) continue;
        std::unordered_map<uint32_t, uint32_t> slot_of, n_kids, kid;
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& e = h.trie[t.base + s];
            if (!slot_is_node(e)) continue;
            slot_of[e.node] = s;
            if (e.parent != 0) n_kids[e.parent]++, kid[e.parent] = s;
        }
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& r = h.trie[t.base + s];
            if (r.parent != NONE && r.token == TOK_TOMB) c.tombs++;
            if (r.parent == NONE || r.token != TOK_TAIL) continue;
            c.records++;
            const TrieSlot& x = h.trie[t.base + (s ^ 1u)];
            if (!slot_is_node(x) || x.node != r.parent) return why = "a record not beside its head", false;
            if (x.token == TOK_PLUS && slot_of.count(x.parent) && (slot_of[x.parent] ^ 1u) == (s ^ 1u)) return why = "a record beside a '+' child that lies beside its parent", false;
            const uint32_t rt[TAIL_K] = {r.hash_begin, r.hash_count, r.node, r.lit_bloom};
            uint32_t node = x.node, k = 0;
            for (; k < TAIL_K; k++) {
                if (n_kids[node] != 1) return why = "a chain node without exactly one child", false;
                const TrieSlot& ch = h.trie[t.base + kid[node]];
                if (ch.token != rt[k]) return why = "a record token that is not the chain's", false;
                node = ch.node;
                if (n_kids[node] == 0) break;
                if (ch.own_count || ch.hash_count) return why = "routes above the leaf of a record", false;
            }
            if (k == TAIL_K) return why = "a chain longer than TAIL_K", false;
            for (uint32_t j = k + 1; j < TAIL_K; j++)
                if (rt[j] != NONE) return why = "a record token behind the leaf", false;
            const TrieSlot& leaf = h.trie[t.base + slot_of[node]];
            const bool hash = (r.own_count & TAIL_HASH) != 0;
            if ((leaf.own_count != 0) == (leaf.hash_count != 0)) return why = "a record on a leaf with both kinds of routes (or none)", false;
            if (hash ? (leaf.hash_begin != r.own_begin || leaf.hash_count != (r.own_count & ~TAIL_HASH))
                     : (leaf.own_begin != r.own_begin || leaf.own_count != r.own_count))
                return why = "a record payload that is not its leaf's", false;
        }
        for (const auto& [node, s] : slot_of) // heads that could have a record
            if (n_kids[node] == 1 && h.trie[t.base + (s ^ 1u)].parent == NONE) c.heads++;
    }
    return true;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 12;
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    const char* words[] = {"a", "b", "c", "d", "e", "f", "g", "h"};
    auto rand_filter = [&]() {
        std::string f;
        const size_t depth = 1 + rnd(7);
        for (size_t l = 0; l < depth; l++) {
            f += l ? "/" : "";
            f += rnd(8) == 0 ? "+" : words[rnd(l < 2 ? 3 : 8)];
        }
        if (rnd(6) == 0) f += "/#";
        return f;
    };
    auto key = [&](const std::string& tn, const std::string& f, uint32_t rcv) { return encode_route_key(tn, f, 1, "0" + std::string("\0", 1) + "r" + std::to_string(rcv) + std::string("\0d", 2)); };
    auto pack = [](const std::vector<std::string>& ks, std::vector<uint8_t>& b, std::vector<uint32_t>& o) {
        b.clear(), o.assign(1, 0);
        for (auto& k : ks) b.insert(b.end(), k.begin(), k.end()), o.push_back((uint32_t)b.size());
        b.resize(b.size() + 16, 0);
    };
    uint64_t records = 0, tombs = 0, applies = 0, checks = 0;
    for (int round = 0; round < rounds; round++) {
        HostExec hx;
        hx.threads = 2;
        DistIndex<HostExec> h(hx);
        h.tiny = round % 2 == 1; // minimal capacities: regions grow during the applies below
        const bool off = round % 4 == 3;
        h.tail_records = !off;
        std::set<std::string> model;
        std::vector<std::string> filters;
        for (size_t i = 0, n = 200 + rnd(3000); i < n; i++) {
            const std::string tn = "t" + std::to_string(rnd(3)), f = rand_filter();
            filters.push_back(f);
            model.insert(key(tn, f, (uint32_t)rnd(3)));
        }
        std::vector<uint8_t> b;
        std::vector<uint32_t> o;
        pack(std::vector<std::string>(model.begin(), model.end()), b, o);
        if (!h.rebuild(b.data(), o.data(), (uint32_t)model.size())) return fprintf(stderr, "rebuild: %s\n", h.error.c_str()), 1;
        for (int step = 0; step < 6; step++) {
            Census c;
            std::string why;
            checks++;
            if (!check_image(h, c, why)) return fprintf(stderr, "round %d step %d: %s\n", round, step, why.c_str()), 1;
            if (off && c.records) return fprintf(stderr, "round %d: records with tail_records off\n", round), 1;
            if (!off && step == 0 && c.records == 0) return fprintf(stderr, "round %d: no records after a rebuild (%llu heads)\n", round, (unsigned long long)c.heads), 1;
            records += c.records, tombs += c.tombs;
            if (step == 5) break;
            if (step == 3) { // a compaction: a new generation, records formed again
                if (!h.compact()) return fprintf(stderr, "compact: %s\n", h.error.c_str()), 1;
                continue;
            }
            // deletes, puts of new receivers on existing filters (id lists), puts of filters that extend existing ones (a new child inside a tail)
            std::vector<std::string> ks;
            std::vector<uint8_t> ops;
            for (size_t i = 0, n = 1 + rnd(60); i < n; i++) {
                const std::string tn = "t" + std::to_string(rnd(3));
                const std::string& f = filters[rnd(filters.size())];
                const int kind = (int)rnd(3);
                if (kind == 0 && !model.empty()) {
                    auto it = model.begin();
                    std::advance(it, rnd(model.size()));
                    ks.push_back(*it), ops.push_back(1);
                } else if (kind == 1) ks.push_back(key(tn, f, 3 + (uint32_t)rnd(1000))), ops.push_back(0);
                else if (f.back() != '#') ks.push_back(key(tn, f + "/" + words[rnd(8)], (uint32_t)rnd(3))), ops.push_back(0);
            }
            pack(ks, b, o);
            if (!h.apply(b.data(), o.data(), ops.data(), (uint32_t)ks.size())) return fprintf(stderr, "apply: %s\n", h.error.c_str()), 1;
            applies++;
            for (size_t i = 0; i < ks.size(); i++) ops[i] ? (void)model.erase(ks[i]) : (void)model.insert(ks[i]);
        }
    }
    if (tombs == 0) return fprintf(stderr, "no apply batch left a tombstone\n"), 1;
    printf("tail check ok: %d rounds, %llu images checked, %llu records, %llu tombstones, %llu apply batches\n", rounds, (unsigned long long)checks,
           (unsigned long long)records, (unsigned long long)tombs, (unsigned long long)applies);
    return 0;
}
