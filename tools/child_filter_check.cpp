// tools/child_filter_check.cpp -- checks the child filter words of the filter trie (bmq_layout.h: the begin word of a node's empty range) on indexes the
// product's own builder makes on the host executor.  The one thing the walk relies on: a word never lacks the bit of a literal child (no false negative).
// In order, per round: a rebuild; apply batches that add children below route-less nodes; batches that attach the first route (own and '#') to such
// nodes; batches that remove those routes again (the words become all-ones); batches that put and delete one key in the same batch beside new children
// of its node; more puts until regions have grown (odd rounds run with minimal capacities: every growth path); a compaction.  After each step every node
// with an empty range must have, in that word, the bit of each of its literal children.  After a rebuild and after a compaction -- both run every key
// through locate -- the words must be EXACT (the OR of the children's bits, never all-ones).  Prints "child filter check ok: ..."
// (tests/test_child_filters.py).
//     g++ -O1 -std=c++17 -pthread -I bifromq_amd/csrc tools/child_filter_check.cpp bifromq_amd/csrc/bmq_codec.cpp -o /tmp/child_filter_check && /tmp/child_filter_check [rounds] [seed]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
    uint64_t nodes = 0, words = 0, pairs = 0, none_words = 0, buckets = 0;
};
// false + message: a word that lacks a child's bit (or, exact: one that is not the OR of its children's bits)
static bool check_image(DistIndex<HostExec>& h, bool exact, Census& c, std::string& why) {
    for (uint32_t d = 0; d < h.dir_slots; d++) {
        const TenantSlot& t = h.dir[d];
        if (!(t.hash_lo | t.hash_hi)) continue;
        c.buckets += t.buckets;
        std::unordered_map<uint32_t, uint32_t> want_own, want_hash; // node id -> OR of its literal children's bits
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& e = h.trie[t.base + s];
            if (!slot_is_node(e) || e.token == TOK_PLUS || e.parent == 0) continue;
            want_own[e.parent] |= 1u << filter_bit_own(e.token);
            want_hash[e.parent] |= 1u << filter_bit_hash(e.token);
            c.pairs++;
        }
        for (uint32_t s = 0; s < 2 * t.buckets; s++) {
            const TrieSlot& x = h.trie[t.base + s];
            if (!slot_is_node(x)) continue;
            c.nodes++;
            const uint32_t wo = want_own.count(x.node) ? want_own[x.node] : 0u, wh = want_hash.count(x.node) ? want_hash[x.node] : 0u;
            if (x.own_count == 0) {
                c.words++, c.none_words += x.own_begin == FILTER_NONE;
                if ((x.own_begin & wo) != wo) return why = "own_begin of a node without own routes lacks the bit of a literal child", false;
                if (exact && x.own_begin != wo) return why = x.own_begin == FILTER_NONE ? "an all-ones own_begin word in a fresh image" : "an own_begin word with bits of no child in a fresh image", false;
            }
            if (x.hash_count == 0) {
                c.words++, c.none_words += x.hash_begin == FILTER_NONE;
                if ((x.hash_begin & wh) != wh) return why = "hash_begin of a node without '#' routes lacks the bit of a literal child", false;
                if (exact && x.hash_begin != wh) return why = x.hash_begin == FILTER_NONE ? "an all-ones hash_begin word in a fresh image" : "a hash_begin word with bits of no child in a fresh image", false;
            }
        }
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
        const size_t depth = 1 + rnd(6);
        for (size_t l = 0; l < depth; l++) {
            f += l ? "/" : "";
            f += rnd(8) == 0 ? "+" : words[rnd(l < 2 ? 3 : 8)];
        }
        return f;
    };
    auto key = [&](const std::string& tn, const std::string& f, uint32_t rcv) { return encode_route_key(tn, f, 1, "0" + std::string("\0", 1) + "r" + std::to_string(rcv) + std::string("\0d", 2)); };
    auto pack = [](const std::vector<std::string>& ks, std::vector<uint8_t>& b, std::vector<uint32_t>& o) {
        b.clear(), o.assign(1, 0);
        for (auto& k : ks) b.insert(b.end(), k.begin(), k.end()), o.push_back((uint32_t)b.size());
        b.resize(b.size() + 16, 0);
    };
    uint64_t checks = 0, pairs = 0, words_seen = 0, none_words = 0, applies = 0, growths = 0;
    for (int round = 0; round < rounds; round++) {
        HostExec hx;
        hx.threads = 2;
        DistIndex<HostExec> h(hx);
        h.tiny = round % 2 == 1; // minimal capacities: regions grow during the applies below
        h.tail_records = round % 4 != 2;
        // the model: (tenant, filter) -> receivers.  Routes sit on the LEAVES of random paths and on a few inner nodes: most inner nodes are route-less.
        std::set<std::pair<std::string, std::string>> filters; // every (tenant, filter) that ever had a route: the directed steps pick from its prefixes
        std::set<std::string> model;
        for (size_t i = 0, n = 200 + rnd(2500); i < n; i++) {
            const std::string tn = "t" + std::to_string(rnd(3));
            std::string f = rand_filter();
            if (rnd(7) == 0) f += "/#";
            filters.insert({tn, f});
            model.insert(key(tn, f, (uint32_t)rnd(3)));
        }
        std::vector<uint8_t> b;
        std::vector<uint32_t> o;
        pack(std::vector<std::string>(model.begin(), model.end()), b, o);
        if (!h.rebuild(b.data(), o.data(), (uint32_t)model.size())) return fprintf(stderr, "rebuild: %s\n", h.error.c_str()), 1;
        // a proper prefix of a random filter: a node that exists; most of them hold no route of their own
        auto rand_prefix = [&]() {
            for (;;) {
                auto it = filters.begin();
                std::advance(it, rnd(filters.size()));
                std::string f = it->second;
                if (f.size() >= 2 && f.compare(f.size() - 2, 2, "/#") == 0) f.resize(f.size() - 2);
                std::vector<size_t> cuts;
                for (size_t i = 0; i < f.size(); i++)
                    if (f[i] == '/') cuts.push_back(i);
                if (cuts.empty()) continue;
                return std::make_pair(it->first, f.substr(0, cuts[rnd(cuts.size())]));
            }
        };
        uint64_t buckets_before = 0;
        std::vector<std::string> held; // keys the "first route" step put: the next step deletes them again
        auto run = [&](const std::vector<std::string>& ks, const std::vector<uint8_t>& ops_in) {
            if (ks.empty()) return true;
            std::vector<uint8_t> ops = ops_in;
            pack(ks, b, o);
            if (!h.apply(b.data(), o.data(), ops.data(), (uint32_t)ks.size())) return false;
            applies++;
            for (size_t i = 0; i < ks.size(); i++) ops[i] ? (void)model.erase(ks[i]) : (void)model.insert(ks[i]);
            return true;
        };
        for (int step = 0; step < 8; step++) {
            // the image as the step before left it
            Census c;
            std::string why;
            checks++;
            const bool exact = step == 0 || step == 7; // behind the rebuild / behind the compaction
            if (!check_image(h, exact, c, why)) return fprintf(stderr, "round %d step %d: %s\n", round, step, why.c_str()), 1;
            pairs += c.pairs, words_seen += c.words, none_words += c.none_words;
            if (step == 0) buckets_before = c.buckets;
            if (step == 6 && h.tiny && c.buckets > buckets_before) growths++;
            if (step == 7) break;
            std::vector<std::string> ks;
            std::vector<uint8_t> ops;
            if (step == 0) { // new children below route-less nodes (and below the others: the words of a range with routes stay route ids)
                for (size_t i = 0, n = 20 + rnd(60); i < n; i++) {
                    const auto [tn, p] = rand_prefix();
                    const std::string f = p + "/n" + std::to_string(rnd(40));
                    filters.insert({tn, f});
                    ks.push_back(key(tn, f, (uint32_t)rnd(3))), ops.push_back(0);
                }
            } else if (step == 1) { // the first route of a node, own and '#': its filter word becomes a route id
                held.clear();
                for (size_t i = 0, n = 20 + rnd(40); i < n; i++) {
                    const auto [tn, p] = rand_prefix();
                    const std::string k = key(tn, rnd(2) ? p : p + "/#", 7);
                    if (model.count(k)) continue;
                    held.push_back(k), ks.push_back(k), ops.push_back(0);
                }
            } else if (step == 2) { // ... and its last route leaves again (all-ones), beside deletes of random routes and new children of the same nodes
                for (const auto& k : held)
                    if (model.count(k)) ks.push_back(k), ops.push_back(1);
                for (size_t i = 0, n = rnd(30); i < n && !model.empty(); i++) {
                    auto it = model.begin();
                    std::advance(it, rnd(model.size()));
                    if (std::find(ks.begin(), ks.end(), *it) == ks.end()) ks.push_back(*it), ops.push_back(1);
                }
            } else if (step == 3) { // children below the nodes whose words are all-ones now, and below fresh ones
                for (size_t i = 0, n = 20 + rnd(40); i < n; i++) {
                    const auto [tn, p] = rand_prefix();
                    const std::string f = p + "/m" + std::to_string(rnd(40));
                    filters.insert({tn, f});
                    ks.push_back(key(tn, f, (uint32_t)rnd(3))), ops.push_back(0);
                }
            } else if (step == 4) { // put and delete of one key in ONE batch (the range is empty before and after), new children of that node in the same batch
                for (size_t i = 0, n = 10 + rnd(30); i < n; i++) {
                    const auto [tn, p] = rand_prefix();
                    const std::string k = key(tn, rnd(2) ? p : p + "/#", 900 + (uint32_t)i);
                    if (model.count(k)) continue;
                    const std::string f = p + "/k" + std::to_string(rnd(40));
                    ks.push_back(k), ops.push_back(0);
                    filters.insert({tn, f});
                    ks.push_back(key(tn, f, (uint32_t)rnd(3))), ops.push_back(0);
                    ks.push_back(k), ops.push_back(1);
                }
            } else if (step == 5) { // many new nodes: regions grow (whole slots are re-inserted into the larger region)
                for (size_t i = 0, n = 400 + rnd(800); i < n; i++) {
                    const auto [tn, p] = rand_prefix();
                    const std::string f = p + "/g" + std::to_string(rnd(60)) + "/" + words[rnd(8)];
                    filters.insert({tn, f});
                    ks.push_back(key(tn, f, (uint32_t)rnd(3))), ops.push_back(0);
                }
            } else { // step 6: a compaction: a new generation, every key through locate again
                if (!h.compact()) return fprintf(stderr, "compact: %s\n", h.error.c_str()), 1;
                continue;
            }
            // (one op per key and batch, except the put + delete pairs of step 4)
            if (step != 4) {
                std::set<std::string> seen;
                std::vector<std::string> k2;
                std::vector<uint8_t> o2;
                for (size_t i = 0; i < ks.size(); i++)
                    if (seen.insert(ks[i]).second) k2.push_back(ks[i]), o2.push_back(ops[i]);
                ks.swap(k2), ops.swap(o2);
            }
            if (!run(ks, ops)) return fprintf(stderr, "apply (round %d step %d): %s\n", round, step, h.error.c_str()), 1;
        }
    }
    if (none_words == 0) return fprintf(stderr, "no range lost its last route: the all-ones path never ran\n"), 1;
    if (rounds > 1 && growths == 0) return fprintf(stderr, "no region grew\n"), 1;
    printf("child filter check ok: %d rounds, %llu images checked, %llu (node, literal child) pairs, %llu filter words, %llu of them all-ones, %llu apply batches, %llu rounds with region growth\n",
           rounds, (unsigned long long)checks, (unsigned long long)pairs, (unsigned long long)words_seen, (unsigned long long)none_words, (unsigned long long)applies,
           (unsigned long long)growths);
    return 0;
}
