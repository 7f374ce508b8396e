// retain_plan_check.cpp -- the plan of a batch of retain ops (bifromq_amd/csrc/bmq_rplan_core.h: what the k_rp_* kernels run per lane) over
// HostExec threads, under sanitizers.  Test tooling: a program of its own, nothing preloaded.  An index the product's own host code makes
// (RetainIndexHost bulk load, then RetainDyn<HostExec> batches: adds, removes, re-adds) is planned against with random batches -- retained
// topics, removed ones, interior nodes, levels below leaves, unknown levels and tenants, heavy duplicates (a few keys thousands of times: the
// CAS table of the grouping under contention), one tenant's bytes at two table indices -- with the group table at its regular size and at its
// minimum (a power of two >= n: nearly full, long probe runs), and compared with the rule written plainly here: a map for the last op of every
// (tenant, topic), the live set for `present`, the codec's retain_message_key.  After every plan the index must be as it was.
//   make -C bifromq_amd/csrc rpcheck      (ASan/UBSan and TSan builds; the CAS table on host threads is what TSan is for)
//   tools/retain_plan_check [rounds] [seed] [threads]
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../bifromq_amd/csrc/bmq_codec.h"
#include "../bifromq_amd/csrc/bmq_exec_host.h"
#include "../bifromq_amd/csrc/bmq_retain_dyn.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

using Key = std::pair<std::string, std::string>; // (tenant, topic)

struct Index {
    RetainIndexHost h;
    HostExec hx;
    RetainDyn<HostExec> rt{hx};
    std::map<Key, uint32_t> live, ever;
    int apply(const std::vector<std::pair<Key, uint8_t>>& ops) { // distinct keys per batch
        if (ops.empty()) return 0;
        std::map<std::string, uint32_t> tix;
        std::string tb, pb;
        std::vector<uint32_t> toff{0}, poff{0}, ot, out(ops.size());
        std::vector<uint8_t> op;
        for (auto& o : ops) {
            if (!tix.count(o.first.first)) {
                const uint32_t at = (uint32_t)tix.size();
                tix[o.first.first] = at;
                tb += o.first.first, toff.push_back((uint32_t)tb.size());
            }
            ot.push_back(tix[o.first.first]);
            pb += o.first.second, poff.push_back((uint32_t)pb.size());
            op.push_back(o.second);
        }
        tb.append(16, '\0'), pb.append(16, '\0');
        if (!rt.apply((const uint8_t*)tb.data(), toff.data(), (uint32_t)tix.size(), ot.data(), (const uint8_t*)pb.data(), poff.data(), op.data(), nullptr, nullptr, (uint32_t)ops.size(), out.data()))
            FAIL("apply failed: %s\n", rt.error.c_str());
        for (size_t i = 0; i < ops.size(); i++) {
            if (ops[i].second == 0) {
                if (out[i] == NONE) FAIL("an add reports no id\n");
                ever[ops[i].first] = out[i], live[ops[i].first] = out[i];
            } else live.erase(ops[i].first);
        }
        return 0;
    }
};

struct Batch {
    std::vector<std::string> tenants; // the table: may hold the same bytes twice
    std::vector<uint32_t> ot;
    std::vector<std::string> topics;
    std::vector<uint8_t> clear;
};

static int run_plan(Index& ix, const Batch& b, uint32_t min_table, const char* what) {
    const uint32_t n = (uint32_t)b.topics.size(), nt = (uint32_t)b.tenants.size();
    std::string tb, pb;
    std::vector<uint32_t> toff{0}, poff{0};
    for (auto& t : b.tenants) tb += t, toff.push_back((uint32_t)tb.size());
    for (auto& p : b.topics) pb += p, poff.push_back((uint32_t)pb.size());
    tb.append(16, '\0'), pb.append(16, '\0');
    // the rule
    std::map<Key, uint32_t> last;
    for (uint32_t i = 0; i < n; i++) last[{b.tenants[b.ot[i]], b.topics[i]}] = i;
    std::vector<uint8_t> w_code(n), w_action(n);
    std::vector<uint32_t> w_winner(n), w_id(n);
    std::vector<int32_t> w_delta(nt, 0);
    std::vector<std::string> w_key(n);
    uint64_t w_by[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; i++) {
        const Key k{b.tenants[b.ot[i]], b.topics[i]};
        const uint32_t w = last[k];
        const auto it = ix.live.find(k);
        const bool present = it != ix.live.end(), clear = b.clear[w] != 0;
        w_code[i] = clear ? 1 : 0, w_winner[i] = w, w_id[i] = present ? it->second : NONE;
        uint32_t a = RP_SUPERSEDED;
        if (i == w) a = clear ? (present ? RP_REMOVE : RP_NONE) : (present ? RP_UPDATE : RP_ADD);
        w_action[i] = (uint8_t)a, w_by[a]++;
        if (a == RP_ADD || a == RP_UPDATE || a == RP_REMOVE) w_key[i] = retain_message_key(k.first, k.second);
        if (a == RP_ADD) w_delta[b.ot[i]]++;
        if (a == RP_REMOVE) w_delta[b.ot[i]]--;
    }
    uint64_t w_bytes = 0;
    for (auto& k : w_key) w_bytes += k.size();
    // the product
    std::vector<uint8_t> code(n, 0xEE), action(n, 0xEE), keys(w_bytes + 8, 0xEE);
    std::vector<uint32_t> winner(n, 0xEEEEEEEEu), id(n, 0xEEEEEEEEu);
    std::vector<int32_t> delta(nt, 77);
    std::vector<unsigned long long> koff(n + 1, 0xEEull);
    const RetainDynInfo before = ix.rt.info;
    RetainDyn<HostExec>::PlanOut o{};
    o.code = code.data(), o.action = action.data(), o.winner = winner.data(), o.topic_id = id.data(), o.delta = delta.data();
    o.key_off = koff.data(), o.keys = keys.data(), o.keys_cap = w_bytes;
    if (!ix.rt.plan((const uint8_t*)tb.data(), toff.data(), nt, b.ot.data(), (const uint8_t*)pb.data(), poff.data(), b.clear.data(), n, min_table, o))
        FAIL("%s: plan failed: %s\n", what, ix.rt.error.c_str());
    if (o.nospace || o.key_bytes != w_bytes) FAIL("%s: %llu key bytes, expected %llu\n", what, (unsigned long long)o.key_bytes, (unsigned long long)w_bytes);
    for (uint32_t a = 0; a < 4; a++)
        if (o.by_action[a] != w_by[a]) FAIL("%s: %llu winners with action %u, expected %llu\n", what, (unsigned long long)o.by_action[a], a, (unsigned long long)w_by[a]);
    for (uint32_t i = 0; i < n; i++) {
        if (code[i] != w_code[i] || action[i] != w_action[i] || winner[i] != w_winner[i] || id[i] != w_id[i])
            FAIL("%s: op %u (%s | %s): code %u action %u winner %u id %u, expected %u %u %u %u\n", what, i, b.tenants[b.ot[i]].c_str(), b.topics[i].c_str(), code[i], action[i], winner[i],
                 id[i], w_code[i], w_action[i], w_winner[i], w_id[i]);
        if (std::string((const char*)keys.data() + koff[i], koff[i + 1] - koff[i]) != w_key[i]) FAIL("%s: op %u: key differs\n", what, i);
    }
    if (delta != w_delta) FAIL("%s: the deltas differ\n", what);
    for (size_t k = w_bytes; k < keys.size(); k++)
        if (keys[k] != 0xEE) FAIL("%s: written behind the last key\n", what);
    const RetainDynInfo& after = ix.rt.info;
    if (after.n_live != before.n_live || after.id_bound != before.id_bound || after.overlay_nodes != before.overlay_nodes || after.batches != before.batches)
        FAIL("%s: the plan changed the index\n", what);
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 8;
    const unsigned long long seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const unsigned threads = argc > 3 ? (unsigned)atoi(argv[3]) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](size_t m) { return (size_t)(rng() % m); };
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "\xF0\x9F\x98", "0", "x"};
    auto rand_topic = [&]() {
        std::string t;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) t += (i ? "/" : "") + alpha[rnd(alpha.size())];
        return t;
    };
    unsigned long long plans = 0, ops_total = 0;
    for (int round = 0; round < rounds; round++) {
        Index ix;
        ix.hx.threads = threads;
        ix.rt.tiny = round % 2 == 1;
        std::set<Key> bulk;
        for (size_t i = 0; i < 300; i++) bulk.insert({rnd(2) ? "t" : "u", rand_topic()});
        bulk.insert({"t", "p/q/r"}), bulk.insert({"", "a/b"});
        std::vector<RetainIndexHost::Item> items;
        for (auto& k : bulk) {
            RetainIndexHost::Item it;
            it.tenant = k.first, it.topic = k.second;
            items.push_back(std::move(it));
        }
        if (round % 4 == 3) items.clear(); // an empty bulk load: everything lives in the overlay
        if (!ix.h.rebuild(std::move(items))) FAIL("round %d: rebuild failed: %s\n", round, ix.h.error.c_str());
        RetainIndexView v{};
        v.nodes = ix.h.nodes.data(), v.edges = ix.h.edges.data(), v.posts = ix.h.posts.data(), v.gps = ix.h.gps.data(), v.tenants = ix.h.tenants.data();
        v.tenant_mask = (uint32_t)ix.h.tenants.size() - 1;
        v.dict = ix.h.dict.data(), v.dict_group_mask = (uint32_t)ix.h.dict.size() / DICT_GROUP - 1, v.pool = ix.h.pool.data();
        if (!ix.rt.reset(v, ix.h)) FAIL("round %d: reset failed: %s\n", round, ix.rt.error.c_str());
        for (uint32_t id = 0; id < ix.h.n_topics; id++) {
            std::string_view tn, tp;
            if (!ix.h.topic(id, tn, tp)) FAIL("round %d: topic(%u)\n", round, id);
            ix.live[{std::string(tn), std::string(tp)}] = id, ix.ever[{std::string(tn), std::string(tp)}] = id;
        }
        std::map<Key, uint8_t> b1, b2, b3;
        for (size_t i = 0; i < 200; i++) b1[{rnd(3) ? "t" : "ov", rand_topic() + (rnd(2) ? "/n" : "")}] = 0;
        b1[{"ov", "p/q/r"}] = 0;
        if (ix.apply({b1.begin(), b1.end()})) return 1;
        for (auto& kv : ix.live)
            if (rnd(4) == 0 && kv.first.second != "p/q/r") b2[kv.first] = 1;
        if (ix.apply({b2.begin(), b2.end()})) return 1;
        for (auto& kv : b2)
            if (rnd(4) == 0) b3[kv.first] = 0;
        if (ix.apply({b3.begin(), b3.end()})) return 1;
        std::vector<Key> pool;
        for (auto& kv : ix.ever) pool.push_back(kv.first);
        for (uint32_t n : {1u, 63u, 64u, 65u, 257u, 4000u, 20000u}) {
            for (int shape = 0; shape < 2; shape++) { // 0: mixed, 1: a few keys many times
                Batch b;
                b.tenants = {"t", "u", "ov", "", "nobody", "t"}; // "t" twice
                auto tenant_index = [&](const std::string& t) {
                    if (t == "t") return rnd(2) ? 0u : 5u;
                    for (uint32_t k = 1; k < 5; k++)
                        if (b.tenants[k] == t) return k;
                    return 4u;
                };
                std::vector<Key> few;
                for (size_t k = 0; k < 1 + rnd(40); k++) few.push_back(pool[rnd(pool.size())]);
                for (uint32_t i = 0; i < n; i++) {
                    Key k;
                    const size_t r = rnd(10);
                    if (shape == 1) k = few[rnd(few.size())];
                    else if (r < 5) k = pool[rnd(pool.size())];
                    else if (r < 6) k = {pool[rnd(pool.size())].first, pool[rnd(pool.size())].second + (rnd(2) ? "/below" : "x")};
                    else if (r < 7) k = {"nobody", rand_topic()};
                    else if (r < 8) {
                        k = pool[rnd(pool.size())];
                        const size_t cut = k.second.rfind('/');
                        if (cut != std::string::npos) k.second.resize(cut); // an interior node, often
                    } else k = {rnd(2) ? "t" : "ov", "fresh/" + std::to_string(rng() % (n / 2 + 1))};
                    const uint32_t ti = tenant_index(k.first);
                    b.ot.push_back(ti), b.topics.push_back(k.second), b.clear.push_back(rnd(3) == 0);
                }
                for (uint32_t min_table : {0u, 1u}) {
                    const std::string what = "round " + std::to_string(round) + ", " + std::to_string(n) + " ops, shape " + std::to_string(shape) + (min_table ? ", minimum table" : "");
                    if (run_plan(ix, b, min_table, what.c_str())) return 1;
                    plans++, ops_total += n;
                }
            }
        }
    }
    printf("retain_plan_check ok: %d rounds, %llu plans, %llu ops, %u threads\n", rounds, plans, ops_total, threads);
    return 0;
}
