// rplan_emu.cpp -- host-side logic test of the kernels of the retain plan (bifromq_amd/csrc/bmq_rplan_kernels.h: k_rp_find, k_rp_group,
// k_rp_classify, k_rp_key_write) under the wave64 emulator of wave_emu.h.  Test tooling.  The kernels run on indexes the product's own host
// code makes (RetainIndexHost bulk load, then RetainDyn<HostExec> batches: adds, removes, re-adds) and are compared with the rule written
// plainly below: a map for the last op of every (tenant bytes, topic bytes), the live set for `present`, the codec's retain_message_key.  A
// serial exclusive sum stands where the device runs hipCUB's scan.
//
// What the cases hold: bulk-loaded topics live and removed, overlay topics live and removed, interior nodes of both parts, levels below
// leaves, unknown levels and tenants, the empty tenant id, empty levels, '$' levels, multi-byte and broken UTF-8, 40 levels, a 255-byte level;
// [retain, clear] and [clear, retain] on present and absent topics, one topic 64 times in one wave, once in each of three waves, under two
// tenants, one tenant's bytes at two table indices; two different keys with the same 32-bit hash (found by search); batch sizes that end
// at, before and behind a wave.  Every batch runs with the group table at its regular size and at its minimum (a power of two >= n: nearly
// full).  The lanes of the emulator run one after the other, so no CAS is ever lost by itself: the harness loses some on purpose -- in front of
// a lane's CAS on an empty slot, a later op with the same key claims it (the state a real interleaving leaves: that op probes the same run
// and finds itself there).  Guard bytes follow every output array.  The run ends with one `rplan emu ok:` line of coverage counts and fails
// (`coverage:`) below their floors.  tests/test_retain_plan_emu.py keeps the harness honest with a table of single-line mutants.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/rplan_emu.cpp bifromq_amd/csrc/bmq_retain.cpp bifromq_amd/csrc/bmq_codec.cpp
//       -o build/rplan_emu -pthread && build/rplan_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <functional>
#include <map>
#include <random>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "bmq_codec.h"
#include "bmq_retain_core.h"

// every atom_cas of bmq_rplan_core.h goes through the harness: a CAS on a slot of the group table may be lost on purpose
namespace bmq {
struct CasHook {
    uint32_t* table = nullptr;
    size_t slots = 0;
    std::function<void(uint32_t* slot, uint32_t desired)> before;
};
inline CasHook& cas_hook() {
    static CasHook h;
    return h;
}
template <class T> inline T rp_emu_cas(T* p, T expect, T desired) {
    if constexpr (std::is_same<T, uint32_t>::value) {
        CasHook& h = cas_hook();
        if (h.before && p >= h.table && p < h.table + h.slots) h.before(p, desired);
    }
    return atom_cas(p, expect, desired);
}
} // namespace bmq
#define atom_cas rp_emu_cas
#include "bmq_rplan_core.h"
#undef atom_cas
#include "bmq_exec_host.h"
#include "bmq_retain_dyn.h"
#include "bmq_rplan_kernels.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static std::map<std::string, unsigned long long> g_cov;
static void hit(const char* what, unsigned long long n = 1) { g_cov[what] += n; }

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
    void add(uint32_t t, const std::string& p, int c) { ot.push_back(t), topics.push_back(p), clear.push_back((uint8_t)c); }
};

constexpr uint8_t GUARD = 0xC7;
constexpr size_t GUARD_N = 32;
template <class T> static std::vector<T> guarded(size_t n) {
    std::vector<T> v(n + GUARD_N);
    memset(v.data(), GUARD, v.size() * sizeof(T));
    return v;
}
template <class T> static bool guard_intact(const std::vector<T>& v, size_t n) {
    const uint8_t* p = (const uint8_t*)(v.data() + n);
    for (size_t k = 0; k < GUARD_N * sizeof(T); k++)
        if (p[k] != GUARD) return false;
    return true;
}

// the kernels as DevExec::rp_plan / rp_key_write launch them, workgroups last to first (ascending: first to last, lane after lane in op order)
static void launch(unsigned long long lanes, uint32_t block, const std::function<void()>& kernel, bool ascending = false) {
    const uint32_t blocks = (uint32_t)((lanes + block - 1) / block), waves = block / 64;
    wemu::grid_size() = blocks;
    for (uint32_t k = 0; k < blocks * waves; k++) {
        const uint32_t at = ascending ? k : blocks * waves - 1 - k;
        wemu::run_wave(at / waves, kernel, at % waves);
    }
}

static int run_plan(Index& ix, const Batch& b, bool min_table, std::mt19937_64& rng, const char* what) {
    const uint32_t n = (uint32_t)b.topics.size(), nt = (uint32_t)b.tenants.size();
    std::string tb, pb;
    std::vector<uint32_t> toff{0}, poff{0};
    for (auto& t : b.tenants) tb += t, toff.push_back((uint32_t)tb.size());
    for (auto& p : b.topics) pb += p, poff.push_back((uint32_t)pb.size());
    tb.append(16, '\0'), pb.append(16, '\0');
    // ---- the rule ----
    std::map<Key, uint32_t> last;
    std::map<Key, std::vector<uint32_t>> members;
    for (uint32_t i = 0; i < n; i++) last[{b.tenants[b.ot[i]], b.topics[i]}] = i, members[{b.tenants[b.ot[i]], b.topics[i]}].push_back(i);
    std::vector<uint8_t> w_code(n), w_action(n);
    std::vector<uint32_t> w_winner(n), w_id(n), next_dup(n, NONE);
    std::vector<int32_t> w_delta(nt, 0);
    std::vector<std::string> w_key(n);
    uint32_t w_by[5] = {0, 0, 0, 0, 0};
    for (auto& kv : members)
        for (size_t k = 0; k + 1 < kv.second.size(); k++) next_dup[kv.second[k]] = kv.second[k + 1];
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
        if (a == RP_REMOVE && b.ot[i] != b.ot[members[k][0]]) hit("a REMOVE filed under another table index than the group's first op");
        if (!present && ix.ever.count(k)) hit(ix.ever[k] < ix.h.n_topics ? "lookups of a removed bulk-loaded topic" : "lookups of a removed overlay topic");
        if (present) hit(it->second < ix.h.n_topics ? "lookups of a live bulk-loaded topic" : "lookups of a live overlay topic");
        hit(a == RP_NONE ? "NONE" : a == RP_ADD ? "ADD" : a == RP_UPDATE ? "UPDATE" : a == RP_REMOVE ? "REMOVE" : "SUPERSEDED");
    }
    // ---- the kernels ----
    uint32_t slots = 8;
    while (slots < (min_table ? n : 2 * n)) slots *= 2;
    if (min_table) {
        slots = 1;
        while (slots < n) slots *= 2;
        hit("plans with the minimum group table");
        if (last.size() * 10 >= (size_t)slots * 9) hit("group tables at least 90 % full");
    }
    auto table = guarded<uint32_t>(slots), rep_of = guarded<uint32_t>(n), lastv = guarded<uint32_t>(n), found = guarded<uint32_t>(n), winner = guarded<uint32_t>(n), ctr = guarded<uint32_t>(RP_C_N);
    auto code = guarded<uint8_t>(n), action = guarded<uint8_t>(n);
    auto delta = guarded<int32_t>(nt);
    auto key_len = guarded<unsigned long long>(n + 1), offs = guarded<unsigned long long>(n + 1);
    memset(table.data(), 0, 4 * (size_t)slots), memset(lastv.data(), 0, 4 * (size_t)n), memset(delta.data(), 0, 4 * (size_t)nt), memset(ctr.data(), 0, 4 * RP_C_N);
    RplanBatch B{};
    B.tenants = (const uint8_t*)tb.data(), B.tenant_off = toff.data(), B.n_tenants = nt, B.op_tenant = b.ot.data();
    B.topics = (const uint8_t*)pb.data(), B.topic_off = poff.data(), B.clear = b.clear.data(), B.n = n;
    B.table = table.data(), B.table_mask = slots - 1, B.rep_of = rep_of.data(), B.last = lastv.data(), B.found = found.data();
    B.code = code.data(), B.action = action.data(), B.winner = winner.data(), B.delta = delta.data(), B.key_len = key_len.data(), B.ctr = ctr.data();
    const RetainMut m = ix.rt.mut_view();
    const RetainDynInfo before = ix.rt.info;
    launch(n, 64, [&]() { k_rp_find(m, B, 1u); });
    // a lost CAS: half of the plans run the grouping in op order (the others last workgroup first, without losses), so that every later op
    // of a lane's key is known not to have run yet -- one of them may claim the slot between the lane's load and its CAS
    const bool lose = rng() % 2 == 0;
    unsigned long long lost = 0;
    cas_hook().table = table.data(), cas_hook().slots = slots;
    if (lose)
        cas_hook().before = [&](uint32_t* slot, uint32_t desired) {
            for (uint32_t j = next_dup[desired - 1u]; j != NONE; j = next_dup[j])
                if (*slot == 0 && rng() % 2 == 0) {
                    *slot = j + 1u;
                    lost++;
                    return;
                }
        };
    launch(n, RPK, [&]() { k_rp_group(B, B.table_mask); }, lose);
    cas_hook().before = nullptr;
    hit("CAS lost to a later op of the same key", lost);
    launch((unsigned long long)n + 1, RPK, [&]() { k_rp_classify(B); });
    unsigned long long run = 0;
    for (uint32_t i = 0; i <= n; i++) offs[i] = run, run += key_len[i];
    auto keys = guarded<uint8_t>((size_t)offs[n]);
    launch(n, RPK, [&]() { k_rp_key_write(B, offs.data(), keys.data()); });
    // ---- compare ----
    if (ctr[RP_C_ERR]) FAIL("%s: count: error bits %#x\n", what, ctr[RP_C_ERR]);
    for (uint32_t a = 0; a < 4; a++)
        if (ctr[RP_C_ACTION + a] != w_by[a]) FAIL("%s: count: %u winners with action %u, expected %u\n", what, ctr[RP_C_ACTION + a], a, w_by[a]);
    for (uint32_t i = 0; i < n; i++) {
        if (code[i] != w_code[i] || action[i] != w_action[i] || winner[i] != w_winner[i] || found[i] != w_id[i])
            FAIL("%s: op %u (%s | %s): code %u action %u winner %u id %u, expected %u %u %u %u\n", what, i, b.tenants[b.ot[i]].c_str(), b.topics[i].c_str(), code[i], action[i], winner[i],
                 found[i], w_code[i], w_action[i], w_winner[i], w_id[i]);
        if (offs[i + 1] - offs[i] != w_key[i].size() || memcmp(keys.data() + offs[i], w_key[i].data(), w_key[i].size()) != 0)
            FAIL("%s: op %u (%s | %s): key of %llu bytes differs from the codec's %zu\n", what, i, b.tenants[b.ot[i]].c_str(), b.topics[i].c_str(), offs[i + 1] - offs[i], w_key[i].size());
    }
    for (uint32_t t = 0; t < nt; t++)
        if (delta[t] != w_delta[t]) FAIL("%s: delta of table entry %u is %d, expected %d\n", what, t, delta[t], w_delta[t]);
    if (!guard_intact(table, slots) || !guard_intact(rep_of, n) || !guard_intact(lastv, n) || !guard_intact(found, n) || !guard_intact(winner, n) || !guard_intact(ctr, RP_C_N) ||
        !guard_intact(code, n) || !guard_intact(action, n) || !guard_intact(delta, nt) || !guard_intact(key_len, (size_t)n + 1) || !guard_intact(keys, (size_t)offs[n]))
        FAIL("%s: guard bytes behind an output array were written\n", what);
    const RetainDynInfo& after = ix.rt.info;
    if (after.n_live != before.n_live || after.id_bound != before.id_bound || after.overlay_nodes != before.overlay_nodes) FAIL("%s: the plan changed the index\n", what);
    hit("plans"), hit("ops", n);
    if (n % 64) hit("batches that end inside a wave");
    return 0;
}

// two different topics with the same rp_hash under tenant `t` (a birthday search through the product's own hash)
static int colliding_topics(const std::string& t, std::string& a, std::string& c) {
    const uint32_t n = 400000;
    std::string tb = t, pb;
    std::vector<uint32_t> toff{0, (uint32_t)t.size()}, poff{0};
    std::mt19937_64 gen(99);
    std::vector<std::string> names;
    for (uint32_t i = 0; i < n; i++) {
        names.push_back("col/" + std::to_string(gen() % 1000000007ull * (i + 1)) + "/" + std::to_string(i));
        pb += names.back(), poff.push_back((uint32_t)pb.size());
    }
    RplanBatch B{};
    B.tenants = (const uint8_t*)tb.data(), B.tenant_off = toff.data(), B.n_tenants = 1, B.topics = (const uint8_t*)pb.data(), B.topic_off = poff.data(), B.n = n;
    std::unordered_map<uint32_t, uint32_t> seen;
    for (uint32_t i = 0; i < n; i++) {
        auto r = seen.emplace(rp_hash(B, i), i);
        if (!r.second) {
            a = names[r.first->second], c = names[i];
            return 0;
        }
    }
    FAIL("coverage: no two of %u topics share a hash\n", n);
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 3;
    const unsigned long long seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345;
    std::mt19937_64 rng(seed);
    auto rnd = [&](size_t m) { return (size_t)(rng() % m); };
    std::string col_a, col_b;
    if (colliding_topics("t", col_a, col_b)) return 1;
    const std::vector<std::string> special = {"/", "a/", "/a", "a//b", "$sys/x", "\xC3\xA9/x", "x/\xE4\xBD\xA0\xE5\xA5\xBD/y", "\xF0\x9F\x98\x84", "cut/\xE4\xBD", "\xF0\x9F\x98/z", "\xC3",
                                              "lone/\xA0\xA0/x", std::string(255, 't')};
    std::string forty;
    for (int i = 0; i < 40; i++) forty += (i ? "/l" : "l") + std::to_string(i);
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "0", "x"};
    auto rand_topic = [&]() {
        std::string t;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) t += (i ? "/" : "") + alpha[rnd(alpha.size())];
        return t;
    };
    for (int round = 0; round < rounds; round++) {
        Index ix;
        ix.hx.threads = 1;
        ix.rt.tiny = round % 2 == 1;
        std::set<Key> bulk;
        for (size_t i = 0; i < 200; i++) bulk.insert({rnd(2) ? "t" : "u", rand_topic()});
        bulk.insert({"t", "p/q/r"}), bulk.insert({"", "a/b"}), bulk.insert({"t", "gone/bulk"}), bulk.insert({"t", "s/1"}), bulk.insert({"u", "s/1"});
        for (size_t k = 0; k < special.size(); k += 2) bulk.insert({"sp", special[k]});
        std::vector<RetainIndexHost::Item> items;
        for (auto& k : bulk) {
            RetainIndexHost::Item it;
            it.tenant = k.first, it.topic = k.second;
            items.push_back(std::move(it));
        }
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
        for (size_t i = 0; i < 150; i++) b1[{rnd(3) ? "t" : "ov", rand_topic() + (rnd(2) ? "/n" : "")}] = 0;
        b1[{"ov", "p/q/r"}] = 0, b1[{"ov", "gone/overlay"}] = 0, b1[{"ov", forty}] = 0, b1[{"ov", "gone/deep/er"}] = 0;
        for (size_t k = 1; k < special.size(); k += 4) b1[{"sp", special[k]}] = 0;
        if (ix.apply({b1.begin(), b1.end()})) return 1;
        for (auto& kv : ix.live)
            if (rnd(4) == 0 && kv.first.second != "p/q/r" && kv.first.second != "s/1" && kv.first.first != "sp" && kv.first.first != "") b2[kv.first] = 1;
        b2[{"t", "gone/bulk"}] = 1, b2[{"ov", "gone/overlay"}] = 1, b2[{"ov", "gone/deep/er"}] = 1;
        if (ix.apply({b2.begin(), b2.end()})) return 1;
        for (auto& kv : b2)
            if (rnd(4) == 0 && kv.first.second.rfind("gone/", 0) != 0) b3[kv.first] = 0;
        if (ix.apply({b3.begin(), b3.end()})) return 1;
        std::vector<Key> pool;
        for (auto& kv : ix.ever) pool.push_back(kv.first);
        const std::vector<std::string> table = {"t", "u", "ov", "", "nobody", "t", "sp"}; // "t" twice: entries 0 and 5
        auto index_of = [&](const std::string& t) {
            if (t == "t") return rnd(2) ? 0u : 5u;
            for (uint32_t k = 1; k < table.size(); k++)
                if (table[k] == t) return k;
            return 4u;
        };
        // ---- the directed batch ----
        {
            Batch b;
            b.tenants = table;
            b.add(0, "p/q/r", 0), b.add(0, "p/q/r", 1);               // present: retain, clear
            b.add(0, "dup/absent-1", 0), b.add(0, "dup/absent-1", 1); // absent: retain, clear
            b.add(2, "p/q/r", 1), b.add(2, "p/q/r", 0);               // present: clear, retain
            b.add(2, "dup/absent-2", 1), b.add(2, "dup/absent-2", 0); // absent: clear, retain
            b.add(0, "s/1", 0), b.add(1, "s/1", 1), b.add(4, "s/1", 0); // one topic, three tenants
            b.add(0, "p/q", 0), b.add(2, "p/q", 1), b.add(0, "p/q/r/s", 0), b.add(2, "p/q/r/s", 1); // interior nodes, levels below leaves
            b.add(0, "gone/bulk", 0), b.add(2, "gone/overlay", 1), b.add(2, "gone/deep", 0), b.add(0, "p/never-seen", 0), b.add(3, "a/b", 1), b.add(3, "a", 0);
            b.add(0, "s/1", 0), b.add(5, "s/1", 1);                   // one tenant at two table indices: one group, REMOVE under entry 5 -- the third op of the group
            b.add(5, "two/idx", 1), b.add(0, "two/idx", 0);
            b.add(0, col_a, 0), b.add(0, col_b, 1);                   // the same hash, different bytes
            for (auto& s : special) b.add(6, s, rnd(2));
            b.add(6, forty, 0), b.add(2, forty, 1);
            while (b.topics.size() % 64) b.add(1, "fill/" + std::to_string(b.topics.size()), rnd(3) == 0);
            for (int k = 0; k < 64; k++) b.add(1, "s/1", k == 63 ? 0 : k % 2); // 64 times in one wave
            for (int w = 0; w < 3; w++) {
                for (int k = 0; k < 64; k++) b.add(1, "fill/" + std::to_string(b.topics.size()), rnd(3) == 0);
                b.topics[b.topics.size() - 59] = "p/q/r", b.ot[b.ot.size() - 59] = 0, b.clear[b.clear.size() - 59] = w < 2; // once per wave
            }
            b.add(1, "tail", 0);
            hit("hash collisions between different keys");
            for (bool mt : {false, true})
                if (run_plan(ix, b, mt, rng, mt ? "directed batch, minimum table" : "directed batch")) return 1;
        }
        // ---- random batches ----
        for (uint32_t n : {1u, 63u, 64u, 65u, 257u, 2000u}) {
            for (int shape = 0; shape < 3; shape++) { // 0: mixed, 1: a few keys many times, 2: one topic under every tenant (equal topics, different tenants)
                Batch b;
                b.tenants = table;
                std::vector<Key> few;
                for (size_t k = 0; k < 1 + rnd(30); k++) few.push_back(pool[rnd(pool.size())]);
                for (uint32_t i = 0; i < n; i++) {
                    Key k;
                    const size_t r = rnd(10);
                    if (shape == 1) k = few[rnd(few.size())];
                    else if (shape == 2) k = {table[rnd(table.size())], "same/" + std::to_string(rnd(n / 6 + 1))};
                    else if (r < 5) k = pool[rnd(pool.size())];
                    else if (r < 6) k = {pool[rnd(pool.size())].first, pool[rnd(pool.size())].second + (rnd(2) ? "/below" : "x")};
                    else if (r < 7) k = {"nobody", rand_topic()};
                    else if (r < 8) {
                        k = pool[rnd(pool.size())];
                        const size_t cut = k.second.rfind('/');
                        if (cut != std::string::npos) k.second.resize(cut);
                    } else k = {rnd(2) ? "t" : "ov", "fresh/" + std::to_string(rng() % (n / 2 + 1))};
                    b.add(index_of(k.first), k.second, rnd(3) == 0);
                }
                for (bool mt : {false, true}) {
                    const std::string what = "round " + std::to_string(round) + ", " + std::to_string(n) + " ops, shape " + std::to_string(shape) + (mt ? ", minimum table" : "");
                    if (run_plan(ix, b, mt, rng, what.c_str())) return 1;
                }
            }
        }
    }
    const std::pair<const char*, unsigned long long> floors[] = {
        {"plans", 30}, {"ops", 10000}, {"NONE", 50}, {"ADD", 50}, {"UPDATE", 50}, {"REMOVE", 50}, {"SUPERSEDED", 500}, {"lookups of a live bulk-loaded topic", 100},
        {"lookups of a removed bulk-loaded topic", 20}, {"lookups of a live overlay topic", 100}, {"lookups of a removed overlay topic", 20}, {"plans with the minimum group table", 15},
        {"group tables at least 90 % full", 1}, {"CAS lost to a later op of the same key", 50}, {"batches that end inside a wave", 10}, {"hash collisions between different keys", 1},
        {"a REMOVE filed under another table index than the group's first op", 1}};
    std::string line;
    for (auto& f : floors) {
        if (g_cov[f.first] < f.second) FAIL("coverage: %s: %llu, at least %llu expected\n", f.first, g_cov[f.first], f.second);
        line += std::string(line.empty() ? "" : ", ") + f.first + " " + std::to_string(g_cov[f.first]);
    }
    printf("rplan emu ok: %s\n", line.c_str());
    return 0;
}
