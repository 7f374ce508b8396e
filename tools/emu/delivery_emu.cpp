// delivery_emu.cpp -- host-side logic test of the kernels of the delivery plan (bifromq_amd/csrc/bmq_delivery_kernels.h: k_dl_scatter,
// k_dl_map, k_dl_assign, k_dl_count, k_dl_merge) under the wave64 emulator of wave_emu.h.  Test tooling: the kernels' LOGIC -- the probe
// of the group table with the bytes of a share-deliverer number, the slot -> group scatter, the byte verify, the dense numbers of the
// groups reached through members only, the sizes and bases of the final groups, the group of a row from the offsets and its rank in the
// other list -- against a stable merge by key BYTES written plainly below.  A serial inclusive sum stands where the device runs hipCUB's
// scan.  The harness builds what the two steps before leave behind (the pairs by group, the member rows by share-deliverer number) and the
// state they leave it in (group table, per-route cache, key bytes of the routes) directly: no index, no grouping, no resolve runs here.
//
// What the cases hold: deliverer keys known to the table and in the batch, known and absent from it, unknown; a share-deliverer number whose
// 64-bit hash was PLANTED in the slot of another key (what a hash collision looks like to the probe: only the byte compare tells); keys
// whose bytes concatenate alike ("1" + "2x", "12" + "x"); lists of 1, 63, 64, 65, 255, 256, 257 and 1025 rows, so that a group's lists end at,
// before and behind a wave and a workgroup; the unresolved and the dead group, each present and absent; batches without shared pairs and
// of shared pairs only.  Workgroups run last to first.  Guard words follow every output array.  The run ends with an `ok` line of coverage
// counts and fails below their floors.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/delivery_emu.cpp -o build/delivery_emu && build/delivery_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <map>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "bmq_delivery_kernels.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static const uint32_t GUARD = 16, GUARD_WORD = 0xC0DEC0DEu;
static std::vector<uint32_t> guarded(size_t n, uint32_t fill) {
    std::vector<uint32_t> v(n + GUARD, fill);
    for (size_t i = n; i < n + GUARD; i++) v[i] = GUARD_WORD;
    return v;
}
static bool guard_intact(const std::vector<uint32_t>& v) {
    for (size_t i = v.size() - GUARD; i < v.size(); i++)
        if (v[i] != GUARD_WORD) return false;
    return true;
}

struct Coverage {
    uint64_t cases = 0, rows = 0, merged = 0, share_only = 0, planted = 0, absent = 0, unresolved = 0, dead = 0, lists_over_block = 0, lists_at_wave = 0, no_shared = 0,
             only_shared = 0, share_heavier = 0;
};

template <class K> static void launch(uint32_t n, K&& kernel) { // grid(n, DL_BLOCK) workgroups of DL_BLOCK / 64 independent waves, last to first
    const uint32_t blocks = (n + DL_BLOCK - 1) / DL_BLOCK;
    for (uint32_t b = blocks; b-- > 0;)
        for (uint32_t w = DL_BLOCK / 64; w-- > 0;) wemu::run_wave(b, kernel, w);
}

struct Key {
    std::string sub, dk;
    std::string bytes() const { return sub + std::string("\0", 1) + dk; }
};

static int one_case(std::mt19937_64& rng, uint32_t shape, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const uint32_t sizes[10] = {1, 2, 63, 64, 65, 255, 256, 257, 1025, 7};
    // ---- deliverer keys: [0, n_table) are known to the group table, the first n_batch of them have pairs in this batch
    const uint32_t n_table = 3 + rnd(12), n_batch = shape == 2 ? 0 : 1 + rnd(n_table), n_own = rnd(4);
    std::vector<Key> keys;
    keys.push_back(Key{"1", "2x"});
    keys.push_back(Key{"12", "x"});
    while (keys.size() < n_table + n_own) keys.push_back(Key{std::to_string(rnd(3)), "d" + std::to_string(keys.size()) + std::string(rnd(3), 'y')});
    for (size_t i = keys.size(); i-- > 1;) std::swap(keys[i], keys[rnd(i + 1)]);
    // ---- routes: two normal routes per table key (ids 2k, 2k + 1), then the shared routes; key bytes "K" flag receiverUrl be16(len)
    const uint32_t n_shared_routes = 1 + rnd(4), id_end = 2 * n_table + n_shared_routes, id_cap = id_end + 8;
    std::vector<uint8_t> kpool(16, 0xEE);
    std::vector<unsigned long long> kref(id_cap, 0ull);
    for (uint32_t id = 0; id < id_end; id++) {
        std::string recv = id < 2 * n_table ? keys[id / 2].sub + std::string("\0", 1) + "inbox" + std::to_string(id) + std::string("\0", 1) + keys[id / 2].dk : "g" + std::to_string(id);
        const size_t off = kpool.size();
        kpool.push_back('K');
        kpool.push_back(id < 2 * n_table ? 1 : 2);
        kpool.insert(kpool.end(), recv.begin(), recv.end());
        kpool.push_back((uint8_t)(recv.size() >> 8));
        kpool.push_back((uint8_t)recv.size());
        kref[id] = (unsigned long long)off | ((unsigned long long)(kpool.size() - off) << KREF_LEN_SHIFT);
    }
    kpool.resize(kpool.size() + 16, 0xEE);
    DistIndexMut ix{};
    ix.kpool = kpool.data();
    ix.kref = kref.data();
    // ---- share-deliverer numbers: a mix of keys in the batch, known but absent, unknown -- and one whose hash is planted on another key's slot
    // (the key that carries the planted hash stands for a key with the SAME hash: its own bytes are not among the numbers)
    const bool plant = shape != 1 && n_batch > 0 && rnd(2);
    const uint32_t planted_on = plant ? rnd(n_batch) : 0xFFFFFFFFu;
    std::vector<Key> sd;
    for (uint32_t k = 0; k < keys.size(); k++)
        if (shape != 1 && k != planted_on && rnd(3) != 0) sd.push_back(keys[k]);
    if (plant) sd.push_back(Key{"7", "planted"});
    for (size_t i = sd.size(); i-- > 1;) std::swap(sd[i], sd[rnd(i + 1)]);
    const uint32_t n_sd = (uint32_t)sd.size();
    std::vector<uint8_t> sd_bytes(8, 0xEE);
    std::vector<uint32_t> sd_off;
    for (const Key& k : sd) {
        sd_off.push_back((uint32_t)sd_bytes.size());
        const std::string b = k.bytes();
        sd_bytes.insert(sd_bytes.end(), b.begin(), b.end());
    }
    sd_off.push_back((uint32_t)sd_bytes.size());
    sd_bytes.resize(sd_bytes.size() + 16, 0xEE);
    // ---- the group table
    FanoutState st{};
    st.seed = 1 + rnd(5);
    st.gt_cap = 4;
    while (st.gt_cap < 2 * (n_table + 1)) st.gt_cap *= 2;
    st.id_cap = id_cap;
    std::vector<unsigned long long> gt_hash(st.gt_cap, 0ull);
    std::vector<uint32_t> gt_rep(st.gt_cap, 0xFFFFFFFFu), dgroup = guarded(id_cap, FO_UNSET);
    auto hash_of = [&](const Key& k) {
        const std::string b = k.bytes();
        const DelivererSpan s = dl_sd_span((const uint8_t*)b.data(), 0, b.size());
        return fo_hash((const uint8_t*)b.data(), s, st.seed);
    };
    for (uint32_t k = 0; k < n_table; k++) {
        const unsigned long long h = hash_of(k == planted_on ? Key{"7", "planted"} : keys[k]);
        uint32_t slot = (uint32_t)(h >> 17) & (st.gt_cap - 1);
        while (gt_hash[slot] != 0) slot = (slot + 1) & (st.gt_cap - 1);
        gt_hash[slot] = h;
        gt_rep[slot] = 2 * k + rnd(2);
        dgroup[2 * k] = dgroup[2 * k + 1] = slot;
    }
    for (uint32_t id = 2 * n_table; id < id_end; id++) dgroup[id] = st.gt_cap;
    st.gt_hash = gt_hash.data();
    st.gt_rep = gt_rep.data();
    st.dgroup = dgroup.data();
    // ---- step 1 as it leaves the pairs: normal groups (in a shuffled order of the keys), the shared slice, the dead group
    const uint32_t n_topics = 1200;
    struct Pair {
        uint32_t topic, route;
    };
    auto some_pairs = [&](uint32_t n, uint32_t r0, uint32_t r1) { // n distinct (topic, route) pairs with route in [r0, r1), ascending
        std::map<std::pair<uint32_t, uint32_t>, int> s;
        n = std::min<uint32_t>(n, (r1 - r0) * n_topics / 2);
        while (s.size() < n) s[{rnd(n_topics), r0 + rnd(r1 - r0)}] = 1;
        std::vector<Pair> v;
        for (auto& e : s) v.push_back(Pair{e.first.first, e.first.second});
        return v;
    };
    std::vector<uint32_t> order(n_batch);
    for (uint32_t k = 0; k < n_batch; k++) order[k] = k;
    for (size_t i = order.size(); i-- > 1;) std::swap(order[i], order[rnd(i + 1)]);
    std::vector<uint32_t> g_topic, g_route, g_off{0}, g_rep;
    std::vector<std::vector<Pair>> norm_of_key(keys.size());
    for (uint32_t k : order) {
        norm_of_key[k] = some_pairs(sizes[rnd(10)], 2 * k, 2 * k + 2);
        g_rep.push_back(norm_of_key[k][0].route);
        for (const Pair& p : norm_of_key[k]) g_topic.push_back(p.topic), g_route.push_back(p.route);
        g_off.push_back((uint32_t)g_topic.size());
    }
    const uint32_t n_norm = n_batch, s0 = (uint32_t)g_topic.size();
    const bool want_shared = shape != 1;
    std::vector<Pair> slice = want_shared ? some_pairs(shape == 3 ? 1200 + rnd(400) : 1 + rnd(700), 2 * n_table, id_end) : std::vector<Pair>();
    for (const Pair& p : slice) g_topic.push_back(p.topic), g_route.push_back(p.route);
    const uint32_t s1 = (uint32_t)g_topic.size();
    if (want_shared) g_rep.push_back(0xFFFFFFFEu), g_off.push_back(s1);
    const bool has_dead = rnd(3) == 0;
    std::vector<Pair> dead = has_dead ? some_pairs(sizes[rnd(10)], id_end, id_end + 40) : std::vector<Pair>();
    for (const Pair& p : dead) g_topic.push_back(p.topic), g_route.push_back(p.route);
    if (has_dead) g_rep.push_back(0xFFFFFFFFu), g_off.push_back((uint32_t)g_topic.size());
    const uint32_t total = (uint32_t)g_topic.size(), n_fgroups = (uint32_t)g_rep.size();
    g_topic.resize(total + GUARD, GUARD_WORD), g_route.resize(total + GUARD, GUARD_WORD), g_off.resize(g_off.size() + GUARD, GUARD_WORD), g_rep.resize(g_rep.size() + GUARD, GUARD_WORD);
    // ---- step 2 as it leaves the rows: every pair of the slice gives 0 .. 3 rows (senders), each filed under a share-deliverer number or unresolved
    struct Row {
        uint32_t pair, sender, member;
    };
    std::vector<std::vector<Row>> rows_of_sd(n_sd + 1);
    uint32_t next_sender = 0;
    for (uint32_t p = 0; p < slice.size(); p++) {
        const uint32_t n = rnd(5) == 0 ? 0 : 1 + rnd(3);
        for (uint32_t k = 0; k < n; k++) {
            const bool unres = n_sd == 0 || rnd(12) == 0;
            rows_of_sd[unres ? n_sd : rnd(n_sd)].push_back(Row{p, n == 1 && rnd(2) ? DL_NONE : next_sender++, unres ? DL_NONE : rnd(9)});
        }
    }
    std::vector<uint32_t> r_pair, r_sender, r_member, r_key, r_off{0}, sd_of_group;
    for (uint32_t k = 0; k <= n_sd; k++) {
        if (rows_of_sd[k].empty()) continue;
        for (const Row& r : rows_of_sd[k]) r_pair.push_back(r.pair), r_sender.push_back(r.sender), r_member.push_back(r.member), r_key.push_back(k);
        r_off.push_back((uint32_t)r_pair.size());
        sd_of_group.push_back(k);
    }
    const uint32_t n_srows = (uint32_t)r_pair.size(), n_sgroups = (uint32_t)sd_of_group.size();
    const bool has_unres = n_sgroups && sd_of_group.back() == n_sd;
    for (auto* v : {&r_pair, &r_sender, &r_member, &r_key, &r_off}) v->resize(v->size() + GUARD, GUARD_WORD);
    // ---- expected: a stable merge by key bytes
    using Out = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>; // topic, route, sender (sorts last), aux
    std::vector<std::vector<Out>> x_groups(n_norm);
    for (uint32_t g = 0; g < n_norm; g++)
        for (const Pair& p : norm_of_key[order[g]]) x_groups[g].push_back(Out{p.topic, p.route, DL_NONE, DL_NONE});
    uint32_t x_merged = 0, x_new = 0;
    std::vector<Out> x_unres;
    for (uint32_t j = 0; j < n_sgroups; j++) {
        std::vector<Out> rows;
        for (uint32_t r = r_off[j]; r < r_off[j + 1]; r++) rows.push_back(Out{slice[r_pair[r]].topic, slice[r_pair[r]].route, r_sender[r], r});
        if (sd_of_group[j] == n_sd) {
            x_unres = rows;
            continue;
        }
        uint32_t g = DL_NONE;
        for (uint32_t q = 0; q < n_norm; q++)
            if (keys[order[q]].bytes() == sd[sd_of_group[j]].bytes()) g = q;
        if (g == DL_NONE) {
            x_groups.push_back(rows);
            x_new++;
            cov.absent += [&] {
                for (uint32_t k = n_batch; k < n_table; k++)
                    if (keys[k].bytes() == sd[sd_of_group[j]].bytes()) return 1;
                return 0;
            }();
            cov.planted += sd[sd_of_group[j]].dk == "planted";
            continue;
        }
        cov.share_heavier += rows.size() > x_groups[g].size();
        std::vector<Out> both(x_groups[g].size() + rows.size());
        std::merge(x_groups[g].begin(), x_groups[g].end(), rows.begin(), rows.end(), both.begin(),
                   [](const Out& a, const Out& b) { return std::make_tuple(std::get<0>(a), std::get<1>(a)) < std::make_tuple(std::get<0>(b), std::get<1>(b)); });
        x_groups[g] = both;
        x_merged++;
    }
    if (has_unres) x_groups.push_back(x_unres);
    if (has_dead) {
        x_groups.emplace_back();
        for (const Pair& p : dead) x_groups.back().push_back(Out{p.topic, p.route, DL_NONE, DL_NONE});
    }
    const uint32_t x_n_groups = (uint32_t)x_groups.size();
    uint32_t x_n_rows = 0;
    for (auto& g : x_groups) x_n_rows += (uint32_t)g.size();
    // ---- the launches, as Delivery::plan and DevExec make them
    const std::string where = "shape " + std::to_string(shape) + " table " + std::to_string(n_table) + " batch " + std::to_string(n_batch) + " numbers " + std::to_string(n_sd) +
                              " pairs " + std::to_string(total) + " member rows " + std::to_string(n_srows);
    const char* what = where.c_str();
    DeliveryPlan P{};
    P.g_topic = g_topic.data(), P.g_route = g_route.data(), P.g_off = g_off.data(), P.g_rep = g_rep.data();
    P.total = total, P.n_fgroups = n_fgroups, P.n_norm = n_norm, P.s0 = s0, P.s1 = s1, P.has_dead = has_dead;
    P.r_pair = r_pair.data(), P.r_sender = r_sender.data(), P.r_off = r_off.data(), P.r_key = r_key.data();
    P.n_srows = n_srows, P.n_sgroups = n_sgroups, P.n_sd = n_sd;
    P.sd_bytes = sd_bytes.data(), P.sd_off = sd_off.data();
    std::vector<uint32_t> slot_group = guarded(st.gt_cap, DL_NONE), tgt = guarded(n_sgroups, 0xABABABABu), is_new = guarded(n_sgroups, 0xABABABABu),
                          new_scan = guarded(n_sgroups, 0xABABABABu);
    P.slot_group = slot_group.data(), P.tgt = tgt.data(), P.is_new = is_new.data(), P.new_scan = new_scan.data();
    if (n_sgroups) {
        if (n_norm) launch(n_norm, [&] { k_dl_scatter(st, P); });
        launch(n_sgroups, [&] { k_dl_map(ix, st, P); });
        for (uint32_t j = 0, run = 0; j < n_sgroups; j++) new_scan[j] = (run += is_new[j]);
        P.n_new = new_scan[n_sgroups - 1];
    }
    if (P.n_new != x_new) FAIL("map: a count of %u groups reached through members only, expected %u (%s)\n", P.n_new, x_new, what);
    P.n_groups = n_norm + P.n_new + (has_unres ? 1u : 0u) + (has_dead ? 1u : 0u);
    P.n_rows = (total - (s1 - s0)) + n_srows;
    if (P.n_groups != x_n_groups || P.n_rows != x_n_rows) FAIL("harness: a count of %u groups / %u rows, the merge has %u / %u (%s)\n", P.n_groups, P.n_rows, x_n_groups, x_n_rows, what);
    if (P.n_rows == 0) return 0;
    std::vector<uint32_t> share_of = guarded(P.n_groups, DL_NONE), cnt = guarded(P.n_groups, 0xABABABABu), cnt_scan = guarded(P.n_groups, 0xABABABABu);
    std::vector<uint32_t> out_topic = guarded(P.n_rows, 0xABABABABu), out_route = guarded(P.n_rows, 0xABABABABu), out_aux = guarded(P.n_rows, 0xABABABABu),
                          out_off = guarded(P.n_groups + 1, 0xABABABABu);
    P.share_of = share_of.data(), P.cnt = cnt.data(), P.cnt_scan = cnt_scan.data();
    P.out_topic = out_topic.data(), P.out_route = out_route.data(), P.out_aux = out_aux.data(), P.out_group_off = out_off.data();
    if (n_sgroups) launch(n_sgroups, [&] { k_dl_assign(P); });
    launch(P.n_groups, [&] { k_dl_count(P); });
    for (uint32_t g = 0, run = 0; g < P.n_groups; g++) cnt_scan[g] = (run += cnt[g]);
    for (uint32_t g = 0; g < P.n_groups; g++)
        if (cnt[g] != x_groups[g].size()) FAIL("count: the row count of group %u is %u, expected %zu (%s)\n", g, cnt[g], x_groups[g].size(), what);
    const uint32_t n = std::max(P.n_rows, P.n_groups + 1);
    launch(n, [&] { k_dl_merge(P, n); });
    for (uint32_t g = 0, at = 0; g < P.n_groups; g++) {
        if (out_off[g] != at) FAIL("offsets: the first row of group %u is %u, expected %u (%s)\n", g, out_off[g], at, what);
        for (const Out& o : x_groups[g]) {
            if (out_topic[at] != std::get<0>(o) || out_route[at] != std::get<1>(o) || out_aux[at] != std::get<3>(o))
                FAIL("output row %u of group %u is (topic %u, route %u, aux %u), expected (%u, %u, %u) (%s)\n", at, g, out_topic[at], out_route[at], out_aux[at], std::get<0>(o),
                     std::get<1>(o), std::get<3>(o), what);
            at++;
        }
        if (g + 1 == P.n_groups && out_off[g + 1] != at) FAIL("offsets: the end row is %u, expected %u (%s)\n", out_off[g + 1], at, what);
    }
    for (const auto* v : {&slot_group, &tgt, &is_new, &new_scan, &share_of, &cnt, &cnt_scan, &out_topic, &out_route, &out_aux, &out_off, &dgroup, &g_topic, &g_route, &g_off, &g_rep,
                          &r_pair, &r_sender, &r_member, &r_key, &r_off})
        if (!guard_intact(*v)) FAIL("a kernel wrote behind an array: a guard row is damaged (%s)\n", what);
    cov.cases++, cov.rows += P.n_rows, cov.merged += x_merged, cov.share_only += x_new, cov.unresolved += has_unres, cov.dead += has_dead;
    cov.no_shared += !want_shared, cov.only_shared += n_norm == 0 && n_srows > 0;
    for (auto& g : x_groups) cov.lists_over_block += g.size() > (size_t)DL_BLOCK, cov.lists_at_wave += g.size() % 64 <= 1 || g.size() % 64 == 63;
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 6;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    Coverage cov;
    int c = 0;
    for (int round = 0; round < rounds; round++)
        for (uint32_t k = 0; k < 24; k++, c++) {
            const uint32_t shape = k % 8 == 5 ? 1 : k % 8 == 6 ? 2 : k % 8 == 7 ? 3 : 0; // 1: no shared pairs, 2: shared pairs only, 3: a slice longer than the normal lists
            if (one_case(rng, shape, cov)) {
                fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                return 1;
            }
        }
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"groups with normal and member rows", cov.merged, 20 * R}, {"groups of members only", cov.share_only, 10 * R}, {"planted hashes", cov.planted, 2 * R},
                  {"keys known to the table and absent from the batch", cov.absent, 3 * R}, {"unresolved groups", cov.unresolved, 5 * R}, {"dead groups", cov.dead, 3 * R},
                  {"groups longer than a workgroup", cov.lists_over_block, 10 * R}, {"groups ending at a wave", cov.lists_at_wave, 5 * R},
                  {"batches without shared pairs", cov.no_shared, 2 * R}, {"batches of shared pairs only", cov.only_shared, 2 * R},
                  {"groups with more member rows than pairs", cov.share_heavier, 5 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("delivery emu ok: %llu cases, %llu rows; merged groups %llu, member-only groups %llu, planted hashes %llu, absent keys %llu, unresolved %llu, dead %llu, "
           "groups over a workgroup %llu, at a wave %llu, no shared pairs %llu, shared pairs only %llu, member-heavy groups %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.rows, (unsigned long long)cov.merged, (unsigned long long)cov.share_only, (unsigned long long)cov.planted,
           (unsigned long long)cov.absent, (unsigned long long)cov.unresolved, (unsigned long long)cov.dead, (unsigned long long)cov.lists_over_block,
           (unsigned long long)cov.lists_at_wave, (unsigned long long)cov.no_shared, (unsigned long long)cov.only_shared, (unsigned long long)cov.share_heavier);
    return 0;
}
