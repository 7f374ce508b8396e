// prefix_emu.cpp -- host-side logic test of k_b_prefix_census (bifromq_amd/csrc/bmq_prefix_kernels.h: the per-prefix census of the route
// keys, bmq_routes_prefix_census) under the wave64 emulator of wave_emu.h.  Test tooling: the kernel's LOGIC -- a wave's stretch of ids,
// the floor search over the sorted prefixes, the walk up the parent links, the reduction per distinct slot and the run a wave carries and
// flushes -- and the control around it (DistIndex::prefix_census: sort, de-duplication, parents, the carry to the parents, the copy out
// through the input-to-slot map) against a per-key loop written plainly below.
//
// The index is built by the product's own host builder (DistIndex over an executor that is HostExec in everything but prefix_census, which
// launches the kernel on the emulator: at the product's grid and at grids of one and two workgroups, the blocks and waves last to first).
// The expected numbers do NOT go through prefix_key_one, key_compare or key_parse: the harness reads every live key's bytes from the key
// pool, looks its flag up in its own record of the keys it made, and tests every prefix of the call against it as std::string does.
//
// The run ends with an `ok` line of the paths it took and fails below their floors: keys whose floor is their answer, keys that walk up
// from a floor that is no prefix of them, keys without any prefix in the table, dead references, lanes past n, launches whose waves take
// several turns, repeated inputs, chains of three parent links.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/prefix_emu.cpp -o build/prefix_emu && build/prefix_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "bmq_prefix_kernels.h"
#include "bmq_dist_index.h"
#include "bmq_exec_host.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

struct Coverage {
    uint64_t cases = 0, ids = 0, floor_hit = 0, walked = 0, no_prefix = 0, dead = 0, past_n = 0, multi_turn = 0, repeats = 0, chain3 = 0, launches = 0;
};

// HostExec in everything but the census pass: that one is the kernel, a wave at a time
struct EmuExec : HostExec {
    uint32_t grid_force = 0;
    uint32_t last_grid = 0, last_n = 0, launches = 0;
    bool prefix_census(const DistIndexMut& ix, uint32_t n, const PrefixTable& T, unsigned long long* table) {
        const uint32_t grid = grid_force ? std::min(grid_force, census_grid(n)) : census_grid(n);
        wemu::grid_size() = grid;
        last_grid = grid, last_n = n, launches++;
        for (uint32_t b = grid; b-- > 0;) // (the blocks last to first, the waves of a block likewise: nothing may depend on the order)
            for (uint32_t w = CENSUS_WAVES; w-- > 0;) wemu::run_wave(b, [&] { k_b_prefix_census(ix, n, T, table); }, w);
        return true;
    }
};

// ---- route keys: 00 | u16be(len tenant) | tenant | (level 00)* | 00 | bucket | flag | receiver | u16be(len receiver) ----
static std::string make_key(const std::string& tenant, uint32_t filter, uint32_t serial, uint32_t flag) {
    std::string k(1, '\0');
    k += (char)(tenant.size() >> 8), k += (char)(tenant.size() & 0xFF);
    k += tenant;
    k += "f" + std::to_string(filter);
    k += '\0';
    if (filter % 3 == 0) k += "lv" + std::string(filter % 11, 'x'), k += '\0';
    k += '\0';
    k += (char)(filter % 7);
    k += (char)flag;
    const std::string recv = "0" + std::string(1, '\0') + "r" + std::to_string(serial) + std::string(1, '\0') + "d";
    k += recv;
    k += (char)(recv.size() >> 8), k += (char)(recv.size() & 0xFF);
    return k;
}
static std::string tenant_cut(const std::string& k) { return k.substr(0, 3 + (((uint8_t)k[1] << 8) | (uint8_t)k[2])); }
static std::string filter_cut(const std::string& k) {
    const size_t rlen = ((uint8_t)k[k.size() - 2] << 8) | (uint8_t)k[k.size() - 1];
    return k.substr(0, k.size() - rlen - 4);
}
static bool starts_with(const std::string& k, const std::string& p) { return k.size() >= p.size() && k.compare(0, p.size(), p) == 0; }

enum Shape { S_RUNS, S_ROUND_ROBIN, S_RANDOM, S_ONE, S_COUNT };

static int one_case(std::mt19937_64& rng, Shape shape, uint32_t pmode, uint32_t deletes_pct, uint32_t grid_force, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    static const char* names[] = {"", "a", "tenant-12-by", "tenant-13-byt", "\xe7\xa7\x9f\xe6\x88\xb7", "tenant-12-bz", "ab", "\xff\xfe"};
    const uint32_t n_tenants = shape == S_ONE ? 1 : 2 + rnd(7);
    std::map<std::string, uint32_t> made; // key -> flag
    std::vector<std::string> order;       // the keys in the order they are handed to the index
    uint32_t serial = 0;
    auto add = [&](uint32_t t, uint32_t filter) {
        const uint32_t flag = 1 + (serial * 7 + serial / 5) % 3;
        std::string k = make_key(names[t], filter, serial++, flag);
        made[k] = flag;
        order.push_back(std::move(k));
    };
    const uint32_t runs[5] = {1, 63, 64, 65, 200};
    switch (shape) {
    case S_RUNS: // filters of 1, 63, 64, 65 and 200 receivers: runs under one filter prefix end on both sides of a wave's border
        for (uint32_t t = 0; t < n_tenants; t++)
            for (uint32_t f = 0; f < 3; f++)
                for (uint32_t i = 0; i < runs[(t + f) % 5]; i++) add(t, f);
        break;
    case S_ROUND_ROBIN: // neighbouring lanes under different filters and tenants
        for (uint32_t i = 0, e = 400 + rnd(600); i < e; i++) add(i % n_tenants, i % 67);
        break;
    case S_ONE:
        for (uint32_t i = 0, e = 300 + rnd(900); i < e; i++) add(0, i / 150);
        break;
    default:
        for (uint32_t i = 0, e = 200 + rnd(1500); i < e; i++) add(rnd(n_tenants), rnd(40));
        break;
    }
    EmuExec hx;
    hx.threads = 1;
    DistIndex<EmuExec> ix(hx);
    auto pack = [&](const std::vector<std::string>& ks, std::vector<uint8_t>& bytes, std::vector<uint32_t>& off) {
        bytes.clear(), off.assign(1, 0u);
        for (const auto& k : ks) {
            bytes.insert(bytes.end(), k.begin(), k.end());
            off.push_back((uint32_t)bytes.size());
        }
        bytes.resize(bytes.size() + 32, 0);
    };
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off;
    if (shape == S_ROUND_ROBIN || (shape == S_RANDOM && rnd(2))) { // through the apply path: ids in op order
        std::vector<uint8_t> ops(order.size(), 0);
        pack(order, bytes, off);
        if (!ix.apply(bytes.data(), off.data(), ops.data(), (uint32_t)order.size())) FAIL("apply: %s\n", ix.error.c_str());
    } else { // a bulk load: ids in key order, every filter one run
        std::vector<std::string> sorted = order;
        std::sort(sorted.begin(), sorted.end());
        pack(sorted, bytes, off);
        if (!ix.rebuild(bytes.data(), off.data(), (uint32_t)sorted.size())) FAIL("rebuild: %s\n", ix.error.c_str());
    }
    if (deletes_pct) { // dead references scattered through the runs
        std::vector<std::string> gone;
        for (const auto& kv : made)
            if (rnd(100) < deletes_pct) gone.push_back(kv.first);
        if (!gone.empty()) {
            std::vector<uint8_t> ops(gone.size(), 1);
            pack(gone, bytes, off);
            if (!ix.apply(bytes.data(), off.data(), ops.data(), (uint32_t)gone.size())) FAIL("apply (deletes): %s\n", ix.error.c_str());
        }
    }
    const DistIndexMut m = ix.mut();
    const uint32_t n = ix.next_id;
    std::vector<std::string> live;
    uint32_t n_dead = 0;
    for (uint32_t id = 0; id < n; id++) {
        const unsigned long long r = m.kref[id];
        const uint32_t len = (uint32_t)(r >> KREF_LEN_SHIFT);
        if (len == 0) {
            n_dead++;
            continue;
        }
        live.emplace_back((const char*)m.kpool + (r & KREF_OFF_MASK), len);
        if (!made.count(live.back())) FAIL("id %u holds a key the harness never made\n", id);
    }
    if (live.empty()) FAIL("a case without live keys\n");
    std::vector<std::string> all;
    for (const auto& kv : made) all.push_back(kv.first);
    // ---- the prefixes of the call
    std::vector<std::string> P;
    auto some = [&]() -> const std::string& { return all[rnd(all.size())]; };
    switch (pmode) {
    case 0: // the tenants and the empty prefix
        for (const auto& k : all) P.push_back(tenant_cut(k));
        std::sort(P.begin(), P.end());
        P.erase(std::unique(P.begin(), P.end()), P.end());
        P.push_back("");
        break;
    case 1: // chains of three parent links: "" < tenant < filter < key
        P.push_back("");
        for (uint32_t i = 0; i < 12; i++) {
            const std::string& k = some();
            P.push_back(k), P.push_back(filter_cut(k)), P.push_back(tenant_cut(k));
        }
        break;
    case 2: { // the floor is a sibling: the table holds a tenant's prefix and ONE of its keys; the keys behind that one walk up
        const std::string& k = all[all.size() / 3];
        P = {tenant_cut(k), k};
        break;
    }
    case 3: // cuts at any byte, repeats, in a shuffled order
        for (uint32_t i = 0, e = 1 + rnd(100); i < e; i++) {
            const std::string& k = some();
            P.push_back(k.substr(0, rnd(k.size() + 1)));
            if (rnd(4) == 0) P.push_back(P[rnd(P.size())]);
        }
        P.push_back(P.front());
        std::shuffle(P.begin(), P.end(), rng);
        break;
    case 4: // absent prefixes around present ones: a key plus a byte, above all keys, a key with its last byte changed; every filter
        for (uint32_t i = 0; i < 8; i++) {
            const std::string& k = some();
            P.push_back(k + std::string(1, '\0')), P.push_back(k + "x"), P.push_back(k.substr(0, k.size() - 1) + "\x7f"), P.push_back(filter_cut(k));
        }
        P.push_back("\xff\xff"), P.push_back(std::string(300, '\0'));
        break;
    case 5: // every filter and every tenant, descending: the largest tables
        for (const auto& k : all) P.push_back(filter_cut(k)), P.push_back(tenant_cut(k));
        std::sort(P.begin(), P.end());
        P.erase(std::unique(P.begin(), P.end()), P.end());
        std::reverse(P.begin(), P.end());
        break;
    default: { // one prefix
        const std::string& k = some();
        P = {rnd(2) ? filter_cut(k) : k.substr(0, 1 + rnd(4))};
        break;
    }
    }
    // ---- expected: every live key against every prefix, as std::string compares; the paths a correct kernel takes, from the sorted table
    std::vector<unsigned long long> want(4 * P.size(), 0);
    std::set<std::string> table(P.begin(), P.end());
    for (const std::string& k : live) {
        for (size_t i = 0; i < P.size(); i++)
            if (starts_with(k, P[i])) want[4 * i + made[k] - 1]++, want[4 * i + 3] += k.size();
        auto f = table.upper_bound(k); // the floor: the last prefix <= k
        if (f == table.begin()) {
            cov.no_prefix++;
            continue;
        }
        --f;
        bool any = false;
        for (const std::string& p : table) any = any || starts_with(k, p);
        if (starts_with(k, *f)) cov.floor_hit++;
        else if (any) cov.walked++;
        else cov.no_prefix++;
    }
    cov.repeats += table.size() < P.size();
    for (const std::string& p : table) {
        uint32_t links = 0;
        for (const std::string& q : table) links += q.size() < p.size() && starts_with(p, q);
        if (links >= 3) {
            cov.chain3++;
            break;
        }
    }
    // ---- the call, as bmq_routes_prefix_census makes it
    pack(P, bytes, off);
    std::vector<uint64_t> out(4 * P.size() + 8, 0xC0DEC0DEull);
    PrefixStats stats;
    hx.grid_force = grid_force;
    hx.launches = 0;
    if (!ix.prefix_census(bytes.data(), off.data(), (uint32_t)P.size(), out.data(), stats, [] {})) FAIL("prefix_census: %s\n", ix.error.c_str());
    if (hx.launches != 1) FAIL("prefix_census launched %u passes, expected one\n", hx.launches);
    const std::string where = "shape " + std::to_string((int)shape) + " prefixes mode " + std::to_string(pmode) + " n " + std::to_string(P.size()) + " ids " +
                              std::to_string(n) + " grid " + std::to_string(hx.last_grid);
    for (size_t i = 0; i < want.size(); i++)
        if (out[i] != want[i])
            FAIL("census: the count of prefix %zu word %zu is %llu, expected %llu (%s)\n", i / 4, i % 4, (unsigned long long)out[i], want[i], where.c_str());
    for (size_t i = want.size(); i < out.size(); i++)
        if (out[i] != 0xC0DEC0DEull) FAIL("census: a count was written behind the output: a guard row is damaged (%s)\n", where.c_str());
    if (stats.n_calls != 1 || stats.n_prefixes != P.size() || stats.n_distinct != table.size() || stats.n_keys_scanned != n)
        FAIL("stats: a count of the call's statistics is off (%s)\n", where.c_str());
    const uint32_t turns = census_turns(n, hx.last_grid);
    cov.multi_turn += turns > 1;
    cov.past_n += (unsigned long long)hx.last_grid * CENSUS_WAVES * turns * 64ull > n;
    cov.dead += n_dead;
    cov.cases++, cov.ids += n, cov.launches++;
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 2;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    Coverage cov;
    int c = 0;
    for (int round = 0; round < rounds; round++)
        for (int shape = 0; shape < S_COUNT; shape++)
            for (uint32_t pmode = 0; pmode < 7; pmode++, c++) {
                static const uint32_t del_pct[3] = {0, 5, 30}, grids[3] = {0, 1, 2};
                if (one_case(rng, (Shape)shape, pmode, del_pct[c % 3], grids[(c / 3) % 3], cov)) {
                    fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                    return 1;
                }
            }
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"keys whose floor is their deepest prefix", cov.floor_hit, 2000 * R},
                  {"keys that walk up from a floor that is no prefix of them", cov.walked, 500 * R},
                  {"keys without a prefix in the table", cov.no_prefix, 500 * R},
                  {"dead references", cov.dead, 200 * R},
                  {"launches with lanes past n", cov.past_n, 10 * R},
                  {"launches whose waves take several turns", cov.multi_turn, 8 * R},
                  {"calls with repeated prefixes", cov.repeats, 4 * R},
                  {"calls with a chain of three parent links", cov.chain3, 4 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("prefix emu ok: %llu cases, %llu ids; floor hits %llu, walks %llu, keys without a prefix %llu, dead references %llu, launches with lanes past n %llu, "
           "multi-turn launches %llu, calls with repeats %llu, with a chain of three links %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.ids, (unsigned long long)cov.floor_hit, (unsigned long long)cov.walked,
           (unsigned long long)cov.no_prefix, (unsigned long long)cov.dead, (unsigned long long)cov.past_n, (unsigned long long)cov.multi_turn,
           (unsigned long long)cov.repeats, (unsigned long long)cov.chain3);
    return 0;
}
