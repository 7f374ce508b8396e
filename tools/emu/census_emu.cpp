// census_emu.cpp -- host-side logic test of k_b_census and k_r_census (bifromq_amd/csrc/bmq_census_kernels.h: the per-tenant census of
// the route keys and of the retained topics handed out since the bulk load) under the wave64 emulator of wave_emu.h.  Test tooling: the
// kernels' LOGIC -- a wave's stretch of ids, the boundary keys staged per wave, the loop over the distinct table slots of a turn, the
// per-flag ballots, the byte sum over the masked lanes, the run a wave carries from turn to turn and where it is flushed -- against a
// per-key loop written plainly below.
//
// k_b_census runs over indexes built by the product's own host builder (DistIndex<HostExec>: bulk loads in key order, so that tenants are
// runs of ids, and bmq_routes_apply-style batches that interleave the tenants; deletes leave dead references).  The expected numbers do
// NOT go through key_parse / key_in_boundary: the harness reads every live key's bytes from the key pool, looks tenant and flag up in its
// own record of the keys it made, and compares with the boundary as std::string does.  k_r_census reads three arrays only (dead bits,
// id_tnode, the bounds), which the harness fills directly.
//
// Besides the table, the number of FLUSHES of every launch (BMQ_CENSUS_FLUSH_HOOK) is compared with a model of the runs: a wave that adds
// after every turn still counts right, only with twenty times the atomics -- the count is what tells.  The run ends with an `ok` line of
// the paths it took and fails below their floors: turns with one slot, with 64 slots, runs carried over a turn and flushed by a slot
// change, runs carried and flushed at the end, dead lanes inside a run, lanes past n.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/census_emu.cpp -o build/census_emu && build/census_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <map>
#include <random>
#include <string>
#include <vector>

static unsigned long long g_flushes = 0;
#define BMQ_CENSUS_FLUSH_HOOK() (++g_flushes)
#include "bmq_census_kernels.h"
#include "bmq_dist_index.h"
#include "bmq_exec_host.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

struct Coverage {
    uint64_t cases = 0, ids = 0, one_slot = 0, slots_64 = 0, carried_change = 0, carried_end = 0, dead_inside = 0, past_n = 0, multi_turn = 0, bounded = 0;
};

// What the launch must do, from the slot of every index (NONE: not counted): flushes, and the paths taken
static unsigned long long model(const std::vector<uint32_t>& slot, uint32_t grid, Coverage& cov) {
    const uint32_t n = (uint32_t)slot.size(), turns = census_turns(n, grid);
    unsigned long long flushes = 0;
    cov.multi_turn += turns > 1;
    for (uint32_t w = 0; w < grid * CENSUS_WAVES; w++) {
        uint32_t run = NONE, run_turn = 0;
        for (uint32_t t = 0; t < turns; t++) {
            const unsigned long long first = ((unsigned long long)w * turns + t) * 64;
            std::vector<uint32_t> order; // distinct slots in the order of their first lane
            bool past = false, dead_in = false;
            uint32_t last_live = NONE;
            for (uint32_t l = 0; l < 64; l++) {
                const unsigned long long i = first + l;
                if (i >= n) {
                    past = true;
                    continue;
                }
                const uint32_t s = slot[i];
                if (s == NONE) continue;
                if (l && last_live == s && slot[i - 1] == NONE) dead_in = true;
                last_live = s;
                if (std::find(order.begin(), order.end(), s) == order.end()) order.push_back(s);
            }
            cov.past_n += past && first < n;
            cov.dead_inside += dead_in;
            cov.one_slot += order.size() == 1 && !past;
            cov.slots_64 += order.size() == 64;
            for (uint32_t s : order) {
                if (s == run) continue;
                if (run != NONE) {
                    flushes++;
                    cov.carried_change += run_turn < t;
                }
                run = s, run_turn = t;
            }
        }
        if (run != NONE) {
            flushes++;
            cov.carried_end += run_turn + 1 < turns;
        }
    }
    return flushes;
}

// ---- route keys: 00 | u16be(len tenant) | tenant | (level 00)* | 00 | bucket | flag | receiver | u16be(len receiver) ----
static std::string make_key(const std::string& tenant, uint32_t serial, uint32_t flag) {
    std::string k(1, '\0');
    k += (char)(tenant.size() >> 8), k += (char)(tenant.size() & 0xFF);
    k += tenant;
    k += "f" + std::to_string(serial);
    k += '\0';
    if (serial % 3 == 0) k += "lv" + std::string(serial % 11, 'x'), k += '\0';
    k += '\0';
    k += (char)(serial % 7);
    k += (char)flag;
    const std::string recv = "0" + std::string(1, '\0') + "r" + std::to_string(serial % 13) + std::string(1, '\0') + "d";
    k += recv;
    k += (char)(recv.size() >> 8), k += (char)(recv.size() & 0xFF);
    return k;
}
static std::vector<std::string> tenant_names(std::mt19937_64& rng, uint32_t n) {
    // the directed ones first: empty, 1, 12, 13 and 40 bytes (the 12-byte inline compare against the name pool), bytes >= 0x80
    std::vector<std::string> t = {"", "a", "tenant-12-by", "tenant-13-byt", std::string(40, 'q'), "\xe7\xa7\x9f\xe6\x88\xb7", "tenant-12-bz", std::string(39, 'q') + "r"};
    while (t.size() < n) {
        std::string s = "t" + std::to_string(t.size());
        if (rng() % 4 == 0) s += std::string(rng() % 30, (char)(0x80 + rng() % 0x7F));
        t.push_back(s);
    }
    t.resize(n);
    return t;
}
struct KeyInfo {
    uint32_t tenant, flag;
};

enum Shape { S_RUNS, S_ROUND_ROBIN, S_RANDOM, S_ONE, S_COUNT };

static int dist_case(std::mt19937_64& rng, Shape shape, uint32_t n_tenants, uint32_t deletes_pct, uint32_t bmode, uint32_t grid_force, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const std::vector<std::string> tn = tenant_names(rng, n_tenants);
    std::map<std::string, KeyInfo> made;
    std::vector<std::string> order; // the keys in the order they are handed to the index
    uint32_t serial = 0;
    auto add = [&](uint32_t t) {
        const uint32_t flag = 1 + (serial * 7 + serial / 5) % 3;
        std::string k = make_key(tn[t], serial++, flag);
        made[k] = KeyInfo{t, flag};
        order.push_back(std::move(k));
    };
    const uint32_t runs[5] = {1, 63, 64, 65, 200};
    switch (shape) {
    case S_RUNS: // tenants of 1, 63, 64, 65 and 200 keys: runs end on both sides of a wave's border
        for (uint32_t t = 0; t < n_tenants; t++)
            for (uint32_t i = 0; i < runs[(t + n_tenants) % 5]; i++) add(t);
        break;
    case S_ROUND_ROBIN: // every lane of a wave a different tenant
        for (uint32_t i = 0, e = n_tenants * (3 + rnd(6)); i < e; i++) add(i % n_tenants);
        break;
    case S_ONE:
        for (uint32_t i = 0, e = 300 + rnd(900); i < e; i++) add(0);
        break;
    default:
        for (uint32_t i = 0, e = 200 + rnd(1500); i < e; i++) add(rnd(n_tenants));
        break;
    }
    HostExec hx;
    hx.threads = 1;
    DistIndex<HostExec> ix(hx);
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
    if (shape == S_ROUND_ROBIN || (shape == S_RANDOM && rnd(2))) { // through the apply path: ids in op order, the tenants interleaved
        std::vector<uint8_t> ops(order.size(), 0);
        pack(order, bytes, off);
        if (!ix.apply(bytes.data(), off.data(), ops.data(), (uint32_t)order.size())) FAIL("apply: %s\n", ix.error.c_str());
    } else { // a bulk load: ids in key order, every tenant one run
        std::vector<std::string> sorted = order;
        std::sort(sorted.begin(), sorted.end());
        pack(sorted, bytes, off);
        if (!ix.rebuild(bytes.data(), off.data(), (uint32_t)sorted.size())) FAIL("rebuild: %s\n", ix.error.c_str());
    }
    if (deletes_pct) { // dead references scattered through the runs; tenant 1 (if any) loses every route
        std::vector<std::string> gone;
        for (const auto& [k, info] : made)
            if (rnd(100) < deletes_pct || (info.tenant == 1 && deletes_pct > 20)) gone.push_back(k);
        if (!gone.empty()) {
            std::vector<uint8_t> ops(gone.size(), 1);
            pack(gone, bytes, off);
            if (!ix.apply(bytes.data(), off.data(), ops.data(), (uint32_t)gone.size())) FAIL("apply (deletes): %s\n", ix.error.c_str());
        }
    }
    const DistIndexMut m = ix.mut();
    const uint32_t n = ix.next_id;
    // ---- the boundary
    std::vector<std::string> all;
    for (const auto& kv : made) all.push_back(kv.first);
    auto prefix_of = [&](uint32_t t) {
        std::string p(1, '\0');
        p += (char)(tn[t].size() >> 8), p += (char)(tn[t].size() & 0xFF);
        return p + tn[t];
    };
    std::string bs, be;
    uint32_t flags = 0;
    switch (bmode) {
    case 0: break;                                                    // none
    case 1: flags = 2, be = all[all.size() / 2]; break;               // cuts inside a tenant
    case 2: flags = 1, bs = all[all.size() / 3]; break;
    case 3: flags = 2, be = prefix_of(rnd(n_tenants)); break;         // ends exactly at a tenant's prefix
    case 4: {                                                         // ... at its upper bound
        be = prefix_of(rnd(n_tenants));
        be.back() = (char)((uint8_t)be.back() + 1);
        flags = 2;
        break;
    }
    case 5: flags = 2; break;                                         // NULL_BOUNDARY: no start, an empty end
    case 6: flags = 3, bs = all[all.size() / 2] + std::string(1, '\0'), be = bs + std::string(1, '\0'); break; // holds nothing
    case 7: flags = 3, bs = all[all.size() / 4], be = all[3 * all.size() / 4] + std::string(300, '\x7f'); break; // an end longer than the LDS copy
    default: {
        const uint32_t a = rnd(all.size()), c = rnd(all.size());
        flags = 3, bs = all[std::min(a, c)].substr(0, 1 + rnd(all[std::min(a, c)].size())), be = all[std::max(a, c)] + "\x01";
        if (!(bs < be)) flags = 1;
        break;
    }
    }
    KeyBoundary kb{};
    kb.start = (const uint8_t*)bs.data(), kb.end = (const uint8_t*)be.data();
    kb.start_len = (uint32_t)bs.size(), kb.end_len = (uint32_t)be.size(), kb.flags = flags;
    cov.bounded += flags != 0;
    // ---- expected: a per-key loop over the key store's bytes, tenant and flag from the harness's own record
    const uint32_t n_dir = ix.dir_slots;
    std::vector<unsigned long long> want(4 * (size_t)n_dir, 0);
    std::vector<uint32_t> slot(n, NONE);
    for (uint32_t id = 0; id < n; id++) {
        const unsigned long long r = m.kref[id];
        const uint32_t len = (uint32_t)(r >> KREF_LEN_SHIFT);
        if (len == 0) continue;
        const std::string k((const char*)m.kpool + (r & KREF_OFF_MASK), len);
        const auto f = made.find(k);
        if (f == made.end()) FAIL("id %u holds a key the harness never made\n", id);
        if ((flags & 1u) && k < bs) continue;
        if ((flags & 2u) && !(k < be)) continue;
        const uint32_t d = ix.tenant_slot.at(tn[f->second.tenant]);
        slot[id] = d;
        want[4 * (size_t)d + f->second.flag - 1]++;
        want[4 * (size_t)d + 3] += len;
    }
    // ---- the launch, as DevExec::census makes it (grid_force: a smaller grid, so that waves take many turns)
    const uint32_t grid = grid_force ? std::min(grid_force, census_grid(n)) : census_grid(n);
    std::vector<unsigned long long> table(4 * (size_t)n_dir + 8, 0);
    for (size_t i = 4 * (size_t)n_dir; i < table.size(); i++) table[i] = 0xC0DEC0DEull;
    wemu::grid_size() = grid;
    g_flushes = 0;
    for (uint32_t b = grid; b-- > 0;) // (the blocks last to first, the waves of a block likewise: nothing may depend on the order)
        for (uint32_t w = CENSUS_WAVES; w-- > 0;) wemu::run_wave(b, [&] { k_b_census(m, n, kb, table.data()); }, w);
    const std::string where = "shape " + std::to_string((int)shape) + " tenants " + std::to_string(n_tenants) + " ids " + std::to_string(n) + " boundary " +
                              std::to_string(bmode) + " grid " + std::to_string(grid);
    for (size_t i = 0; i < want.size(); i++)
        if (table[i] != want[i])
            FAIL("census: the count of slot %zu word %zu is %llu, expected %llu (%s)\n", i / 4, i % 4, table[i], want[i], where.c_str());
    for (size_t i = want.size(); i < table.size(); i++)
        if (table[i] != 0xC0DEC0DEull) FAIL("census: a count was written behind the table: a guard row is damaged (%s)\n", where.c_str());
    const unsigned long long x_flushes = model(slot, grid, cov);
    if (g_flushes != x_flushes) FAIL("flushes: a count of %llu, the model of the runs expects %llu (%s)\n", g_flushes, x_flushes, where.c_str());
    cov.cases++, cov.ids += n;
    return 0;
}

// k_r_census over hand-filled per-id arrays: ids below base_n are bulk-loaded (never counted here), the rest belong to tenant nodes
static int retain_case(std::mt19937_64& rng, Shape shape, uint32_t n_tenants, uint32_t grid_force, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const uint32_t bases[5] = {0, 1, 64, 100, 777};
    const uint32_t base_n = bases[rnd(5)], n_ov = shape == S_RUNS ? 0 : 100 + rnd(1500);
    std::vector<uint32_t> tnode;
    const uint32_t runs[5] = {1, 63, 64, 65, 200};
    if (shape == S_RUNS)
        for (uint32_t t = 0; t < n_tenants; t++) tnode.insert(tnode.end(), runs[t % 5], 1 + 3 * t);
    else
        for (uint32_t i = 0; i < n_ov; i++) tnode.push_back(1 + 3 * (shape == S_ROUND_ROBIN ? i % n_tenants : (shape == S_ONE ? 0 : rnd(n_tenants))));
    const uint32_t n = (uint32_t)tnode.size(), n_ids = base_n + n, id_cap = n_ids + 70, n_nodes = 3 * n_tenants + 2;
    std::vector<uint32_t> id_tnode(id_cap, NONE);
    std::vector<unsigned long long> dead((id_cap + 63) / 64 + 1, 0ull);
    std::vector<uint32_t> slot(n, NONE);
    std::vector<unsigned long long> want(n_nodes, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t id = base_n + i;
        id_tnode[id] = tnode[i] | (rnd(5) == 0 ? ID_SYS : 0u); // '$' topics count
        if (rnd(6) == 0) dead[id >> 6] |= 1ull << (id & 63u);
        else slot[i] = tnode[i], want[tnode[i]]++;
    }
    for (uint32_t id = n_ids; id < id_cap; id++) id_tnode[id] = 1, dead[id >> 6] |= 1ull << (id & 63u); // never handed out
    RetainMut m{};
    m.base_n = base_n, m.id_cap = id_cap, m.id_tnode = id_tnode.data(), m.dead_bits = dead.data();
    const uint32_t grid = grid_force ? std::min(grid_force, census_grid(n)) : census_grid(n);
    std::vector<unsigned long long> table(n_nodes + 8, 0);
    for (size_t i = n_nodes; i < table.size(); i++) table[i] = 0xC0DEC0DEull;
    wemu::grid_size() = grid;
    g_flushes = 0;
    for (uint32_t b = 0; b < grid; b++)
        for (uint32_t w = 0; w < CENSUS_WAVES; w++) wemu::run_wave(b, [&] { k_r_census(m, n_ids, table.data()); }, w);
    const std::string where = "retain shape " + std::to_string((int)shape) + " tenants " + std::to_string(n_tenants) + " base " + std::to_string(base_n) + " ids " +
                              std::to_string(n) + " grid " + std::to_string(grid);
    for (size_t i = 0; i < want.size(); i++)
        if (table[i] != want[i]) FAIL("retain census: the count of node %zu is %llu, expected %llu (%s)\n", i, table[i], want[i], where.c_str());
    for (size_t i = want.size(); i < table.size(); i++)
        if (table[i] != 0xC0DEC0DEull) FAIL("retain census: a count was written behind the table: a guard row is damaged (%s)\n", where.c_str());
    const unsigned long long x_flushes = model(slot, grid, cov);
    if (g_flushes != x_flushes) FAIL("flushes: a count of %llu, the model of the runs expects %llu (%s)\n", g_flushes, x_flushes, where.c_str());
    cov.cases++, cov.ids += n;
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
            for (uint32_t bmode = 0; bmode < 10; bmode++, c++) {
                const uint32_t n_tenants = shape == S_ONE ? 1 : (shape == S_ROUND_ROBIN ? 70 : (shape == S_RUNS ? 10 : 2 + (uint32_t)(rng() % 78)));
                static const uint32_t del_pct[3] = {0, 5, 30}, grids[3] = {0, 1, 2};
                // (the interleaved shape keeps every key under the boundaries that hold everything: turns of 64 distinct tenants)
                const uint32_t deletes = shape == S_ROUND_ROBIN && (bmode == 0 || bmode == 7) ? 0 : del_pct[c % 3], grid_force = grids[(c / 3) % 3];
                if (dist_case(rng, (Shape)shape, n_tenants, deletes, bmode, grid_force, cov) || (bmode < 3 && retain_case(rng, (Shape)shape, n_tenants, grid_force, cov))) {
                    fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                    return 1;
                }
            }
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"turns with one slot", cov.one_slot, 80 * R},
                  {"turns with 64 slots", cov.slots_64, 4 * R},
                  {"carried runs flushed by a slot change", cov.carried_change, 20 * R},
                  {"carried runs flushed at the end", cov.carried_end, 20 * R},
                  {"turns with dead lanes inside a run", cov.dead_inside, 50 * R},
                  {"turns with lanes past n", cov.past_n, 20 * R},
                  {"launches whose waves take several turns", cov.multi_turn, 10 * R},
                  {"launches with a boundary", cov.bounded, 20 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("census emu ok: %llu cases, %llu ids; turns with one slot %llu, with 64 slots %llu, carried runs flushed by a change %llu, at the end %llu, "
           "dead lanes inside a run %llu, lanes past n %llu, multi-turn launches %llu, bounded launches %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.ids, (unsigned long long)cov.one_slot, (unsigned long long)cov.slots_64,
           (unsigned long long)cov.carried_change, (unsigned long long)cov.carried_end, (unsigned long long)cov.dead_inside, (unsigned long long)cov.past_n,
           (unsigned long long)cov.multi_turn, (unsigned long long)cov.bounded);
    return 0;
}
