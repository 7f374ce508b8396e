// caps_emu.cpp -- host-side logic test of the kernels of the fan-out caps over a match CSR (bifromq_amd/csrc/bmq_caps_kernels.h:
// k_caps_classify, k_caps_rows, k_caps_list, k_caps_rank, k_caps_write) under the wave64 emulator of wave_emu.h.  Test tooling: the kernels'
// LOGIC -- the class of a route from the tail of its key, the per-wave counts of a row's classes, the rank of a member among the keys of its
// class and row, the keep decision at the cap, the place of an event, the compaction of the survivors, the row offsets and class counts --
// against the contract written plainly below: per row, the members of a class sorted by key BYTES (std::string order of unsigned bytes), the
// first `cap` kept, the others reported.  Serial inclusive sums stand where the device runs hipCUB's scan.  The harness builds the key pool
// and the reference table of an index directly: no index is built here.
//
// What the cases hold: route ids in an order unrelated to their keys' (a rank by id is wrong almost everywhere); key bytes above 0x7F
// (a signed compare is wrong); keys that share 5, 17 and 40 leading bytes (a compare step is 16); class sizes of 1, 63, 64, 65, 130 and 300 members, so that a
// class ends at, before and behind a wave and spans workgroups; caps of 0, 1, m - 1, m, m + 1 and "none"; rows exactly as long as their
// smaller cap (copied through) and one longer; empty rows, in front, between and behind; dead ids and ids never handed out, in classified
// and in free rows; receiverUrls whose digit prefix is "", "1", "01", "11", "1x"; a caps table of three entries; an event buffer smaller
// than the events.  Workgroups run last to first.  Guard words follow every output array.  The run ends with an `ok` line of coverage counts
// and fails below their floors.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/caps_emu.cpp -o build/caps_emu && build/caps_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <random>
#include <string>
#include <vector>

#include "bmq_caps_kernels.h"

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
    uint64_t cases = 0, rows = 0, free_rows = 0, ranked_rows = 0, at_min = 0, events = 0, dead_classified = 0, dead_free = 0, class_at_wave = 0, rows_over_block = 0,
             truncated = 0, cap_zero = 0, cap_exact = 0, disorder = 0;
};

// a per-item pass as DevExec launches it: min(ceil(n / CAPS_BLOCK), CAPS_BLOCKS) workgroups of four independent waves, last to first
template <class K> static void launch_strided(unsigned long long n, K&& kernel) {
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((n + CAPS_BLOCK - 1) / CAPS_BLOCK, CAPS_BLOCKS);
    wemu::grid_size() = blocks;
    for (uint32_t b = blocks; b-- > 0;)
        for (uint32_t w = CAPS_BLOCK / 64; w-- > 0;) wemu::run_wave(b, kernel, w);
}

struct Route {
    std::string key;
    uint32_t cls; // 0 transient, 1 persistent, 2 group
};

static int one_case(std::mt19937_64& rng, uint32_t shape, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const uint32_t sizes[8] = {1, 2, 63, 64, 65, 130, 300, 7};
    const char* prefixes[3] = {"T\x01" "a/b", "T\x01" "a/b" "0123456789ab", "T\x01" "a/b" "0123456789abcdefghijklmnopqrstuvwxyz0"}; // 5, 17 and 40 shared bytes
    const char* pers_recv[3] = {"1", "01", "1x"};
    const char* trans_recv[4] = {"", "0", "11", "x1"};
    // ---- rows of members by class; every member is a route of its own, ids are dealt out in a shuffled order afterwards
    const uint32_t n_rows = shape == 3 ? 1 + rnd(3) : 4 + rnd(9);
    struct RowPlan {
        uint32_t np, ng, nt, n_dead, caps;
    };
    std::vector<RowPlan> plan(n_rows);
    std::vector<Route> routes;
    std::vector<std::vector<uint32_t>> row_routes(n_rows);
    for (uint32_t r = 0; r < n_rows; r++) {
        RowPlan& p = plan[r];
        const bool empty = shape != 3 && (r == 0 || r + 1 == n_rows || rnd(6) == 0);
        p.np = empty ? 0 : (shape == 3 ? sizes[4 + rnd(3)] : sizes[rnd(8)] % 70);
        p.ng = empty ? 0 : (shape == 3 ? sizes[2 + rnd(5)] : sizes[rnd(8)] % 70);
        p.nt = empty ? 0 : rnd(6);
        p.n_dead = empty ? 0 : rnd(3);
        p.caps = rnd(3);
        const char* pre = prefixes[rnd(3)];
        for (uint32_t k = 0; k < p.np + p.ng + p.nt; k++) {
            const uint32_t cls = k < p.np ? 1u : (k < p.np + p.ng ? 2u : 0u);
            std::string recv = cls == 2 ? "g" : std::string(cls == 1 ? pers_recv[rnd(3)] : trans_recv[rnd(4)]) + std::string("\0", 1) + "inbox";
            // unique, and ordered by bytes that are unrelated to the order the ids are dealt out in; bytes above 0x7F among them
            std::string uniq;
            for (int q = 0; q < 3; q++) uniq.push_back((char)(uint8_t)rnd(256));
            uniq += std::to_string(routes.size());
            std::string key = std::string(pre) + uniq;
            key.push_back(cls == 2 ? (char)(2 + rnd(2)) : (char)1);
            recv += uniq + std::string("\0", 1) + "dk";
            key += recv;
            key.push_back((char)(uint8_t)(recv.size() >> 8));
            key.push_back((char)(uint8_t)recv.size());
            row_routes[r].push_back((uint32_t)routes.size());
            routes.push_back(Route{key, cls});
        }
    }
    // ---- ids: a shuffle of the routes; some ids are dead (their reference is 0), some lie behind id_end
    if (routes.empty()) return 0;
    const uint32_t n_routes = (uint32_t)routes.size(), id_end = n_routes + 4, id_cap = id_end + 8;
    std::vector<uint32_t> id_of(n_routes);
    for (uint32_t i = 0; i < n_routes; i++) id_of[i] = i;
    for (size_t i = id_of.size(); i-- > 1;) std::swap(id_of[i], id_of[rnd(i + 1)]);
    std::vector<uint8_t> kpool(32, 0xEE);
    std::vector<unsigned long long> kref(id_cap, 0ull);
    std::vector<int> class_of_id(id_cap + 16, -1); // -1: dead / never handed out
    std::vector<std::string> key_of_id(id_cap + 16);
    for (uint32_t i = 0; i < n_routes; i++) {
        const uint32_t id = id_of[i];
        const size_t off = kpool.size();
        kpool.insert(kpool.end(), routes[i].key.begin(), routes[i].key.end());
        kref[id] = (unsigned long long)off | ((unsigned long long)routes[i].key.size() << KREF_LEN_SHIFT);
        class_of_id[id] = (int)routes[i].cls;
        key_of_id[id] = routes[i].key;
    }
    kpool.resize(kpool.size() + 32, 0xEE);
    // (ids id_end .. id_cap - 1 get a live-looking reference: only the bound on id_end keeps them dead)
    for (uint32_t id = id_end; id < id_cap; id++) kref[id] = kref[id_of[0]];
    DistIndexMut ix{};
    ix.kpool = kpool.data();
    ix.kref = kref.data();
    ix.id_cap = id_cap;
    // ---- the CSR: a row's ids ascending, its dead ids among them
    std::vector<uint32_t> row_ptr{0}, ids;
    for (uint32_t r = 0; r < n_rows; r++) {
        std::vector<uint32_t> row;
        for (uint32_t i : row_routes[r]) row.push_back(id_of[i]);
        for (uint32_t k = 0; k < plan[r].n_dead; k++) row.push_back(k == 0 ? n_routes + rnd(4) : id_end + rnd(8) + (k - 1) * 8); // unused id / never handed out
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        ids.insert(ids.end(), row.begin(), row.end());
        row_ptr.push_back((uint32_t)ids.size());
    }
    const uint32_t total = (uint32_t)ids.size();
    if (total == 0) return 0;
    // ---- caps: entry 0 binds both classes of some row, entry 1 is exactly a row's length or a class's size, entry 2 never binds one class
    const uint32_t some = rnd(n_rows), len_some = row_ptr[some + 1] - row_ptr[some], INF = 0x7FFFFFFFu;
    const uint32_t around[6] = {0, 1, plan[some].np ? plan[some].np - 1 : 0, plan[some].np, plan[some].np + 1, 3};
    std::vector<int32_t> max_pf{(int32_t)around[rnd(6)], (int32_t)(rnd(2) ? len_some : INF), (int32_t)(rnd(2) ? INF : 2)};
    std::vector<int32_t> max_gf{(int32_t)(rnd(3) ? rnd(5) : plan[some].ng), (int32_t)(rnd(2) ? len_some : plan[some].ng), (int32_t)(rnd(2) ? 1 : INF)};
    std::vector<uint32_t> row_caps(n_rows);
    for (uint32_t r = 0; r < n_rows; r++) row_caps[r] = plan[r].caps;
    const bool no_table = shape == 2; // every row under entry 0
    // ---- expected: the contract, plainly
    std::vector<uint32_t> x_row_ptr{0}, x_ids, x_cc;
    std::vector<int32_t> x_ev;
    for (uint32_t r = 0; r < n_rows; r++) {
        const uint32_t t = no_table ? 0u : row_caps[r], pf = (uint32_t)max_pf[t], gf = (uint32_t)max_gf[t], n = row_ptr[r + 1] - row_ptr[r];
        const bool is_dead_in = [&] {
            for (uint32_t i = row_ptr[r]; i < row_ptr[r + 1]; i++)
                if (ids[i] >= id_end || class_of_id[ids[i]] < 0) return true;
            return false;
        }();
        cov.rows++;
        if (n <= std::min(pf, gf)) {
            x_ids.insert(x_ids.end(), ids.begin() + row_ptr[r], ids.begin() + row_ptr[r + 1]);
            x_row_ptr.push_back((uint32_t)x_ids.size());
            x_cc.push_back(0xFFFFFFFFu), x_cc.push_back(0xFFFFFFFFu);
            cov.free_rows += n > 0, cov.at_min += n > 0 && n == std::min(pf, gf), cov.dead_free += is_dead_in;
            continue;
        }
        cov.dead_classified += is_dead_in;
        cov.at_min += n == std::min(pf, gf) + 1;
        std::vector<uint32_t> member[3];
        for (uint32_t i = row_ptr[r]; i < row_ptr[r + 1]; i++)
            if (ids[i] < id_end && class_of_id[ids[i]] >= 0) member[class_of_id[ids[i]]].push_back(ids[i]);
        std::vector<uint8_t> gone(id_cap + 16, 0);
        bool ranked = false;
        for (uint32_t c = 1; c <= 2; c++) {
            const uint32_t cap = c == 1 ? pf : gf;
            std::vector<uint32_t> by_key = member[c];
            std::sort(by_key.begin(), by_key.end(), [&](uint32_t a, uint32_t b) { return key_of_id[a] < key_of_id[b]; }); // std::string: unsigned bytes, a proper prefix first
            cov.disorder += by_key != member[c];
            cov.cap_zero += cap == 0 && !by_key.empty(), cov.cap_exact += cap == by_key.size() && cap > 0;
            cov.class_at_wave += by_key.size() > cap && (by_key.size() % 64 <= 1 || by_key.size() % 64 == 63);
            for (size_t k = cap; k < by_key.size(); k++) {
                gone[by_key[k]] = 1;
                x_ev.insert(x_ev.end(), {(int32_t)(c - 1), (int32_t)r, (int32_t)by_key[k], (int32_t)cap});
                ranked = true;
            }
            x_cc.push_back((uint32_t)std::min<size_t>(cap, by_key.size()));
        }
        cov.ranked_rows += ranked, cov.rows_over_block += ranked && n > CAPS_BLOCK;
        for (uint32_t i = row_ptr[r]; i < row_ptr[r + 1]; i++)
            if (ids[i] < id_end && class_of_id[ids[i]] >= 0 && !gone[ids[i]]) x_ids.push_back(ids[i]);
        x_row_ptr.push_back((uint32_t)x_ids.size());
    }
    const uint32_t x_n_events = (uint32_t)(x_ev.size() / 4);
    cov.events += x_n_events;
    const uint32_t events_cap = shape == 1 && x_n_events > 1 ? x_n_events / 2 : x_n_events + 3;
    cov.truncated += events_cap < x_n_events;
    // ---- the launches, as Caps::run and DevExec make them
    const std::string where = "shape " + std::to_string(shape) + " rows " + std::to_string(n_rows) + " pairs " + std::to_string(total) + " caps (" + std::to_string(max_pf[0]) + "," +
                              std::to_string(max_gf[0]) + ") (" + std::to_string(max_pf[1]) + "," + std::to_string(max_gf[1]) + ") (" + std::to_string(max_pf[2]) + "," +
                              std::to_string(max_gf[2]) + ")";
    const char* what = where.c_str();
    std::vector<uint8_t> cls(total + GUARD, 0xAB), mode(n_rows + GUARD, 0xAB);
    std::vector<uint32_t> row_cnt = guarded(2 * n_rows, 0), ev_cnt = guarded(2 * n_rows, 0xABABABABu), ev_scan = guarded(2 * n_rows, 0xABABABABu),
                          keep = guarded(total, 0xABABABABu), keep_scan = guarded(total, 0xABABABABu), work = guarded(total, 0xABABABABu), fb_rows = guarded(n_rows, 0xABABABABu),
                          ctr = guarded(CAPS_CTRS, 0), out_row_ptr = guarded(n_rows + 1, 0xABABABABu), out_ids = guarded(x_ids.size(), 0xABABABABu),
                          out_cc = guarded(2 * n_rows, 0xABABABABu), out_ev = guarded(4 * (size_t)events_cap, 0xABABABABu);
    CapsBatch b{};
    b.row_ptr = row_ptr.data(), b.ids = ids.data(), b.n_rows = n_rows, b.total = total, b.id_end = id_end;
    b.row_caps = no_table ? nullptr : row_caps.data(), b.max_pf = max_pf.data(), b.max_gf = max_gf.data(), b.n_caps = 3;
    b.cls = cls.data(), b.mode = mode.data(), b.row_cnt = row_cnt.data(), b.ev_cnt = ev_cnt.data(), b.ev_scan = ev_scan.data(), b.keep = keep.data(), b.keep_scan = keep_scan.data();
    b.work = work.data(), b.fb_rows = fb_rows.data(), b.ctr = ctr.data();
    b.out_row_ptr = out_row_ptr.data(), b.out_ids = out_ids.data(), b.out_class_counts = out_cc.data(), b.out_events = (int32_t*)out_ev.data(), b.events_cap = events_cap;
    launch_strided(total, [&] { k_caps_classify(ix, b); });
    launch_strided(n_rows, [&] { k_caps_rows(b); });
    for (uint32_t s = 0, run = 0; s < 2 * n_rows; s++) ev_scan[s] = (run += ev_cnt[s]);
    launch_strided(total, [&] { k_caps_list(b); });
    if (ctr[CAPS_C_ERR]) FAIL("classify: the error word is %u although every row is sound (%s)\n", ctr[CAPS_C_ERR], what);
    if (ctr[CAPS_C_FALLBACK]) FAIL("harness: a row count of %u left to the host (%s)\n", ctr[CAPS_C_FALLBACK], what);
    if (ctr[CAPS_C_EVENTS] != x_n_events) FAIL("rows: an event count of %u, expected %u (%s)\n", ctr[CAPS_C_EVENTS], x_n_events, what);
    const uint32_t n_work = ctr[CAPS_C_WORK];
    if (n_work > total) FAIL("list: a work count of %u for %u pairs (%s)\n", n_work, total, what);
    if (n_work) {
        const uint32_t blocks = (n_work + CAPS_BLOCK / 64 - 1) / (CAPS_BLOCK / 64);
        wemu::grid_size() = blocks;
        for (uint32_t blk = blocks; blk-- > 0;)
            for (uint32_t w = CAPS_BLOCK / 64; w-- > 0;) wemu::run_wave(blk, [&] { k_caps_rank(ix, b, n_work); }, w);
    }
    for (uint32_t i = 0, run = 0; i < total; i++) {
        if (keep[i] > 1) FAIL("a keep flag of pair %u was never settled: row %u (%s)\n", i, fo_row_of(row_ptr.data(), n_rows, i), what);
        keep_scan[i] = (run += keep[i]);
    }
    if (keep_scan[total - 1] != x_ids.size()) FAIL("keep: a count of %u surviving ids, expected %zu (%s)\n", keep_scan[total - 1], x_ids.size(), what);
    const uint32_t n = std::max(total, n_rows + 1);
    launch_strided(n, [&] { k_caps_write(b, n); });
    for (uint32_t r = 0; r <= n_rows; r++)
        if (out_row_ptr[r] != x_row_ptr[r]) FAIL("offsets: output row %u begins at %u, expected %u (%s)\n", r, out_row_ptr[r], x_row_ptr[r], what);
    for (size_t k = 0; k < x_ids.size(); k++)
        if (out_ids[k] != x_ids[k]) FAIL("ids: place %zu of output row %u holds id %u, expected %u (%s)\n", k, fo_row_of(x_row_ptr.data(), n_rows, (uint32_t)k), out_ids[k], x_ids[k], what);
    for (uint32_t s = 0; s < 2 * n_rows; s++)
        if (out_cc[s] != x_cc[s]) FAIL("class count %u of row %u is %u, expected %u (%s)\n", s & 1, s / 2, out_cc[s], x_cc[s], what);
    for (uint32_t k = 0; k < std::min(events_cap, x_n_events); k++)
        for (uint32_t f = 0; f < 4; f++)
            if ((int32_t)out_ev[4 * k + f] != x_ev[4 * k + f])
                FAIL("event %u of row %d: field %u is %d, expected %d (%s)\n", k, x_ev[4 * k + 1], f, (int32_t)out_ev[4 * k + f], x_ev[4 * k + f], what);
    for (const auto* v : {&row_cnt, &ev_cnt, &ev_scan, &keep, &keep_scan, &work, &fb_rows, &ctr, &out_row_ptr, &out_ids, &out_cc, &out_ev})
        if (!guard_intact(*v)) FAIL("a kernel wrote behind an array: a guard row is damaged (%s)\n", what);
    for (uint32_t k = 0; k < GUARD; k++)
        if (cls[total + k] != 0xAB || mode[n_rows + k] != 0xAB) FAIL("a kernel wrote behind an array: a guard row of the classes is damaged (%s)\n", what);
    cov.cases++;
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
            const uint32_t shape = k % 8 == 5 ? 1 : k % 8 == 6 ? 2 : k % 8 == 7 ? 3 : 0; // 1: a short event buffer, 2: no row_caps, 3: few rows with large classes
            if (one_case(rng, shape, cov)) {
                fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                return 1;
            }
        }
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"rows copied through", cov.free_rows, 8 * R},
                  {"rows with a class over its cap", cov.ranked_rows, 20 * R},
                  {"rows at or one over their smaller cap", cov.at_min, 2 * R},
                  {"events", cov.events, 200 * R},
                  {"classified rows with dead ids", cov.dead_classified, 8 * R},
                  {"free rows with dead ids", cov.dead_free, 3 * R},
                  {"classes over their cap that end at a wave", cov.class_at_wave, 3 * R},
                  {"ranked rows longer than a workgroup", cov.rows_over_block, R},
                  {"event buffers smaller than the events", cov.truncated, 2 * R},
                  {"classes under a cap of 0", cov.cap_zero, 3 * R},
                  {"classes exactly at their cap", cov.cap_exact, 2 * R},
                  {"classes whose id order is not their key order", cov.disorder, 20 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("caps emu ok: %llu cases, %llu rows; copied through %llu, ranked %llu, at the smaller cap %llu, events %llu, dead ids in classified rows %llu / in free rows %llu, "
           "classes at a wave %llu, rows over a workgroup %llu, short event buffers %llu, caps of 0 %llu, classes at their cap %llu, classes out of id order %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.rows, (unsigned long long)cov.free_rows, (unsigned long long)cov.ranked_rows, (unsigned long long)cov.at_min,
           (unsigned long long)cov.events, (unsigned long long)cov.dead_classified, (unsigned long long)cov.dead_free, (unsigned long long)cov.class_at_wave,
           (unsigned long long)cov.rows_over_block, (unsigned long long)cov.truncated, (unsigned long long)cov.cap_zero, (unsigned long long)cov.cap_exact,
           (unsigned long long)cov.disorder);
    return 0;
}
