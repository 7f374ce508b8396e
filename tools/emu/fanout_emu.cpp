// fanout_emu.cpp -- host-side logic test of k_fo_hist and k_fo_scatter (bifromq_amd/csrc/bmq_fanout_kernels.h: the counting sort of the
// fan-out grouping's fast path, which exists only as gfx950 kernels) under the wave64 emulator of wave_emu.h.  Test tooling: the kernels'
// LOGIC -- the gather of the dense group number per pair and the pairs that have none yet, the transposed histogram and its end mark, the
// multi-chunk prefix over the keys with its carry, the row of a tile's first pair behind runs of empty rows, the window of row ends and how
// it moves on, the stable rank among the pairs of a key from one ballot per key bit, the running offsets in LDS, the copy out in whole
// runs -- against a stable sort of the pairs by key written plainly below.  A serial exclusive sum stands where the device runs hipCUB's
// scan.  No index is needed: k_fo_hist reads only dgroup[], dense[] and ids[], which the harness fills directly (group slots, gt_cap for
// shared subscriptions, FO_DEAD_ID, FO_UNSET and slot | FO_NEW).
//
// FanoutFast::tile is a run-time field, so tiles of 64, 128 and 192 pairs run beside the product's 1024: tile borders are cheap and frequent.
// The waves of a workgroup are independent (each owns its LDS slice, no __syncthreads), so they run one after the other, each with its
// wave index (threadIdx.x = wave * 64 + lane).  Before every wave of k_fo_scatter its LDS slice is filled with garbage (k_fo_hist's counters
// are a function static here: they keep what the wave before left, which is garbage of the same kind); guard words follow every output array.
//
// Besides the outputs, the number of cross-lane operations of every k_fo_scatter wave is compared with a model (prefix chunks, segments,
// key bits, moves of the row window): a window that starts too far back or moves on in steps other than 64 rows still finds the right
// rows, only later -- the count is what tells.  The run ends with an `ok` line of coverage counts and fails below their floors.
//
// k_fo_dense and k_fo_groups2 are 1024-thread workgroups with __syncthreads: they do not fit a single-wave emulator and stay covered by
// tests/test_fanout_shapes_gpu.py alone.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/fanout_emu.cpp -o build/fanout_emu && build/fanout_emu [rounds] [seed]
//   -DFANOUT_EMU_KEY_BITS_BIAS=1: the control hands over one key bit too few (a mutant of the control, tests/test_fanout_emu.py)
//   add -fsanitize=address,undefined (ASAN_OPTIONS=detect_stack_use_after_return=0: the lanes are ucontext fibers): the LDS buffer of
//   k_fo_scatter is a heap block of exactly the launch's size here, so a read or write past it is reported
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <random>
#include <string>
#include <vector>

// the device builtins the sources that come along with bmq_dist_kernels.h spell out (as in walk_emu.cpp)
#define __align__(n)
inline uint32_t wemu_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (s & 3u))); }
#define __builtin_amdgcn_alignbyte(hi, lo, s) wemu_alignbyte((hi), (lo), (s))
#define __builtin_amdgcn_readlane(v, l) ((int)bmq::read_lane((uint32_t)(v), (uint32_t)(l)))
#define __builtin_amdgcn_s_getreg(x) 0u
#define __ffs(x) __builtin_ffs(x)
#define __popc(x) __builtin_popcount(x)
namespace bmq {
inline uint32_t lds_word_at(const uint32_t* words, uint32_t rel) {
    uint32_t w;
    memcpy(&w, reinterpret_cast<const uint8_t*>(words) + rel, 4);
    return w;
}
inline void __syncthreads() { // (k_fo_dense / k_fo_groups2 compile along and are never run here: see above)
    fprintf(stderr, "wave_emu: __syncthreads in a single-wave emulator\n");
    abort();
}
static unsigned char* fo_lds = nullptr; // the dynamic LDS of k_fo_scatter: supplied per launch below
} // namespace bmq
using bmq::__syncthreads;
#include "bmq_fanout_kernels.h"

#ifndef FANOUT_EMU_KEY_BITS_BIAS
#define FANOUT_EMU_KEY_BITS_BIAS 0
#endif

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static const uint32_t GUARD = 16, GUARD_WORD = 0xC0DEC0DEu;
template <class T> static std::vector<T> guarded(size_t n, T fill) {
    std::vector<T> v(n + GUARD, fill);
    for (size_t i = n; i < n + GUARD; i++) v[i] = (T)GUARD_WORD;
    return v;
}
template <class T> static bool guard_intact(const std::vector<T>& v) {
    for (size_t i = v.size() - GUARD; i < v.size(); i++)
        if (v[i] != (T)GUARD_WORD) return false;
    return true;
}

struct Coverage {
    uint64_t cases = 0, pairs = 0, tiles = 0, window_moves = 0, multi_chunk = 0, seg_64_keys = 0, seg_one_key = 0, tiles_behind_empty = 0, unset_cases = 0,
             bins_2 = 0, bins_max = 0, rows_over_tile = 0;
};

enum Pattern { P_ONE, P_ROUND_ROBIN, P_RUNS, P_SKEWED, P_SHARED, P_DEAD, P_MIX, P_RANDOM, P_COUNT };

// keys (dense group numbers < n_bins; n_bins - 2: shared, n_bins - 1: dead) of n pairs
static void make_keys(std::mt19937_64& rng, Pattern pat, uint32_t n_bins, uint32_t n, std::vector<uint32_t>& key) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const uint32_t K = n_bins - 2;
    auto live = [&](uint32_t fallback) { return K ? rnd(K) : fallback; };
    const size_t end = key.size() + n;
    while (key.size() < end) {
        const uint32_t left = (uint32_t)(end - key.size());
        switch (pat) {
        case P_ONE: key.insert(key.end(), left, K ? K / 2 : n_bins - 2); break;
        case P_ROUND_ROBIN:
            for (uint32_t i = 0; i < left; i++) key.push_back(K ? i % K : n_bins - 2 + (i & 1u));
            break;
        case P_RUNS: {
            const uint32_t k = live(n_bins - 1), len = std::min(left, 50 + rnd(350));
            key.insert(key.end(), len, k);
            break;
        }
        case P_SKEWED: {
            const double u = (double)(rng() >> 11) / (double)(1ull << 53);
            key.push_back(K ? (uint32_t)(K * u * u * u * u) : n_bins - 2);
            break;
        }
        case P_SHARED: key.insert(key.end(), left, n_bins - 2); break;
        case P_DEAD: key.insert(key.end(), left, n_bins - 1); break;
        case P_MIX: make_keys(rng, (Pattern)rnd(P_MIX), n_bins, std::min(left, 1 + rnd(300)), key); break;
        default: key.push_back(rnd(n_bins)); break;
        }
    }
}

// row lengths of one of the shapes of tests/fanout_cases.py, sized by the tile
static std::vector<uint32_t> make_rows(std::mt19937_64& rng, uint32_t shape, uint32_t tile) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    std::vector<uint32_t> rows;
    auto empty = [&](uint32_t n) { rows.insert(rows.end(), n, 0u); };
    auto small = [&](uint32_t total) {
        const uint32_t pick[8] = {0, 0, 1, 1, 2, 3, 5, 9};
        while (total) {
            const uint32_t n = std::min(total, pick[rnd(8)]);
            rows.push_back(n);
            total -= n;
        }
        empty(rnd(3));
    };
    const uint32_t totals[10] = {1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4097};
    switch (shape) {
    case 0: small(totals[rnd(10)]); break;
    case 1: small(tile * (1 + rnd(4)) + rnd(3) - 1); break;          // totals at the tile's own borders
    case 2: rows.push_back(tile * 2 + tile / 2 + rnd(64)); break;    // one row that holds everything: it spans three tiles
    case 3: rows.insert(rows.end(), tile * 2 + 400 + rnd(100), 1u); break; // every row of length 1
    case 4: {                                                        // runs of empty rows before, between and behind the pairs
        empty(300);
        const uint32_t runs[5] = {63, 64, 65, 129, 1000};
        for (uint32_t i = 0; i < 5; i++) {
            rows.push_back(1 + rnd(9));
            empty(runs[i]);
        }
        rows.push_back(70);
        empty(400);
        break;
    }
    case 5: {                                                        // pairs at multiples of the tile are the first behind a run of empty rows
        const uint32_t runs[4] = {129, 64, 65, 1000};
        for (uint32_t i = 0; i < 4; i++) {
            if (i & 1u) {
                rows.push_back(10);
                empty(63);
                rows.push_back(tile - 10);
            } else rows.push_back(tile);
            empty(runs[i]);
        }
        rows.push_back(1 + rnd(tile));
        empty(rnd(300));
        break;
    }
    default: {                                                       // random mix
        uint32_t total = 0;
        const uint32_t want = 500 + rnd(5000);
        while (total < want) {
            const uint32_t n = rnd(2) ? 0u : (rnd(100) == 0 ? 700 + rnd(800) : 1 + rnd(6));
            rows.push_back(n);
            total += n;
        }
        break;
    }
    }
    return rows;
}

static int one_case(std::mt19937_64& rng, uint32_t n_bins, uint32_t tile, uint32_t shape, Pattern pat, bool with_unset, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const std::vector<uint32_t> row_len = make_rows(rng, shape, tile);
    const uint32_t n_topics = (uint32_t)row_len.size();
    std::vector<uint32_t> row_ptr = guarded<uint32_t>(n_topics + 1, 0u);
    for (uint32_t t = 0; t < n_topics; t++) row_ptr[t + 1] = row_ptr[t] + row_len[t];
    const uint32_t total = row_ptr[n_topics];
    if (total == 0) return 0;
    std::vector<uint32_t> key;
    make_keys(rng, pat, n_bins, total, key);
    // ---- the group table as k_fo_dense leaves it, and a per-id cache that holds every kind of entry
    const uint32_t K = n_bins - 2;
    uint32_t gt_cap = 4;
    while (gt_cap < 2 * K) gt_cap *= 2;
    std::vector<uint8_t> used(gt_cap, 0);
    for (uint32_t k = 0; k < K;) {
        const uint32_t s = rnd(gt_cap);
        if (!used[s]) used[s] = 1, k++;
    }
    std::vector<uint16_t> dense = guarded<uint16_t>(gt_cap, 0);
    std::vector<uint32_t> slot_of(K);
    for (uint32_t s = 0, run = 0; s < gt_cap; s++) {
        dense[s] = (uint16_t)run;
        if (used[s]) slot_of[run++] = s;
    }
    // id i carries key i % n_bins; ids in [id_end, id_cap) were never handed out although their cache words look alive
    const uint32_t per = 4, id_end = n_bins * per, id_cap = id_end + 64;
    std::vector<uint32_t> dgroup = guarded<uint32_t>(id_cap, 0u);
    for (uint32_t i = 0; i < id_cap; i++) {
        const uint32_t k = i % n_bins;
        dgroup[i] = k < K ? slot_of[k] : (k == K ? gt_cap : FO_DEAD_ID);
        if (i >= id_end) dgroup[i] = K ? slot_of[i % K] : gt_cap;
    }
    uint32_t x_need = 0;
    std::vector<uint8_t> id_unset(id_cap, 0);
    if (with_unset) // some live ids have no group slot yet / were mapped in this pass and are not verified
        for (uint32_t i = 0; i < id_end; i++)
            if (i % n_bins < K + 1 && rnd(5) == 0) {
                dgroup[i] = rnd(2) || i % n_bins == K ? FO_UNSET : (dgroup[i] | FO_NEW);
                id_unset[i] = 1;
            }
    std::vector<uint32_t> ids = guarded<uint32_t>(total, 0u);
    for (uint32_t p = 0; p < total; p++) {
        const uint32_t k = key[p];
        if (k == n_bins - 1 && rnd(2)) {
            const uint32_t far[4] = {id_end + rnd(64), id_cap + rnd(1000), 0x7FFFFFFFu, 0xFFFFFFFDu};
            ids[p] = far[rnd(4)];
        } else ids[p] = k + n_bins * rnd(per);
        if (ids[p] < id_end && id_unset[ids[p]]) x_need++, key[p] = n_bins - 1; // (what k_fo_hist files them under until the refill)
    }
    if (with_unset && x_need == 0) return 0;
    // ---- expected: counts per (key, tile), run starts, the pairs in a stable order by key
    const uint32_t n_tiles = (total + tile - 1) / tile;
    const size_t hist_n = (size_t)n_bins * n_tiles;
    std::vector<uint32_t> x_cnt(hist_n + 1, 0), x_start(hist_n + 1, 0);
    for (uint32_t p = 0; p < total; p++) x_cnt[(size_t)key[p] * n_tiles + p / tile]++;
    for (size_t i = 0, run = 0; i <= hist_n; i++) x_start[i] = (uint32_t)run, run += x_cnt[i];
    std::vector<uint32_t> topic_of(total);
    for (uint32_t t = 0; t < n_topics; t++)
        for (uint32_t p = row_ptr[t]; p < row_ptr[t + 1]; p++) topic_of[p] = t;
    std::vector<uint32_t> x_topic(total), x_route(total);
    {
        std::vector<uint32_t> at(n_bins + 1, 0);
        for (uint32_t p = 0; p < total; p++) at[key[p] + 1]++;
        for (uint32_t b = 0; b < n_bins; b++) at[b + 1] += at[b];
        for (uint32_t p = 0; p < total; p++) {
            const uint32_t j = at[key[p]]++;
            x_topic[j] = topic_of[p], x_route[j] = ids[p];
        }
    }
    // ---- the launch, as Fanout::group_fast and DevExec::fo_fast make it
    std::vector<uint16_t> key16 = guarded<uint16_t>(total, (uint16_t)0xABAB);
    std::vector<uint32_t> hist = guarded<uint32_t>(hist_n + 1, 0xDEADBEEFu);
    std::vector<uint32_t> out_topic = guarded<uint32_t>(total, 0xABABABABu), out_route = guarded<uint32_t>(total, 0xABABABABu);
    std::vector<uint32_t> need_fill = guarded<uint32_t>(1, 0u);
    DistIndexMut ix{};
    FanoutState st{};
    st.dgroup = dgroup.data(), st.gt_cap = gt_cap, st.id_cap = id_cap;
    FanoutFast f{};
    f.row_ptr = row_ptr.data(), f.ids = ids.data(), f.n_topics = n_topics, f.total = total, f.id_end = id_end;
    f.tile = tile, f.n_tiles = n_tiles, f.n_bins = n_bins;
    f.key_bits = 1;
    while ((1u << f.key_bits) < f.n_bins) f.key_bits++;
    f.key_bits -= std::min<uint32_t>(f.key_bits - 1, FANOUT_EMU_KEY_BITS_BIAS);
    f.dense = dense.data(), f.key16 = key16.data(), f.hist = hist.data(), f.out_topic = out_topic.data(), f.out_route = out_route.data();
    f.need_fill = need_fill.data();
    const char* what = "";
    std::string where = "n_bins " + std::to_string(n_bins) + " tile " + std::to_string(tile) + " shape " + std::to_string(shape) + " pattern " +
                        std::to_string((int)pat) + " total " + std::to_string(total) + " rows " + std::to_string(n_topics);
    what = where.c_str();
    const uint32_t hist_blocks = (n_tiles + FO_WAVES - 1) / FO_WAVES;
    for (uint32_t b = 0; b < hist_blocks; b++) // (the blocks last to first, the waves of a block likewise: nothing may depend on the order)
        for (uint32_t w = FO_WAVES; w-- > 0;) wemu::run_wave(hist_blocks - 1 - b, [&] { k_fo_hist(ix, st, f); }, w);
    if (need_fill[0] != x_need) FAIL("need_fill: a count of %u pairs without a group slot, expected %u (%s)\n", need_fill[0], x_need, what);
    for (uint32_t p = 0; p < total; p++)
        if (key16[p] != key[p]) FAIL("key16: the row of pair %u (id %u) has key %u, expected %u (%s)\n", p, ids[p], key16[p], key[p], what);
    for (size_t i = 0; i <= hist_n; i++) // (the end mark too: a 0 that the scan turns into the total)
        if (hist[i] != x_cnt[i]) FAIL("hist: the count of word %zu (key %zu tile %zu) is %u, expected %u (%s)\n", i, i / n_tiles, i % n_tiles, hist[i], x_cnt[i], what);
    if (!guard_intact(key16) || !guard_intact(hist) || !guard_intact(need_fill)) FAIL("k_fo_hist wrote behind key16 / hist / need_fill: a guard row is damaged (%s)\n", what);
    if (with_unset) { // the control maps the ids and starts over: nothing else of this launch is used
        cov.unset_cases++;
        return 0;
    }
    for (size_t i = 0, run = 0; i <= hist_n; i++) { // the scan: an exclusive sum in place, the end mark included
        const uint32_t c = hist[i];
        hist[i] = (uint32_t)run, run += c;
    }
    for (size_t i = 0; i <= hist_n; i++)
        if (hist[i] != x_start[i]) FAIL("run start: the row of word %zu is %u, expected %u (%s)\n", i, hist[i], x_start[i], what);
    const uint32_t lds_wave = fo_scatter_lds(n_bins, tile), sc_blocks = (n_tiles + FO_SC_WAVES - 1) / FO_SC_WAVES;
    const uint32_t chunks = fo_scatter_bins(n_bins) / 64;
    for (uint32_t b = 0; b < sc_blocks; b++)
        for (uint32_t w = FO_SC_WAVES; w-- > 0;) {
            const uint32_t blk = (b * 5 + 2) % sc_blocks; // (a scrambled order; every block once when 5 and sc_blocks are coprime, else below)
            std::vector<unsigned char> lds((size_t)FO_SC_WAVES * lds_wave);
            for (auto& c : lds) c = (unsigned char)(0xA0u + (rng() & 0x5Fu));
            fo_lds = lds.data();
            const unsigned long long before = wemu::st().rendezvous;
            wemu::run_wave(blk, [&] { k_fo_scatter(f); }, w);
            fo_lds = nullptr;
            // the cross-lane operations of the wave against the model: 7 per prefix chunk, the hand-over, then per segment 8 per look at the
            // row window (one look + one per move), a ballot of the lanes in range, one per key bit, the leader's offset, the hand-over
            const uint32_t t = blk * FO_SC_WAVES + w;
            unsigned long long x_ops = 0;
            if (t < n_tiles) {
                const uint32_t p0 = t * tile, p1 = std::min(total, p0 + tile);
                uint32_t wbase = topic_of[p0];
                x_ops = 7ull * chunks + 1;
                for (uint32_t s = p0; s < p1; s += 64) {
                    const uint32_t last = topic_of[std::min(p1, s + 64) - 1];
                    uint32_t moves = 0;
                    while (last >= wbase + 64) wbase += 64, moves++;
                    x_ops += 8ull * (1 + moves) + f.key_bits + 3;
                }
            }
            const unsigned long long ops = wemu::st().rendezvous - before;
            if (ops != x_ops) FAIL("cross-lane operations: a count of %llu for tile %u, the model expects %llu (%s)\n", ops, t, x_ops, what);
        }
    if (sc_blocks % 5 == 0) { // (the kernel is idempotent: run the blocks the scrambled order left out)
        std::vector<unsigned char> lds((size_t)FO_SC_WAVES * lds_wave, 0xEE);
        fo_lds = lds.data();
        for (uint32_t b = 0; b < sc_blocks; b++)
            for (uint32_t w = 0; w < FO_SC_WAVES; w++) wemu::run_wave(b, [&] { k_fo_scatter(f); }, w);
        fo_lds = nullptr;
    }
    for (uint32_t j = 0; j < total; j++)
        if (out_topic[j] != x_topic[j] || out_route[j] != x_route[j])
            FAIL("output row %u is (topic %u, route %u), expected (%u, %u) (%s)\n", j, out_topic[j], out_route[j], x_topic[j], x_route[j], what);
    if (!guard_intact(out_topic) || !guard_intact(out_route) || !guard_intact(hist) || !guard_intact(row_ptr) || !guard_intact(ids) || !guard_intact(dgroup) ||
        !guard_intact(dense))
        FAIL("k_fo_scatter wrote behind an array: a guard row is damaged (%s)\n", what);
    // ---- what this case covered
    cov.cases++, cov.pairs += total, cov.tiles += n_tiles;
    cov.bins_2 += n_bins == 2, cov.bins_max += n_bins == FO_MAX_BINS;
    for (uint32_t t = 0; t < n_topics; t++) cov.rows_over_tile += row_len[t] > tile;
    for (uint32_t t = 0; t < n_tiles; t++) {
        const uint32_t p0 = t * tile, p1 = std::min(total, p0 + tile);
        cov.multi_chunk += chunks > 1;
        const uint32_t r = topic_of[p0];
        cov.tiles_behind_empty += t > 0 && r > 0 && row_ptr[r] == p0 && row_ptr[r - 1] == p0;
        uint32_t wbase = r;
        for (uint32_t s = p0; s < p1; s += 64) {
            const uint32_t e = std::min(p1, s + 64);
            while (topic_of[e - 1] >= wbase + 64) wbase += 64, cov.window_moves++;
            if (e - s < 64) continue;
            std::vector<uint32_t> ks(key.begin() + s, key.begin() + e);
            std::sort(ks.begin(), ks.end());
            const size_t distinct = std::unique(ks.begin(), ks.end()) - ks.begin();
            cov.seg_64_keys += distinct == 64, cov.seg_one_key += distinct == 1;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 6;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    Coverage cov;
    const uint32_t tiles[4] = {64, 128, 192, 1024};
    const uint32_t bins[12] = {2, 3, 64, 65, 66, 128, 129, 515, 1025, 1026, 0, 0}; // (0: a random count)
    int c = 0;
    for (int round = 0; round < rounds; round++)
        for (uint32_t shape = 0; shape < 7; shape++)
            for (int pat = 0; pat < P_COUNT; pat++, c++) {
                uint32_t n_bins = bins[(c + round) % 12];
                if (n_bins == 0) n_bins = 2 + (uint32_t)(rng() % (FO_MAX_BINS - 1));
                const uint32_t tile = tiles[(c / 3 + round) % 4];
                const bool with_unset = c % 5 == 2;
                if (one_case(rng, n_bins, tile, shape, (Pattern)pat, with_unset, cov)) {
                    fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                    return 1;
                }
            }
    // the floors: per round at least this much of every path the kernels take rarely
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"window moves", cov.window_moves, 100 * R},          {"tiles with a multi-chunk prefix", cov.multi_chunk, 100 * R},
                  {"segments with 64 distinct keys", cov.seg_64_keys, 20 * R}, {"segments with one key", cov.seg_one_key, 100 * R},
                  {"tiles starting behind an empty run", cov.tiles_behind_empty, 10 * R}, {"launches with unmapped ids", cov.unset_cases, 3 * R},
                  {"cases with 2 bins", cov.bins_2, 2 * R},              {"cases with FO_MAX_BINS bins", cov.bins_max, 2 * R},
                  {"rows longer than a tile", cov.rows_over_tile, 10 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("fanout emu ok: %llu cases, %llu pairs, %llu tiles; window moves %llu, multi-chunk prefixes %llu, segments of 64 keys %llu, of one key %llu, "
           "tiles behind an empty run %llu, launches with unmapped ids %llu, 2 bins %llu, %u bins %llu, rows longer than a tile %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.pairs, (unsigned long long)cov.tiles, (unsigned long long)cov.window_moves,
           (unsigned long long)cov.multi_chunk, (unsigned long long)cov.seg_64_keys, (unsigned long long)cov.seg_one_key, (unsigned long long)cov.tiles_behind_empty,
           (unsigned long long)cov.unset_cases, (unsigned long long)cov.bins_2, FO_MAX_BINS, (unsigned long long)cov.bins_max, (unsigned long long)cov.rows_over_tile);
    return 0;
}
