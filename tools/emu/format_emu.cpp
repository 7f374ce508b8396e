// format_emu.cpp -- host-side logic test of the kernels of the RANGES result format (bifromq_amd/csrc/bmq_format_kernels.h: k_fmt_count,
// k_fmt_emit) under the wave64 emulator of wave_emu.h.  Test tooling: the kernels' LOGIC -- the counts of ranges and side ids per row, the
// order of a row's ranges (ascending by first id up to FMT_SORT_MAX ranges, as matched beyond), the move of the indirect lists into the side
// array of the result, the count of rows whose ranges overlap, the refusal to write into buffers that are too small or for a batch that is
// incomplete -- against a plain restatement of the contract of include/bmq.h (bmq_match_wait_ranges) written below.  Two serial exclusive
// sums stand where the device runs hipCUB's scan.  The harness builds what the walk leaves behind (pair_off, pair_cnt, pairs, the id lists in
// route_pos) directly: no index and no walk run here (tools/emu/walk_emu.cpp runs the same two kernels behind the real walk).
//
// What the cases hold: batches of 0, 1, 255, 256, 257 and 513 rows (the grid is that of enqueue_ranges: n + 1 threads, so n = 256 puts
// t == n into a block of its own); rows of 0, 1, 2, 31, 32, 33 and 64 ranges given ascending, descending and shuffled; empty direct ranges
// (whose begin word is anything: the index keeps a child filter word there) and empty indirect ranges first, last and between others; rows
// of empty ranges only; two and three indirect lists in a row; id sets that interleave, that touch, a list that begins inside the range
// before it; buffers that fit exactly and that are one short, each alone; a batch the walk or the expansion did not complete.  Every array
// the kernels write is pre-filled with garbage, the sums are reused from batch to batch, guard words follow both result buffers.  The run
// ends with an `ok` line of coverage counts and fails below their floors.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/format_emu.cpp -o build/format_emu && build/format_emu [rounds] [seed]
//   add -fsanitize=address,undefined (ASAN_OPTIONS=detect_stack_use_after_return=0: the lanes are ucontext fibers)
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <map>
#include <random>
#include <string>
#include <vector>

// the device builtins the kernels' sources spell out (bmq_dist_kernels.h comes along with bmq_format_kernels.h)
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
} // namespace bmq
#include "bmq_format_kernels.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static const uint32_t GUARD = 16, GUARD_WORD = 0xC0DEC0DEu, FILL = 0xABABABABu;
static const uint32_t CONTRACT_SORT_MAX = 32; // include/bmq.h: "rows of more than 32 ranges: as matched" -- the harness' own figure, not the kernels' FMT_SORT_MAX

struct InRange { // a matched range as the walk leaves it
    bool indirect;
    std::vector<uint32_t> ids; // direct: consecutive
    uint32_t begin_word;       // what an EMPTY direct range carries in `begin` (a child filter word: anything)
};
using Row = std::vector<InRange>;

enum Mode { M_EXACT, M_ROOMY, M_SHORT_RANGES, M_SHORT_SIDE, M_STATUS };

struct Coverage {
    uint64_t batches = 0, rows = 0, ranges = 0, side_ids = 0, rows_32 = 0, rows_over = 0, empty_ranges = 0, empty_only_rows = 0, overlap_rows = 0, multi_list_rows = 0, short_caps = 0,
             incomplete = 0, unsorted_small = 0, batches_two_overlaps = 0, exact = 0;
};

template <class K> static void launch(uint32_t n_threads, K&& kernel) { // workgroups of 256 threads = 4 waves; last to first
    const uint32_t blocks = (n_threads + 255) / 256;
    wemu::grid_size() = blocks;
    for (uint32_t b = blocks; b-- > 0;)
        for (uint32_t w = 4; w-- > 0;) wemu::run_wave(b, kernel, w);
}

static uint32_t first_of(const InRange& r) { return r.ids.front(); }

// the contract, restated: the order a row's ranges must come in -- non-empty ranges only (where empty ones stand among ordered ranges is not
// promised) for rows of up to CONTRACT_SORT_MAX ranges -- and whether the consumer sees an overlap while expanding in that order
static bool expected_overlap(const Row& row, std::vector<const InRange*>& order) {
    order.clear();
    for (auto& r : row)
        if (!r.ids.empty()) order.push_back(&r);
    if (row.size() <= CONTRACT_SORT_MAX) std::stable_sort(order.begin(), order.end(), [](const InRange* a, const InRange* b) { return first_of(*a) < first_of(*b); });
    bool bad = false;
    for (size_t i = 1; i < order.size(); i++) bad |= order[i]->ids.front() <= order[i - 1]->ids.back();
    return bad;
}

static unsigned long long g_sums[4] = {0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull}; // reused from batch to batch

static int run_batch(std::mt19937_64& rng, const std::vector<Row>& rows, Mode mode, uint32_t status, const char* what, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    const uint32_t n = (uint32_t)rows.size();
    // ---- what the walk leaves: the rows' pairs anywhere in the pair buffer, the id lists anywhere in route_pos
    std::vector<uint32_t> place(n);
    for (uint32_t t = 0; t < n; t++) place[t] = t;
    for (size_t i = place.size(); i-- > 1;) std::swap(place[i], place[rnd(i + 1)]);
    std::vector<MatchRange> pairs;
    std::vector<uint32_t> route_pos(3, 0x7E57AB1Eu), pair_off(n + 1, 0x7FFFFFF0u), pair_cnt(n + 1, 0x7FFFFFF0u); // (entry n: never to be read)
    unsigned long long need_r = 0, need_s = 0;
    for (uint32_t t : place) {
        for (uint32_t g = rnd(3); g > 0; g--) pairs.push_back(MatchRange{0x7E57AB1Eu, 0x7E57AB1Eu & ~RANGE_INDIRECT});
        pair_off[t] = (uint32_t)pairs.size(), pair_cnt[t] = (uint32_t)rows[t].size();
        for (auto& r : rows[t]) {
            if (r.indirect) {
                pairs.push_back(MatchRange{(uint32_t)route_pos.size(), (uint32_t)r.ids.size() | RANGE_INDIRECT});
                route_pos.insert(route_pos.end(), r.ids.begin(), r.ids.end());
                if (rnd(2)) route_pos.push_back(0x7E57AB1Eu);
                need_s += r.ids.size();
            } else pairs.push_back(MatchRange{r.ids.empty() ? r.begin_word : r.ids[0], (uint32_t)r.ids.size()});
            need_r++;
        }
    }
    pairs.resize(pairs.size() + 4, MatchRange{0x7E57AB1Eu, 3});
    route_pos.resize(route_pos.size() + 4, 0x7E57AB1Eu);
    const bool incomplete = mode == M_STATUS;
    if ((mode == M_SHORT_RANGES && need_r == 0) || (mode == M_SHORT_SIDE && need_s == 0)) FAIL("harness: a short-buffer case without a row to be short of (%s)\n", what);
    const unsigned long long range_cap = mode == M_SHORT_RANGES ? need_r - 1 : mode == M_ROOMY ? need_r + 1 + rnd(40) : need_r;
    const unsigned long long side_cap = mode == M_SHORT_SIDE ? need_s - 1 : mode == M_ROOMY ? need_s + 1 + rnd(40) : need_s;
    Counters ctr{};
    ctr.status = status;
    std::vector<uint32_t> cnt(2 * (n + 1) + GUARD, FILL), ptr(2 * (n + 1) + GUARD, FILL), out_side(side_cap + GUARD, FILL);
    std::vector<MatchRange> out_ranges(range_cap + GUARD, MatchRange{FILL, FILL});
    for (uint32_t i = 0; i < GUARD; i++) {
        cnt[2 * (n + 1) + i] = ptr[2 * (n + 1) + i] = out_side[side_cap + i] = GUARD_WORD;
        out_ranges[range_cap + i] = MatchRange{GUARD_WORD, GUARD_WORD};
    }
    FmtArgs f{};
    f.ix.route_pos = route_pos.data();
    f.pair_off = pair_off.data(), f.pair_cnt = pair_cnt.data(), f.pairs = pairs.data(), f.ctr = &ctr, f.n_topics = n;
    f.cnt_r = cnt.data(), f.cnt_s = cnt.data() + (n + 1), f.range_ptr = ptr.data(), f.side_ptr = ptr.data() + (n + 1);
    f.out_ranges = out_ranges.data(), f.range_cap = range_cap, f.out_side = out_side.data(), f.side_cap = side_cap, f.sums = g_sums;
    // ---- the launches of enqueue_ranges (bmq_engine.hip)
    launch(n + 1, [&] { k_fmt_count(f); });
    for (uint32_t t = 0; t <= n; t++) {
        const uint32_t xr = t < n && !incomplete ? (uint32_t)rows[t].size() : 0u;
        uint32_t xs = 0;
        if (t < n && !incomplete)
            for (auto& r : rows[t]) xs += r.indirect ? (uint32_t)r.ids.size() : 0u;
        if (f.cnt_r[t] != xr || f.cnt_s[t] != xs) FAIL("k_fmt_count: row %u of %u: a count of %u ranges / %u side ids, expected %u / %u (%s)\n", t, n, f.cnt_r[t], f.cnt_s[t], xr, xs, what);
    }
    for (uint32_t t = 0, run_r = 0, run_s = 0; t <= n; t++) f.range_ptr[t] = run_r, f.side_ptr[t] = run_s, run_r += f.cnt_r[t], run_s += f.cnt_s[t];
    launch(n + 1, [&] { k_fmt_emit(f); });
    // ---- the verdict
    for (uint32_t i = 0; i < GUARD; i++)
        if (cnt[2 * (n + 1) + i] != GUARD_WORD || ptr[2 * (n + 1) + i] != GUARD_WORD || out_side[side_cap + i] != GUARD_WORD || out_ranges[range_cap + i].begin != GUARD_WORD ||
            out_ranges[range_cap + i].count != GUARD_WORD)
            FAIL("a kernel wrote behind an array: guard row %u is damaged (%s)\n", i, what);
    const bool is_short = mode == M_SHORT_RANGES || mode == M_SHORT_SIDE;
    const unsigned long long x_r = incomplete ? 0 : need_r, x_s = incomplete ? 0 : need_s, x_flags = (incomplete ? 2ull : 0ull) | (is_short ? 1ull : 0ull);
    if (g_sums[0] != x_r || g_sums[1] != x_s) FAIL("sums: a count of %llu ranges / %llu side ids, expected %llu / %llu (%s)\n", g_sums[0], g_sums[1], x_r, x_s, what);
    if (g_sums[3] != x_flags) FAIL("sums: a flag count word of %llu, expected %llu (bit 0: buffers too small, bit 1: batch incomplete) (%s)\n", g_sums[3], x_flags, what);
    uint32_t x_bad = 0;
    if (incomplete || is_short) { // nothing may be written to either result buffer
        for (unsigned long long i = 0; i < range_cap; i++)
            if (out_ranges[i].begin != FILL || out_ranges[i].count != FILL) FAIL("output row of ranges written at %llu although the batch is %s (%s)\n", i, incomplete ? "incomplete" : "too large", what);
        for (unsigned long long i = 0; i < side_cap; i++)
            if (out_side[i] != FILL) FAIL("output row of side ids written at %llu although the batch is %s (%s)\n", i, incomplete ? "incomplete" : "too large", what);
    } else {
        std::vector<const InRange*> order;
        std::vector<uint8_t> side_seen(need_s, 0);
        for (uint32_t t = 0; t < n; t++) {
            const Row& row = rows[t];
            const uint32_t rp = f.range_ptr[t], sp0 = f.side_ptr[t], sp1 = f.side_ptr[t + 1];
            const bool over = row.size() > CONTRACT_SORT_MAX;
            x_bad += expected_overlap(row, order);
            // every output range resolved to (kind, ids); indirect lists inside the row's side slice, no two over the same words
            std::vector<std::pair<bool, std::vector<uint32_t>>> got, in;
            std::vector<std::vector<uint32_t>> got_nonempty;
            for (size_t i = 0; i < row.size(); i++) {
                const MatchRange q = out_ranges[rp + i];
                const uint32_t len = q.count & ~RANGE_INDIRECT;
                std::vector<uint32_t> ids;
                if (q.count & RANGE_INDIRECT) {
                    if (q.begin < sp0 || (unsigned long long)q.begin + len > sp1) FAIL("output row %u range %zu: the list [%u, +%u) leaves the row's side slice [%u, %u) (%s)\n", t, i, q.begin, len, sp0, sp1, what);
                    for (uint32_t k = 0; k < len; k++) {
                        if (side_seen[q.begin + k]++) FAIL("output row %u range %zu: side word %u belongs to two lists (%s)\n", t, i, q.begin + k, what);
                        ids.push_back(out_side[q.begin + k]);
                    }
                } else {
                    if (len > (1u << 20)) FAIL("output row %u range %zu: a direct range of %u ids (%s)\n", t, i, len, what);
                    for (uint32_t k = 0; k < len; k++) ids.push_back(q.begin + k);
                }
                if (!ids.empty()) got_nonempty.push_back(ids);
                got.emplace_back((q.count & RANGE_INDIRECT) != 0, ids);
                if (over && (got.back().first != row[i].indirect || ids != row[i].ids))
                    FAIL("output row %u (%zu ranges: as matched) range %zu is not the %zu-th matched range (%s)\n", t, row.size(), i, i, what);
            }
            for (auto& r : row) in.emplace_back(r.indirect, r.ids);
            std::sort(got.begin(), got.end()), std::sort(in.begin(), in.end());
            if (got != in) FAIL("output row %u (%zu ranges): the id lists are not those of the matched ranges (%s)\n", t, row.size(), what);
            if (got_nonempty.size() != order.size()) FAIL("output row %u: %zu non-empty ranges, expected %zu (%s)\n", t, got_nonempty.size(), order.size(), what);
            for (size_t i = 0; i < order.size(); i++)
                if (got_nonempty[i] != order[i]->ids)
                    FAIL("output row %u (%zu ranges): order: non-empty range %zu begins with id %u, expected %u (%s)\n", t, row.size(), i, got_nonempty[i][0], order[i]->ids[0], what);
        }
        for (unsigned long long i = 0; i < need_s; i++)
            if (!side_seen[i]) FAIL("output row of side ids: word %llu of %llu belongs to no list (%s)\n", i, need_s, what);
    }
    if (g_sums[2] != x_bad) FAIL("sums: a count of %llu rows whose ranges overlap, expected %u (%s)\n", g_sums[2], x_bad, what);
    // ---- coverage
    cov.batches++, cov.rows += n, cov.ranges += x_r, cov.side_ids += x_s, cov.short_caps += is_short, cov.incomplete += incomplete, cov.exact += mode == M_EXACT;
    if (!incomplete && !is_short) {
        cov.overlap_rows += x_bad, cov.batches_two_overlaps += x_bad >= 2;
        for (auto& row : rows) {
            uint32_t lists = 0, empties = 0;
            for (auto& r : row) lists += r.indirect && !r.ids.empty(), empties += r.ids.empty();
            cov.rows_32 += row.size() == CONTRACT_SORT_MAX, cov.rows_over += row.size() > CONTRACT_SORT_MAX, cov.empty_ranges += empties, cov.empty_only_rows += !row.empty() && empties == row.size();
            cov.multi_list_rows += lists >= 2;
            bool asc = true;
            uint32_t last = 0, have = 0;
            for (auto& r : row)
                if (!r.ids.empty()) asc = asc && (!have || r.ids[0] > last), last = r.ids[0], have = 1;
            cov.unsorted_small += !asc && row.size() <= CONTRACT_SORT_MAX;
        }
    }
    return 0;
}

// ---- case builders
static InRange direct(uint32_t begin, uint32_t count) {
    InRange r{false, {}, begin};
    for (uint32_t k = 0; k < count; k++) r.ids.push_back(begin + k);
    return r;
}
static InRange list(std::vector<uint32_t> ids) { return InRange{true, std::move(ids), 0}; }

// a row of k ranges over disjoint id sets with distinct first ids: direct ranges, lists, groups of two or three lists whose ids interleave, ranges
// that touch the one before; a few of them empty; in ascending (0), descending (1) or shuffled (2) order
static Row random_row(std::mt19937_64& rng, uint32_t k, uint32_t order, bool allow_overlap, bool allow_empty) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    Row row;
    uint32_t cursor = rnd(1000);
    while (row.size() < k) {
        const uint32_t kind = rnd(10);
        if (allow_empty && kind == 0) {
            row.push_back(rnd(2) ? list({}) : direct(rnd(3) ? (uint32_t)rng() : rnd(4), 0));
            continue;
        }
        cursor += rnd(3) == 0 ? 0 : 1 + rnd(50); // (0: touches the range before it)
        if (allow_overlap && kind == 1 && row.size() + 2 <= k) { // two or three lists dealt from one run of ids
            const uint32_t m = row.size() + 3 <= k && rnd(2) ? 3 : 2;
            std::vector<std::vector<uint32_t>> l(m);
            for (uint32_t i = 0, nn = 2 * m + rnd(6); i < nn; i++) l[i < m ? i : rnd(m)].push_back(cursor), cursor += 1 + rnd(3);
            for (auto& ids : l) row.push_back(list(ids));
        } else if (kind < 5) {
            std::vector<uint32_t> ids;
            for (uint32_t i = 0, nn = 1 + rnd(5); i < nn; i++) ids.push_back(cursor), cursor += 1 + rnd(4);
            row.push_back(list(ids));
        } else {
            const uint32_t c = 1 + rnd(6);
            row.push_back(direct(cursor, c));
            cursor += c;
        }
    }
    if (order == 1) std::reverse(row.begin(), row.end());
    if (order == 2)
        for (size_t i = row.size(); i-- > 1;) std::swap(row[i], row[rnd(i + 1)]);
    return row;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 6;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    Coverage cov;
    int c = 0;
    std::string name;
#define RUN(rows, mode, status, ...)                                                                                                    \
    do {                                                                                                                                \
        char nm[200];                                                                                                                   \
        snprintf(nm, sizeof nm, __VA_ARGS__);                                                                                           \
        name = std::string(nm) + "; case " + std::to_string(c) + ", rounds " + std::to_string(rounds) + " seed " + std::to_string(seed); \
        if (run_batch(rng, rows, mode, status, name.c_str(), cov)) return 1;                                                            \
        c++;                                                                                                                            \
    } while (0)
    const uint32_t row_sizes[7] = {0, 1, 2, 31, 32, 33, 64};
    // ---- directed: every batch size, rows of every size in every order
    for (uint32_t n : {0u, 1u, 255u, 256u, 257u, 513u}) {
        std::vector<Row> rows;
        for (uint32_t t = 0; t < n; t++) rows.push_back(random_row(rng, n == 1 ? 3 : (t % 5 == 0 ? row_sizes[(t / 5) % 7] : rnd(9)), t % 3, true, true));
        RUN(rows, M_EXACT, 0u, "directed: a batch of %u rows, buffers that fit exactly", n);
        RUN(rows, M_ROOMY, (uint32_t)(ST_NOSPACE | ST_WANT_MIXED), "directed: a batch of %u rows, roomy buffers, a status that leaves the ranges valid", n);
    }
    for (uint32_t order = 0; order < 3; order++) {
        std::vector<Row> rows;
        for (uint32_t k : row_sizes) rows.push_back(random_row(rng, k, order, false, false));
        RUN(rows, M_EXACT, 0u, "directed: rows of 0, 1, 2, 31, 32, 33, 64 ranges, order %u, disjoint and apart", order);
        rows.clear();
        for (uint32_t k : row_sizes) rows.push_back(random_row(rng, k, order, true, true));
        RUN(rows, M_EXACT, 0u, "directed: rows of 0, 1, 2, 31, 32, 33, 64 ranges, order %u, interleaved lists and empty ranges", order);
    }
    { // empty ranges first, last and between; rows of empty ranges only; the begin word of an empty direct range is anything
        std::vector<Row> rows;
        for (uint32_t word : {0u, 7u, 0xFFFFFFFFu, 0x80000001u})
            for (int ind = 0; ind < 2; ind++) {
                auto E = [&] { return ind ? list({}) : direct(word, 0); };
                rows.push_back({E(), direct(10, 3), direct(5, 2)});
                rows.push_back({direct(10, 3), direct(5, 2), E()});
                rows.push_back({direct(10, 3), E(), direct(5, 2)});
                rows.push_back({direct(5, 2), E(), direct(10, 3)});
                rows.push_back({list({20, 22}), E(), direct(10, 3), E(), list({4, 30})});
                rows.push_back({E()});
                rows.push_back({E(), E(), list({}), direct(word, 0)});
            }
        RUN(rows, M_EXACT, 0u, "directed: empty ranges first, last, between; rows of empty ranges only");
    }
    { // several lists in a row; interleaving and touching sets; a list that begins inside the range before it
        std::vector<Row> rows;
        rows.push_back({list({7, 9}), list({1, 3})});
        rows.push_back({list({7, 9}), list({1, 3}), list({4, 5, 6})});
        rows.push_back({list({1, 5, 9}), list({2, 6})});                 // interleaved
        rows.push_back({list({2, 6}), direct(3, 2), list({1, 9})});      // interleaved, three ways
        rows.push_back({direct(0, 5), direct(5, 5), list({10, 11})});    // touching, disjoint
        rows.push_back({list({10, 11}), direct(5, 5), direct(0, 5)});    // ... given descending
        rows.push_back({direct(10, 10), list({15, 40})});                // the list's first id lies inside the range before it
        rows.push_back({list({15, 40}), direct(10, 10)});
        rows.push_back({direct(10, 10), list({19, 40})});                // ... at its very last id
        rows.push_back({direct(10, 10), list({20, 40})});                // ... and just behind it: no overlap
        rows.push_back({list({10, 12, 14}), list({14 + 1, 16})});        // a list that touches the list before it
        rows.push_back({list({10, 12, 14}), list({13, 16})});            // ... that begins below its last id
        RUN(rows, M_EXACT, 0u, "directed: lists, interleaving, touching sets");
    }
    { // buffers one short, each alone; a batch that is incomplete
        std::vector<Row> rows;
        for (uint32_t t = 0; t < 300; t++) rows.push_back(random_row(rng, 1 + rnd(6), 2, true, true));
        rows.push_back({list({3, 5}), direct(1, 1)});
        RUN(rows, M_EXACT, 0u, "directed: 301 rows, exact fit");
        RUN(rows, M_SHORT_RANGES, 0u, "directed: 301 rows, the range buffer one short");
        RUN(rows, M_SHORT_SIDE, 0u, "directed: 301 rows, the side buffer one short");
        for (uint32_t st : {(uint32_t)ST_NEED_PAIRS, (uint32_t)ST_NEED_SLOW, (uint32_t)ST_NEED_SCRATCH, (uint32_t)ST_NEED_SPILL, (uint32_t)ST_RERUN, (uint32_t)ST_RANGE,
                            (uint32_t)(ST_RANGE | ST_NOSPACE)})
            RUN(rows, M_STATUS, st, "directed: 301 rows, Counters.status %u: the batch is incomplete", st);
        RUN(rows, M_ROOMY, 0u, "directed: 301 rows, behind the refused batches");
    }
    // ---- random rounds
    for (int round = 0; round < rounds; round++)
        for (uint32_t k = 0; k < 12; k++) {
            const uint32_t ns[6] = {1, 7, 64, 255, 256, 300};
            const uint32_t n = ns[rnd(6)];
            std::vector<Row> rows;
            for (uint32_t t = 0; t < n; t++) rows.push_back(random_row(rng, rnd(6) == 0 ? row_sizes[rnd(7)] : rnd(5) == 0 ? 25 + rnd(16) : rnd(9), rnd(3), true, true));
            unsigned long long need_r = 0, need_s = 0;
            for (auto& row : rows)
                for (auto& r : row) need_r++, need_s += r.indirect ? r.ids.size() : 0;
            const uint32_t m = rnd(8);
            if (m == 0 && need_r) RUN(rows, M_SHORT_RANGES, 0u, "random: %u rows, the range buffer one short", n);
            else if (m == 1 && need_s) RUN(rows, M_SHORT_SIDE, 0u, "random: %u rows, the side buffer one short", n);
            else if (m == 2) RUN(rows, M_STATUS, rnd(2) ? (uint32_t)ST_RANGE : (uint32_t)ST_NEED_PAIRS << rnd(2), "random: %u rows, an incomplete batch", n);
            else RUN(rows, m & 1 ? M_EXACT : M_ROOMY, rnd(2) ? (uint32_t)ST_NOSPACE : 0u, "random: %u rows", n);
        }
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"rows of exactly 32 ranges", cov.rows_32, 6}, {"rows of more than 32 ranges", cov.rows_over, 12}, {"empty ranges", cov.empty_ranges, 100},
                  {"rows of empty ranges only", cov.empty_only_rows, 4}, {"rows whose ranges overlap", cov.overlap_rows, 50}, {"batches with two and more such rows", cov.batches_two_overlaps, 5},
                  {"rows with two and more lists", cov.multi_list_rows, 100}, {"rows of up to 32 ranges given out of order", cov.unsorted_small, 100},
                  {"batches one short of a buffer", cov.short_caps, 2}, {"incomplete batches", cov.incomplete, 7}, {"batches that fit exactly", cov.exact, 10}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds, (unsigned long long)seed);
            return 1;
        }
    printf("format emu ok: %llu batches, %llu rows, %llu ranges, %llu side ids; rows of 32 ranges %llu, of more %llu, empty ranges %llu, rows of empty ranges only %llu, "
           "overlapping rows %llu, rows with several lists %llu, unordered rows of up to 32 ranges %llu, short buffers %llu, incomplete batches %llu, exact fits %llu\n",
           (unsigned long long)cov.batches, (unsigned long long)cov.rows, (unsigned long long)cov.ranges, (unsigned long long)cov.side_ids, (unsigned long long)cov.rows_32,
           (unsigned long long)cov.rows_over, (unsigned long long)cov.empty_ranges, (unsigned long long)cov.empty_only_rows, (unsigned long long)cov.overlap_rows,
           (unsigned long long)cov.multi_list_rows, (unsigned long long)cov.unsorted_small, (unsigned long long)cov.short_caps, (unsigned long long)cov.incomplete, (unsigned long long)cov.exact);
    return 0;
}
