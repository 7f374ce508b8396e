// retain_dyn_emu.cpp -- host-side logic test of the kernels that answer a retain match on a CHURNED index (bifromq_amd/csrc/bmq_retain_kernels.h:
// dead ids inside the bulk-loaded id space, an overlay trie beside it) under the wave64 emulator of wave_emu.h.  Test tooling, three parts:
//   A  the kernels BEHIND the walks -- k_retain_sums, k_retain_rowptr_dyn, k_retain_expand_dyn, k_limit_select, k_limit_compact, k_limit_count_live,
//      k_limit_copy_live -- on range lists the harness writes itself (two lists per row, a dead bitmap with its rank directory, expire_at), against a
//      plain loop over ids: directed cases for every boundary the kernels have (RXD_SHORT, ranges across bitmap words, the first / last word masks of
//      a streamed range, the four-word loop and its remainder, base_n inside a word, 64-range chunks, LIM_FAST, the cursor over two lists, expiry at
//      equality, super-block borders) and random ones;
//   B  retain_walk_body itself -- <false, true> (k_retain_overlay) and <true> (k_retain_walk_deep) -- on indexes the product's own host code makes
//      (RetainIndexHost bulk load, then RetainDyn<HostExec> batches: adds, removes, re-adds), against a brute force over the live topic strings;
//   C  the chain the engine launches: retain_walk_rounds<8, DYN> + the overlay body + the deep pass + sums, row pointers, expansion -- the place where
//      the live counts of the walks and the bitmap arithmetic of the expansion must agree.
// Every kernel run here is a one-wave workgroup or a workgroup of INDEPENDENT waves (k_retain_expand_dyn: a row per wave; the 256-thread limit kernels:
// a row per thread), so __syncthreads() is the wave's rendezvous in this file.  The run ends with one `retain dyn emu ok:` line of the paths it took and
// fails (`coverage:`) if one of them was not reached.  tests/test_retain_dyn_emu.py keeps the harness honest with a table of single-line mutants.
//   g++ -O1 -g -std=c++17 [-DBMQ_R_FRONT=8 -DBMQ_R_OUT=8 -DBMQ_OV_OUT=8] -I bifromq_amd/csrc -I tools/emu tools/emu/retain_dyn_emu.cpp bifromq_amd/csrc/bmq_retain.cpp
//       bifromq_amd/csrc/bmq_codec.cpp -o build/retain_dyn_emu -pthread && build/retain_dyn_emu [cases] [seed]
//   add -fsanitize=address,undefined (ASAN_OPTIONS=detect_stack_use_after_return=0: the lanes are ucontext fibers): LDS arrays are function statics here, so a read or
//   write past one is reported (none at either geometry; OV_OUT must hold a whole wave's matches, hence 64 in the small one); UBSan names rw_seg's `m >> off` with
//   off == 64 in bmq_rwalk_kernel.h -- the slot behind the last lane handed out, whose n == 0 masks the result to 0
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "bmq_codec.h"
#include "bmq_dist_index.h"
#include "bmq_exec_host.h"

// the device builtins the kernels' sources spell out
#define __align__(n)
inline uint32_t wemu_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (s & 3u))); }
#define __builtin_amdgcn_alignbyte(hi, lo, s) wemu_alignbyte((hi), (lo), (s))
#define __builtin_amdgcn_readlane(v, l) ((int)bmq::read_lane((uint32_t)(v), (uint32_t)(l)))
#define __builtin_amdgcn_s_getreg(x) 0u
#define __ffs(x) __builtin_ffs(x)
#define __popc(x) __builtin_popcount(x)
// (see the head of the file: one-wave workgroups and workgroups of independent waves only)
#define __syncthreads() bmq::wave_sync()
#define __threadfence_block() ((void)0)
namespace bmq {
inline uint32_t lds_word_at(const uint32_t* words, uint32_t rel) {
    uint32_t w;
    memcpy(&w, reinterpret_cast<const uint8_t*>(words) + rel, 4);
    return w;
}
} // namespace bmq
#include "bmq_retain_dyn.h"
#include "bmq_retain_kernels.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static std::map<std::string, unsigned long long> g_cov;
static void hit(const char* what, unsigned long long n = 1) { g_cov[what] += n; }

static std::vector<std::string> split(std::string_view s, char sep) {
    std::vector<std::string> out;
    size_t b = 0;
    for (size_t i = 0; i <= s.size(); i++)
        if (i == s.size() || s[i] == sep) {
            out.emplace_back(s.substr(b, i - b));
            b = i + 1;
        }
    return out;
}
// a wildcard in the first level never matches a '$' topic; '#' also matches the level it hangs off (rwalk_emu.cpp)
static bool filter_matches(const std::vector<std::string>& f, const std::vector<std::string>& t) {
    for (size_t i = 0; i < f.size(); i++) {
        const bool wild0 = i == 0 && !t.empty() && !t[0].empty() && t[0][0] == '$';
        if (f[i] == "#" && i + 1 == f.size()) return !wild0;
        if (i >= t.size()) return false;
        if (f[i] == "+") {
            if (wild0) return false;
            continue;
        }
        if (f[i] != t[i]) return false;
    }
    return f.size() == t.size();
}

constexpr uint32_t CANARY = 0xCACACACAu;

// ---- what the walks leave behind: two range lists per row ----------------------------------------------------------------------------------
struct Lists {
    uint32_t n = 0;
    std::vector<uint32_t> off1, cnt1, rc1, off2, cnt2, rc2;
    std::vector<MatchRange> p1, p2;
    bool has_ov = false;
    RetainOvList ov() const { return has_ov ? RetainOvList{off2.data(), cnt2.data(), rc2.data(), p2.data()} : RetainOvList{nullptr, nullptr, nullptr, nullptr}; }
};
struct Back { // what k_retain_sums / k_retain_rowptr_dyn / k_retain_expand_dyn produced
    std::vector<uint32_t> row_ptr, out, sort_list;
    std::vector<unsigned long long> wave_sums, super_sums;
    unsigned long long total = 0;
    Counters ctr{};
};
static BatchArgs batch_of(Lists& L, Back& B) {
    BatchArgs a{};
    a.n_topics = L.n;
    a.tpw_shift = 6;
    a.n_blocks = (L.n + 63) / 64;
    a.pair_off = L.off1.data(), a.pair_cnt = L.cnt1.data(), a.route_cnt = L.rc1.data(), a.pairs = L.p1.data();
    a.wave_sums = B.wave_sums.data(), a.super_sums = B.super_sums.data();
    a.ctr = &B.ctr;
    return a;
}
static void run_backend(Lists& L, const unsigned long long* dead_bits, const uint32_t* dead_rank, uint32_t base_n_arg, uint32_t sort_cap, unsigned long long out_cap,
                        size_t out_alloc, uint32_t preset, Back& B) {
    const uint32_t n = L.n, n_blocks = (n + 63) / 64;
    B = Back{};
    B.row_ptr.assign(n + 2, CANARY), B.out.assign(out_alloc + 64, CANARY), B.sort_list.assign(sort_cap + 4, CANARY);
    B.wave_sums.assign(n_blocks + 1, 0xABABull), B.super_sums.assign(((n_blocks >> SUPER_SHIFT) + 1) * SUPER_STRIDE, 0);
    B.ctr.status = preset;
    BatchArgs a = batch_of(L, B);
    a.sort_list = B.sort_list.data(), a.sort_cap = sort_cap;
    a.out_row_ptr = B.row_ptr.data(), a.out_ids = B.out.data(), a.out_capacity = out_cap, a.out_total = &B.total;
    const RetainOvList ov = L.ov();
    wemu::grid_size() = n_blocks;
    for (uint32_t blk = 0; blk < n_blocks; blk++) wemu::run_wave(blk, [&]() { k_retain_sums(a, ov); });
    for (uint32_t blk = 0; blk < n_blocks; blk++) wemu::run_wave(blk, [&]() { k_retain_rowptr_dyn(a, ov); });
    const uint32_t xg = (n + RXD_WAVES - 1) / RXD_WAVES;
    wemu::grid_size() = xg;
    // (the last row first: what a wave writes behind its row's end then lands on ids that are already there, and stays for the row check to see --
    // in ascending order the next row's wave would tidy it away)
    for (uint32_t blk = xg; blk-- > 0;)
        for (uint32_t w = RXD_WAVES; w-- > 0;) wemu::run_wave(blk, [&]() { k_retain_expand_dyn(a, ov, dead_bits, dead_rank, base_n_arg); }, w);
}
// rows[i]: the ids of row i in the order the lists name them (exact) or ascending (sorted_only: rows the expansion lists are sorted here first)
static int check_backend(const char* what, const Lists& L, const Back& B, const std::vector<std::vector<uint32_t>>& rows, bool sorted_only, size_t out_alloc) {
    const uint32_t n = L.n;
    if (B.ctr.status) FAIL("%s: row check: status %#x\n", what, B.ctr.status);
    unsigned long long at = 0;
    std::vector<unsigned long long> ws((n + 63) / 64, 0), ss(B.super_sums.size(), 0);
    std::set<uint32_t> listed(B.sort_list.begin(), B.sort_list.begin() + std::min<size_t>(B.ctr.sort_count, B.sort_list.size() - 4));
    if (listed.size() != B.ctr.sort_count) FAIL("%s: listing: %u rows counted, %zu distinct rows listed\n", what, B.ctr.sort_count, listed.size());
    for (uint32_t i = 0; i < n; i++) {
        if (B.row_ptr[i] != at) FAIL("%s: row %u begins at %u, expected %llu\n", what, i, B.row_ptr[i], at);
        std::vector<uint32_t> got(B.out.begin() + at, B.out.begin() + at + rows[i].size());
        const bool asc = std::adjacent_find(got.begin(), got.end(), std::greater_equal<uint32_t>()) == got.end();
        if (!asc && !listed.count(i)) FAIL("%s: listing: row %u (%zu ids) is not ascending and not on the sort list\n", what, i, got.size());
        if (asc && listed.count(i)) FAIL("%s: listing: row %u (%zu ids) is ascending and on the sort list\n", what, i, got.size());
        if (!asc) hit("A rows listed for the sort"), std::sort(got.begin(), got.end());
        std::vector<uint32_t> want = rows[i];
        if (sorted_only || !asc) std::sort(want.begin(), want.end());
        if (got != want) {
            fprintf(stderr, "%s: row %u differs (%zu ids):", what, i, want.size());
            for (size_t k = 0; k < want.size(); k++)
                if (got[k] != want[k]) {
                    fprintf(stderr, " at %zu got %u expected %u\n", k, got[k], want[k]);
                    break;
                }
            return 1;
        }
        ws[i / 64] += rows[i].size(), ss[(size_t)(i / 64 >> SUPER_SHIFT) * SUPER_STRIDE] += rows[i].size();
        at += rows[i].size();
    }
    if (B.row_ptr[n] != at || B.total != at || B.ctr.total_ids != at) FAIL("%s: row %u (the total): %u / %llu / %llu, expected %llu\n", what, n, B.row_ptr[n], B.total, B.ctr.total_ids, at);
    if (B.row_ptr[n + 1] != CANARY) FAIL("%s: row pointer written behind row %u\n", what, n);
    for (size_t k = at; k < out_alloc + 64; k++)
        if (B.out[k] != CANARY) FAIL("%s: id %u written behind the last row (at %zu, total %llu)\n", what, B.out[k], k, at);
    for (size_t k = 0; k < ws.size(); k++)
        if (B.wave_sums[k] != ws[k]) FAIL("%s: sum of the row block %zu is %llu, expected %llu\n", what, k, B.wave_sums[k], ws[k]);
    if (B.super_sums != ss) FAIL("%s: the super-block sums of the row counts differ\n", what);
    return 0;
}

// ---- Part A ---------------------------------------------------------------------------------------------------------------------------------
struct CaseA {
    std::string name;
    uint32_t base_n = 0, n_ids = 0; // ids [0, base_n) are bulk-loaded, [base_n, n_ids) the overlay's
    std::vector<std::vector<MatchRange>> bulk, ov;
    std::vector<uint8_t> dead; // [n_ids]; only ids below base_n
    std::vector<unsigned long long> expire;
    std::vector<uint32_t> limit, limit2;
    unsigned long long now = 1000000;
    bool big = false;    // super-block cases: the CSR kernels only
    bool low_ov = false; // the second list may name bulk-loaded ids (the product never does)
    size_t rows() const { return bulk.size(); }
};
static const uint32_t LENS[9] = {1, 2, 15, 16, 17, 63, 64, 65, 400}, OFFS[4] = {0, 1, 48, 63};
static const uint32_t LIMS[7] = {0, 1, 63, 64, 10, 65, 0xFFFFFFFFu}, LIMS2[7] = {65, 0xFFFFFFFFu, 0, 1, 63, 64, 10};

static void finish_case(CaseA& c, int expire_mode, std::mt19937_64& rng) {
    c.ov.resize(c.rows());
    c.dead.resize(c.n_ids, 0);
    c.expire.assign(c.n_ids, RETAIN_NEVER);
    for (size_t i = 0; i < c.rows(); i++) {
        for (size_t list = 0; list < 2; list++)
            for (auto& r : list ? c.ov[i] : c.bulk[i])
                for (uint32_t o = 0; o < r.count; o++) {
                    unsigned long long& e = c.expire[r.begin + o];
                    if (expire_mode == 1 && o < 64) e = c.now - 5;
                    if (expire_mode == 2 && o < 128) e = c.now - 5;
                    if (expire_mode == 3 && e == RETAIN_NEVER) {
                        const unsigned long long pick[6] = {c.now, c.now + 1, c.now - 1, RETAIN_NEVER, 1, c.now + 1};
                        e = pick[rng() % 6];
                    }
                }
    }
    for (uint32_t id = 0; id < c.n_ids; id++)
        if (c.dead[id]) c.expire[id] = 0;
    if (c.limit.empty())
        for (size_t i = 0; i < c.rows(); i++) c.limit.push_back(LIMS[(i + c.rows()) % 7]), c.limit2.push_back(LIMS2[(i + c.base_n) % 7]);
}

static int run_case(CaseA& c) {
    const uint32_t n = (uint32_t)c.rows();
    const char* what = c.name.c_str();
    // the dead bitmap: bits from n_ids on are set; the rank directory in front of every word (and one behind the last)
    const uint32_t words = c.n_ids / 64 + 2;
    std::vector<unsigned long long> bits(words, 0);
    std::vector<uint32_t> rank(words + 1, 0);
    bool use_dead = false;
    for (uint32_t id = 0; id < words * 64; id++)
        if (id >= c.n_ids || c.dead[id]) bits[id >> 6] |= 1ull << (id & 63u);
    for (uint32_t id = 0; id < c.n_ids; id++) {
        if (c.dead[id] && id >= c.base_n) FAIL("%s: generator: overlay id %u is dead\n", what, id);
        use_dead |= c.dead[id] != 0;
    }
    for (uint32_t w = 0; w < words; w++) rank[w + 1] = rank[w] + (uint32_t)__builtin_popcountll(bits[w]);
    hit(use_dead ? "A cases with dead ids" : "A cases without dead ids (base_n passed as 0)");
    // the two lists, with stale entries between the rows' slices; the model of every row
    Lists L;
    L.n = n, L.has_ov = false;
    for (auto& r : c.ov) L.has_ov |= !r.empty();
    if (c.name.find("no overlay list") != std::string::npos) L.has_ov = false;
    L.off1.resize(n), L.cnt1.resize(n), L.rc1.resize(n), L.off2.resize(n), L.cnt2.resize(n), L.rc2.resize(n);
    std::vector<std::vector<uint32_t>> rows(n);
    for (uint32_t i = 0; i < n; i++) {
        for (int list = 0; list < 2; list++) {
            auto& src = list ? c.ov[i] : c.bulk[i];
            auto& dst = list ? L.p2 : L.p1;
            for (uint32_t g = 0; g < (i * 7 + list) % 3; g++) dst.push_back(MatchRange{0xDEAD0000u, 0xFFFFu});
            (list ? L.off2 : L.off1)[i] = (uint32_t)dst.size();
            (list ? L.cnt2 : L.cnt1)[i] = (uint32_t)src.size();
            uint32_t live = 0, prev_end = 0;
            for (size_t k = 0; k < src.size(); k++) {
                const MatchRange r = src[k];
                if (r.count == 0 || r.begin + r.count > c.n_ids) FAIL("%s: generator: range [%u, +%u)\n", what, r.begin, r.count);
                if (list == 0 && (r.begin + r.count > c.base_n || (k && r.begin < prev_end))) FAIL("%s: generator: bulk range %zu of row %u\n", what, k, i);
                if (list == 1 && !c.low_ov && (r.begin < c.base_n || r.count != 1)) FAIL("%s: generator: overlay entry %zu of row %u\n", what, k, i);
                prev_end = r.begin + r.count;
                dst.push_back(r);
                uint32_t dead_in = 0;
                for (uint32_t id = r.begin; id < r.begin + r.count; id++) {
                    if (c.dead[id]) dead_in++;
                    else rows[i].push_back(id), live++;
                }
                // ---- which of the expansion's paths this range takes ----
                if (list == 0 && !c.big) {
                    const uint32_t b = r.begin, e = b + r.count;
                    for (int li = 0; li < 9; li++)
                        for (int oi = 0; oi < 4; oi++)
                            if (r.count == LENS[li] && (b & 63u) == OFFS[oi]) hit(("A range of " + std::to_string(LENS[li]) + " ids at word offset " + std::to_string(OFFS[oi])).c_str());
                    const bool is_long = r.count > RXD_SHORT;
                    if (e == c.base_n) hit(is_long ? "A streamed range ends at base_n" : "A short range ends at base_n");
                    if (!is_long && ((e - 1) >> 6) != (b >> 6) && (bits[(b >> 6) + 1] & ((1ull << (e & 63u)) - 1ull))) hit("A short range with a dead id in its second word");
                    if (is_long && dead_in) {
                        const uint32_t wb = b >> 6, we = (e - 1) >> 6;
                        if (wb == we && (e & 63u)) hit("A streamed range inside one word, clipped");
                        if (we > wb && (e & 63u)) hit("A streamed range with a partial last word");
                        if (we > wb && !(e & 63u)) hit("A streamed range ending on a word border");
                        if (we - wb >= 6 && (we - wb - 1) % 4) hit("A streamed range: four-word loop with a remainder");
                        if (dead_in == r.count) hit("A streamed range wholly dead");
                    }
                    if (is_long && !dead_in && use_dead) hit("A streamed range without a dead id (the clean copy)");
                    if (dead_in == r.count) hit("A ranges wholly dead");
                    if (b == 0) hit("A ranges that begin at id 0");
                }
            }
            (list ? L.rc2 : L.rc1)[i] = live;
        }
        const size_t nr = c.bulk[i].size() + c.ov[i].size();
        if (nr == 64 || nr == 65 || nr == 129) hit(("A rows of " + std::to_string(nr) + " ranges").c_str());
        if (nr && rows[i].empty()) hit("A rows of live length 0 with ranges");
    }
    if (!L.has_ov)
        for (uint32_t i = 0; i < n; i++) L.cnt2[i] = 0xDEAD; // (never read then)
    L.p1.push_back(MatchRange{0, 0}), L.p2.push_back(MatchRange{0, 0});
    unsigned long long total = 0;
    uint32_t n_unsorted = 0;
    for (auto& r : rows) total += r.size(), n_unsorted += !std::is_sorted(r.begin(), r.end());
    if (c.base_n % 64 <= 1 || c.base_n % 64 == 63) hit(("A base_n % 64 == " + std::to_string(c.base_n % 64)).c_str());
    if (n == 1 || (n >= 63 && n <= 65) || c.big) hit(("A n_topics " + std::to_string(n)).c_str());
    const uint32_t base_arg = use_dead ? c.base_n : 0u;
    Back B;
    run_backend(L, bits.data(), rank.data(), base_arg, n_unsorted + 2, total + 7, total, 0, B);
    if (check_backend(what, L, B, rows, false, total)) return 1;
    hit("A rows expanded", n), hit("A ids expanded", total);
    if (c.big) return 0;
    // ---- capacities that are too small; a status word that blocks ----
    if (n_unsorted) {
        run_backend(L, bits.data(), rank.data(), base_arg, n_unsorted - 1, total, total, 0, B);
        if (B.ctr.status != ST_NEED_SORTLIST || B.ctr.sort_count != n_unsorted) FAIL("%s: listing: a sort list of %u for %u rows leaves status %#x, count %u\n", what, n_unsorted - 1, n_unsorted, B.ctr.status, B.ctr.sort_count);
        if (B.sort_list[n_unsorted - 1] != CANARY) FAIL("%s: listing: written behind the sort list\n", what);
        hit("A sort list too small");
    }
    if (total) {
        run_backend(L, bits.data(), rank.data(), base_arg, n_unsorted + 2, total - 1, total, 0, B);
        if (!(B.ctr.status & ST_NOSPACE) || B.total != total) FAIL("%s: row check: an id buffer of %llu for %llu ids leaves status %#x, total %llu\n", what, total - 1, total, B.ctr.status, B.total);
        for (uint32_t v : B.out)
            if (v != CANARY) FAIL("%s: row check: ids written although the buffer is too small\n", what);
        hit("A id buffer too small");
        run_backend(L, bits.data(), rank.data(), base_arg, n_unsorted + 2, total, total, ST_NEED_PAIRS, B);
        for (uint32_t v : B.out)
            if (v != CANARY) FAIL("%s: row check: ids written although the walk asked for a re-run\n", what);
        if (B.ctr.sort_count) FAIL("%s: listing: rows listed although the walk asked for a re-run\n", what);
        hit("A expansion blocked by the status word");
    }
    // ---- match(limit, now): k_limit_select + k_limit_compact on the lists ----
    auto live_at = [&](uint32_t id) { return c.expire[id] > c.now; };
    std::vector<std::vector<uint32_t>> sel(n);
    std::vector<uint32_t> want_counts(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t lim = std::min(c.limit[i], LIM_FAST);
        for (int k = 0; k < 7; k++)
            if (c.limit[i] == LIMS[k] && k < 4) hit(("A k_limit_select with limit " + std::to_string(LIMS[k])).c_str());
        uint32_t in_first = 0;
        for (int list = 0; list < (L.has_ov ? 2 : 1); list++) {
            std::vector<MatchRange> rs = list ? c.ov[i] : c.bulk[i];
            if (list && !std::is_sorted(rs.begin(), rs.end(), [](const MatchRange& x, const MatchRange& y) { return x.begin < y.begin; }) && sel[i].size() < lim) hit("A k_limit_select over an unordered overlay list");
            std::sort(rs.begin(), rs.end(), [](const MatchRange& x, const MatchRange& y) { return x.begin < y.begin; });
            for (size_t k = 0; k < rs.size() && sel[i].size() < lim; k++) {
                if (rs[k].begin == 0) hit("A k_limit_select takes a range at id 0");
                if (k && rs[k].begin == rs[k - 1].begin + rs[k - 1].count) hit("A k_limit_select takes an adjacent range");
                uint32_t expired_run = 0;
                bool head = true;
                for (uint32_t o = 0; o < rs[k].count && sel[i].size() < lim; o++) {
                    const uint32_t id = rs[k].begin + o;
                    if (c.expire[id] == c.now) hit("A expire_at == now");
                    if (c.expire[id] == c.now + 1) hit("A expire_at == now + 1");
                    if (live_at(id)) sel[i].push_back(id), head = false;
                    else if (head && !c.dead[id]) expired_run++;
                }
                if (expired_run >= 64 && expired_run < 128) hit("A the first 64 ids of a range expired");
                if (expired_run >= 128) hit("A the first 128 ids of a range expired");
            }
            if (list == 0) in_first = (uint32_t)sel[i].size();
        }
        if (L.has_ov && lim && !c.ov[i].empty()) {
            uint32_t first_all = 0;
            for (auto& r : c.bulk[i])
                for (uint32_t o = 0; o < r.count; o++) first_all += live_at(r.begin + o);
            if (first_all == lim) hit("A quota met exactly at the end of the first list");
            if (in_first && in_first < lim && sel[i].size() > in_first) hit("A quota continued into the overlay list");
        }
        want_counts[i] = L.rc1[i] + (L.has_ov ? L.rc2[i] : 0u);
    }
    for (uint32_t grid = 1; grid <= 3; grid++) {
        for (uint32_t preset : {0u, (uint32_t)ST_NEED_PAIRS}) {
            if (preset && grid != 2) continue;
            std::vector<uint32_t> tmp((size_t)n * LIM_FAST + 64, CANARY), kept(n + 1, CANARY), counts(n + 1, CANARY);
            Back B2;
            B2.ctr.status = preset;
            B2.wave_sums.resize(1), B2.super_sums.resize(SUPER_STRIDE);
            BatchArgs a = batch_of(L, B2);
            const RetainOvList ov = L.ov();
            wemu::grid_size() = grid;
            for (uint32_t blk = 0; blk < grid; blk++)
                wemu::run_wave(blk, [&]() { k_limit_select(a, ov, c.limit.data(), c.expire.data(), c.now, n, tmp.data(), kept.data(), counts.data()); });
            if (kept[n] != CANARY || counts[n] != CANARY) FAIL("%s: limit row %u: written behind the last filter\n", what, n);
            for (uint32_t i = 0; i < n; i++) {
                const std::vector<uint32_t> none;
                const auto& want = preset ? none : sel[i];
                if (kept[i] != want.size() || counts[i] != (preset ? 0u : want_counts[i]))
                    FAIL("%s: limit row %u (limit %u, grid %u): kept %u counts %u, expected %zu and %u\n", what, i, c.limit[i], grid, kept[i], counts[i], want.size(), preset ? 0u : want_counts[i]);
                for (uint32_t k = 0; k < LIM_FAST; k++) {
                    const uint32_t v = tmp[(size_t)i * LIM_FAST + k], w = k < want.size() ? want[k] : CANARY;
                    if (v != w) FAIL("%s: limit row %u (limit %u, grid %u): slot %u holds %#x, expected %#x\n", what, i, c.limit[i], grid, k, v, w);
                }
            }
            for (size_t k = (size_t)n * LIM_FAST; k < tmp.size(); k++)
                if (tmp[k] != CANARY) FAIL("%s: limit row %u: a slot behind the last filter's was written\n", what, n);
            if (preset) {
                hit("A k_limit_select blocked by the status word");
                continue;
            }
            if (grid != 1) continue;
            std::vector<uint32_t> rp(n + 1, 0);
            for (uint32_t i = 0; i < n; i++) rp[i + 1] = rp[i] + kept[i];
            std::vector<uint32_t> out(rp[n] + 64, CANARY);
            wemu::grid_size() = (n + 255) / 256;
            for (uint32_t blk = 0; blk < (n + 255) / 256; blk++)
                for (uint32_t w = 0; w < 4; w++) wemu::run_wave(blk, [&]() { k_limit_compact(tmp.data(), rp.data(), n, out.data()); }, w);
            size_t at = 0;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t id : sel[i])
                    if (out[at++] != id) FAIL("%s: limit row %u: compacted id %u, expected %u\n", what, i, out[at - 1], id);
            for (; at < out.size(); at++)
                if (out[at] != CANARY) FAIL("%s: limit row %u: k_limit_compact wrote behind the last row\n", what, n);
            hit("A filters through k_limit_select", n);
        }
    }
    // ---- limits above LIM_FAST: k_limit_count_live + k_limit_copy_live on the finished CSR (rows ascending) ----
    {
        std::vector<uint32_t> rp(n + 1, 0), ids;
        for (uint32_t i = 0; i < n; i++) {
            std::vector<uint32_t> r = rows[i];
            std::sort(r.begin(), r.end());
            ids.insert(ids.end(), r.begin(), r.end());
            rp[i + 1] = (uint32_t)ids.size();
        }
        ids.push_back(0);
        std::vector<uint32_t> kept(n + 2, CANARY), counts(n + 1, CANARY);
        const uint32_t g = (n + 255) / 256;
        wemu::grid_size() = g;
        for (uint32_t blk = 0; blk < g; blk++)
            for (uint32_t w = 0; w < 4; w++)
                wemu::run_wave(blk, [&]() { k_limit_count_live(rp.data(), ids.data(), c.limit2.data(), c.expire.data(), c.now, n, kept.data(), counts.data()); }, w);
        std::vector<std::vector<uint32_t>> want(n);
        std::vector<uint32_t> nrp(n + 1, 0);
        for (uint32_t i = 0; i < n; i++) {
            for (uint32_t k = rp[i]; k < rp[i + 1] && want[i].size() < c.limit2[i]; k++)
                if (live_at(ids[k])) want[i].push_back(ids[k]);
            if (kept[i] != want[i].size() || counts[i] != rp[i + 1] - rp[i]) FAIL("%s: limit row %u (limit %u, CSR path): kept %u counts %u, expected %zu and %u\n", what, i, c.limit2[i], kept[i], counts[i], want[i].size(), rp[i + 1] - rp[i]);
            nrp[i + 1] = nrp[i] + kept[i];
            if (c.limit2[i] == 65 || c.limit2[i] == 0xFFFFFFFFu) hit(c.limit2[i] == 65 ? "A CSR limit path with limit 65" : "A CSR limit path with limit 0xFFFFFFFF");
            uint32_t all_live = 0;
            for (uint32_t k = rp[i]; k < rp[i + 1]; k++) all_live += live_at(ids[k]);
            if (all_live > want[i].size()) hit("A CSR limit path stops inside a row");
        }
        if (kept[n] != CANARY) FAIL("%s: limit row %u (CSR path): written behind the last filter\n", what, n);
        std::vector<uint32_t> out(nrp[n] + 64, CANARY);
        for (uint32_t blk = 0; blk < g; blk++)
            for (uint32_t w = 0; w < 4; w++) wemu::run_wave(blk, [&]() { k_limit_copy_live(rp.data(), nrp.data(), ids.data(), c.expire.data(), c.now, n, out.data()); }, w);
        size_t at = 0;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t id : want[i])
                if (out[at++] != id) FAIL("%s: limit row %u (limit %u, CSR path): id %u, expected %u\n", what, i, c.limit2[i], out[at - 1], id);
        for (; at < out.size(); at++)
            if (out[at] != CANARY) FAIL("%s: limit row %u (CSR path): k_limit_copy_live wrote behind the last row\n", what, n);
    }
    hit("A cases");
    return 0;
}

// the dead patterns of the directed geometry case (ids by the layout of geometry_case)
static const char* const DEAD_PATTERNS[9] = {"none", "id 0", "the last bulk id", "63 and 64", "every id = 0 or 63 (mod 64)", "one whole word", "six whole words of a streamed range",
                                             "every id of a range", "everything"};
static CaseA geometry_case(int pattern, uint32_t base_mod, int expire_mode, std::mt19937_64& rng) {
    CaseA c;
    c.name = std::string("geometry, dead: ") + DEAD_PATTERNS[pattern] + ", base_n % 64 = " + std::to_string(base_mod);
    c.base_n = 64 * 70 + base_mod;
    c.n_ids = c.base_n + 40;
    c.dead.assign(c.n_ids, 0);
    std::vector<MatchRange> all; // every length at every word offset, packed from id 0 on where the offsets allow (adjacent ranges)
    uint32_t cursor = 0;
    for (int li = 0; li < 9; li++)
        for (int oi = 0; oi < 4; oi++) {
            while ((cursor & 63u) != OFFS[oi]) cursor++;
            const MatchRange r{cursor, LENS[li]};
            cursor += LENS[li];
            all.push_back(r);
            c.bulk.push_back({r});
        }
    c.bulk.push_back(all);
    c.bulk.push_back({MatchRange{c.base_n - 5, 5}});                                         // a short range up to base_n
    c.bulk.push_back({MatchRange{c.base_n - 100, 100}});                                     // a streamed one
    c.bulk.push_back({MatchRange{c.base_n - 130, 30}, MatchRange{c.base_n - 100, 100}});     // adjacent, the second up to base_n
    c.bulk.push_back({MatchRange{0, 17}});
    c.bulk.push_back({MatchRange{64 * 50 + 3, 40}});                                         // streamed, inside one word
    c.bulk.push_back({MatchRange{64 * 52, 40}});
    c.bulk.push_back({MatchRange{64 * 50 + 60, 10}, MatchRange{64 * 51 + 60, 16}});          // short ones across a word border
    c.bulk.push_back({});
    const size_t n_rows = c.bulk.size();
    c.ov.resize(n_rows);
    for (size_t i = 0; i < n_rows; i += 3)
        for (uint32_t k = 0; k < 1 + i % 5; k++) c.ov[i].push_back(MatchRange{c.base_n + (uint32_t)((i + 7 * k) % 40), 1});
    for (auto& r : c.ov) std::sort(r.begin(), r.end(), [](const MatchRange& x, const MatchRange& y) { return x.begin < y.begin; });
    for (auto& r : c.ov) r.erase(std::unique(r.begin(), r.end(), [](const MatchRange& x, const MatchRange& y) { return x.begin == y.begin; }), r.end());
    const MatchRange r400 = all[8 * 4 + 1]; // the range of 400 ids that begins at word offset 1
    auto kill = [&](uint32_t id) {
        if (id < c.base_n) c.dead[id] = 1;
    };
    switch (pattern) {
    case 1: kill(0); break;
    case 2: kill(c.base_n - 1); break;
    case 3: kill(63), kill(64); break;
    case 4:
        for (uint32_t id = 0; id < c.base_n; id++)
            if ((id & 63u) == 0 || (id & 63u) == 63) kill(id);
        break;
    case 5:
        for (uint32_t id = 0; id < 64; id++) kill(((r400.begin >> 6) + 2) * 64 + id), kill(64 * 50 + id), kill(64 * 51 + id);
        break;
    case 6:
        for (uint32_t id = 0; id < 6 * 64; id++) kill(((r400.begin >> 6) + 1) * 64 + id);
        break;
    case 7:
        for (int li : {1, 4, 7, 8})
            for (uint32_t o = 0; o < all[li * 4 + 2].count; o++) kill(all[li * 4 + 2].begin + o);
        for (uint32_t o = 0; o < 100; o++) kill(c.base_n - 100 + o);
        break;
    case 8:
        for (uint32_t id = 0; id < c.base_n; id++) kill(id);
        break;
    default: break;
    }
    hit((std::string("A dead pattern: ") + DEAD_PATTERNS[pattern]).c_str());
    finish_case(c, expire_mode, rng);
    return c;
}
// rows of many ranges; the out-of-order check of the expansion (64-range chunks, the hand-over from the first list to the second)
static CaseA chunk_case(uint32_t base_mod, std::mt19937_64& rng) {
    CaseA c;
    c.name = "rows of 64, 65 and 129 ranges, disorder at chunk borders";
    c.base_n = 64 * 12 + base_mod;
    c.n_ids = c.base_n + 400;
    c.dead.assign(c.n_ids, 0);
    for (uint32_t id = 5; id < c.base_n; id += 11) c.dead[id] = 1;
    auto singles = [&](uint32_t first, uint32_t cnt, uint32_t step) {
        std::vector<MatchRange> r;
        for (uint32_t k = 0; k < cnt; k++) r.push_back(MatchRange{first + k * step, 1 + (k % 5 == 4 && step > 2 ? 2u : 0u)});
        return r;
    };
    auto ovs = [&](uint32_t first, uint32_t cnt) {
        std::vector<MatchRange> r;
        for (uint32_t k = 0; k < cnt; k++) r.push_back(MatchRange{c.base_n + first + k, 1});
        return r;
    };
    for (uint32_t nr : {64u, 65u, 129u}) c.bulk.push_back(singles(3, nr, 4)), c.ov.push_back({});
    for (uint32_t nr : {64u, 65u, 129u}) c.bulk.push_back({}), c.ov.push_back(ovs(1, nr));
    c.bulk.push_back(singles(0, 60, 3)), c.ov.push_back(ovs(0, 69)); // 129 over both lists
    { // the ONLY disorder lies between entries 63 and 64 of the overlay list: what the wave carries from one chunk of 64 ranges to the next
        std::vector<MatchRange> o = ovs(10, 100);
        o[64].begin = c.base_n + 5;
        c.bulk.push_back({}), c.ov.push_back(o);
        hit("A the only disorder lies between entries 63 and 64");
    }
    { // ... and the same border inside the first list's successor: 64 bulk ranges, then an overlay list in order
        c.bulk.push_back(singles(1, 64, 2)), c.ov.push_back(ovs(0, 3));
    }
    { // disorder between the last bulk range and the first overlay id (cannot happen in the product: overlay ids lie above base_n; here the second list
      // is given a bulk id on purpose -- the row must be listed, which documents the check)
        c.bulk.push_back({MatchRange{2, 1}, MatchRange{100, 20}});
        c.ov.push_back({MatchRange{50, 1}, MatchRange{c.base_n + 2, 1}});
        c.low_ov = true;
        hit("A disorder between the last bulk range and the first overlay id");
    }
    c.bulk.push_back({}), c.ov.push_back({MatchRange{c.base_n + 9, 1}, MatchRange{c.base_n + 8, 1}});          // two ids, out of order
    c.bulk.push_back({}), c.ov.push_back({MatchRange{c.base_n + 9, 1}});                                      // one id
    c.bulk.push_back({MatchRange{5, 1}}), c.ov.push_back({MatchRange{c.base_n + 9, 1}});                      // one id: 5 is dead
    c.bulk.push_back({MatchRange{6, 9}}), c.ov.push_back({MatchRange{c.base_n + 3, 1}, MatchRange{c.base_n + 1, 1}, MatchRange{c.base_n + 2, 1}});
    hit("A a row of two ids out of order");
    finish_case(c, 3, rng);
    return c;
}
static CaseA limit_case(std::mt19937_64& rng) {
    CaseA c;
    c.name = "match(limit, now) over two lists";
    c.base_n = 64 * 20 + 1;
    c.n_ids = c.base_n + 100;
    c.dead.assign(c.n_ids, 0);
    auto row = [&](std::vector<MatchRange> b, std::vector<MatchRange> o, uint32_t lim) { c.bulk.push_back(b), c.ov.push_back(o), c.limit.push_back(lim), c.limit2.push_back(lim); };
    const uint32_t B = c.base_n;
    for (uint32_t lim : {0u, 1u, 9u, 10u, 11u, 12u, 63u, 64u, 65u, 0xFFFFFFFFu}) {
        row({MatchRange{0, 4}, MatchRange{4, 3}, MatchRange{20, 3}}, {MatchRange{B + 3, 1}, MatchRange{B + 1, 1}, MatchRange{B + 2, 1}}, lim); // 10 bulk ids, adjacent ranges, from id 0
        row({MatchRange{100, 400}}, {MatchRange{B + 5, 1}}, lim);
        row({MatchRange{600, 200}, MatchRange{800, 70}}, {}, lim);
        row({}, {MatchRange{B + 40, 1}, MatchRange{B + 20, 1}, MatchRange{B + 30, 1}}, lim);
    }
    row({MatchRange{900, 50}}, {}, 1); // (the last row: whatever is written behind its one id lands in the canaries)
    finish_case(c, 0, rng);
    for (uint32_t o = 0; o < 64; o++) c.expire[100 + o] = c.now;          // the first 64 ids of a range expired (at equality)
    for (uint32_t o = 0; o < 128; o++) c.expire[600 + o] = c.now - 1;     // the first 128
    c.expire[728] = c.now + 1;
    c.expire[B + 20] = c.now, c.expire[B + 30] = c.now + 1;
    return c;
}
static CaseA rows_case(uint32_t n, bool big, std::mt19937_64& rng) {
    CaseA c;
    c.name = std::to_string(n) + " rows";
    c.big = big;
    c.base_n = 64 * 6 + 63;
    c.n_ids = c.base_n + 64;
    c.dead.assign(c.n_ids, 0);
    for (uint32_t id = 1; id < c.base_n; id += 3) c.dead[id] = 1;
    c.bulk.resize(n), c.ov.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        if (big && i % 5 != 0 && i != n - 1 && i % 16384 > 2) continue;
        c.bulk[i].push_back(MatchRange{i % (c.base_n - 3), 1 + i % 3});
        if (i % 4 == 0) c.ov[i].push_back(MatchRange{c.base_n + i % 64, 1});
    }
    finish_case(c, 3, rng);
    return c;
}
static CaseA random_case(int k, std::mt19937_64& rng) {
    auto rnd = [&](size_t m) { return (uint32_t)(rng() % m); };
    CaseA c;
    c.name = "random case " + std::to_string(k);
    const uint32_t mods[5] = {0, 1, 63, 17, 40};
    c.base_n = 64 * (2 + rnd(30)) + mods[rnd(5)];
    c.n_ids = c.base_n + (rnd(4) ? 1 + rnd(300) : 0);
    c.dead.assign(c.n_ids, 0);
    const uint32_t mode = rnd(6);
    for (uint32_t id = 0; id < c.base_n; id++) {
        if (mode == 1) c.dead[id] = rnd(20) == 0;
        else if (mode == 2) c.dead[id] = rnd(2);
        else if (mode == 3) c.dead[id] = (id >> 6) & 1u;
        else if (mode == 4) c.dead[id] = (id & 63u) == 0 || (id & 63u) == 63;
        else if (mode == 5) c.dead[id] = rnd(20) != 0;
    }
    const uint32_t n = 1 + rnd(rnd(4) ? 12 : 140);
    for (uint32_t i = 0; i < n; i++) {
        std::vector<MatchRange> b, o;
        const uint32_t shape = rnd(6);
        uint32_t cursor = rnd(c.base_n);
        if (shape == 0) cursor = 0;
        const uint32_t want = shape == 5 ? 0 : (shape == 4 ? 60 + rnd(90) : 1 + rnd(6));
        for (uint32_t q = 0; q < want && cursor < c.base_n; q++) {
            uint32_t len = rnd(3) ? LENS[rnd(9)] : 1 + rnd(130);
            if (shape == 4) len = 1 + rnd(3);
            len = std::min(len, c.base_n - cursor);
            b.push_back(MatchRange{cursor, len});
            cursor += len + (rnd(3) ? rnd(70) : 0);
        }
        const uint32_t n_ov = c.n_ids - c.base_n;
        if (n_ov && rnd(3)) {
            std::set<uint32_t> pick;
            const uint32_t m = rnd(3) ? 1 + rnd(8) : 1 + rnd(n_ov);
            for (uint32_t q = 0; q < m; q++) pick.insert(c.base_n + rnd(n_ov));
            for (uint32_t id : pick) o.push_back(MatchRange{id, 1});
            if (rnd(3) == 0) std::shuffle(o.begin(), o.end(), rng);
        }
        c.bulk.push_back(b), c.ov.push_back(o);
    }
    finish_case(c, (int)rnd(4), rng);
    for (auto& l : c.limit)
        if (rnd(3) == 0) l = rnd(70);
    return c;
}

static int part_a(int cases, std::mt19937_64& rng) {
    std::vector<CaseA> list;
    int em = 0;
    for (int p = 0; p < 9; p++)
        for (uint32_t m : {0u, 1u, 63u}) list.push_back(geometry_case(p, m, em++ % 4, rng));
    for (uint32_t m : {0u, 1u, 63u}) list.push_back(chunk_case(m, rng));
    list.push_back(limit_case(rng));
    {
        CaseA c = limit_case(rng);
        c.name += " (no overlay list)";
        for (auto& o : c.ov) o.clear();
        list.push_back(c);
    }
    for (uint32_t n : {1u, 63u, 64u, 65u}) list.push_back(rows_case(n, false, rng));
    for (uint32_t n : {16385u, 32769u}) list.push_back(rows_case(n, true, rng));
    for (int k = 0; k < cases; k++) list.push_back(random_case(k, rng));
    for (auto& c : list)
        if (run_case(c)) return 1;
    return 0;
}

// ---- Parts B and C: an index the product's host code makes, churned ---------------------------------------------------------------------------
using Key = std::pair<std::string, std::string>; // (tenant, topic)
struct Index {
    RetainIndexHost h;
    HostExec hx;
    RetainDyn<HostExec> rt{hx};
    std::map<Key, uint32_t> live, ever;
    RetainIndexView view{};
    int apply(const std::vector<std::pair<Key, uint8_t>>& ops) { // distinct keys per batch
        if (ops.empty()) return 0;
        std::map<std::string, uint32_t> tix;
        std::string tb, pb;
        std::vector<uint32_t> toff{0}, poff{0}, ot;
        std::vector<uint8_t> op;
        std::vector<unsigned long long> ts;
        std::vector<uint32_t> ex;
        for (auto& o : ops) {
            if (!tix.count(o.first.first)) {
                tix[o.first.first] = (uint32_t)tix.size();
                tb += o.first.first, toff.push_back((uint32_t)tb.size());
            }
            ot.push_back(tix[o.first.first]);
            pb += o.first.second, poff.push_back((uint32_t)pb.size());
            op.push_back(o.second), ts.push_back(5000ull << 16), ex.push_back(100);
        }
        tb.append(16, '\0'), pb.append(16, '\0');
        std::vector<uint32_t> out(ops.size());
        if (!rt.apply((const uint8_t*)tb.data(), toff.data(), (uint32_t)tix.size(), ot.data(), (const uint8_t*)pb.data(), poff.data(), op.data(), ts.data(), ex.data(), (uint32_t)ops.size(), out.data()))
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
static std::string chain(const std::string& head, size_t levels, const std::string& last = std::string()) {
    std::string s = head;
    for (size_t k = 1; k < levels; k++) s += "/" + (k + 1 == levels && !last.empty() ? last : std::to_string(k));
    return s;
}

struct WalkOut { // one range list as a walk leaves it
    std::vector<uint32_t> pair_off, pair_cnt, route_cnt;
    std::vector<MatchRange> pairs;
    unsigned long long pair_cap = 0;
};
static int ids_of(const char* what, const WalkOut& w, uint32_t i, uint32_t id_bound, std::vector<uint32_t>& got) {
    got.clear();
    if (w.pair_cnt[i] > w.pair_cap || (w.pair_cnt[i] && w.pair_off[i] + (unsigned long long)w.pair_cnt[i] > w.pair_cap)) FAIL("%s: row %u: range list out of bounds\n", what, i);
    for (uint32_t k = 0; k < w.pair_cnt[i]; k++) {
        const MatchRange m = w.pairs[w.pair_off[i] + k];
        if (m.count == 0 || m.count > id_bound || m.begin + m.count > id_bound) FAIL("%s: row %u: range %u is [%u, +%u)\n", what, i, k, m.begin, m.count);
        for (uint32_t j = 0; j < m.count; j++) got.push_back(m.begin + j);
    }
    return 0;
}

static int part_bc(int round, std::mt19937_64& rng) {
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    const bool churn_bulk = round % 3 != 2; // (every third round: adds only -- an overlay, no dead bulk id, base_n passed as 0)
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "$x", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "0", "x", "q"};
    auto rand_topic = [&]() {
        std::string t;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) t += (i ? "/" : "") + alpha[rnd(alpha.size())];
        return t;
    };
    const uint32_t big = std::max(R_OUT, R_FRONT) * 7 / 6 + 60 + (uint32_t)rnd(30); // (every seventh is removed below)
    Index ix;
    ix.hx.threads = 2;
    ix.rt.tiny = true;
    // ---- the bulk load ----
    std::set<Key> bulk;
    for (size_t i = 0; i < 250; i++) bulk.insert({"t", rand_topic()});
    for (const char* t : {"a", "a/b", "b/c", "b/c/d", "x", "o/k", "p/z"}) bulk.insert({"nosys", t});
    bulk.insert({"deep", chain("d", 16)}), bulk.insert({"deep", chain("d", 17)}), bulk.insert({"deep", chain("e", 17)}), bulk.insert({"deep", chain("d", 20)});
    bulk.insert({"deep", chain("d", 70)}), bulk.insert({"deep", chain("d", 300)}), bulk.insert({"deep", chain("d", 17, "b")}), bulk.insert({"deep", "$s/" + chain("d", 17)});
    for (uint32_t k = 0; k < 50; k++) bulk.insert({"both", "o/b" + std::to_string(k)});
    bulk.insert({"both", "$sys/b"});
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
    // ---- batches: adds under loaded tenants and tenants that exist in the overlay only, '$' levels, empty levels; removes; re-adds ----
    std::map<Key, uint8_t> b1;
    for (size_t i = 0; i < 60; i++) b1[{"t", rand_topic() + (rnd(2) ? "/n" : "")}] = 0;
    b1[{"t", "$new/x"}] = 0;
    const std::pair<const char*, uint32_t> ov_tenants[5] = {{"ovA", OV_OUT}, {"ovB", OV_OUT + 1}, {"ovC", big}, {"both", OV_OUT + 1}, {"ovD", R_OUT + 1}};
    for (auto& ot : ov_tenants)
        for (uint32_t k = 0; k < ot.second; k++) b1[{ot.first, "o/" + std::to_string(1000 + k)}] = 0;
    for (const char* t : {"ovA", "ovC"}) b1[{t, "$sys/q"}] = 0, b1[{t, "$sys/x/y"}] = 0, b1[{t, "p/a"}] = 0, b1[{t, "p/a/b"}] = 0, b1[{t, "p//x"}] = 0, b1[{t, ""}] = 0, b1[{t, "x"}] = 0;
    b1[{"deep", chain("d", 17, "x")}] = 0, b1[{"deep", chain("d", 16, "y")}] = 0, b1[{"deep", chain("d", 300, "x")}] = 0, b1[{"deep", chain("d", 40)}] = 0, b1[{"deep", chain("e", 18)}] = 0;
    b1[{"deep", "$s/" + chain("d", 17, "x")}] = 0;
    if (ix.apply({b1.begin(), b1.end()})) return 1;
    std::map<Key, uint8_t> b2;
    {
        uint32_t k = 0;
        for (auto& kv : ix.live) {
            const bool is_bulk = kv.second < ix.h.n_topics;
            const std::string& tn = kv.first.first;
            if (is_bulk && !churn_bulk) continue;
            if (tn == "t" && rnd(3) == 0) b2[kv.first] = 1;
            if ((tn == "ovC" || tn == "both") && kv.first.second.rfind("o/", 0) == 0 && k++ % 7 == 0) b2[kv.first] = 1;
        }
        b2[{"ovA", "p/a"}] = 1, b2[{"ovC", "p/a"}] = 1; // dead overlay topics under live descendants
        b2[{"deep", chain("e", 18)}] = 1;
        if (churn_bulk) b2[{"deep", chain("d", 20)}] = 1, b2[{"nosys", "b/c"}] = 1;
    }
    if (ix.apply({b2.begin(), b2.end()})) return 1;
    std::map<Key, uint8_t> b3;
    for (auto& kv : b2)
        if (rnd(4) == 0 && kv.first.second != "p/a" && kv.first.first != "deep") b3[kv.first] = 0;
    if (ix.apply({b3.begin(), b3.end()})) return 1;
    v.dyn = ix.rt.view();
    v.expire_at = ix.rt.expire_at();
    const uint32_t id_bound = (uint32_t)ix.rt.info.id_bound, base_n = v.dyn.base_n;
    if ((v.dyn.use_dead != 0) != churn_bulk) FAIL("round %d: use_dead %u\n", round, v.dyn.use_dead);
    hit(churn_bulk ? "BC rounds with dead bulk ids" : "BC rounds without dead bulk ids");
    // ---- the filters ----
    const std::vector<std::string> tn_list = {"t", "nosys", "deep", "both", "ovA", "ovB", "ovC", "nobody", "ovD"};
    std::string tbytes, fbytes;
    std::vector<uint32_t> toff{0}, foff{0}, ft;
    std::vector<std::string> flt;
    for (auto& t : tn_list) tbytes += t, toff.push_back((uint32_t)tbytes.size());
    auto add = [&](uint32_t t, const std::string& f) { flt.push_back(f), ft.push_back(t); };
    for (uint32_t t = 0; t < tn_list.size(); t++) {
        for (const char* f : {"#", "+", "+/#", "+/+", "o/#", "o/+", "o/+/#", "p/#", "p/a", "p/+", "p/+/+", "$sys/#", "+/x", "+/q", "$sys/+", "", "/#"}) add(t, f);
        for (int k = 0; k < 4; k++) {
            std::string f;
            const size_t depth = 1 + rnd(5);
            for (size_t d = 0; d < depth; d++) f += (d ? "/" : "") + (d + 1 == depth && rnd(3) == 0 ? std::string("#") : rnd(3) == 0 ? std::string("+") : alpha[rnd(alpha.size())]);
            add(t, f);
        }
    }
    const uint32_t DEEP_T = 2;
    add(DEEP_T, chain("d", 16)), add(DEEP_T, chain("d", 16, "y")), add(DEEP_T, chain("d", 16, "+")), add(DEEP_T, chain("d", 16, "#")); // 16 levels: not deep
    add(DEEP_T, chain("d", 17)), add(DEEP_T, chain("d", 17, "x")), add(DEEP_T, chain("d", 17, "+")), add(DEEP_T, chain("d", 17, "#")), add(DEEP_T, chain("d", 18, "#"));
    add(DEEP_T, chain("+", 17)), add(DEEP_T, chain("+", 17, "+")), add(DEEP_T, chain("+", 18, "#")), add(DEEP_T, "+/" + chain("+", 16, "+"));
    add(DEEP_T, chain("d", 300)), add(DEEP_T, chain("d", 300, "+")), add(DEEP_T, chain("d", 299, "#")), add(DEEP_T, "$s/" + chain("d", 17, "+"));
    add(0, chain("a", 17, "#")), add(4, chain("o", 20)), add(7, chain("d", 17));
    add(DEEP_T, chain("d", 20)), add(DEEP_T, chain("e", 18)); // (removed above: a bulk-loaded topic in the churned rounds, an overlay topic)
    for (int k = 0; k < 6; k++) {
        const size_t depth = 17 + rnd(54);
        std::string f = rnd(3) ? "d" : "+";
        for (size_t d = 1; d < depth; d++) f += "/" + (d + 1 == depth && rnd(3) == 0 ? std::string("#") : rnd(5) == 0 ? std::string("+") : std::to_string(d));
        add(DEEP_T, f);
    }
    const uint32_t n = (uint32_t)flt.size();
    for (auto& f : flt) fbytes += f, foff.push_back((uint32_t)fbytes.size());
    while (fbytes.size() % 16) fbytes.push_back('\0');
    fbytes.append(16, '\0'), tbytes.append(32, '\0');
    // ---- the brute force, and which paths the filters take ----
    std::vector<std::vector<uint32_t>> exp(n), exp_ov(n);
    std::vector<uint32_t> nlev(n), deep_rows;
    std::map<std::string, bool> has_sys_bulk, has_sys_ov;
    std::map<std::pair<std::string, std::string>, uint32_t> kids; // children per (tenant, parent path) in the overlay (nodes, dead topics included)
    for (auto& kv : ix.ever) {
        const bool sys = !kv.first.second.empty() && kv.first.second[0] == '$';
        if (kv.second < base_n) has_sys_bulk[kv.first.first] |= sys;
        else has_sys_ov[kv.first.first] |= sys;
    }
    std::set<std::pair<std::string, std::string>> ov_nodes;
    for (auto& kv : ix.ever)
        if (kv.second >= base_n) {
            const auto lv = split(kv.first.second, '/');
            std::string path;
            for (size_t d = 0; d < lv.size(); d++) {
                const std::string parent = path;
                path += "\x01" + lv[d];
                if (ov_nodes.insert({kv.first.first, path}).second) kids[{kv.first.first, parent}]++;
            }
        }
    for (uint32_t i = 0; i < n; i++) {
        const auto fl = split(flt[i], '/');
        nlev[i] = (uint32_t)fl.size();
        const std::string& tn = tn_list[ft[i]];
        bool bulk_hit = false, ov_hit = false;
        for (auto& kv : ix.live)
            if (kv.first.first == tn && filter_matches(fl, split(kv.first.second, '/'))) {
                exp[i].push_back(kv.second);
                (kv.second < base_n ? bulk_hit : ov_hit) = true;
                if (kv.second >= base_n) exp_ov[i].push_back(kv.second);
            }
        std::sort(exp[i].begin(), exp[i].end()), std::sort(exp_ov[i].begin(), exp_ov[i].end());
        const bool hash = fl.back() == "#";
        if (nlev[i] <= RW_LV) {
            const size_t m = exp_ov[i].size();
            if (m == OV_OUT) hit("B overlay rows of exactly OV_OUT ids");
            if (m == OV_OUT + 1) hit("B overlay rows of OV_OUT + 1 ids");
            if (m > R_OUT) hit("B overlay rows of more than R_OUT ids (the second, writing walk)");
            if (m == R_OUT + 1) hit("B overlay rows of exactly R_OUT + 1 ids");
            if (m > OV_OUT) hit(hash ? "B overlay buffer flushed inside the '#' loop" : "B overlay buffer flushed at the filter's end");
            if (fl.size() >= 2 && (fl[1] == "+" || fl[1] == "#") && fl[0] != "+" && kids[{tn, "\x01" + fl[0]}] > R_FRONT) hit("B overlay frontier beyond R_FRONT");
            if (has_sys_ov[tn] && fl[0] == "+") hit("B '$' child of the overlay skipped by '+' at level 0");
            if (has_sys_ov[tn] && fl[0] == "#") hit("B '$' child of the overlay skipped by '#' at level 0");
            if (flt[i] == "p/#" && ix.ever.count({tn, "p/a"}) && !ix.live.count({tn, "p/a"}) && ix.live.count({tn, "p/a/b"}) && ix.ever[{tn, "p/a"}] >= base_n) hit("B a dead overlay topic above a live one");
            if (flt[i] == "#" && ix.h.by_name.count(tn)) hit(has_sys_bulk[tn] ? "C the filter '#' on a tenant with a '$' run" : "C the filter '#' on a tenant without a '$' run");
        } else {
            deep_rows.push_back(i);
            if (nlev[i] == 17 && bulk_hit && ov_hit) hit("B a deep filter of 17 levels matches a bulk and an overlay topic");
            if (hash && !exp[i].empty()) hit("B a deep filter ending in '#' with matches");
            if (fl[0] == "+" && bulk_hit) hit("B a deep filter with a mixed frontier chunk");
            if (nlev[i] >= 300) hit("B a deep filter of 300 levels");
            if (exp[i].empty() && ix.ever.count({tn, flt[i]}) && ix.ever[{tn, flt[i]}] < base_n) hit("B a deep literal filter names a dead bulk topic");
        }
    }
    // ---- B1: retain_walk_body<false, true>, the body of k_retain_overlay, from tiny capacities ----
    const uint32_t grid = 1 + (uint32_t)rnd(3);
    RetainArgs r{};
    r.ix = v;
    r.tenants = (const uint8_t*)tbytes.data(), r.tenant_off = toff.data(), r.n_tenants = (uint32_t)tn_list.size();
    r.filter_tenant = ft.data(), r.filters = (const uint8_t*)fbytes.data(), r.filter_off = foff.data(), r.n_filters = n;
    std::vector<uint32_t> deep_list(n + 1, 0xDEAD);
    r.deep_list = deep_list.data();
    uint32_t gcap = 4;
    std::vector<uint2> gscratch;
    std::vector<SubAlloc> subs(2 * N_SUB);
    auto fresh = [&](WalkOut& w) {
        w.pair_off.assign(n, 0xDEAD), w.pair_cnt.assign(n, 0xDEAD), w.route_cnt.assign(n, 0xDEAD);
        w.pairs.assign(w.pair_cap, MatchRange{0xDEAD0000u, 0xFFFFu});
        for (auto& s : subs) s.used = 0;
        gscratch.assign((size_t)grid * 2 * gcap + 1, make_uint2(0xABABABABu, 0xABABABABu));
        r.gscratch = gscratch.data(), r.gcap = gcap;
    };
    auto args_of = [&](WalkOut& w, Counters& ctr, SubAlloc* sub) {
        BatchArgs a{};
        a.n_topics = n, a.tpw_shift = 6, a.n_blocks = (n + 63) / 64;
        a.pair_off = w.pair_off.data(), a.pair_cnt = w.pair_cnt.data(), a.route_cnt = w.route_cnt.data(), a.pairs = w.pairs.data(), a.pair_cap = w.pair_cap;
        a.subs = sub, a.ctr = &ctr;
        return a;
    };
    WalkOut wo;
    wo.pair_cap = N_SUB * 8ull;
    wemu::grid_size() = grid;
    for (int attempt = 0;; attempt++) {
        if (attempt > 24) FAIL("round %d: overlay walk: growth does not converge (gcap %u, pair_cap %llu)\n", round, gcap, wo.pair_cap);
        fresh(wo);
        Counters ctr{};
        BatchArgs ao = args_of(wo, ctr, subs.data() + N_SUB);
        for (uint32_t blk = 0; blk < grid; blk++) wemu::run_wave(blk, [&]() { retain_walk_body<false, true>(r, ao); });
        if (ctr.status & ~(ST_NEED_SPILL | ST_RETAIN_FRONT)) FAIL("round %d: overlay walk: status %#x\n", round, ctr.status);
        if (ctr.slow_count) FAIL("round %d: overlay walk: listing of %u deep filters (the walk of the bulk-loaded index lists them)\n", round, ctr.slow_count);
        if (!ctr.status) break;
        if (ctr.status & ST_NEED_SPILL) wo.pair_cap *= 2, hit("B overlay walk re-run for its range list");
        if (ctr.status & ST_RETAIN_FRONT) gcap *= 4, hit("B overlay walk re-run for its frontier");
    }
    std::vector<uint32_t> got;
    for (uint32_t i = 0; i < n; i++) {
        if (ids_of("overlay walk", wo, i, id_bound, got)) return 1;
        const std::vector<uint32_t> none;
        const auto& want = nlev[i] <= RW_LV ? exp_ov[i] : none;
        if (!std::is_sorted(got.begin(), got.end())) {
            if (got.size() <= OV_OUT) FAIL("round %d: overlay walk: row %u '%s': %zu ids fit the buffer and come out unordered\n", round, i, flt[i].c_str(), got.size());
            hit("B overlay rows that come out unordered"), std::sort(got.begin(), got.end());
        }
        if (got != want || wo.route_cnt[i] != want.size() || wo.pair_cnt[i] != want.size())
            FAIL("round %d: overlay walk: row %u '%s' of tenant '%s': %zu ids (route_cnt %u, %u ranges), expected %zu\n", round, i, flt[i].c_str(), tn_list[ft[i]].c_str(), got.size(), wo.route_cnt[i], wo.pair_cnt[i], want.size());
        hit("B overlay ids", want.size());
    }
    hit("B filters through the overlay walk", n);
    // ---- B2: retain_walk_body<true>, the body of k_retain_walk_deep: the listed filters, both tries ----
    const uint32_t deep_maxl = 512;
    std::vector<uint32_t> deep_levels((size_t)grid * 6 * (deep_maxl + 1), 0xABABABABu);
    r.deep_levels = deep_levels.data(), r.deep_maxl = deep_maxl;
    std::vector<uint32_t> dl = deep_rows;
    std::shuffle(dl.begin(), dl.end(), rng);
    std::copy(dl.begin(), dl.end(), deep_list.begin());
    WalkOut wd;
    wd.pair_cap = N_SUB * 2ull;
    uint32_t gcap_ov = gcap;
    gcap = 4;
    for (int attempt = 0;; attempt++) {
        if (attempt > 24) FAIL("round %d: deep walk: growth does not converge (gcap %u, pair_cap %llu)\n", round, gcap, wd.pair_cap);
        fresh(wd);
        Counters ctr{};
        ctr.slow_count = (uint32_t)dl.size();
        BatchArgs a = args_of(wd, ctr, subs.data());
        for (uint32_t blk = 0; blk < grid; blk++) wemu::run_wave(blk, [&]() { retain_walk_body<true>(r, a); });
        if (ctr.status & ~(ST_NEED_PAIRS | ST_RETAIN_FRONT)) FAIL("round %d: deep walk: status %#x\n", round, ctr.status);
        if (!ctr.status) break;
        if (ctr.status & ST_NEED_PAIRS) wd.pair_cap *= 2, hit("B deep walk re-run for its range list");
        if (ctr.status & ST_RETAIN_FRONT) gcap *= 4;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (nlev[i] <= RW_LV) {
            if (wd.pair_cnt[i] != 0xDEAD) FAIL("round %d: deep walk: row %u is not listed and was written\n", round, i);
            continue;
        }
        if (ids_of("deep walk", wd, i, id_bound, got)) return 1;
        std::vector<uint32_t> kept;
        for (uint32_t id : got)
            if (!id_dead(v.dyn.dead_bits, id)) kept.push_back(id);
        std::sort(kept.begin(), kept.end());
        if (kept != exp[i] || wd.route_cnt[i] != exp[i].size())
            FAIL("round %d: deep walk: row %u '%.40s...' (%u levels): %zu live ids (route_cnt %u), expected %zu\n", round, i, flt[i].c_str(), nlev[i], kept.size(), wd.route_cnt[i], exp[i].size());
        hit("B deep filters"), hit("B deep ids", exp[i].size());
    }
    // ---- C: the chain of a batch -- k_retain_walk's body, the overlay's list, the deep pass, sums, row pointers, expansion ----
    gcap = std::max(gcap, gcap_ov);
    WalkOut wc;
    wc.pair_cap = N_SUB * 64ull;
    uint32_t rw_cap = 4;
    Counters ctr{};
    for (int attempt = 0;; attempt++) {
        if (attempt > 24) FAIL("round %d: chain: growth does not converge\n", round);
        fresh(wc);
        std::fill(deep_list.begin(), deep_list.end(), 0xDEAD);
        std::vector<uint32_t> arena((size_t)grid * 8 * 2 * rw_cap + 4, 0xABABABABu);
        r.rw_arena = arena.data(), r.rw_cap = rw_cap;
        ctr = Counters{};
        BatchArgs a = args_of(wc, ctr, subs.data());
        std::vector<unsigned long long> super((n / 64 / 256 + 2) * SUPER_STRIDE, 0), wsum(n / 64 + 1, 0);
        a.super_sums = super.data(), a.wave_sums = wsum.data();
        for (uint32_t blk = 0; blk < grid; blk++)
            wemu::run_wave(blk, [&]() {
                static RwLds<8> L;
                if (v.dyn.use_dead) retain_walk_rounds<8, true>(r, a, L);
                else retain_walk_rounds<8, false>(r, a, L);
            });
        for (uint32_t blk = 0; blk < grid; blk++) wemu::run_wave(blk, [&]() { retain_walk_body<true>(r, a); });
        if (ctr.status & ~(ST_NEED_PAIRS | ST_RETAIN_LIST | ST_RETAIN_FRONT)) FAIL("round %d: chain: status %#x\n", round, ctr.status);
        if (!ctr.status) break;
        if (ctr.status & ST_NEED_PAIRS) wc.pair_cap *= 2;
        if (ctr.status & ST_RETAIN_LIST) rw_cap *= 4;
        if (ctr.status & ST_RETAIN_FRONT) gcap *= 4;
    }
    if (ctr.slow_count != deep_rows.size()) FAIL("round %d: chain: listing of %u deep filters, expected %zu\n", round, ctr.slow_count, deep_rows.size());
    Lists L;
    L.n = n, L.has_ov = true;
    L.off1 = wc.pair_off, L.cnt1 = wc.pair_cnt, L.rc1 = wc.route_cnt, L.p1 = wc.pairs;
    L.off2 = wo.pair_off, L.cnt2 = wo.pair_cnt, L.rc2 = wo.route_cnt, L.p2 = wo.pairs;
    unsigned long long total = 0;
    for (uint32_t i = 0; i < n; i++) {
        total += exp[i].size();
        if ((unsigned long long)L.rc1[i] + L.rc2[i] != exp[i].size())
            FAIL("round %d: chain: row %u '%.60s' of tenant '%s': the walks count %u + %u live ids, expected %zu\n", round, i, flt[i].c_str(), tn_list[ft[i]].c_str(), L.rc1[i], L.rc2[i], exp[i].size());
    }
    Back B;
    run_backend(L, v.dyn.dead_bits, v.dyn.dead_rank, v.dyn.use_dead ? base_n : 0u, n, total, total, 0, B);
    if (check_backend(("round " + std::to_string(round) + ": chain").c_str(), L, B, exp, true, total)) return 1;
    hit("C rows", n), hit("C ids", total);
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 40;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    if (part_a(cases, rng)) return 1;
    const int rounds = std::max(3, cases / 12);
    for (int round = 0; round < rounds; round++)
        if (part_bc(round, rng)) return 1;
    // ---- the floors: every directed case and every rarely taken path must have been reached ----
    std::vector<std::string> need = {"A cases with dead ids", "A cases without dead ids (base_n passed as 0)", "A short range ends at base_n", "A streamed range ends at base_n",
                                     "A short range with a dead id in its second word", "A streamed range inside one word, clipped", "A streamed range with a partial last word",
                                     "A streamed range ending on a word border", "A streamed range: four-word loop with a remainder", "A streamed range wholly dead",
                                     "A streamed range without a dead id (the clean copy)", "A ranges wholly dead", "A ranges that begin at id 0", "A rows of 64 ranges", "A rows of 65 ranges",
                                     "A rows of 129 ranges", "A rows of live length 0 with ranges", "A rows listed for the sort", "A sort list too small", "A id buffer too small",
                                     "A expansion blocked by the status word", "A k_limit_select blocked by the status word", "A k_limit_select over an unordered overlay list",
                                     "A k_limit_select takes a range at id 0", "A k_limit_select takes an adjacent range", "A expire_at == now", "A expire_at == now + 1",
                                     "A the first 64 ids of a range expired", "A the first 128 ids of a range expired", "A quota met exactly at the end of the first list",
                                     "A quota continued into the overlay list", "A CSR limit path with limit 65", "A CSR limit path with limit 0xFFFFFFFF", "A CSR limit path stops inside a row",
                                     "A the only disorder lies between entries 63 and 64", "A disorder between the last bulk range and the first overlay id", "A a row of two ids out of order", "A n_topics 1", "A n_topics 63", "A n_topics 64", "A n_topics 65",
                                     "A n_topics 16385", "A n_topics 32769", "A base_n % 64 == 0", "A base_n % 64 == 1", "A base_n % 64 == 63",
                                     "BC rounds with dead bulk ids", "BC rounds without dead bulk ids", "B overlay rows of exactly OV_OUT ids", "B overlay rows of OV_OUT + 1 ids",
                                     "B overlay rows of more than R_OUT ids (the second, writing walk)", "B overlay buffer flushed inside the '#' loop", "B overlay buffer flushed at the filter's end",
                                     "B overlay frontier beyond R_FRONT", "B '$' child of the overlay skipped by '+' at level 0", "B '$' child of the overlay skipped by '#' at level 0",
                                     "B a dead overlay topic above a live one", "B a deep filter of 17 levels matches a bulk and an overlay topic", "B a deep filter ending in '#' with matches",
                                     "B a deep filter with a mixed frontier chunk", "B a deep filter of 300 levels", "B a deep literal filter names a dead bulk topic", "B overlay rows of exactly R_OUT + 1 ids", "B overlay walk re-run for its range list", "B overlay walk re-run for its frontier",
                                     "B deep walk re-run for its range list", "C the filter '#' on a tenant with a '$' run", "C the filter '#' on a tenant without a '$' run"};
    for (int li = 0; li < 9; li++)
        for (int oi = 0; oi < 4; oi++) need.push_back("A range of " + std::to_string(LENS[li]) + " ids at word offset " + std::to_string(OFFS[oi]));
    for (int p = 0; p < 9; p++) need.push_back(std::string("A dead pattern: ") + DEAD_PATTERNS[p]);
    for (uint32_t l : {0u, 1u, 63u, 64u}) need.push_back("A k_limit_select with limit " + std::to_string(l));
    for (auto& k : need)
        if (g_cov[k] == 0) FAIL("coverage: no case reached '%s' (%d cases, seed %llu, R_FRONT %u R_OUT %u OV_OUT %u)\n", k.c_str(), cases, (unsigned long long)seed, R_FRONT, R_OUT, OV_OUT);
    printf("retain dyn emu ok: %d random cases, %d index rounds, seed %llu, R_FRONT %u R_OUT %u OV_OUT %u;", cases, rounds, (unsigned long long)seed, R_FRONT, R_OUT, OV_OUT);
    for (auto& kv : g_cov) printf(" %s: %llu;", kv.first.c_str(), kv.second);
    printf("\n");
    return 0;
}
