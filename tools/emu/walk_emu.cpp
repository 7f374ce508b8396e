// walk_emu.cpp -- host-side logic test of the dist direction's match kernels -- k_walk<TC, QC, PC, MIXED> (bmq_walk_kernel.h), k_walk_slow
// (bmq_dist_kernels.h) and k_expand behind them -- under the wave64 emulator of wave_emu.h, on indexes the product's own builder makes
// (bmq_dist_index.h through HostExec: the code the builder kernels run).  Test tooling: the kernels' LOGIC -- tokeniser and ragged token
// table, chunked waves, the work stack and the range buffer with their spill chains (smallest LDS lists), tenants of a wave walked one after
// the other, the MIXED instantiation for batches that are not grouped by tenant, '$' topics, empty levels, unknown tenants, topics deeper than
// FAST_LEVELS (k_walk_slow), indexes after mutations (id lists, indirect ranges), a directed family of unary chains for the tail records (every chain
// length, '+'/literal mask and leaf kind; topics that end inside a chain with a row behind them that continues it), a sequence of index states per round
// (fresh, a random batch, seven directed steps on the family's chains, region growth, compaction, records that begin with '+'; alternate rounds without
// records), every batch with the child filter words read and ignored, the count of discovered nodes of every batch (and of every row of the ordered
// batches) against a model of the trie's nodes, and the whole pipeline of an engine with bmq_config.dedup_sorted
// (k_dd_adj_heads -> k_dd_adj_scatter -> the walk kernels on the dense batch -> k_fill_adj -> k_expand, wired as launch_dist wires them) on
// ordered batches full of repeats -- against a brute force over the model's route keys (the rule of SURVEY.md 8a-0); behind k_expand of every batch the kernels
// of the RANGES result format (bmq_format_kernels.h) over the pairs the walk left, read by a consumer that follows include/bmq.h to the letter (run_format).  What the GPU makes of the same source is what tests/ (-m gpu) check against the oracle.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/walk_emu.cpp bifromq_amd/csrc/bmq_codec.cpp -o build/walk_emu -pthread && build/walk_emu [rounds] [seed]
//   add -fsanitize=address,undefined (ASAN_OPTIONS=detect_stack_use_after_return=0: the lanes are ucontext fibers): LDS arrays are function statics here, so a read or
//   write past one is reported -- both harnesses run clean that way (round 5)
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
namespace bmq {
inline uint32_t lds_word_at(const uint32_t* words, uint32_t rel) { // (bmq_dedup_adj_kernels.h comes along with bmq_dist_kernels.h)
    uint32_t w;
    memcpy(&w, reinterpret_cast<const uint8_t*>(words) + rel, 4);
    return w;
}
} // namespace bmq
#include "bmq_dist_kernels.h"
#include "bmq_format_kernels.h"

using namespace bmq;

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
// the rule itself, on level lists
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

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

template <class T> static T* buf(std::vector<uint8_t>& store, size_t n) {
    store.assign(n * sizeof(T) + 64, 0);
    return reinterpret_cast<T*>(store.data());
}

// the large areas kernels only read where they wrote (pairs, spill chunks, slow-walk scratch, ids): whatever the batch before left there, like device memory
template <class T> static T* buf_stale(std::vector<uint8_t>& store, size_t n) {
    if (store.size() < n * sizeof(T) + 64) store.assign(n * sizeof(T) + 64, 0xA5);
    return reinterpret_cast<T*>(store.data());
}

struct Coverage {
    uint64_t rows = 0, ids = 0, batches = 0, mixed = 0, slow_rows = 0, spills = 0, chunked = 0, sorted_rows = 0, after_apply = 0, two_tenant_waves = 0;
    uint64_t adj_batches = 0, adj_rows = 0, adj_walked = 0, adj_slow = 0;
    uint64_t split_blocks = 0, split_overflow = 0, split_adj = 0; // k_expand: heavy blocks expanded by four waves, blocks the list had no room for
    uint64_t fmt_ranges = 0, fmt_side_rows = 0, fmt_over_rows = 0, fmt_empty = 0, fmt_empty_lists = 0, fmt_overlap_rows = 0, fmt_overlap_over = 0, fmt_adj_rows = 0, fmt_fresh_rows = 0, fmt_fresh_over = 0, fmt_fresh_overlap_over = 0; // the RANGES format behind the walk
};

// The RANGES result format (bmq_format_kernels.h) over the pairs the walk left, launched as enqueue_ranges launches it; then a consumer that follows
// include/bmq.h to the letter: a row's ranges expanded in the order given, the row ordered only where a non-empty range begins at or below the last id
// of the non-empty range before it.  Its rows must be `rows` (which main compares with the brute force), its count of ordered rows sums[2].
static bool g_fresh_index = false; // the batch runs on an index as a rebuild / compaction left it: ids are ranks in key order
static int run_format(const BatchArgs& a, const std::vector<std::vector<uint32_t>>& rows, Coverage& cov, bool adj) {
    const uint32_t n = a.n_topics;
    static std::vector<uint8_t> s_cnt, s_ptr, s_out, s_side;
    static unsigned long long sums[4] = {~0ull, ~0ull, ~0ull, ~0ull}; // (reused from batch to batch, like the slot's)
    FmtArgs f{};
    f.ix = a.ix, f.pair_off = a.pair_off, f.pair_cnt = a.pair_cnt, f.pairs = a.pairs, f.ctr = a.ctr, f.n_topics = n;
    f.range_cap = 0, f.side_cap = 0; // an exact fit
    for (uint32_t t = 0; t < n; t++) {
        f.range_cap += a.pair_cnt[t];
        for (uint32_t i = 0; i < a.pair_cnt[t]; i++) {
            const uint32_t c = a.pairs[a.pair_off[t] + i].count;
            if (c & RANGE_INDIRECT) f.side_cap += c & ~RANGE_INDIRECT;
        }
    }
    f.cnt_r = buf_stale<uint32_t>(s_cnt, 2 * (size_t)(n + 1)), f.cnt_s = f.cnt_r + (n + 1);
    f.range_ptr = buf_stale<uint32_t>(s_ptr, 2 * (size_t)(n + 1)), f.side_ptr = f.range_ptr + (n + 1);
    f.out_ranges = buf_stale<MatchRange>(s_out, f.range_cap + 1), f.out_side = buf_stale<uint32_t>(s_side, f.side_cap + 1), f.sums = sums;
    const uint32_t blocks = (n + 1 + 255) / 256;
    wemu::grid_size() = blocks;
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t w = 0; w < 4; w++) wemu::run_wave(b, [&] { k_fmt_count(f); }, w);
    for (uint32_t t = 0, rr = 0, rs = 0; t <= n; t++) f.range_ptr[t] = rr, f.side_ptr[t] = rs, rr += f.cnt_r[t], rs += f.cnt_s[t];
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t w = 0; w < 4; w++) wemu::run_wave(b, [&] { k_fmt_emit(f); }, w);
    if (sums[3] != 0) FAIL("format: flags %llu on a complete batch with buffers that fit\n", sums[3]);
    if (sums[0] != f.range_cap || sums[1] != f.side_cap) FAIL("format: %llu ranges / %llu side ids, the pairs hold %llu / %llu\n", sums[0], sums[1], f.range_cap, f.side_cap);
    unsigned long long flagged = 0;
    for (uint32_t t = 0; t < n; t++) {
        std::vector<uint32_t> ids;
        bool bad = false, have = false, side = false;
        uint32_t last = 0, prev_first = 0;
        const uint32_t nr = f.range_ptr[t + 1] - f.range_ptr[t];
        for (uint32_t i = 0; i < nr; i++) {
            const MatchRange q = f.out_ranges[f.range_ptr[t] + i];
            const uint32_t len = q.count & ~RANGE_INDIRECT;
            if (q.count & RANGE_INDIRECT) {
                side = true;
                if (q.begin < f.side_ptr[t] || q.begin + len > f.side_ptr[t + 1]) FAIL("format row %u: the list [%u, +%u) leaves the row's side slice [%u, %u)\n", t, q.begin, len, f.side_ptr[t], f.side_ptr[t + 1]);
            }
            cov.fmt_empty += len == 0, cov.fmt_empty_lists += len == 0 && (q.count & RANGE_INDIRECT);
            if (len == 0) continue;
            const uint32_t first = (q.count & RANGE_INDIRECT) ? f.out_side[q.begin] : q.begin;
            if (have && first <= last) bad = true;
            if (have && nr <= 32 && first <= prev_first) FAIL("format row %u (%u ranges): first id %u behind first id %u: not ascending\n", t, nr, first, prev_first);
            prev_first = first;
            for (uint32_t k = 0; k < len; k++) ids.push_back((q.count & RANGE_INDIRECT) ? f.out_side[q.begin + k] : q.begin + k);
            last = ids.back(), have = true;
        }
        if (bad) std::sort(ids.begin(), ids.end());
        if (ids != rows[t]) FAIL("format row %u (%u ranges%s): the strict consumer's row of %zu ids is not the expanded row of %zu ids\n", t, nr, bad ? ", ordered" : "", ids.size(), rows[t].size());
        flagged += bad;
        // include/bmq.h: no row of up to 32 ranges overlaps after a rebuild; rows of more come as matched, and the walk does not match in id order
        if (g_fresh_index && bad && nr <= 32) FAIL("format row %u (%u ranges): ranges overlap on an index without mutations\n", t, nr);
        cov.fmt_fresh_rows += g_fresh_index, cov.fmt_fresh_over += g_fresh_index && nr > 32, cov.fmt_fresh_overlap_over += g_fresh_index && bad && nr > 32;
        cov.fmt_ranges += nr, cov.fmt_side_rows += side, cov.fmt_over_rows += nr > 32, cov.fmt_overlap_over += bad && nr > 32, cov.fmt_adj_rows += adj;
    }
    if (sums[2] != flagged) FAIL("format: a count of %llu rows whose ranges overlap, the strict consumer ordered %llu rows\n", sums[2], flagged);
    cov.fmt_overlap_rows += flagged;
    return 0;
}

// one batch through walk (+ slow) + expand; rows -> sorted id lists
template <int TC, int QC, int PC>
static int run_batch(const DistIndexView& ix, const std::vector<std::string>& tnames, const std::vector<uint32_t>& tt, const std::vector<std::string>& topics, uint32_t tpw_shift,
                     std::vector<std::vector<uint32_t>>& rows, Coverage& cov, bool adj, unsigned long long& n_visit, std::vector<uint32_t>& row_visit) {
    const uint32_t n = (uint32_t)topics.size();
    std::vector<uint8_t> tb, pb;
    std::vector<uint32_t> toff{0}, poff{0};
    for (auto& s : tnames) tb.insert(tb.end(), s.begin(), s.end()), toff.push_back((uint32_t)tb.size());
    for (auto& s : topics) pb.insert(pb.end(), s.begin(), s.end()), poff.push_back((uint32_t)pb.size());
    tb.resize(tb.size() + 32, 0), pb.resize(pb.size() + 32, 0);
    // the topic bytes 16-byte aligned, as the ABI asks
    std::vector<uint8_t> pstore(pb.size() + 32);
    uint8_t* pal = pstore.data() + ((16 - ((uintptr_t)pstore.data() & 15)) & 15);
    memcpy(pal, pb.data(), pb.size());
    const uint32_t nb = (n + (1u << tpw_shift) - 1) >> tpw_shift, n_super = ((nb - 1) >> SUPER_SHIFT) + 1;
    // (static: the large ones -- 32 MB of spill area -- keep their pages from batch to batch; buf() zeroes them)
    static std::vector<uint8_t> s_heavy;
    static std::vector<uint8_t> s_po, s_pc, s_rc, s_pairs, s_subs, s_super, s_stats, s_spill, s_ws, s_slow, s_scr, s_sort, s_ctr, s_row, s_ids, s_tot;
    static std::vector<uint8_t> s_drow, s_mask, s_cnt, s_asup, s_ctop, s_coff, s_cten, s_crep, s_cpo, s_cpc, s_crc, s_vis; // bmq_config.dedup_sorted: the dense batch and its results
    BatchArgs a{};
    a.ix = ix;
    a.tenants = tb.data(), a.tenant_off = toff.data(), a.n_tenants = (uint32_t)tnames.size();
    a.topic_tenant = tt.data(), a.topics = pal, a.topic_off = poff.data(), a.n_topics = n;
    a.pair_cap = 1u << 19, a.spill_cap = 1u << 21, a.slow_cap = n + 8, a.scratch_cap = 1u << 20, a.sort_cap = n + 8;
    a.n_blocks = nb, a.tpw_shift = tpw_shift;
    a.qcap = QC, a.pcap = PC;
    const uint64_t out_cap = 1u << 20;
    bool mixed = false;
    for (int attempt = 0; attempt < 3; attempt++) {
        a.pair_off = buf<uint32_t>(s_po, n), a.pair_cnt = buf<uint32_t>(s_pc, n), a.route_cnt = buf<uint32_t>(s_rc, n);
        a.pairs = buf_stale<MatchRange>(s_pairs, a.pair_cap), a.subs = buf<SubAlloc>(s_subs, 2 * N_SUB + 1);
        a.subs = reinterpret_cast<SubAlloc*>(((uintptr_t)a.subs + 127) & ~(uintptr_t)127);
        a.super_sums = buf<unsigned long long>(s_super, (size_t)n_super * SUPER_STRIDE), a.blk_stats = buf<uint4>(s_stats, nb);
        a.spill = buf_stale<uint4>(s_spill, a.spill_cap), a.wave_sums = buf<unsigned long long>(s_ws, nb);
        a.slow_list = buf<uint32_t>(s_slow, a.slow_cap), a.scratch = buf_stale<uint32_t>(s_scr, a.scratch_cap), a.sort_list = buf<uint32_t>(s_sort, a.sort_cap);
        a.ctr = buf<Counters>(s_ctr, 1);
        a.heavy_list = nullptr, a.heavy_cap = 0;
        if (tpw_shift == 6 && (n & 1u)) a.heavy_cap = 1 + (n >> 1) % 3, a.heavy_list = buf<uint32_t>(s_heavy, a.heavy_cap), a.split_ranges = 24, a.split_ids = 40; // (a list of 1-3 entries: it overflows)
        a.out_row_ptr = buf<uint32_t>(s_row, n + 1), a.out_ids = buf_stale<uint32_t>(s_ids, out_cap), a.out_capacity = out_cap;
        a.out_total = buf<unsigned long long>(s_tot, 1);
        wemu::grid_size() = nb;
        BatchArgs w = a; // what the walk kernels run on
        AdjFill gf{};
        if (adj) { // the wiring of launch_dist (bmq_engine.hip) for an engine with bmq_config.dedup_sorted
            AdjArgs g{};
            g.topics = a.topics, g.topic_off = a.topic_off, g.topic_tenant = a.topic_tenant, g.n_topics = n, g.n_blocks = nb, g.tpw_shift = tpw_shift;
            g.drow = buf<uint32_t>(s_drow, n), g.blk_mask = buf<unsigned long long>(s_mask, nb), g.blk_cnt = buf<unsigned long long>(s_cnt, nb);
            g.super_cnt = buf<unsigned long long>(s_asup, (size_t)n_super * SUPER_STRIDE);
            g.c_cap = pb.size() + 64;
            s_ctop.assign(g.c_cap + 128, 0xCD);
            g.c_topics = s_ctop.data() + ((16 - ((uintptr_t)s_ctop.data() & 15)) & 15);
            g.c_off = buf<uint32_t>(s_coff, n + 1), g.c_tenant = buf<uint32_t>(s_cten, n), g.c_rep = buf<uint32_t>(s_crep, n), g.ctr = a.ctr;
            for (uint32_t b = 0; b < nb; b++) wemu::run_wave(b, [&] { k_dd_adj_heads(g); });
            for (uint32_t b = 0; b < nb; b++) wemu::run_wave(nb - 1 - b, [&] { k_dd_adj_scatter(g); });
            if (a.ctr->status & ST_NEED_ADJ) FAIL("the dense batch did not fit a buffer as large as the batch\n");
            a.rep = g.drow, a.visit_cnt = buf<uint32_t>(s_vis, n);
            w = a;
            w.topics = g.c_topics, w.topic_off = g.c_off, w.topic_tenant = g.c_tenant, w.rep = g.c_rep;
            w.pair_off = buf<uint32_t>(s_cpo, n), w.pair_cnt = buf<uint32_t>(s_cpc, n), w.route_cnt = buf<uint32_t>(s_crc, n);
            gf = AdjFill{g.drow, w.pair_off, w.pair_cnt, w.route_cnt, w.visit_cnt};
        }
        for (uint32_t b = 0; b < nb; b++) {
            if (mixed) wemu::run_wave(b, [&] { k_walk<TC, QC, PC, true>(w); });
            else wemu::run_wave(b, [&] { k_walk<TC, QC, PC, false>(w); });
        }
        if ((a.ctr->status & ST_WANT_MIXED) && !mixed) { // the batch is not grouped by tenant: once more through the instantiation for that (bmq_engine.hip)
            mixed = true;
            cov.mixed++;
            continue;
        }
        if (a.ctr->status & ST_RERUN) FAIL("walk asked for larger buffers: status %u (the harness' are meant to be large enough)\n", a.ctr->status);
        if (a.ctr->slow_count) {
            cov.slow_rows += a.ctr->slow_count;
            if (adj) cov.adj_slow += a.ctr->slow_count;
            wemu::grid_size() = 2;
            for (uint32_t b = 0; b < 2; b++) wemu::run_wave(b, [&] { k_walk_slow(w); });
            if (a.ctr->status & ST_RERUN) FAIL("slow walk asked for larger buffers: status %u\n", a.ctr->status);
        }
        if (adj) {
            wemu::grid_size() = nb;
            for (uint32_t b = 0; b < nb; b++) wemu::run_wave(b, [&] { k_fill_adj(a, gf); });
            cov.adj_batches++, cov.adj_rows += n, cov.adj_walked += a.ctr->n_walked;
        }
        break;
    }
    {
        unsigned long long spilled = 0; // records handed out by the spill area's sub-allocators: a full range buffer was flushed, a full stack parked
        for (uint32_t i = 0; i < N_SUB; i++) spilled += a.subs[N_SUB + i].used;
        if (spilled) cov.spills++;
    }
    { // k_expand's grid as launch_dist lays it out: the helper waves of the heavy blocks in front
        const uint32_t grid = nb + (EXPAND_PARTS - 1) * a.heavy_cap;
        wemu::grid_size() = grid;
        for (uint32_t b = 0; b < grid; b++) wemu::run_wave(b, [&] { k_expand(a); });
        const uint32_t listed = std::min(a.ctr->heavy_count, a.heavy_cap);
        cov.split_blocks += listed, cov.split_overflow += a.ctr->heavy_count - listed;
        if (adj) cov.split_adj += listed;
        for (uint32_t i = 0; i < listed; i++)
            if (a.heavy_list[i] >= nb || a.blk_stats[a.heavy_list[i]].w != 1u) FAIL("heavy list entry %u: block %u is not flagged\n", i, a.heavy_list[i]);
    }
    if (a.ctr->status & (ST_NOSPACE | ST_RANGE | ST_RERUN)) FAIL("expand: status %u\n", a.ctr->status);
    if (*a.out_total != a.out_row_ptr[n]) FAIL("total %llu, row_ptr[n] %u\n", *a.out_total, a.out_row_ptr[n]);
    rows.assign(n, {});
    std::set<uint32_t> to_sort(a.sort_list, a.sort_list + std::min(a.ctr->sort_count, a.sort_cap));
    cov.sorted_rows += to_sort.size();
    for (uint32_t t = 0; t < n; t++) {
        rows[t].assign(a.out_ids + a.out_row_ptr[t], a.out_ids + a.out_row_ptr[t + 1]);
        if (to_sort.count(t)) std::sort(rows[t].begin(), rows[t].end()); // (k_sort_rows' business)
        else if (!std::is_sorted(rows[t].begin(), rows[t].end())) FAIL("row %u is not ascending and not listed for k_sort_rows\n", t);
        cov.ids += rows[t].size();
    }
    cov.rows += n, cov.batches++;
    if (run_format(a, rows, cov, adj)) return 1;
    n_visit = a.ctr->n_visit; // (summed by k_expand from the walk's block records / added by k_walk_slow)
    row_visit.clear();
    if (adj) // BatchArgs.visit_cnt is wired: per row of the dense batch; row t's figure is that of its run head
        for (uint32_t t = 0; t < n; t++) row_visit.push_back(a.visit_cnt[a.rep[t]]);
    return 0;
}

// The count of discovered nodes the walk must report (N_visit, the root excluded): the trie holds a node for every prefix (without a
// trailing '#') of every filter PUT since the last rebuild / compaction -- a delete removes routes, never nodes; a compaction builds from the live
// keys.  A topic discovers the nodes whose path matches one of its prefixes level by level, '+' matching any level but a '$' first one.
struct VisitModel {
    std::set<std::string> nodes; // tenant \0 level \0 level \0 ...
    void add(const std::string& tenant, const std::vector<std::string>& f) {
        std::string p = tenant + '\0';
        for (auto& l : f) {
            if (l == "#" && &l == &f.back()) break;
            p += l + '\0';
            nodes.insert(p);
        }
    }
    uint32_t visits(const std::string& tenant, const std::vector<std::string>& t) const {
        std::vector<std::string> frontier{tenant + '\0'}, next;
        uint32_t v = 0;
        for (size_t d = 0; d < t.size() && !frontier.empty(); d++) {
            next.clear();
            for (auto& p : frontier) {
                if (nodes.count(p + t[d] + '\0')) next.push_back(p + t[d] + '\0');
                if (!(d == 0 && !t[0].empty() && t[0][0] == '$') && nodes.count(p + "+" + '\0')) next.push_back(p + "+" + '\0');
            }
            v += (uint32_t)next.size();
            frontier.swap(next);
        }
        return v;
    }
};

// The tail family (tenant "fam"): below a literal stem of its own, one unary chain per chain length k (1 .. TAIL_K + 2: behind TAIL_K levels the record
// sits deeper), '+'/literal mask over the k levels and leaf kind (own routes / "<chain>/#" routes).  Chain tokens are a, b, c -- levels topics also START
// with: a topic that ends inside a chain is followed in the wave's token table by one whose first tokens continue the chain.
struct Chain {
    uint32_t idx, k;
    bool hash;
    std::vector<std::string> stem, lv, fill; // fill: the chain's levels with known tokens in the '+' positions
    std::string filter(size_t n_chain) const { // the stem and the first n_chain levels of the chain
        std::string f;
        for (auto& s : stem) f += (f.empty() ? "" : "/") + s;
        for (size_t i = 0; i < n_chain; i++) f += "/" + lv[i];
        return f;
    }
};
static std::string join(const std::vector<std::string>& v, size_t from = 0) {
    std::string s;
    for (size_t i = from; i < v.size(); i++) s += (i > from ? "/" : "") + v[i];
    return s;
}
static const char* const FAM_V[3] = {"a", "b", "c"};
static std::vector<Chain> make_family() {
    std::vector<Chain> out;
    for (uint32_t k = 1; k <= TAIL_K + 2; k++) {
        std::vector<uint32_t> masks;
        if (k <= TAIL_K) for (uint32_t m = 0; m < (1u << k); m++) masks.push_back(m);
        else masks = {0u, (1u << k) - 1u, 0x15u & ((1u << k) - 1u), 0x2Au & ((1u << k) - 1u)};
        for (uint32_t m : masks)
            for (int hash = 0; hash < 2; hash++) {
                Chain c;
                c.idx = (uint32_t)out.size(), c.k = k, c.hash = hash != 0;
                const std::string name = std::string(FAM_V[c.idx % 3]) + "0k" + std::to_string(k) + "m" + std::to_string(m) + (hash ? "h" : "o");
                if (c.idx % 4 == 1) c.stem = {"st", name};
                else if (c.idx % 4 == 3) c.stem = {"$fam", name}; // (a '$' first level: the root's wildcards must not match it)
                else c.stem = {name};
                for (uint32_t l = 0; l < k; l++) {
                    c.lv.push_back(((m >> l) & 1u) ? "+" : FAM_V[(l + c.idx) % 3]);
                    c.fill.push_back(((m >> l) & 1u) ? FAM_V[(l + c.idx + 1) % 3] : c.lv.back());
                }
                out.push_back(c);
            }
    }
    return out;
}
// a chain's topics, as blocks of rows that stay together in batch order: {short topic, the neighbour that continues its chain} pairs, the others alone
static void family_topics(const Chain& c, std::vector<std::vector<std::string>>& blocks) {
    std::vector<std::string> base = c.stem;
    base.insert(base.end(), c.fill.begin(), c.fill.end());
    const size_t ns = c.stem.size();
    blocks.push_back({join(base)});                                       // the full path
    for (size_t len = 1; len < base.size(); len++) {                      // every proper prefix
        std::vector<std::string> p(base.begin(), base.begin() + (long)len);
        if (len < ns) blocks.push_back({join(p)});
        else { // ends with len - ns levels of the chain consumed: the row behind it starts with the chain's next levels (+ one more on every other chain)
            std::vector<std::string> nb(c.fill.begin() + (long)(len - ns), c.fill.end());
            if ((c.idx + len) & 1u) nb.push_back("a");
            blocks.push_back({join(p), join(nb)});
        }
    }
    blocks.push_back({join(base) + "/a"}), blocks.push_back({join(base) + "/a/b"}); // one and two levels beyond the leaf
    for (uint32_t i = 0; i < c.k; i++) {                                            // one level off at each position
        std::vector<std::string> p = base;
        p[ns + i] = "zz"; // (a level the dictionary does not know)
        blocks.push_back({join(p)});
        p[ns + i] = FAM_V[(i + c.idx + 2) % 3]; // (a known one that is neither the chain's nor the fill)
        blocks.push_back({join(p)});
        if (c.lv[i] == "+") { // '+' positions: a level the dictionary does not know, the empty level
            p[ns + i] = "qq" + std::to_string(c.idx), blocks.push_back({join(p)});
            p[ns + i] = "", blocks.push_back({join(p)});
        }
    }
    if (ns == 1) blocks.push_back({"$" + join(base)}); // (a '$' first level where the stem is the first level: no such stem)
    for (const char* l : {"n", "m"}) { // the children the directed steps put below the chain's inner node
        std::vector<std::string> p(base.begin(), base.begin() + (long)(ns + c.idx % c.k));
        p.push_back(l);
        blocks.push_back({join(p)});
    }
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 12;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    const std::vector<std::string> tenants = {"t", "tenantB", "x", "a-much-longer-tenant-identifier", ""};
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "+", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "0", "exactly-16-bytes", "#"};
    auto rand_filter = [&](size_t max_depth) {
        std::string f;
        const size_t depth = 1 + rnd(max_depth);
        for (size_t i = 0; i < depth; i++) {
            if (i) f += '/';
            if (i + 1 == depth && rnd(5) == 0) f += "#";
            else {
                std::string l = alpha[rnd(alpha.size())];
                if (l == "#") l = "#x";
                f += l;
            }
        }
        return f;
    };
    auto rand_topic = [&](size_t max_depth) {
        std::string t;
        const size_t depth = 1 + rnd(max_depth);
        for (size_t i = 0; i < depth; i++) {
            if (i) t += '/';
            std::string l = alpha[rnd(alpha.size())];
            if (l == "+" || l == "#") l = "zz";
            t += l;
        }
        return t;
    };
    auto rand_key = [&](size_t max_depth) {
        const std::string& tn = tenants[rnd(tenants.size())];
        const uint8_t flag = rnd(10) == 0 ? 2 : 1;
        return encode_route_key(tn, rand_filter(max_depth), flag,
                                flag == 1 ? std::to_string(rnd(3)) + std::string("\0", 1) + "inbox" + std::to_string(rnd(40)) + std::string("\0d", 2) + std::to_string(rnd(12))
                                          : "g" + std::to_string(rnd(3)));
    };
    auto fam_key = [](const std::string& filter, const std::string& rcv) { return encode_route_key("fam", filter, 1, std::string("0\0", 2) + rcv + std::string("\0d", 2)); };
    const std::vector<Chain> family = make_family();
    auto chain_keys = [&](const Chain& c) { // the leaf's routes: one receiver, on every third chain two
        std::vector<std::string> ks;
        const std::string f = c.filter(c.k) + (c.hash ? "/#" : "");
        ks.push_back(fam_key(f, "leaf" + std::to_string(c.idx)));
        if (c.idx % 3 == 0) ks.push_back(fam_key(f, "second" + std::to_string(c.idx)));
        return ks;
    };
    Coverage cov;
    unsigned long long moved_plus = 0, visits_compared = 0, rows_visit_compared = 0, states = 0, continuation_pairs = 0, ordered_pairs = 0;
    for (int round = 0; round < rounds; round++) {
        HostExec hx;
        hx.threads = 2;
        DistIndex<HostExec> h(hx);
        h.tiny = round % 3 != 2;
        h.tail_records = round % 2 == 0; // (alternate rounds: no records -- the same rows and the same visits)
        std::map<std::string, uint32_t> model;
        VisitModel vis;
        const size_t max_depth = round % 4 == 3 ? 22 : 5; // (every fourth round: filters and topics deeper than FAST_LEVELS)
        auto note_put = [&](const std::string& key) {
            RouteKeyParts kp;
            if (decode_route_key(key, kp)) vis.add(std::string(kp.tenant), split(kp.esc_filter, '\0'));
        };
        {
            std::set<std::string> ks;
            const size_t nk = 1 + rnd(round % 3 == 0 ? 4000 : 600);
            for (size_t i = 0; i < nk; i++) ks.insert(rand_key(max_depth));
            if (round % 4 == 1) // a family that branches at every level (tenant "x"): every mix of literal and '+' over five levels, and '#' behind every prefix of those --
                                // a wave of such topics holds hundreds of pending items (both stacks of the work list are parked) and emits more than 64 ranges in one sink
                for (uint32_t m = 0; m < 32; m++)
                    for (uint32_t d = 1; d <= 5; d++) {
                        std::string f;
                        for (uint32_t l = 0; l < d; l++) f += (l ? "/" : "") + (((m >> l) & 1u) ? std::string("+") : "w" + std::to_string(l));
                        if (d < 5 && (m >> d) != 0) continue;
                        ks.insert(encode_route_key("x", f, 1, std::string("0\0wide\0d", 8) + std::to_string(m))); // (below depth 5: a node with routes of its own AND '#' routes)
                        if (d < 5) ks.insert(encode_route_key("x", f + "/#", 1, std::string("0\0wide#\0d", 9) + std::to_string(m)));
                    }
            for (size_t i = 0; i < 40; i++) ks.insert(encode_route_key("t", "a/b", 1, "0" + std::string("\0", 1) + "fan" + std::to_string(i) + std::string("\0d", 2))); // one filter, many receivers
            // the tail family, and beside it the root's '+' child P0 and its '+' child PP0 with many literal children each (their Bloom words fill up:
            // the child filter words of P0 / PP0 are what spares the probes) and a route of their own (it leaves and comes back below)
            for (auto& c : family)
                for (auto& k : chain_keys(c)) ks.insert(k);
            ks.insert(fam_key("+", "p0")), ks.insert(fam_key("+/+", "pp0"));
            // a filter whose id set becomes a list and is emptied: "el/x" holds one route from here, gets two by apply and loses all three; its sibling "el/+" keeps one
            ks.insert(fam_key("el/x", "e0")), ks.insert(fam_key("el/+", "sib"));
            for (uint32_t i = 0; i < 40; i++) ks.insert(fam_key("+/f" + std::to_string(i), "p0c")), ks.insert(fam_key("+/+/f" + std::to_string(i), "pp0c"));
            std::vector<uint8_t> bytes;
            std::vector<uint32_t> off{0};
            uint32_t r = 0;
            for (auto& k : ks) {
                model[k] = r++;
                note_put(k);
                bytes.insert(bytes.end(), k.begin(), k.end());
                off.push_back((uint32_t)bytes.size());
            }
            bytes.resize(bytes.size() + 16, 0);
            if (!h.rebuild(bytes.data(), off.data(), (uint32_t)ks.size())) FAIL("rebuild: %s\n", h.error.c_str());
        }
        uint32_t next_id = (uint32_t)model.size();
        // one apply batch, mirrored in the model: ops in order; the n-th put of the batch gets id next_id + n whether it is new or not
        auto apply_ops = [&](const std::vector<std::string>& keys, const std::vector<uint8_t>& ops) -> int {
            uint32_t put_no = 0;
            for (size_t i = 0; i < keys.size(); i++) {
                if (ops[i]) model.erase(keys[i]);
                else {
                    if (!model.count(keys[i])) model[keys[i]] = next_id + put_no;
                    note_put(keys[i]);
                    put_no++;
                }
            }
            next_id += put_no;
            std::vector<uint8_t> bytes;
            std::vector<uint32_t> off{0};
            for (auto& k : keys) bytes.insert(bytes.end(), k.begin(), k.end()), off.push_back((uint32_t)bytes.size());
            bytes.resize(bytes.size() + 16, 0);
            if (!h.apply(bytes.data(), off.data(), ops.data(), (uint32_t)keys.size())) FAIL("apply: %s\n", h.error.c_str());
            cov.after_apply++;
            return 0;
        };
        // The index states of a round, all four batch kinds matched after each.  The directed steps each take a part of the family of their own (chain
        // index mod 8), so that the records of the other chains live on beside the tombstones.  The steps that add no node come first: with the minimal
        // capacities of `tiny` every new node grows the tenant's region, and a growth drops its records and tombstones (every third round is not tiny).
        enum { S_FRESH, S_RANDOM, S_OWN_ON_INNER, S_OTHER_KIND, S_LEAVE, S_BACK, S_BELOW_INNER, S_BLINK, S_GROW, S_COMPACT, S_MOVED_PLUS, S_COUNT, S_DIRECTED = S_OWN_ON_INNER };
        static const char* const state_name[S_COUNT] = {"fresh", "random batch", "own route on an inner chain node", "other kind of route on a leaf", "last route leaves", "route comes back",
                                                        "put below an inner chain node", "put + delete in one batch", "region growth", "compacted", "'+' children moved to their hashed homes"};
        for (int state = 0; state < S_COUNT; state++) {
            std::vector<std::string> keys;
            std::vector<uint8_t> ops;
            auto put = [&](const std::string& k) { keys.push_back(k), ops.push_back(0); };
            auto del = [&](const std::string& k) { keys.push_back(k), ops.push_back(1); };
            auto part = [&](const Chain& c) { return (int)(c.idx % 8) == state - S_DIRECTED; };
            if (state == S_RANDOM) { // ids out of key order, id lists, dead ids
                const size_t nm = 1 + rnd(400);
                for (size_t i = 0; i < nm; i++) {
                    if (!model.empty() && rnd(2)) {
                        auto it = model.begin();
                        std::advance(it, rnd(std::min<size_t>(model.size(), 300)));
                        del(it->first);
                    } else put(rand_key(max_depth));
                }
            }
            for (auto& c : family) {
                if (state < S_DIRECTED || state >= S_COMPACT || !part(c)) continue;
                const size_t j = c.idx % c.k; // the inner node: the stem and j levels of the chain (j = 0: the head itself)
                const std::string tag = std::to_string(c.idx);
                if (state == S_BELOW_INNER) put(fam_key(c.filter(j) + "/n", "below" + tag));
                if (state == S_OWN_ON_INNER) put(fam_key(c.filter(j), "inner" + tag));
                if (state == S_OTHER_KIND) put(fam_key(c.filter(c.k) + (c.hash ? "" : "/#"), "other" + tag));
                if (state == S_LEAVE)
                    for (auto& k : chain_keys(c)) del(k);
                if (state == S_BLINK) { // (a new child beside, as in the child filter test)
                    const std::string k = fam_key(c.filter(c.k) + (c.hash ? "/#" : ""), "blink" + tag);
                    put(k), put(fam_key(c.filter(j) + "/m", "beside" + tag)), del(k);
                }
                if (state == S_GROW)
                    for (uint32_t g = 0; g < 12; g++) put(fam_key(c.filter(j) + "/g" + std::to_string(g) + "/w", "grow" + tag));
            }
            if (state == S_BACK)
                for (auto& c : family)
                    if ((int)(c.idx % 8) == S_LEAVE - S_DIRECTED)
                        for (auto& k : chain_keys(c)) put(k);
            // the own routes of P0 and PP0 leave with the leaves and come back with them: in between their own filter words are all-ones
            if (state == S_LEAVE) del(fam_key("+", "p0")), del(fam_key("+/+", "pp0"));
            if (state == S_OWN_ON_INNER) put(fam_key("el/x", "e1")), put(fam_key("el/x", "e2"));
            if (state == S_OTHER_KIND) del(fam_key("el/x", "e0")), del(fam_key("el/x", "e1")), del(fam_key("el/x", "e2"));
            if (state == S_BACK) put(fam_key("+", "p0")), put(fam_key("+/+", "pp0"));
            if (!keys.empty() && apply_ops(keys, ops)) return 1;
            if (state == S_COMPACT) { // a new generation from the live keys: ids are ranks again, nodes without routes below them are gone
                if (!h.compact()) FAIL("compact: %s\n", h.error.c_str());
                uint32_t r = 0;
                vis.nodes.clear();
                for (auto& e : model) e.second = r++, note_put(e.first);
                next_id = r;
            }
            if (state == S_MOVED_PLUS) {
                // A hand-made image, the only one here.  The builder puts the '+' child of X beside X whenever that slot is free, and a record needs the very
                // same slot: no image it makes holds a record whose FIRST level is '+', yet the walk promises to read one (r0 == TOK_PLUS).  So: in
                // the family's tenant every '+' child that lies beside a parent it is the only child of moves to where the layout puts it when the slot is
                // taken -- the first free slot from its hashed home on -- and the tail pass runs again: the parent now carries a record that begins with
                // '+'.  (Where the pass forms none, a tombstone keeps the vacated slot occupied: probe chains that ran across it stay whole.)
                if (!h.tail_records) continue;
                for (uint32_t d = 0; d < h.dir_slots; d++) {
                    const TenantSlot t = h.dir[d];
                    if (!(t.hash_lo | t.hash_hi) || t.name_len != 3 || memcmp(t.name12, "fam", 3) != 0) continue;
                    std::map<uint32_t, uint32_t> n_kids;
                    for (uint32_t sl = 0; sl < 2 * t.buckets; sl++)
                        if (slot_is_node(h.trie[t.base + sl])) n_kids[h.trie[t.base + sl].parent]++;
                    std::vector<std::pair<uint32_t, uint32_t>> vacated; // (slot, parent's node id)
                    for (uint32_t sl = 0; sl < 2 * t.buckets; sl++) {
                        const TrieSlot p = h.trie[t.base + sl], xs = h.trie[t.base + (sl ^ 1u)];
                        if (!slot_is_node(p) || p.token != TOK_PLUS || !slot_is_node(xs) || xs.node != p.parent || n_kids[xs.node] != 1) continue;
                        uint32_t bk = edge_bucket(p.parent, TOK_PLUS, t.buckets), dst = NONE;
                        for (uint32_t probes = 0; probes < t.buckets && dst == NONE; probes++, bk = bk + 1 == t.buckets ? 0 : bk + 1)
                            for (uint32_t j = 0; j < 2 && dst == NONE; j++)
                                if (h.trie[t.base + 2 * bk + j].parent == NONE) dst = 2 * bk + j;
                        if (dst == NONE) continue;
                        h.trie[t.base + dst] = p;
                        h.trie[t.base + sl] = FREE_SLOT;
                        vacated.emplace_back(sl, xs.node);
                    }
                    if (!h.form_tails()) FAIL("tail pass: %s\n", h.error.c_str());
                    for (auto& v : vacated)
                        if (h.trie[t.base + v.first].parent == NONE) h.trie[t.base + v.first] = TrieSlot{v.second, TOK_TOMB, 0, 0, 0, 0, NONE, 0};
                        else moved_plus++;
                }
            }
            states++;
            // the model per tenant: (filter levels, id)
            std::map<std::string, std::vector<std::pair<std::vector<std::string>, uint32_t>>> by_tenant;
            for (auto& e : model) {
                RouteKeyParts kp;
                if (!decode_route_key(e.first, kp)) FAIL("model key does not decode\n");
                by_tenant[std::string(kp.tenant)].emplace_back(split(kp.esc_filter, '\0'), e.second);
            }
            const bool directed = state >= S_DIRECTED && state < S_COMPACT;
            for (int bt = 0; bt < 4; bt++) {
                std::vector<std::string> tnames = tenants;
                tnames.push_back("ghost"); // a tenant the index does not know
                tnames.push_back("fam");
                const uint32_t fam_t = (uint32_t)tnames.size() - 1;
                const uint32_t shifts[3] = {6, 4, 2};
                const bool sweep = state == S_FRESH && bt == 0 && h.tail_records; // once per round with records: every topic of every chain, on the fresh image
                const uint32_t tpw_shift = sweep ? 6 : shifts[(round + bt + state) % 3];
                const uint32_t n0 = 1 + (uint32_t)rnd(directed ? 12 : tpw_shift == 6 ? (state == S_FRESH ? 330 : 60) : (state == S_FRESH ? 60 : 30)); // (the round's first batches as large as ever; the many after them small)
                // rows in blocks that stay together: a random topic alone; a family chain's short topic with the row that continues its chain
                std::vector<std::vector<std::pair<uint32_t, std::string>>> blocks;
                for (uint32_t i = 0; i < n0; i++) {
                    if (round % 4 == 1 && rnd(3) != 0) { // the branching family's topics: the full path, a prefix of it, one level off
                        std::string t;
                        const uint32_t d = rnd(3) == 0 ? 1 + (uint32_t)rnd(5) : 5, off = rnd(5) == 0 ? (uint32_t)rnd(5) : 99;
                        for (uint32_t l = 0; l < d; l++) t += (l ? "/" : "") + (l == off ? std::string("zz") : "w" + std::to_string(l));
                        blocks.push_back({{2u /* "x" */, t}});
                    } else blocks.push_back({{(uint32_t)rnd(tnames.size() - 1), rnd(12) == 0 ? std::string() : rand_topic(max_depth)}});
                }
                // the family: the chains of the step just taken (a directed state) and a few of the others
                std::vector<std::pair<std::string, std::string>> pairs; // (short topic, continuation) of this batch
                for (auto& c : family) {
                    const bool touched = directed && ((int)(c.idx % 8) == state - S_DIRECTED || (state == S_BACK && (int)(c.idx % 8) == S_LEAVE - S_DIRECTED));
                    if (!sweep && rnd(touched ? (tpw_shift == 6 ? 4 : 6) : directed ? 80 : (tpw_shift == 6 ? (state == S_MOVED_PLUS ? 12 : 30) : 50)) != 0) continue;
                    std::vector<std::vector<std::string>> fb;
                    family_topics(c, fb);
                    for (auto& b : fb) {
                        if (!sweep && rnd(2)) continue; // (half of a chain's topics per batch)
                        std::vector<std::pair<uint32_t, std::string>> blk;
                        for (auto& t : b) blk.emplace_back(fam_t, t);
                        if (b.size() == 2) pairs.emplace_back(b[0], b[1]), continuation_pairs++;
                        blocks.insert(blocks.begin() + (long)rnd(blocks.size() + 1), blk); // (anywhere among the others: a wave of an ungrouped batch holds many tenants)
                    }
                }
                blocks.insert(blocks.begin() + (long)rnd(blocks.size() + 1), {{fam_t, "el/x"}}); // (the emptied list and its sibling)
                std::vector<std::pair<uint32_t, std::string>> rowsrc;
                for (auto& b : blocks) rowsrc.insert(rowsrc.end(), b.begin(), b.end());
                const bool grouped = bt != 2; // the third batch of a state arrives in any order: waves hold many tenants each (MIXED)
                const bool ordered = bt == 3;  // the fourth: ordered by (tenant, topic), every row up to four times -- through the neighbour-compare kernels (dedup_sorted)
                if (ordered) {
                    const size_t m = rowsrc.size();
                    for (size_t i = 0; i < m; i++)
                        for (size_t c = rnd(state == S_FRESH ? 4 : 2); c > 0; c--) rowsrc.push_back(rowsrc[i]);
                    std::sort(rowsrc.begin(), rowsrc.end());
                    // An ordered batch decides itself who follows whom.  For two of the pairs the rows that sort between the short topic and its
                    // continuation are taken out: the continuation's tokens then lie directly behind the short topic's in the dense batch too.
                    for (int n_pairs = 0, tries = 0; n_pairs < 2 && tries < 20 && !pairs.empty(); tries++) {
                        const auto& pr = pairs[rnd(pairs.size())];
                        const std::pair<uint32_t, std::string> lo{fam_t, pr.first}, hi{fam_t, pr.second};
                        if (!(lo < hi)) continue;
                        auto b = std::upper_bound(rowsrc.begin(), rowsrc.end(), lo), e = std::lower_bound(rowsrc.begin(), rowsrc.end(), hi);
                        if (b == rowsrc.begin() || *(b - 1) != lo || e == rowsrc.end() || *e != hi || e < b) continue; // (an earlier cut took one of them)
                        rowsrc.erase(b, e);
                        n_pairs++, ordered_pairs++;
                    }
                } else if (grouped) std::stable_sort(rowsrc.begin(), rowsrc.end(), [](auto& x, auto& y) { return x.first < y.first; });
                std::vector<uint32_t> tt;
                std::vector<std::string> topics;
                for (auto& r : rowsrc) tt.push_back(r.first), topics.push_back(r.second);
                const bool small_lists = (round + bt + state) % 2 == 1; // the smallest LDS lists: stack and range buffer spill all the time
                const uint32_t n = (uint32_t)topics.size();             // (the ordered batch grew)
                const char* const order_name = ordered ? "ordered + dedup_sorted" : grouped ? "grouped" : "any order";
                // what the rule and the node model say
                std::vector<std::vector<uint32_t>> want(n);
                std::vector<uint32_t> want_visit(n, 0);
                unsigned long long want_visits = 0;
                for (uint32_t i = 0; i < n; i++) {
                    const auto tl = split(topics[i], '/');
                    auto it = by_tenant.find(tnames[tt[i]]);
                    if (it != by_tenant.end())
                        for (auto& fe : it->second)
                            if (filter_matches(fe.first, tl)) want[i].push_back(fe.second);
                    std::sort(want[i].begin(), want[i].end());
                    want_visits += want_visit[i] = vis.visits(tnames[tt[i]], tl);
                }
                // every batch twice: the walk reading the child filter words and ignoring them -- the same rows, the same visits
                for (int sw = 0; sw < 2; sw++) {
                    DistIndexView ix = h.view();
                    ix.filter_off = sw ? 0xFFFFFFFFu : 0u;
                    g_fresh_index = state == S_FRESH || state == S_COMPACT;
                    std::vector<std::vector<uint32_t>> got;
                    std::vector<uint32_t> row_visit;
                    unsigned long long n_visit = 0;
                    const int rc = small_lists ? run_batch<BMQ_WALK_GEOM_SMALLEST>(ix, tnames, tt, topics, tpw_shift, got, cov, ordered, n_visit, row_visit)
                                               : run_batch<BMQ_WALK_GEOM_DEFAULT>(ix, tnames, tt, topics, tpw_shift, got, cov, ordered, n_visit, row_visit);
#define WHERE "round %d state '%s' batch %d (n %u, tpw %u, %s, %s lists, tail records %s, child filters %s; seed %llu)"
#define WHERE_ARGS round, state_name[state], bt, n, 1u << tpw_shift, order_name, small_lists ? "smallest" : "default", h.tail_records ? "on" : "off", sw ? "ignored" : "read", (unsigned long long)seed
                    if (rc) FAIL(WHERE " failed\n", WHERE_ARGS);
                    for (uint32_t i = 0; i < n; i++)
                        if (got[i] != want[i])
                            FAIL(WHERE " row %u: tenant '%s' topic '%s': kernels give %zu ids, the rule %zu\n", WHERE_ARGS, i, tnames[tt[i]].c_str(), topics[i].c_str(), got[i].size(), want[i].size());
                    for (uint32_t i = 0; i < (uint32_t)row_visit.size(); i++, rows_visit_compared++)
                        if (row_visit[i] != want_visit[i])
                            FAIL(WHERE " row %u: tenant '%s' topic '%s': visits: the walk counts %u discovered nodes, the trie of the filters put holds %u\n", WHERE_ARGS, i, tnames[tt[i]].c_str(),
                                 topics[i].c_str(), row_visit[i], want_visit[i]);
                    if (n_visit != want_visits) FAIL(WHERE ": visits: Counters.n_visit %llu, the trie of the filters put holds %llu\n", WHERE_ARGS, n_visit, want_visits);
                    visits_compared++;
                }
            }
        }
    }
    printf("walk emu ok: %d rounds, %llu batches (%llu through the MIXED instantiation, %llu on an index after mutations), %llu rows, %llu ids, %llu rows through k_walk_slow, "
           "%llu batches with spill chains, %llu rows left to k_sort_rows; %llu ordered batches through the neighbour-compare kernels (%llu rows, %llu walked, %llu of those by k_walk_slow)\n",
           rounds, (unsigned long long)cov.batches, (unsigned long long)cov.mixed, (unsigned long long)cov.batches - 8ull * rounds, (unsigned long long)cov.rows, (unsigned long long)cov.ids,
           (unsigned long long)cov.slow_rows, (unsigned long long)cov.spills, (unsigned long long)cov.sorted_rows, (unsigned long long)cov.adj_batches, (unsigned long long)cov.adj_rows,
           (unsigned long long)cov.adj_walked, (unsigned long long)cov.adj_slow);
    printf("index states: %llu (fresh, random batch, seven directed steps, compacted, '+' children moved -- per round), every batch with the child filter words read and ignored; visits: %llu batches "
           "compared with the node model, %llu rows of ordered batches one by one; %llu short topics with a continuation row behind them (%llu of them in ordered batches); %llu records that begin with '+' made by hand\n",
           states, visits_compared, rows_visit_compared, continuation_pairs, ordered_pairs, moved_plus);
    printf("k_expand splitting: %llu heavy blocks expanded by four waves (%llu of them behind k_fill_adj), %llu more the list had no room for\n", (unsigned long long)cov.split_blocks,
           (unsigned long long)cov.split_adj, (unsigned long long)cov.split_overflow);
    if (rounds >= 8 && (!cov.split_blocks || !cov.split_overflow || !cov.split_adj)) FAIL("coverage: the cases missed k_expand's split blocks: %llu listed, %llu overflowed, %llu in ordered batches\n",
                                                                                         (unsigned long long)cov.split_blocks, (unsigned long long)cov.split_overflow, (unsigned long long)cov.split_adj);
    printf("RANGES format behind every batch: %llu ranges, %llu rows with side lists, %llu rows of more than 32 ranges (%llu of them with overlapping ranges), %llu empty ranges (%llu of them "
           "emptied id lists), %llu rows the strict consumer ordered, %llu rows of ordered batches; on indexes without mutations %llu rows, %llu of more than 32 ranges, %llu of those with overlapping ranges\n",
           (unsigned long long)cov.fmt_ranges, (unsigned long long)cov.fmt_side_rows, (unsigned long long)cov.fmt_over_rows, (unsigned long long)cov.fmt_overlap_over,
           (unsigned long long)cov.fmt_empty, (unsigned long long)cov.fmt_empty_lists, (unsigned long long)cov.fmt_overlap_rows, (unsigned long long)cov.fmt_adj_rows,
           (unsigned long long)cov.fmt_fresh_rows, (unsigned long long)cov.fmt_fresh_over, (unsigned long long)cov.fmt_fresh_overlap_over);
    // (no floor on empty ranges: an id list emptied by deletes goes back to (0, 0) -- bmq_build_core.h, the end of the group step -- and k_walk emits no range of count 0;
    // the directed filter "el/x" below is such a list.  tools/emu/format_emu.cpp feeds the format kernels empty ranges directly)
    if (rounds >= 8 && (!cov.fmt_side_rows || !cov.fmt_over_rows || !cov.fmt_fresh_over || !cov.fmt_overlap_rows || !cov.fmt_adj_rows))
        FAIL("coverage: the cases missed a shape of the RANGES format: rows with side lists %llu, rows of more than 32 ranges %llu (%llu on an index without mutations), ordered rows %llu\n",
             (unsigned long long)cov.fmt_side_rows, (unsigned long long)cov.fmt_over_rows, (unsigned long long)cov.fmt_fresh_over, (unsigned long long)cov.fmt_overlap_rows);
    printf("k_walk's work stack and range buffer: the range buffer flushed %llu times, the stack parked %llu times, %llu chunks taken back\n", walk_cov.flushes, walk_cov.parks, walk_cov.restores);
    if (rounds >= 8 && (walk_cov.flushes < 20 || walk_cov.parks < 20 || walk_cov.restores < 20)) FAIL("coverage: the cases hardly touched the cold paths of k_walk's lists\n");
    printf("tail records: %llu read, %llu chain levels resolved from them, %llu leaves reached, %llu tombstones met\n", walk_cov.tails, walk_cov.tail_levels, walk_cov.tail_leaves, walk_cov.tombs);
    if (rounds >= 8 && (walk_cov.tails < 100 || walk_cov.tail_leaves == 0)) FAIL("coverage: the cases hardly read a tail record\n");
    // the coverage a run must reach: every record length and leaf kind reached, stopped at and run out of at every level; '+' at every record level;
    // a tombstone; every child filter site with a spared probe and an all-ones word
    int missing = 0;
    for (uint32_t k = 1; k <= TAIL_K; k++)
        for (uint32_t kind = 0; kind < 2; kind++) {
            printf("  k=%u %s: leaf reached %llu; stopped after j levels:", k, kind ? "'#' " : "own", walk_cov.tail_reach[k][kind]);
            for (uint32_t j = 0; j < k; j++) printf(" %u:%llu", j, walk_cov.tail_stop[k][kind][j]);
            printf("; topic ran out after j:");
            for (uint32_t j = 1; j < k; j++) printf(" %u:%llu", j, walk_cov.tail_short[k][kind][j]);
            printf("\n");
            missing += walk_cov.tail_reach[k][kind] == 0;
            for (uint32_t j = 0; j < k; j++) missing += walk_cov.tail_stop[k][kind][j] == 0;
            for (uint32_t j = 1; j < k; j++) missing += walk_cov.tail_short[k][kind][j] == 0;
        }
    printf("  '+' matched at record level 1..4: %llu %llu %llu %llu\n", walk_cov.tail_plus[0], walk_cov.tail_plus[1], walk_cov.tail_plus[2], walk_cov.tail_plus[3]);
    for (uint32_t j = 0; j < TAIL_K; j++) missing += walk_cov.tail_plus[j] == 0;
    missing += walk_cov.tombs == 0;
    static const char* const site[3] = {"boot P0/PP0", "drain node", "drain '+' sibling"};
    for (int s = 0; s < 3; s++) {
        printf("  child filter words, %s: %llu probes spared, %llu decisions on an all-ones word\n", site[s], walk_cov.cf_spared[s], walk_cov.cf_ones[s]);
        missing += (walk_cov.cf_spared[s] == 0) + (walk_cov.cf_ones[s] == 0);
    }
    if (rounds >= 8 && missing) FAIL("coverage: %d of the tail record / child filter cases above were never met\n", missing);
    if (rounds >= 8 && (!cov.mixed || !cov.slow_rows || !cov.spills || !cov.adj_slow || cov.adj_walked >= cov.adj_rows)) FAIL("coverage: the cases missed a path: mixed %llu slow %llu spills %llu\n", (unsigned long long)cov.mixed, (unsigned long long)cov.slow_rows, (unsigned long long)cov.spills);
    return 0;
}
