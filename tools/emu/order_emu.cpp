// order_emu.cpp -- host-side logic test of the kernels of the key-ordered window (bifromq_amd/csrc/bmq_order_kernels.h: k_o_flag, k_o_pivots,
// k_o_bucket, k_o_scatter, k_o_leaves) under the wave64 emulator of wave_emu.h.  Test tooling: the kernels' LOGIC -- the cursor staged in
// LDS per wave, the ballot compaction of the candidates, the ranking of the pivots (a wave per pivot, ballots of 64 compares), the binary search over them, the per-wave histogram,
// the scatter that takes a bin's places with one atomic per wave and bin, the rank sort of a bucket -- each against a brute force over
// std::sort with memcmp written plainly below.  No index runs here: the harness builds a key pool and its references directly.
//
// What the cases hold: keys over a five-letter alphabet with bytes >= 0x80, stems of 0, 15, 16, 17, 33, 100 and 300 bytes, keys that are proper
// prefixes of one another, random gaps between the keys of the pool (so that what follows a key differs and every alignment occurs), dead
// ids; cursors absent, equal to a key, a proper prefix of one, a key plus a byte, below and above all keys, longer than a wave and longer than the LDS staging,
// given by id, inclusive and exclusive; grids of 1 to 3 workgroups, so that every pass strides; lists that end at, before and behind a
// wave; bins that are dropped; buckets of 1, 2, 63 .. 65, 255 .. 257 and ORDER_BUCKET_MAX keys with keep below and at n.  Workgroups and
// waves run last to first.  Guard words follow every output array.  The run ends with an `ok` line of coverage counts and fails below
// their floors.
//   g++ -O1 -g -std=c++17 -I bifromq_amd/csrc -I tools/emu tools/emu/order_emu.cpp -o build/order_emu && build/order_emu [rounds] [seed]
#define BMQ_WAVE_EMU 1
#include "wave_emu.h"

#include <random>
#include <set>
#include <string>
#include <vector>

#include "bmq_order_kernels.h"

using namespace bmq;

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

static const uint32_t GUARD = 16, GUARD_WORD = 0xC0DEC0DEu, FILL = 0xABABABABu;
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
// KV order: unsigned bytes, a proper prefix first
static bool key_less(const std::string& a, const std::string& b) {
    const size_t m = std::min(a.size(), b.size());
    const int d = m ? memcmp(a.data(), b.data(), m) : 0;
    return d ? d < 0 : a.size() < b.size();
}

struct Coverage {
    uint64_t cases = 0, flagged = 0, dead = 0, long_cursor = 0, staged_cursor = 0, by_id = 0, exclusive_hit = 0, strided = 0, prefix_pairs = 0, dropped_bins = 0, pivot_bins = 0,
             multi_bin_waves = 0, leaves = 0, partial_leaves = 0, full_leaves = 0;
};

template <class K> static void launch_waves(uint32_t blocks, K&& kernel) { // one-wave workgroups, last to first
    wemu::grid_size() = blocks;
    for (uint32_t b = blocks; b-- > 0;) wemu::run_wave(b, kernel, 0);
}
template <class K> static void launch(uint32_t blocks, K&& kernel) { // workgroups of ORD_BLOCK / 64 independent waves, last to first
    wemu::grid_size() = blocks;
    for (uint32_t b = blocks; b-- > 0;)
        for (uint32_t w = ORD_BLOCK / 64; w-- > 0;) wemu::run_wave(b, kernel, w);
}

static int one_case(std::mt19937_64& rng, uint32_t shape, Coverage& cov) {
    auto rnd = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    // ---- the keys
    const char alphabet[5] = {'\0', '\x7f', (char)0x80, (char)0xff, 'a'};
    auto word = [&](uint32_t n) {
        std::string s(n, 'a');
        for (auto& ch : s) ch = alphabet[rnd(5)];
        return s;
    };
    const uint32_t stem_len[7] = {0, 15, 16, 17, 33, 100, 300};
    std::vector<std::string> stems;
    for (uint32_t l : stem_len) stems.push_back(word(l));
    const uint32_t n_keys = shape == 0 ? 1 + rnd(40) : shape == 1 ? 600 + rnd(900) : 2000 + rnd(1500);
    std::set<std::string> uniq;
    while (uniq.size() < n_keys) {
        std::string k = stems[rnd(7)] + word(rnd(shape == 0 ? 3 : 12));
        if (k.empty()) k = "a";
        uniq.insert(k);
        if (rnd(4) == 0) uniq.insert(k + word(1 + rnd(3))); // a key and a proper prefix of it
    }
    std::vector<std::string> keys(uniq.begin(), uniq.end());
    for (size_t i = keys.size(); i-- > 1;) std::swap(keys[i], keys[rnd(i + 1)]);
    // ---- the pool: ids in a shuffled order, dead ids between them, random gaps
    const uint32_t n_ids = (uint32_t)keys.size() + rnd(keys.size() / 4 + 2), id_cap = n_ids + 8;
    std::vector<uint8_t> kpool(16);
    for (auto& b : kpool) b = (uint8_t)alphabet[rnd(5)];
    std::vector<unsigned long long> kref(id_cap, 0ull);
    std::vector<std::string> key_of(id_cap);
    std::vector<uint32_t> live_ids;
    {
        std::vector<uint32_t> slots(n_ids);
        for (uint32_t i = 0; i < n_ids; i++) slots[i] = i;
        for (size_t i = slots.size(); i-- > 1;) std::swap(slots[i], slots[rnd(i + 1)]);
        slots.resize(keys.size());
        std::sort(slots.begin(), slots.end());
        for (size_t k = 0; k < keys.size(); k++) {
            for (uint32_t g = rnd(4); g > 0; g--) kpool.push_back((uint8_t)alphabet[rnd(5)]);
            const size_t off = kpool.size();
            kpool.insert(kpool.end(), keys[k].begin(), keys[k].end());
            kref[slots[k]] = (unsigned long long)off | ((unsigned long long)keys[k].size() << KREF_LEN_SHIFT);
            key_of[slots[k]] = keys[k];
            live_ids.push_back(slots[k]);
        }
    }
    for (uint32_t g = 0; g < 32; g++) kpool.push_back((uint8_t)alphabet[rnd(5)]); // (readable 32 bytes past the last key)
    cov.dead += n_ids - live_ids.size();
    DistIndexMut ix{};
    ix.kpool = kpool.data();
    ix.kref = kref.data();
    ix.id_cap = id_cap;
    auto by_key = [&](uint32_t a, uint32_t b) { return key_less(key_of[a], key_of[b]); };
    std::vector<uint32_t> sorted_ids = live_ids;
    std::sort(sorted_ids.begin(), sorted_ids.end(), by_key);
    for (size_t i = 1; i < sorted_ids.size(); i++) {
        const std::string &a = key_of[sorted_ids[i - 1]], &b = key_of[sorted_ids[i]];
        cov.prefix_pairs += a.size() < b.size() && b.compare(0, a.size(), a) == 0;
    }
    const std::string where = "shape " + std::to_string(shape) + " keys " + std::to_string(keys.size()) + " ids " + std::to_string(n_ids);
    const char* what = where.c_str();

    // ---- k_o_flag: every kind of cursor
    std::vector<uint32_t> cand_kept;
    for (uint32_t kind = 0; kind < 10; kind++) {
        const std::string& some = key_of[live_ids[rnd(live_ids.size())]];
        std::string lo;
        uint32_t flags = 1u, id = 0;
        switch (kind) {
        case 0: flags = 0; break;
        case 1: lo = some; break;
        case 2: lo = some.substr(0, some.size() - 1); break;
        case 3: lo = some + std::string(1, '\0'); break;
        case 4: lo = ""; break;
        case 5: lo = std::string(2, (char)0xff) + "\xff"; break;
        case 6: { // the longest key: past the LDS staging when the stem of 300 bytes is in use
            lo = key_of[live_ids[0]];
            for (uint32_t i : live_ids)
                if (key_of[i].size() > lo.size()) lo = key_of[i];
            cov.long_cursor += lo.size() > ORD_LDS;
            break;
        }
        case 9: // a key of more than a wave's bytes that still fits the LDS staging, if there is one
            lo = some;
            for (uint32_t i : live_ids)
                if (key_of[i].size() > 64 && key_of[i].size() <= ORD_LDS) lo = key_of[i];
            cov.staged_cursor += lo.size() > 64 && lo.size() <= ORD_LDS;
            break;
        case 7:
        case 8: // by id: the bytes are the pool's
            id = live_ids[rnd(live_ids.size())];
            lo = key_of[id];
            flags |= 4u;
            cov.by_id++;
            break;
        }
        if (flags && (kind == 8 || rnd(2))) flags |= 2u;
        std::vector<uint8_t> lo_buf(lo.begin(), lo.end());
        lo_buf.resize(lo_buf.size() + 8, 0x5A);
        OrderCursor c{};
        c.key = (flags & 4u) ? nullptr : lo_buf.data();
        c.len = (flags & 4u) ? 0u : (uint32_t)lo.size();
        c.flags = flags;
        c.id = id;
        std::vector<uint32_t> cand = guarded(n_ids, FILL), n_cand = guarded(1, 0u);
        const uint32_t blocks = 1 + rnd(3);
        cov.strided += (uint64_t)blocks * ORD_BLOCK < n_ids;
        launch(blocks, [&] { k_o_flag(ix, n_ids, c, cand.data(), n_cand.data()); });
        std::vector<uint32_t> exp;
        for (uint32_t i : live_ids) {
            const bool below = key_less(key_of[i], lo), equal = key_of[i] == lo;
            if (!(flags & 1u) || (!below && !((flags & 2u) && equal))) exp.push_back(i);
            cov.exclusive_hit += (flags & 3u) == 3u && equal;
        }
        if (n_cand[0] != exp.size()) FAIL("flag: a count of %u candidates, expected %zu (cursor kind %u flags %u, %s)\n", n_cand[0], exp.size(), kind, flags, what);
        std::vector<uint32_t> got(cand.begin(), cand.begin() + n_cand[0]);
        std::sort(got.begin(), got.end());
        std::sort(exp.begin(), exp.end());
        if (got != exp) FAIL("flag: the candidate row differs from the brute force (cursor kind %u flags %u, %s)\n", kind, flags, what);
        for (size_t i = n_cand[0]; i < n_ids; i++)
            if (cand[i] != FILL) FAIL("flag: a row behind the count was written (cursor kind %u, %s)\n", kind, what);
        if (!guard_intact(cand) || !guard_intact(n_cand)) FAIL("flag: a guard row is damaged (%s)\n", what);
        cov.flagged += exp.size();
        if (kind == 0) cand_kept = std::vector<uint32_t>(cand.begin(), cand.begin() + n_cand[0]);
    }

    // ---- k_o_pivots / k_o_bucket / k_o_scatter over the candidates of the cursor-less pass
    const uint32_t n = (uint32_t)cand_kept.size();
    const uint32_t P = std::min<uint32_t>(n, shape == 0 ? 1 + rnd(7) : ORDER_PIVOTS), stride = n / P, nb = 2 * P + 1;
    std::vector<uint32_t> list = cand_kept;
    list.resize(n + GUARD, GUARD_WORD);
    std::vector<uint32_t> piv = guarded(P, FILL);
    launch_waves(P, [&] { k_o_pivots(ix, list.data(), stride, P, piv.data()); });
    std::vector<uint32_t> x_piv;
    for (uint32_t j = 0; j < P; j++) x_piv.push_back(list[(size_t)j * stride]);
    std::sort(x_piv.begin(), x_piv.end(), by_key);
    for (uint32_t j = 0; j < P; j++)
        if (piv[j] != x_piv[j]) FAIL("pivots: rank %u holds id %u, expected %u (%s)\n", j, piv[j], x_piv[j], what);
    if (!guard_intact(piv)) FAIL("pivots: a guard row is damaged (%s)\n", what);
    std::vector<uint16_t> bins(n + GUARD, 0xEEEE);
    std::vector<uint32_t> hist = guarded(nb, 0u);
    launch(1 + rnd(3), [&] { k_o_bucket(ix, list.data(), n, piv.data(), P, bins.data(), hist.data()); });
    std::vector<uint32_t> x_hist(nb, 0u);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t below = 0, is_piv = 0;
        for (uint32_t j = 0; j < P; j++) below += key_less(key_of[piv[j]], key_of[list[i]]), is_piv |= piv[j] == list[i];
        const uint32_t x = 2 * below + is_piv;
        if (bins[i] != x) FAIL("bucket: the bin of row %u is %u, expected %u (%s)\n", i, bins[i], x, what);
        x_hist[x]++;
        cov.pivot_bins += is_piv;
    }
    for (uint32_t b = 0; b < nb; b++)
        if (hist[b] != x_hist[b]) FAIL("bucket: the count of bin %u is %u, expected %u (%s)\n", b, hist[b], x_hist[b], what);
    for (uint32_t i = n; i < n + GUARD; i++)
        if (bins[i] != 0xEEEE) FAIL("bucket: a bin row behind the list was written (%s)\n", what);
    if (!guard_intact(hist)) FAIL("bucket: a guard row is damaged (%s)\n", what);
    // the scatter: some bins dropped, the kept ones laid out in bin order from a random offset
    std::vector<uint32_t> base = guarded(nb, ORDER_DROP), cursor = guarded(nb, 0u);
    const uint32_t dst_off = rnd(5);
    uint32_t acc = dst_off;
    const uint32_t cut = rnd(nb + 1);
    for (uint32_t b = 0; b < nb; b++) {
        if (b >= cut && rnd(3)) {
            cov.dropped_bins += x_hist[b] != 0;
            continue;
        }
        base[b] = acc;
        acc += x_hist[b];
    }
    std::vector<uint32_t> dst = guarded(acc, FILL);
    launch(1 + rnd(3), [&] { k_o_scatter(list.data(), bins.data(), n, base.data(), cursor.data(), dst.data()); });
    for (uint32_t b = 0; b < nb; b++) {
        if (base[b] == ORDER_DROP) {
            if (cursor[b] != 0) FAIL("scatter: a count of %u places taken in the dropped bin %u (%s)\n", cursor[b], b, what);
            continue;
        }
        if (cursor[b] != x_hist[b]) FAIL("scatter: a count of %u places taken in bin %u, expected %u (%s)\n", cursor[b], b, x_hist[b], what);
        std::multiset<uint32_t> got(dst.begin() + base[b], dst.begin() + base[b] + x_hist[b]), exp;
        for (uint32_t i = 0; i < n; i++)
            if (bins[i] == b) exp.insert(list[i]);
        if (got != exp) FAIL("scatter: the row of bin %u differs from the brute force (%s)\n", b, what);
    }
    for (uint32_t i = 0; i < dst_off; i++)
        if (dst[i] != FILL) FAIL("scatter: a row in front of the first bin was written (%s)\n", what);
    for (uint32_t t = 0; t + 64 <= n; t += 64) {
        std::set<uint32_t> kept;
        for (uint32_t i = t; i < t + 64; i++)
            if (base[bins[i]] != ORDER_DROP) kept.insert(bins[i]);
        cov.multi_bin_waves += kept.size() > 1;
    }
    if (!guard_intact(dst) || !guard_intact(cursor) || !guard_intact(base) || !guard_intact(list)) FAIL("scatter: a guard row is damaged (%s)\n", what);

    // ---- k_o_leaves: buckets cut from the candidate list (list 0) and from a rotated copy (list 1)
    std::vector<uint32_t> list1(list.begin(), list.begin() + n);
    std::rotate(list1.begin(), list1.begin() + n / 3, list1.end());
    list1.resize(n + GUARD, GUARD_WORD);
    const uint32_t sizes[10] = {1, 2, 63, 64, 65, 255, 256, 257, ORDER_BUCKET_MAX, 7};
    std::vector<OrderLeaf> leaves;
    uint32_t out_n = rnd(3);
    for (uint32_t at = 0; at < n && leaves.size() < 6;) {
        const uint32_t sz = std::min<uint32_t>(shape == 2 && leaves.empty() ? ORDER_BUCKET_MAX : sizes[rnd(10)], n - at), keep = rnd(3) == 0 ? 1 + rnd(sz) : sz;
        leaves.push_back(OrderLeaf{rnd(2), at, sz, keep, out_n});
        out_n += keep;
        at += sz + rnd(3);
    }
    std::vector<uint32_t> out = guarded(out_n, FILL);
    launch_waves((uint32_t)leaves.size() * ORDER_BUCKET_MAX, [&] { k_o_leaves(ix, list.data(), list1.data(), leaves.data(), out.data()); });
    for (const OrderLeaf& lf : leaves) {
        const std::vector<uint32_t>& src = lf.list ? list1 : list;
        std::vector<uint32_t> x(src.begin() + lf.off, src.begin() + lf.off + lf.n);
        std::sort(x.begin(), x.end(), by_key);
        for (uint32_t r = 0; r < lf.keep; r++)
            if (out[lf.out_off + r] != x[r]) FAIL("leaves: output row %u of a bucket of %u (keep %u) holds id %u, expected %u (%s)\n", r, lf.n, lf.keep, out[lf.out_off + r], x[r], what);
        cov.leaves++, cov.partial_leaves += lf.keep < lf.n, cov.full_leaves += lf.n == ORDER_BUCKET_MAX;
    }
    for (uint32_t i = 0; i < leaves[0].out_off; i++)
        if (out[i] != FILL) FAIL("leaves: a row in front of the first bucket was written (%s)\n", what);
    if (!guard_intact(out)) FAIL("leaves: a guard row is damaged (%s)\n", what);
    cov.cases++;
    return 0;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 3;
    const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
    std::mt19937_64 rng(seed);
    Coverage cov;
    int c = 0;
    for (int round = 0; round < rounds; round++)
        for (uint32_t k = 0; k < 8; k++, c++) {
            const uint32_t shape = k < 3 ? 0 : k < 6 ? 1 : 2; // a handful of keys; more than a workgroup round; 255 pivots and full buckets
            if (one_case(rng, shape, cov)) {
                fprintf(stderr, "case %d failed (rounds %d seed %llu)\n", c, rounds, (unsigned long long)seed);
                return 1;
            }
        }
    const uint64_t R = (uint64_t)rounds;
    struct Floor {
        const char* name;
        uint64_t got, want;
    } floors[] = {{"candidates", cov.flagged, 5000 * R}, {"dead ids", cov.dead, 100 * R}, {"cursors past the LDS staging", cov.long_cursor, 2 * R}, {"cursors by id", cov.by_id, 16 * R}, {"staged cursors of more than a wave's bytes", cov.staged_cursor, 4 * R},
                  {"exclusive cursors equal to a key", cov.exclusive_hit, 8 * R}, {"passes that stride", cov.strided, 10 * R}, {"keys that are a prefix of the next", cov.prefix_pairs, 100 * R},
                  {"dropped bins that hold keys", cov.dropped_bins, 20 * R}, {"pivots binned", cov.pivot_bins, 500 * R}, {"waves with several kept bins", cov.multi_bin_waves, 20 * R},
                  {"buckets ranked", cov.leaves, 20 * R}, {"buckets cut at keep", cov.partial_leaves, 3 * R}, {"buckets of ORDER_BUCKET_MAX", cov.full_leaves, 1 * R}};
    for (const Floor& fl : floors)
        if (fl.got < fl.want) {
            fprintf(stderr, "coverage: %s: %llu, the floor is %llu (rounds %d seed %llu)\n", fl.name, (unsigned long long)fl.got, (unsigned long long)fl.want, rounds,
                    (unsigned long long)seed);
            return 1;
        }
    printf("order emu ok: %llu cases; candidates %llu, dead ids %llu, long cursors %llu, cursors by id %llu, exclusive hits %llu, strided passes %llu, prefix pairs %llu, "
           "dropped bins %llu, pivots binned %llu, multi-bin waves %llu, buckets %llu, cut %llu, full %llu\n",
           (unsigned long long)cov.cases, (unsigned long long)cov.flagged, (unsigned long long)cov.dead, (unsigned long long)cov.long_cursor, (unsigned long long)cov.by_id,
           (unsigned long long)cov.exclusive_hit, (unsigned long long)cov.strided, (unsigned long long)cov.prefix_pairs, (unsigned long long)cov.dropped_bins,
           (unsigned long long)cov.pivot_bins, (unsigned long long)cov.multi_bin_waves, (unsigned long long)cov.leaves, (unsigned long long)cov.partial_leaves,
           (unsigned long long)cov.full_leaves);
    return 0;
}
