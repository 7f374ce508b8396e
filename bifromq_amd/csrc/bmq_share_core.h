// bmq_share_core.h -- receivers of shared subscriptions: the step behind the fan-out grouping (bmq_fanout_core.h) for the routes it leaves in
// its 0xFFFFFFFE group.  Per-item functions, BMQ_HD like the fan-out grouping: gfx950 kernels in bmq_share_kernels.h (wired through
// bmq_exec_dev.h), host threads in bmq_exec_host.h, control in bmq_share.h.
//
// What it replaces.  DeliverExecutorGroup.send(GroupMatching, ...) (DW/DeliverExecutorGroup.java:242-278): an unordered share ($share,
// route-key flag 2) sends the topic's whole message pack to ONE member of GroupMatching.receiverList (SCHEMA/cache/GroupMatching.java:41-50),
// picked at random; an ordered share ($oshare, flag 3) sends every publisher's messages to the member RendezvousHash.get picks for
// (publisher, group) (base-util/.../RendezvousHash.java:45-61): the highest murmur3_128(seed 0) over [int32 LE ClientInfo.hashCode()]
// [UTF-8 receiverUrl], asLong() = h1 of MurmurHash3_x64_128 compared as a SIGNED long, strict '>' in list order (first of equals wins).
// The chosen member is a NormalMatching: it lands in the delivery group of ITS DelivererKey(subBrokerId, delivererKey).
//
// Member tables.  MurmurHash3_x64_128 eats 16-byte blocks [k1 | k2]; each word is mixed (k1: *c1, rotl 31, *c2; k2: *c2, rotl 33, *c1) before
// it enters the h1 / h2 chain, and the tail's words are mixed the same way.  The mix does not depend on the chain, and the 4 sender bytes
// come first, so only k1 of entry 0 depends on the sender: everything else is mixed when the table is loaded.  A member whose message
// (4 + url bytes) is `len` long has ceil(len / 16) ENTRIES: len / 16 full blocks, then the tail (zero padded: mix(0) = 0, so absent words
// drop out by themselves).  A table of n members and E = the longest member's entries is
//   pool64[off64 + row * n + m]   row 0: mixed k2 of entry 0; row 2j - 1 / 2j: mixed k1 / k2 of entry j >= 1
//   pool32[off32 + m]             len;  [off32 + n + m]: url bytes 0..3 (LE, zero padded);  [off32 + 2n + m]: share-deliverer number
// so that lanes = consecutive members read consecutive words.  A score is one k1 mix plus the dependent chain of its entries.
#pragma once
#include "bmq_build_core.h"

namespace bmq {

constexpr uint32_t SH_NONE = 0xFFFFFFFFu;
constexpr uint32_t SH_MAX_MEMBERS = 65535;
constexpr unsigned long long SH_C1 = 0x87c37b91114253d5ull, SH_C2 = 0x4cf5ad432745937full;

BMQ_HD unsigned long long sh_rotl(unsigned long long x, int r) { return (x << r) | (x >> (64 - r)); }
BMQ_HD unsigned long long sh_mix_k1(unsigned long long k) { return sh_rotl(k * SH_C1, 31) * SH_C2; }
BMQ_HD unsigned long long sh_mix_k2(unsigned long long k) { return sh_rotl(k * SH_C2, 33) * SH_C1; }
BMQ_HD unsigned long long sh_fmix(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

struct ShareDesc { // one member table (32 bytes)
    unsigned long long off64, off32;
    uint32_t n;       // members (1 .. SH_MAX_MEMBERS)
    uint32_t entries; // E: the longest member's 16-byte entries (>= 1)
    uint32_t ordered; // 1: $oshare (route-key flag 3), 0: $share (flag 2)
    uint32_t pad;
};
struct ShareTables { // exec memory
    const uint32_t* slot_of; // [id_cap] route id -> index into desc, or SH_NONE
    uint32_t id_cap;
    const ShareDesc* desc;
    const unsigned long long* pool64;
    const uint32_t* pool32;
    uint32_t n_sd; // share-deliverer numbers handed out so far: the sort key of the unresolved rows
};

struct ShareBatch {
    const uint32_t *pair_topic, *pair_route; // [n_pairs]
    const uint32_t* sender_off;              // [n_topics + 1]
    const uint32_t* sender_hash;             // [n_senders] ClientInfo.hashCode() as its 32 bits
    uint32_t n_pairs, n_topics, n_senders, n_rows;
    uint32_t id_end; // route ids handed out so far
    unsigned long long nonce;
    uint32_t *slot, *cnt, *cnt_scan;                              // [n_pairs] table of the pair's route (pass 1), rows of the pair, their inclusive scan
    unsigned long long* totals;                                   // [2] 64-bit sums of pass 1: rows, scores (members x senders of the ordered pairs)
    uint32_t *row_pair, *row_sender, *row_member;                 // [n_rows] in (pair, sender) order
    uint32_t *key, *key_sorted, *pos, *pos_sorted;                // [n_rows] sort key = share-deliverer number, value = row
    uint32_t *head, *head_scan;                                   // [n_rows] (alias key / pos: dead after the sort)
    uint32_t *out_pair, *out_sender, *out_member, *group_off;     // the caller's
    uint32_t row_cap, group_cap;
    uint32_t* flags; // [4]: groups, 1 = the unresolved group is present
};

// h1 of MurmurHash3_x64_128(seed 0) over [sender LE][url of member m], from the member's pre-mixed words
BMQ_HD long long sh_score(const ShareTables& T, const ShareDesc& d, uint32_t m, uint32_t sender) {
    const uint32_t* p32 = T.pool32 + d.off32;
    const uint32_t len = p32[m];
    const unsigned long long* row = T.pool64 + d.off64 + m;
    const uint32_t n_full = len >> 4, n_entries = (len + 15u) >> 4;
    unsigned long long h1 = 0, h2 = 0;
    unsigned long long k1 = sh_mix_k1((unsigned long long)sender | ((unsigned long long)p32[d.n + m] << 32)), k2 = row[0];
    for (uint32_t j = 0;;) {
        if (j < n_full) {
            h1 ^= k1;
            h1 = sh_rotl(h1, 27) + h2;
            h1 = h1 * 5 + 0x52dce729ull;
            h2 ^= k2;
            h2 = sh_rotl(h2, 31) + h1;
            h2 = h2 * 5 + 0x38495ab5ull;
        } else { // the tail
            h1 ^= k1;
            h2 ^= k2;
        }
        if (++j >= n_entries) break;
        row += (size_t)d.n;
        k1 = row[0];
        row += (size_t)d.n;
        k2 = row[0];
    }
    h1 ^= len;
    h2 ^= len;
    h1 += h2;
    h2 += h1;
    return (long long)(sh_fmix(h1) + sh_fmix(h2));
}
// rendezvous order: the higher signed score, among equals the lower index
BMQ_HD bool sh_better(long long s, uint32_t m, long long best_s, uint32_t best_m) { return s > best_s || (s == best_s && m < best_m); }

// the member an unordered share sends a topic's message pack to (include/bmq.h states this formula: tests restate it)
BMQ_HD uint32_t sh_pick(unsigned long long nonce, uint32_t topic, uint32_t route_id, uint32_t n) {
    const unsigned long long x = sh_fmix((nonce ^ (((unsigned long long)route_id << 32) | topic)) + 0x9E3779B97F4A7C15ull);
    return (uint32_t)(((x >> 32) * n) >> 32);
}

// table of pair i's route, SH_NONE: no table, a dead or unknown id, a topic index out of range
BMQ_HD uint32_t sh_slot_of(const DistIndexMut& ix, const ShareTables& T, const ShareBatch& b, uint32_t i) {
    const uint32_t id = b.pair_route[i];
    if (id >= b.id_end || id >= T.id_cap || b.pair_topic[i] >= b.n_topics) return SH_NONE;
    if (ix.kref[id] == 0) return SH_NONE; // deleted since
    return T.slot_of[id];
}
// a carried table's entry in the directory of the new generation (Share::carry): new_id[i] = the id its route key has there, SH_NONE = not found
BMQ_HD void sh_rekey_one(uint32_t* slot_of, uint32_t id_cap, const uint32_t* new_id, const uint32_t* slot, uint32_t i) {
    const uint32_t id = new_id[i];
    if (id < id_cap) slot_of[id] = slot[i];
}
BMQ_HD uint32_t sh_senders_of(const ShareBatch& b, uint32_t t, uint32_t& first) {
    const uint32_t lo = b.sender_off[t], hi = b.sender_off[t + 1];
    first = lo;
    return hi >= lo && hi <= b.n_senders ? hi - lo : 0u;
}
// pass 1, one lane per pair: its table (looked up once: the later passes read slot[]) and its delivery rows -> rows; scores = the hashes they cost
BMQ_HD uint32_t sh_count_one(const DistIndexMut& ix, const ShareTables& T, const ShareBatch& b, uint32_t i, unsigned long long& scores) {
    const uint32_t slot = sh_slot_of(ix, T, b, i);
    uint32_t c = 1, first;
    scores = 0;
    if (slot != SH_NONE && T.desc[slot].ordered) {
        c = sh_senders_of(b, b.pair_topic[i], first);
        scores = (unsigned long long)c * T.desc[slot].n;
    }
    b.slot[i] = slot;
    b.cnt[i] = c;
    return c;
}
// pass 2 (after the inclusive scan), one lane per row: its pair and sender
BMQ_HD void sh_row_one(const ShareTables& T, const ShareBatch& b, uint32_t r) {
    uint32_t lo = 0, hi = b.n_pairs; // the first pair whose scan exceeds r
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (b.cnt_scan[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t i = lo;
    b.row_pair[r] = i;
    const uint32_t slot = b.slot[i];
    uint32_t s = SH_NONE;
    if (slot != SH_NONE && T.desc[slot].ordered) {
        uint32_t first;
        (void)sh_senders_of(b, b.pair_topic[i], first);
        s = first + (r - (b.cnt_scan[i] - b.cnt[i]));
    }
    b.row_sender[r] = s;
}
// pass 3, one item per row (the gfx950 kernel spreads a row's members over lanes: k_sh_resolve): the member and the sort key
BMQ_HD void sh_store_row(const ShareTables& T, const ShareBatch& b, uint32_t r, const ShareDesc* d, uint32_t member) {
    b.row_member[r] = member;
    b.key[r] = d ? T.pool32[d->off32 + 2ull * d->n + member] : T.n_sd;
    b.pos[r] = r;
}
BMQ_HD void sh_resolve_one(const ShareTables& T, const ShareBatch& b, uint32_t r) {
    const uint32_t i = b.row_pair[r];
    const uint32_t slot = b.slot[i];
    if (slot == SH_NONE) return sh_store_row(T, b, r, nullptr, SH_NONE);
    const ShareDesc d = T.desc[slot];
    if (!d.ordered) return sh_store_row(T, b, r, &d, sh_pick(b.nonce, b.pair_topic[i], b.pair_route[i], d.n));
    const uint32_t sender = b.sender_hash[b.row_sender[r]];
    uint32_t best_m = 0;
    long long best_s = sh_score(T, d, 0, sender);
    for (uint32_t m = 1; m < d.n; m++) {
        const long long s = sh_score(T, d, m, sender);
        if (s > best_s) best_s = s, best_m = m;
    }
    sh_store_row(T, b, r, &d, best_m);
}
// pass 4, one lane per SORTED position j: whether it starts a group (head aliases key: written a kernel after key_sorted was)
BMQ_HD void sh_head_one(const ShareBatch& b, uint32_t j) { b.head[j] = (j == 0 || b.key_sorted[j] != b.key_sorted[j - 1]) ? 1u : 0u; }
// ... and the row itself, when the caller's buffers hold all rows
BMQ_HD void sh_emit_one(const ShareBatch& b, uint32_t j) {
    const uint32_t p = b.pos_sorted[j];
    b.out_pair[j] = b.row_pair[p];
    b.out_sender[j] = b.row_sender[p];
    b.out_member[j] = b.row_member[p];
}
// pass 5 (after the inclusive scan of head[]): group heads fill the offsets
BMQ_HD void sh_group_one(const ShareTables& T, const ShareBatch& b, uint32_t j) {
    if (j + 1 == b.n_rows) {
        const uint32_t n = b.head_scan[j];
        b.flags[0] = n;
        b.flags[1] = b.key_sorted[j] == T.n_sd ? 1u : 0u;
        if (n <= b.group_cap) b.group_off[n] = b.n_rows;
    }
    if (!b.head[j]) return;
    const uint32_t g = b.head_scan[j] - 1;
    if (g < b.group_cap) b.group_off[g] = j;
}

} // namespace bmq
