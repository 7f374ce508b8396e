// bmq_prefix_core.h -- the per-key function of the per-prefix census (DistIndex::prefix_census, bmq_routes_prefix_census): under which of
// a batch of byte prefixes does a live route key lie?  The dist worker's split hinter asks a KV range, for every key prefix a mutation batch
// touched, how many records lie under the prefix (reader.size([prefix, upperBound(prefix))), DW/hinter/FanoutSplitHinter.java:175-178); here
// ONE pass over the key store answers for all prefixes of the batch.
//
// The table: the DISTINCT prefixes of a call, sorted in key_compare order (unsigned bytes, a proper prefix first), each with the index of
// its PARENT -- the longest other prefix of the table that is a proper prefix of it, NONE without one.  A key is counted under the DEEPEST
// prefix of the table that is a prefix of it, and the control carries every slot's sums to its parent afterwards (a child sorts behind
// its parent, so one pass in reverse table order does it): a key then counts for every prefix that is a prefix of it, at one add per key.
//
// The deepest prefix: let F be the FLOOR of the key, the last entry <= key.  Every entry P that is a prefix of the key is F or an ancestor
// of F: P <= key gives P <= F, and P <= F <= key with P a prefix of key makes P a prefix of F (every string between P and an extension of
// P starts with P).  F itself is often NOT a prefix of the key while an ancestor is: table {a, ab} and key ac -- the floor is the sibling
// ab, the answer a.  So the walk goes from the floor up the parent links to the first entry that is a prefix of the key; the ancestors of
// F are ordered by length, so the first hit is the deepest.
// The gfx950 kernel over it is bmq_prefix_kernels.h (k_b_prefix_census); HostExec loops over the same function.  Nothing here writes.
#pragma once
#include "bmq_build_core.h"

namespace bmq {

constexpr uint32_t PREFIX_MAX = 65536; // BMQ_PREFIX_MAX

// the table of a call in exec memory: prefix i is bytes[off[i], off[i + 1])
struct PrefixTable {
    const uint8_t* bytes;
    const uint32_t* off;    // [n + 1]
    const uint32_t* parent; // [n]
    uint32_t n;
    uint32_t pad0;
};
// is p[0, pl) a prefix of k[0, kl)?  (a key equal to the prefix: yes)
BMQ_HD bool prefix_is_of(const uint8_t* p, unsigned long long pl, const uint8_t* k, unsigned long long kl) {
    if (pl > kl) return false;
    const unsigned long long m = pl < kl ? pl : kl;
    return key_compare(p, m, k, m) == 0;
}
// the floor of key k in the table: the last prefix <= k, NONE if every prefix is above it
BMQ_HD uint32_t prefix_floor(const PrefixTable& T, const uint8_t* k, unsigned long long kl) {
    uint32_t lo = 0, hi = T.n; // -> the number of prefixes <= k
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key_compare(T.bytes + T.off[mid], T.off[mid + 1] - T.off[mid], k, kl) <= 0) lo = mid + 1;
        else hi = mid;
    }
    return lo == 0 ? NONE : lo - 1;
}
// one key reference: the table slot of the deepest prefix of the key if the key is live and has one, NONE otherwise; flag = 1 normal,
// 2 unordered share, 3 ordered share; len = the key's length.  Reads only.
BMQ_HD uint32_t prefix_key_one(const DistIndexMut& ix, uint32_t id, const PrefixTable& T, uint32_t& flag, uint32_t& len) {
    const unsigned long long r = ix.kref[id];
    len = (uint32_t)(r >> KREF_LEN_SHIFT);
    if (len == 0) return NONE; // a dead reference
    const unsigned long long off = r & KREF_OFF_MASK;
    const uint8_t* k = ix.kpool + off;
    uint32_t s = prefix_floor(T, k, len);
    while (s != NONE) {
        if (prefix_is_of(T.bytes + T.off[s], T.off[s + 1] - T.off[s], k, len)) break;
        s = T.parent[s];
    }
    if (s == NONE) return NONE;
    KeyView v;
    if (!key_parse(ix.kpool, off, off + len, v)) return NONE; // (the index holds well-formed keys only)
    flag = v.flag;
    return s;
}

// what the prefix censuses of an engine did so far (bmq_prefix_census_info): calls, prefixes passed, distinct ones, distinct ones with a
// parent, key references scanned, the longest chain of parent links
struct PrefixStats {
    uint64_t n_calls = 0, n_prefixes = 0, n_distinct = 0, n_nested = 0, n_keys_scanned = 0, max_chain = 0;
};

} // namespace bmq
