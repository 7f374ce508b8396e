// bmq_share_kernels.h -- gfx950 kernels of the shared-subscription resolve (bmq_share_core.h).  The passes over pairs / rows are one lane
// per item; k_sh_resolve is the hot one: a row's members are spread over a sub-group of W lanes (lane = member: the pre-mixed words
// of consecutive members are consecutive in HBM), ceil(n / W) rounds of sh_score -- 64-bit integer multiply chains in VGPR pairs --,
// then an arg-max over the sub-group by __shfl_xor on (signed score, lowest index).  W = 8 / 16 packs 8 / 4 rows into a wave64, as
// most groups have a handful of members; 64 serves tables of hundreds (the control picks W from the mean table size).
#pragma once
#include <hip/hip_runtime.h>

#include "bmq_share_core.h"

namespace bmq {

constexpr int SH_BLOCK = 256;

__global__ __launch_bounds__(SH_BLOCK) void k_sh_count(DistIndexMut ix, ShareTables T, ShareBatch b) {
    const uint32_t i = blockIdx.x * SH_BLOCK + threadIdx.x;
    unsigned long long rows = 0, scores = 0; // 64-bit sums: a wave adds up, its first lane adds to the batch's totals
    if (i < b.n_pairs) rows = sh_count_one(ix, T, b, i, scores);
    for (int o = 32; o >= 1; o >>= 1) {
        rows += __shfl_down(rows, o);
        scores += __shfl_down(scores, o);
    }
    if ((threadIdx.x & 63) == 0 && (rows | scores)) {
        atomicAdd(b.totals, rows);
        atomicAdd(b.totals + 1, scores);
    }
}
__global__ __launch_bounds__(SH_BLOCK) void k_sh_rows(ShareTables T, ShareBatch b) {
    const uint32_t r = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (r < b.n_rows) sh_row_one(T, b, r);
}
// rows row0 .. row0 + n (a launch covers at most 2^24 rows: n * W threads stay far below 2^32)
template <int W> __global__ __launch_bounds__(SH_BLOCK) void k_sh_resolve(ShareTables T, ShareBatch b, uint32_t row0, uint32_t n) {
    static_assert(W >= 2 && W <= 64 && (W & (W - 1)) == 0, "sub-group width");
    const uint32_t local = (blockIdx.x * SH_BLOCK + threadIdx.x) / W, lane = threadIdx.x & (W - 1);
    const bool live = local < n; // (no early exit: every lane of a sub-group takes part in the shuffles below)
    const uint32_t r = row0 + local;
    uint32_t slot = SH_NONE, i = 0;
    if (live) {
        i = b.row_pair[r];
        slot = b.slot[i];
    }
    ShareDesc d{};
    if (slot != SH_NONE) d = T.desc[slot];
    long long best_s = 0;
    uint32_t best_m = SH_NONE; // SH_NONE: this lane scored no member (it loses every comparison below)
    if (slot != SH_NONE && d.ordered) {
        const uint32_t sender = b.sender_hash[b.row_sender[r]];
        for (uint32_t m = lane; m < d.n; m += W) {
            const long long s = sh_score(T, d, m, sender);
            if (best_m == SH_NONE || s > best_s) best_s = s, best_m = m; // (a lane's members ascend: strict '>' keeps the first of equals)
        }
    }
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) {
        const long long os = __shfl_xor(best_s, o, W);
        const uint32_t om = __shfl_xor(best_m, o, W);
        if (om != SH_NONE && (best_m == SH_NONE || sh_better(os, om, best_s, best_m))) best_s = os, best_m = om;
    }
    if (!live || lane != 0) return;
    if (slot == SH_NONE) return sh_store_row(T, b, r, nullptr, SH_NONE);
    if (!d.ordered) best_m = sh_pick(b.nonce, b.pair_topic[i], b.pair_route[i], d.n);
    sh_store_row(T, b, r, &d, best_m);
}
__global__ __launch_bounds__(SH_BLOCK) void k_sh_heads(ShareBatch b, int emit) {
    const uint32_t j = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (j >= b.n_rows) return;
    sh_head_one(b, j);
    if (emit) sh_emit_one(b, j);
}
__global__ __launch_bounds__(SH_BLOCK) void k_sh_groups(ShareTables T, ShareBatch b) {
    const uint32_t j = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (j < b.n_rows) sh_group_one(T, b, j);
}
// the directory of a new generation of the route index (Share::carry): table i goes to the id its route key has there.  One lane per
// carried table into a directory filled with SH_NONE before; the ids are distinct (a key has one id), so no two lanes write one word.
__global__ __launch_bounds__(SH_BLOCK) void k_sh_rekey(uint32_t* slot_of, uint32_t id_cap, const uint32_t* new_id, const uint32_t* slot, uint32_t n) {
    const uint32_t i = blockIdx.x * SH_BLOCK + threadIdx.x;
    if (i < n) sh_rekey_one(slot_of, id_cap, new_id, slot, i);
}

} // namespace bmq
