// bmq_order_kernels.h -- gfx950 kernels of the key-ordered window (bmq_order_core.h; the control is DistIndex::window):
//   k_o_flag     one lane per route id: live and at / behind the cursor?  The candidates are compacted per wave (ballot, popcount, ONE
//                atomic per wave and round) into a list of ids.  The cursor key is staged in LDS as k_b_boundary stages its keys.
//   k_o_pivots   <= 255 pivot keys, taken at a fixed stride of a list, are ranked by counting: one wave per pivot, 64 compares a step.
//   k_o_bucket   one lane per id of a list: a binary search over the sorted pivots gives its bin; a histogram in LDS, then one atomic
//                per bin that is not empty.
//   k_o_scatter  one lane per id: the ids of the bins that are kept move to their bin's place in the other list; lanes of a wave that
//                share a bin take their places with ONE atomic (a ballot per distinct bin of the wave).
//   k_o_leaves   a bucket of <= ORDER_BUCKET_MAX keys is ranked by counting, one wave per key; the ranks below `keep` are written out.
// The waves of a workgroup are independent throughout (each owns its slice of LDS, no workgroup barrier), the grids of the per-id passes
// are bounded and stride (ORD_BLOCKS workgroups at most), and every kernel only reads the index.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/order_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>
#endif

#include "bmq_order_core.h"

namespace bmq {

constexpr uint32_t ORD_BLOCK = 256;   // lanes per workgroup: four independent waves
constexpr uint32_t ORD_BLOCKS = 2048; // workgroups of a per-id pass at most: 256 CUs x 8
constexpr uint32_t ORD_LDS = 256;     // cursor bytes staged per wave; a longer cursor is read where it lies

#ifdef BMQ_WAVE_EMU
inline void o_sync() { wave_sync(); }
inline unsigned long long o_ballot(bool p) { return ballot64(p); }
inline uint32_t o_below(unsigned long long m) { return rank_below(m); }
#else
__device__ __forceinline__ void o_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ unsigned long long o_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t o_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
#endif

__global__ __launch_bounds__(ORD_BLOCK) void k_o_flag(DistIndexMut ix, uint32_t n_ids, OrderCursor c, uint32_t* cand, uint32_t* n_cand) {
    __shared__ uint8_t s_key[ORD_BLOCK / 64][ORD_LDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    order_cursor_resolve(ix, c);
    if ((c.flags & 1u) && c.len <= ORD_LDS) {
        for (uint32_t p = lane; p < c.len; p += 64) s_key[wave][p] = c.key[p];
        o_sync();
        c.key = s_key[wave];
    }
    for (unsigned long long base = (unsigned long long)blockIdx.x * ORD_BLOCK + wave * 64u; base < n_ids; base += (unsigned long long)gridDim.x * ORD_BLOCK) {
        const unsigned long long i = base + lane;
        const bool in = i < n_ids && order_flag_one(ix, (uint32_t)i, c);
        const unsigned long long m = o_ballot(in);
        if (m == 0) continue; // (the same in every lane)
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(n_cand, (uint32_t)__popcll(m));
        at = __shfl(at, 0);
        if (in) cand[at + o_below(m)] = (uint32_t)i;
    }
}

// the keys of a strided list below its key j, counted by ONE wave: 64 compares a step, a ballot and a popcount (the same in every lane)
__device__ __forceinline__ uint32_t o_rank_wave(const DistIndexMut& ix, const uint32_t* ids, uint32_t n, uint32_t stride, uint32_t j, uint32_t lane) {
    uint32_t rank = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64) {
        const uint32_t k = k0 + lane;
        rank += (uint32_t)__popcll(o_ballot(k < n && order_below_one(ix, ids, stride, k, j)));
    }
    return rank;
}
// one wave per pivot (a grid of P one-wave workgroups)
__global__ __launch_bounds__(64) void k_o_pivots(DistIndexMut ix, const uint32_t* list, uint32_t stride, uint32_t P, uint32_t* piv) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const uint32_t rank = o_rank_wave(ix, list, P, stride, j, lane);
    if (lane == 0) piv[rank] = list[(size_t)j * stride];
}

__global__ __launch_bounds__(ORD_BLOCK) void k_o_bucket(DistIndexMut ix, const uint32_t* list, uint32_t n, const uint32_t* piv, uint32_t P, uint16_t* bins, uint32_t* hist) {
    __shared__ uint32_t s_hist[ORD_BLOCK / 64][ORDER_BINS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nb = 2 * P + 1;
    for (uint32_t b = lane; b < nb; b += 64) s_hist[wave][b] = 0;
    o_sync();
    for (unsigned long long base = (unsigned long long)blockIdx.x * ORD_BLOCK + wave * 64u; base < n; base += (unsigned long long)gridDim.x * ORD_BLOCK) {
        const unsigned long long i = base + lane;
        if (i < n) {
            const uint32_t bin = order_bin_one(ix, list[i], piv, P);
            bins[i] = (uint16_t)bin;
            atomicAdd(&s_hist[wave][bin], 1u);
        }
    }
    o_sync();
    for (uint32_t b = lane; b < nb; b += 64) {
        const uint32_t v = s_hist[wave][b];
        if (v) atomicAdd(hist + b, v);
    }
}

// base[bin]: where the bin's ids begin in dst, ORDER_DROP for a bin that is dropped; cursor[bin]: ids of the bin placed so far (zeroed)
__global__ __launch_bounds__(ORD_BLOCK) void k_o_scatter(const uint32_t* list, const uint16_t* bins, uint32_t n, const uint32_t* base, uint32_t* cursor, uint32_t* dst) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long tile = (unsigned long long)blockIdx.x * ORD_BLOCK + wave * 64u; tile < n; tile += (unsigned long long)gridDim.x * ORD_BLOCK) {
        const unsigned long long i = tile + lane;
        const uint32_t bin = i < n ? bins[i] : 0u;
        const uint32_t to = i < n ? base[bin] : ORDER_DROP;
        const uint32_t id = i < n ? list[i] : 0u;
        bool pending = to != ORDER_DROP;
        unsigned long long left = o_ballot(pending);
        while (left != 0) { // one round per distinct bin among the wave's kept ids (the same in every lane)
            const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t lb = __shfl(bin, (int)leader);
            const bool mine = pending && bin == lb;
            const unsigned long long m = o_ballot(mine);
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(cursor + lb, (uint32_t)__popcll(m));
            at = __shfl(at, (int)leader);
            if (mine) {
                dst[to + at + o_below(m)] = id;
                pending = false;
            }
            left &= ~m;
        }
    }
}

// one wave per key slot of a bucket (a grid of n_leaves * ORDER_BUCKET_MAX one-wave workgroups; the slots behind a bucket's keys leave at once)
__global__ __launch_bounds__(64) void k_o_leaves(DistIndexMut ix, const uint32_t* list0, const uint32_t* list1, const OrderLeaf* leaves, uint32_t* out) {
    const OrderLeaf lf = leaves[blockIdx.x / ORDER_BUCKET_MAX];
    const uint32_t j = blockIdx.x % ORDER_BUCKET_MAX, lane = threadIdx.x;
    if (j >= lf.n) return;
    const uint32_t* src = (lf.list ? list1 : list0) + lf.off;
    const uint32_t rank = o_rank_wave(ix, src, lf.n, 1u, j, lane);
    if (lane == 0 && rank < lf.keep) out[lf.out_off + rank] = src[j];
}

} // namespace bmq
