// bmq_caps_kernels.h -- gfx950 kernels of the fan-out caps over a match CSR (bmq_caps_core.h; the control is bmq_caps.h):
//   k_caps_classify  one lane per pair: the class of its route, from the tail of its key.  The members of the two capped classes are
//                    counted per wave and row (a ballot per distinct row of the wave's 64 pairs, ONE atomic per row, class and wave), so a
//                    row of a million pairs costs its counters sixteen thousand adds, not a million.
//   k_caps_rows      one lane per row: over its caps or not, its events per class, who ranks it; the rows left to the host are listed.
//   k_caps_list      one lane per pair: the pairs that need no rank are settled, the others are compacted into the work list (ballot,
//                    popcount, one atomic per wave).
//   k_caps_rank      one wave per pair of the work list: the members of its class in its row with a smaller key are counted 64 at a time
//                    (as k_o_leaves ranks a bucket); lane 0 keeps the pair or writes its event.
//   k_caps_write     one lane per pair / row: survivors to their place behind the scan of the keep flags, row offsets, class counts.
// The waves of a workgroup are independent throughout (no LDS, no workgroup barrier); the per-pair passes stride over a bounded grid; every
// kernel only reads the index.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/caps_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>
#endif

#include "bmq_caps_core.h"

namespace bmq {

constexpr uint32_t CAPS_BLOCK = 256;   // lanes per workgroup: four independent waves
constexpr uint32_t CAPS_BLOCKS = 2048; // workgroups of a per-pair pass at most: 256 CUs x 8

#ifdef BMQ_WAVE_EMU
inline unsigned long long caps_ballot(bool p) { return ballot64(p); }
inline uint32_t caps_lanes_below(unsigned long long m) { return rank_below(m); }
#else
__device__ __forceinline__ unsigned long long caps_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t caps_lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
#endif

__global__ __launch_bounds__(CAPS_BLOCK) void k_caps_classify(DistIndexMut ix, CapsBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t err = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < b.total; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long i = base + lane;
        const bool in = i < b.total;
        const uint32_t r = in ? fo_row_of(b.row_ptr, b.n_rows, (uint32_t)i) : 0u;
        const uint32_t c = in ? caps_classify_one(ix, b, (uint32_t)i, r, &err) : (uint32_t)CAPS_FREE;
        if (in) b.cls[i] = (uint8_t)c;
        bool pending = c == CAPS_PERSISTENT || c == CAPS_GROUP;
        unsigned long long left = caps_ballot(pending);
        while (left != 0) { // one round per distinct row among the wave's capped pairs (the same in every lane)
            const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t lr = __shfl(r, (int)leader);
            const bool mine = pending && r == lr;
            const unsigned long long mp = caps_ballot(mine && c == CAPS_PERSISTENT), mg = caps_ballot(mine && c == CAPS_GROUP);
            if (lane == leader) {
                if (mp) atomicAdd(b.row_cnt + 2 * (size_t)lr, (uint32_t)__popcll(mp));
                if (mg) atomicAdd(b.row_cnt + 2 * (size_t)lr + 1, (uint32_t)__popcll(mg));
            }
            if (mine) pending = false;
            left &= ~(mp | mg);
        }
    }
    if (err) atomicOr(b.ctr + CAPS_C_ERR, err);
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_caps_rows(CapsBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < b.n_rows; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long r = base + lane;
        const uint32_t full = r < b.n_rows ? caps_row_one(b, (uint32_t)r) : (uint32_t)CAPS_ROW_THROUGH, m = full & 3u;
        if (full & CAPS_BAD_INDEX) atomicOr(b.ctr + CAPS_C_ERR, (uint32_t)CAPS_ERR_INDEX);
        const unsigned long long mc = caps_ballot(m != CAPS_ROW_THROUGH), mr = caps_ballot(m == CAPS_ROW_RANKED), mf = caps_ballot(m == CAPS_ROW_FALLBACK);
        uint32_t at = 0;
        if (lane == 0) {
            if (mc) atomicAdd(b.ctr + CAPS_C_CLASSIFIED, (uint32_t)__popcll(mc));
            if (mr) atomicAdd(b.ctr + CAPS_C_RANKED, (uint32_t)__popcll(mr));
            if (mf) at = atomicAdd(b.ctr + CAPS_C_FALLBACK, (uint32_t)__popcll(mf));
        }
        at = __shfl(at, 0);
        if (m == CAPS_ROW_FALLBACK) b.fb_rows[at + caps_lanes_below(mf)] = (uint32_t)r;
    }
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_caps_list(CapsBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) b.ctr[CAPS_C_EVENTS] = b.ev_scan[2 * (size_t)b.n_rows - 1]; // (total > 0: there is a row)
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < b.total; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long i = base + lane;
        const bool rank = i < b.total && caps_list_one(b, (uint32_t)i, fo_row_of(b.row_ptr, b.n_rows, (uint32_t)i));
        const unsigned long long m = caps_ballot(rank);
        if (m == 0) continue; // (the same in every lane)
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(b.ctr + CAPS_C_WORK, (uint32_t)__popcll(m));
        at = __shfl(at, 0);
        if (rank) b.work[at + caps_lanes_below(m)] = (uint32_t)i;
    }
}

// the members of p's class in row [lo, hi) below p's key, counted by ONE wave: 64 compares a step, a ballot and a popcount (the same in every lane)
__device__ __forceinline__ uint32_t caps_rank_wave(const DistIndexMut& ix, const CapsBatch& b, uint32_t lo, uint32_t hi, uint32_t p, uint32_t lane) {
    uint32_t rank = 0;
    for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
        const uint32_t k = k0 + lane;
        rank += (uint32_t)__popcll(caps_ballot(k < hi && caps_below_one(ix, b, k, p)));
    }
    return rank;
}
// one wave per pair of the work list (a grid of ceil(n_work / 4) workgroups of four waves)
__global__ __launch_bounds__(CAPS_BLOCK) void k_caps_rank(DistIndexMut ix, CapsBatch b, uint32_t n_work) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long item = (unsigned long long)blockIdx.x * (CAPS_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= n_work) return; // (the whole wave)
    const uint32_t p = b.work[item];
    const uint32_t r = fo_row_of(b.row_ptr, b.n_rows, p);
    const uint32_t rank = caps_rank_wave(ix, b, b.row_ptr[r], b.row_ptr[r + 1], p, lane);
    if (lane == 0) caps_settle_one(b, p, r, rank);
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_caps_write(CapsBatch b, uint32_t n) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * CAPS_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CAPS_BLOCK) caps_write_one(b, (uint32_t)i);
}

} // namespace bmq
