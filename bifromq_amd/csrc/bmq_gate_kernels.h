// bmq_gate_kernels.h -- gfx950 kernels of the submit-time fan-out gate over a match CSR (bmq_gate_core.h; the control is bmq_gate.h):
//   k_gate_classify  one lane per pair, EVERY pair: the class of its route, from the tail of its key (one random line of the key pool per
//                    pair).  The live members of the three classes are counted per wave and row (a ballot per distinct row of the wave's
//                    64 pairs, ONE atomic per row, class and wave, as k_caps_classify counts).
//   k_gate_rows      one lane per row: the row rule (gate_row_rule), kept counts, flags, who ranks it; the rows left to the host are listed.
//                    The meter is summed per wave and distinct table entry (a round per entry among the wave's rows: a butterfly over the
//                    lanes of that entry) in front of ONE 64-bit and one 32-bit atomic add per entry and wave -- a batch has about a
//                    thousand consecutive rows per tenant, so a wave usually holds one entry.
//   k_gate_list      one lane per pair: the pairs that need no rank are settled, the others are compacted into the work list.
//   k_gate_rank      one wave per pair of the work list: caps_rank_wave, the counting rank of the caps, over the gate's classes; lane 0
//                    keeps the pair or not.
//   k_gate_write     one lane per pair / row / table entry: survivors to their place behind the scan of the keep flags, row offsets, flags,
//                    kept counts, meters.
// The waves of a workgroup are independent throughout (no LDS, no workgroup barrier); the per-pair passes stride over a bounded grid; every
// kernel only reads the index; every atomic is a plain vector atomic on global memory.
#pragma once
#include "bmq_caps_kernels.h"
#include "bmq_gate_core.h"

namespace bmq {

__global__ __launch_bounds__(CAPS_BLOCK) void k_gate_classify(DistIndexMut ix, GateBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t total = b.c.total;
    uint32_t err = 0;
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < total; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long i = base + lane;
        const bool in = i < total;
        const uint32_t r = in ? fo_row_of(b.c.row_ptr, b.c.n_rows, (uint32_t)i) : 0u;
        const uint32_t c = in ? gate_classify_one(ix, b, (uint32_t)i, &err) : (uint32_t)CAPS_DEAD;
        if (in) b.c.cls[i] = (uint8_t)c;
        bool pending = c != CAPS_DEAD;
        unsigned long long left = caps_ballot(pending);
        while (left != 0) { // one round per distinct row among the wave's live pairs (the same in every lane)
            const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t lr = __shfl(r, (int)leader);
            const bool mine = pending && r == lr;
            const unsigned long long mp = caps_ballot(mine && c == CAPS_PERSISTENT), mt = caps_ballot(mine && c == CAPS_TRANSIENT), mg = caps_ballot(mine && c == CAPS_GROUP);
            if (lane == leader) {
                if (mp) atomicAdd(b.row_cnt + 3 * (size_t)lr, (uint32_t)__popcll(mp));
                if (mt) atomicAdd(b.row_cnt + 3 * (size_t)lr + 1, (uint32_t)__popcll(mt));
                if (mg) atomicAdd(b.row_cnt + 3 * (size_t)lr + 2, (uint32_t)__popcll(mg));
            }
            if (mine) pending = false;
            left &= ~(mp | mt | mg);
        }
    }
    if (err) atomicOr(b.c.ctr + GATE_C_ERR, err);
}

// the sum of v over the wave, the same in every lane: a butterfly of six exchanges (the lanes that do not belong to the sum pass 0)
__device__ __forceinline__ unsigned long long gate_sum_wave(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_gate_rows(GateBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_rows = b.c.n_rows;
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < n_rows; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long r = base + lane;
        const bool in = r < n_rows;
        uint32_t t = 0, record = 0, n = 0, fl = 0;
        unsigned long long meter = 0;
        const uint32_t full = in ? gate_row_one(b, (uint32_t)r, t, meter, record) : (uint32_t)CAPS_ROW_CLASSIFIED, m = full & 3u;
        if (full & CAPS_BAD_INDEX) atomicOr(b.c.ctr + GATE_C_ERR, (uint32_t)CAPS_ERR_INDEX);
        else if (in) {
            n = b.row_cnt[3 * r] + b.row_cnt[3 * r + 1] + b.row_cnt[3 * r + 2];
            fl = b.flags[r];
        }
        const unsigned long long m1 = caps_ballot(n == 1), mn = caps_ballot(n > 1), mx = caps_ballot((fl & ~(uint32_t)GATE_INLINE) != 0), mr = caps_ballot(m == CAPS_ROW_RANKED),
                                 mf = caps_ballot(m == CAPS_ROW_FALLBACK);
        uint32_t at = 0;
        if (lane == 0) {
            if (m1) atomicAdd(b.c.ctr + GATE_C_SINGLE, (uint32_t)__popcll(m1));
            if (mn) atomicAdd(b.c.ctr + GATE_C_GATED, (uint32_t)__popcll(mn));
            if (mx) atomicAdd(b.c.ctr + GATE_C_FLAGGED, (uint32_t)__popcll(mx));
            if (mr) atomicAdd(b.c.ctr + GATE_C_RANKED, (uint32_t)__popcll(mr));
            if (mf) at = atomicAdd(b.c.ctr + GATE_C_FALLBACK, (uint32_t)__popcll(mf));
        }
        at = __shfl(at, 0);
        if (m == CAPS_ROW_FALLBACK) b.c.fb_rows[at + caps_lanes_below(mf)] = (uint32_t)r;
        // the meter: one round per distinct table entry among the wave's rows with a record
        bool pending = record != 0;
        unsigned long long left = caps_ballot(pending);
        while (left != 0) {
            const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t lt = __shfl(t, (int)leader);
            const bool mine = pending && t == lt;
            const unsigned long long mm = caps_ballot(mine);
            const unsigned long long sum = gate_sum_wave(mine ? meter : 0ull);
            if (lane == leader) {
                if (sum) atomicAdd(b.meter_bytes + lt, sum);
                atomicAdd(b.meter_records + lt, (uint32_t)__popcll(mm));
            }
            if (mine) pending = false;
            left &= ~mm;
        }
    }
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_gate_list(GateBatch b) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t total = b.c.total;
    for (unsigned long long base = (unsigned long long)blockIdx.x * CAPS_BLOCK + wave * 64u; base < total; base += (unsigned long long)gridDim.x * CAPS_BLOCK) {
        const unsigned long long i = base + lane;
        const bool rank = i < total && gate_list_one(b, (uint32_t)i, fo_row_of(b.c.row_ptr, b.c.n_rows, (uint32_t)i));
        const unsigned long long m = caps_ballot(rank);
        if (m == 0) continue; // (the same in every lane)
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(b.c.ctr + GATE_C_WORK, (uint32_t)__popcll(m));
        at = __shfl(at, 0);
        if (rank) b.c.work[at + caps_lanes_below(m)] = (uint32_t)i;
    }
}

// one wave per pair of the work list (a grid of ceil(n_work / 4) workgroups of four waves)
__global__ __launch_bounds__(CAPS_BLOCK) void k_gate_rank(DistIndexMut ix, GateBatch b, uint32_t n_work) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long item = (unsigned long long)blockIdx.x * (CAPS_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= n_work) return; // (the whole wave)
    const uint32_t p = b.c.work[item];
    const uint32_t r = fo_row_of(b.c.row_ptr, b.c.n_rows, p);
    const uint32_t rank = caps_rank_wave(ix, b.c, b.c.row_ptr[r], b.c.row_ptr[r + 1], p, lane);
    if (lane == 0) gate_settle_one(b, p, r, rank);
}

__global__ __launch_bounds__(CAPS_BLOCK) void k_gate_write(GateBatch b, uint32_t n, uint32_t rows) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * CAPS_BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CAPS_BLOCK) gate_write_one(b, (uint32_t)i, rows != 0);
}

} // namespace bmq
