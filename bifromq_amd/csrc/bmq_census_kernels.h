// bmq_census_kernels.h -- gfx950 kernels of the per-tenant census calls: bmq_routes_tenant_stats (k_b_census: live route keys per tenant
// and flag inside a KV boundary, TenantsStats.doReset, DW/TenantsStats.java:229-246) and bmq_retain_tenant_counts (k_r_census: retained
// topics per tenant among the ids handed out since the bulk load, RS/RetainStoreCoProc.java:279-296).  Both only read the index.
//
// One lane per key reference / topic id; the per-lane work is census_key_one / census_topic_one (bmq_build_core.h / bmq_retain_core.h,
// the functions HostExec runs too).  What this file adds is how a WAVE counts:
//   - Ids follow the append order of the key pool (and overlay ids the order of the batches), so the ids of a wave mostly belong to one
//     tenant.  One atomic per lane would put every add of a tenant's keys on the same few words, and a hot word serialises in the L2
//     atomic unit (bmq_build_core.h, N_CTR_LANES).  So a wave first reduces its lanes per distinct table slot: the slot of the first
//     lane still to do is broadcast, one ballot finds the lanes that share it, popcounts of the per-flag ballots are the counts and a
//     cross-lane sum over the masked lanes the bytes.  A wave of one tenant takes one turn of that loop, a wave of 64 tenants 64.
//   - A wave owns a CONTIGUOUS stretch of ids (n / waves, rounded up to whole turns of 64), not a stride of the grid: neighbouring
//     turns then continue the same tenant, and the wave CARRIES (slot, sums) in registers from turn to turn -- wave-uniform values --
//     and adds them to the table only when the slot changes and after its last turn.  On the C3 index (10 M keys, 1000 tenants,
//     8192 waves of 20 turns) that is one or two flushes per wave instead of twenty.
//   - The boundary keys are staged in LDS per wave (each wave its own slice, so no workgroup barrier: the waves stay independent),
//     as k_b_boundary stages them per workgroup: the compare of every lane reads them by broadcast.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/census_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>

#include "bmq_dist_kernels.h" // wave_sync
#endif

#include "bmq_build_core.h"
#include "bmq_retain_core.h"

#ifndef BMQ_CENSUS_FLUSH_HOOK // (the emulator harness counts the flushes of a wave against its model of the runs)
#define BMQ_CENSUS_FLUSH_HOOK() ((void)0)
#endif

namespace bmq {

constexpr uint32_t CENSUS_WAVES = 4;     // waves per workgroup (independent)
constexpr uint32_t CENSUS_BLOCKS = 2048; // 256 CUs x 8 workgroups of 256 lanes
constexpr uint32_t CENSUS_TURNS = 4;     // a wave takes at least this many turns of 64 ids before the grid grows (small inputs carry too)
constexpr uint32_t CENSUS_LDS = 256;     // bytes of each boundary key a wave stages (a longer key is read where it lies)
// workgroups of a launch over n ids
__host__ __device__ inline uint32_t census_grid(uint32_t n) {
    const unsigned long long per = 64ull * CENSUS_WAVES * CENSUS_TURNS, g = ((unsigned long long)n + per - 1) / per;
    return g < 1 ? 1u : (g > CENSUS_BLOCKS ? CENSUS_BLOCKS : (uint32_t)g);
}
// turns of 64 ids every wave of a grid of `blocks` workgroups takes
__host__ __device__ inline uint32_t census_turns(uint32_t n, uint32_t blocks) {
    const unsigned long long per = 64ull * CENSUS_WAVES * blocks;
    return (uint32_t)(((unsigned long long)n + per - 1) / per);
}

// the sums a wave carries: wave-uniform (every lane holds the same values)
struct CensusRun {
    uint32_t slot; // NONE: nothing carried
    uint32_t c[3]; // keys with flag 1 / 2 / 3 (k_r_census: topics in c[0])
    unsigned long long bytes;
};
// table: W 64-bit words per slot -- W = 4: three counts and the bytes; W = 1: one count
template <uint32_t W> __device__ __forceinline__ void census_flush(unsigned long long* table, const CensusRun& run, uint32_t lane) {
    if (run.slot == NONE) return;
    if (lane == 0) {
        BMQ_CENSUS_FLUSH_HOOK();
        unsigned long long* t = table + (size_t)W * run.slot;
        if (run.c[0]) atomicAdd(t, (unsigned long long)run.c[0]);
        if (W == 4) {
            if (run.c[1]) atomicAdd(t + 1, (unsigned long long)run.c[1]);
            if (run.c[2]) atomicAdd(t + 2, (unsigned long long)run.c[2]);
            if (run.bytes) atomicAdd(t + 3, run.bytes);
        }
    }
}
// One turn: every lane of the wave comes with its slot (NONE: nothing to count), flag and length.  All 64 lanes call it together.
template <uint32_t W>
__device__ __forceinline__ void census_turn(unsigned long long* table, CensusRun& run, uint32_t slot, uint32_t flag, uint32_t len, uint32_t lane) {
    unsigned long long todo = __ballot(slot != NONE);
    while (todo) { // (wave-uniform: one turn of the loop per distinct slot)
        const uint32_t s = __shfl(slot, (uint32_t)__ffsll((long long)todo) - 1u);
        const bool mine = slot == s;
        const unsigned long long mask = __ballot(mine);
        uint32_t c0, c1 = 0, c2 = 0;
        unsigned long long bytes = 0;
        if (W == 4) {
            c0 = (uint32_t)__popcll(__ballot(mine && flag == 1u));
            c1 = (uint32_t)__popcll(__ballot(mine && flag == 2u));
            c2 = (uint32_t)__popcll(__ballot(mine && flag == 3u));
            // a key is shorter than 2^24 bytes (the reference keeps 24 bits of it): 64 of them sum up in 32 bits
            uint32_t b = mine ? len : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) b += (uint32_t)__shfl_xor(b, d);
            bytes = b;
        } else c0 = (uint32_t)__popcll(mask);
        if (s != run.slot) { // the run ends here: its sums go to the table, a new one starts
            census_flush<W>(table, run, lane);
            run.slot = s;
            run.c[0] = run.c[1] = run.c[2] = 0;
            run.bytes = 0;
        }
        run.c[0] += c0;
        run.c[1] += c1;
        run.c[2] += c2;
        run.bytes += bytes;
        todo &= ~mask;
    }
}

// table[4 * directory slot + {0, 1, 2, 3}] += live keys of kref[0, n) inside `b` with flag 1 / 2 / 3, and their bytes
__global__ __launch_bounds__(CENSUS_WAVES * 64) void k_b_census(DistIndexMut ix, uint32_t n, KeyBoundary b, unsigned long long* table) {
    __shared__ uint8_t s_key[CENSUS_WAVES][2][CENSUS_LDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if ((b.flags & 1u) && b.start_len <= CENSUS_LDS) {
        for (uint32_t p = lane; p < b.start_len; p += 64) s_key[wave][0][p] = b.start[p];
    }
    if ((b.flags & 2u) && b.end_len <= CENSUS_LDS) {
        for (uint32_t p = lane; p < b.end_len; p += 64) s_key[wave][1][p] = b.end[p];
    }
    wave_sync();
    if ((b.flags & 1u) && b.start_len <= CENSUS_LDS) b.start = s_key[wave][0];
    if ((b.flags & 2u) && b.end_len <= CENSUS_LDS) b.end = s_key[wave][1];
    const uint32_t turns = census_turns(n, gridDim.x);
    const unsigned long long first = ((unsigned long long)blockIdx.x * CENSUS_WAVES + wave) * turns * 64ull; // the wave's stretch of ids
    CensusRun run{NONE, {0, 0, 0}, 0};
    for (uint32_t t = 0; t < turns; t++) {
        const unsigned long long i = first + (unsigned long long)t * 64 + lane;
        uint32_t flag = 0, len = 0;
        const uint32_t slot = i < n ? census_key_one(ix, (uint32_t)i, b, flag, len) : NONE;
        census_turn<4>(table, run, slot, flag, len, lane);
    }
    census_flush<4>(table, run, lane);
}

// table[tenant node] += retained topics among the overlay ids [m.base_n, n_ids)
__global__ __launch_bounds__(CENSUS_WAVES * 64) void k_r_census(RetainMut m, uint32_t n_ids, unsigned long long* table) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n = n_ids - m.base_n;
    const uint32_t turns = census_turns(n, gridDim.x);
    const unsigned long long first = ((unsigned long long)blockIdx.x * CENSUS_WAVES + wave) * turns * 64ull;
    CensusRun run{NONE, {0, 0, 0}, 0};
    for (uint32_t t = 0; t < turns; t++) {
        const unsigned long long i = first + (unsigned long long)t * 64 + lane;
        const uint32_t slot = i < n ? census_topic_one(m, m.base_n + (uint32_t)i) : NONE;
        census_turn<1>(table, run, slot, 1u, 0u, lane);
    }
    census_flush<1>(table, run, lane);
}

} // namespace bmq
