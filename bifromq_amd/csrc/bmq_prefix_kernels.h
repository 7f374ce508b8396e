// bmq_prefix_kernels.h -- gfx950 kernel of the per-prefix census (bmq_routes_prefix_census; the control is DistIndex::prefix_census):
//   k_b_prefix_census   one lane per key reference of kref[0, n): prefix_key_one (bmq_prefix_core.h, the function HostExec runs too) gives
//                       the table slot of the deepest prefix of the lane's key -- a binary search over the sorted prefixes, then a walk up
//                       the parent links -- and the wave adds to table[4 * slot ..] as k_b_census does (bmq_census_kernels.h): the lanes of
//                       a turn are reduced per distinct slot (census_turn<4>), a wave owns a contiguous stretch of ids and carries
//                       (slot, sums) from turn to turn (census_flush<4> when the slot changes and after its last turn).  Ids follow the
//                       append order of the key pool, so the keys under one filter mostly follow each other: a run of them is one flush.
// The lanes of a wave search the same table with neighbouring keys: the upper steps of the search read the same prefixes in every lane
// (one request per step), the prefix bytes and the offsets stay in L2 (a table of 65 536 filter prefixes is a few MB).  Per lane the
// search keeps three words (lo, hi, the key reference): no per-lane array, no scratch, no LDS, and nothing waits for another wave.
// The kernel only reads the index.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/prefix_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>
#endif

#include "bmq_census_kernels.h"
#include "bmq_prefix_core.h"

namespace bmq {

// table[4 * table slot + {0, 1, 2, 3}] += live keys of kref[0, n) whose deepest prefix in T is that slot, with flag 1 / 2 / 3, and their bytes
__global__ __launch_bounds__(CENSUS_WAVES * 64) void k_b_prefix_census(DistIndexMut ix, uint32_t n, PrefixTable T, unsigned long long* table) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t turns = census_turns(n, gridDim.x);
    const unsigned long long first = ((unsigned long long)blockIdx.x * CENSUS_WAVES + wave) * turns * 64ull; // the wave's stretch of ids
    CensusRun run{NONE, {0, 0, 0}, 0};
    for (uint32_t t = 0; t < turns; t++) {
        const unsigned long long i = first + (unsigned long long)t * 64 + lane;
        uint32_t flag = 0, len = 0;
        const uint32_t slot = i < n ? prefix_key_one(ix, (uint32_t)i, T, flag, len) : NONE;
        census_turn<4>(table, run, slot, flag, len, lane);
    }
    census_flush<4>(table, run, lane); // the sums the wave still carries
}

} // namespace bmq
