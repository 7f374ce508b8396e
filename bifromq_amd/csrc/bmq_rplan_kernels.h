// bmq_rplan_kernels.h -- gfx950 kernels of the retain plan (bmq_rplan_core.h; the control is RetainDyn::plan, the entry point
// bmq_retain_plan of bmq_rplan_engine.inc).  One lane per op throughout:
//   k_rp_find       rp_find_one: dictionary + edge hash of the bulk-loaded index, then the overlay trie -- O(levels) dependent line fetches
//                   per op, bound by memory latency, so one-wave workgroups as k_r_locate has them: the occupancy comes from the number of
//                   ops.  Only reads the index.
//   k_rp_group      rp_group_one: the lane hashes its own bytes and probes the group table; CAS claims, never a wait.
//   k_rp_classify   rp_classify_one; the winners are counted per action by a ballot per wave, ONE atomic per action and wave; the deltas are
//                   summed per wave and distinct tenant-table entry in front of ONE atomic per entry and wave (a batch of one tenant sent
//                   47 k atomics to one word before: 549 us of the kernel, profiles/retain_plan/README.md); lane n writes the closing 0 of
//                   the key lengths.
//   k_rp_key_write  (behind the 64-bit exclusive scan of the key lengths) rp_key_write_one: a lane composes its whole key byte by byte at
//                   out + offs[i], the shape k_r_key_write was measured with (profiles/retain_keys/README.md) -- here the strings are the
//                   batch's own, in one piece each.
// No workgroup barrier and no LDS in the source; every write is a vector store or a HIP atomic on global memory.  Registers, scratch and
// occupancy: profiles/retain_plan/README.md.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/rplan_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>
#endif

#include "bmq_caps_kernels.h"
#include "bmq_rplan_core.h"

namespace bmq {

constexpr int RPK = 256;

__global__ __launch_bounds__(64) void k_rp_find(RetainMut m, RplanBatch b, uint32_t have_index) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 64 + threadIdx.x;
    if (i < b.n) rp_find_one(m, b, (uint32_t)i, have_index != 0);
}
__global__ __launch_bounds__(RPK) void k_rp_group(RplanBatch b, uint32_t mask) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RPK + threadIdx.x;
    if (i < b.n) rp_group_one(b, (uint32_t)i, mask);
}
__global__ __launch_bounds__(RPK) void k_rp_classify(RplanBatch b) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RPK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t action = RP_SUPERSEDED, dt = 0;
    int32_t dv = 0;
    if (i < b.n) action = rp_classify_one(b, (uint32_t)i, dt, dv);
    else if (i == b.n) b.key_len[i] = 0ull;
    for (uint32_t a = RP_NONE; a <= RP_REMOVE; a++) {
        const unsigned long long mk = caps_ballot(action == a);
        if (lane == 0 && mk) atomicAdd(b.ctr + RP_C_ACTION + a, (uint32_t)__popcll(mk));
    }
    // the deltas: one round per distinct tenant-table entry among the wave's adding / removing winners (the same in every lane), ONE atomic
    // per entry and wave -- the sum is taken modulo 2^32, which is what an int32 add is
    bool pending = dv != 0;
    unsigned long long left = caps_ballot(pending);
    while (left != 0) {
        const uint32_t leader = (uint32_t)__ffsll((long long)left) - 1u;
        const uint32_t lt = __shfl(dt, (int)leader);
        const bool mine = pending && dt == lt;
        const unsigned long long up = caps_ballot(mine && dv > 0), down = caps_ballot(mine && dv < 0);
        const uint32_t sum = (uint32_t)__popcll(up) - (uint32_t)__popcll(down);
        if (lane == leader && sum != 0) atomicAdd(reinterpret_cast<uint32_t*>(b.delta) + lt, sum);
        if (mine) pending = false;
        left &= ~(up | down);
    }
}
__global__ __launch_bounds__(RPK) void k_rp_key_write(RplanBatch b, const unsigned long long* offs, uint8_t* out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RPK + threadIdx.x;
    if (i < b.n) rp_key_write_one(b, (uint32_t)i, offs, out);
}

} // namespace bmq
