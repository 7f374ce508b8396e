// bmq_delivery_kernels.h -- gfx950 kernels of the delivery plan (bmq_delivery_core.h).  One lane per item throughout: the map runs over the
// share groups of a batch (hundreds), the count over its final groups, the merge over its delivery rows.  k_dl_merge is the one that
// moves data: a lane reads its pair (consecutive lanes: consecutive words of g_topic / g_route, or of r_pair), takes its group from the
// wave's hint (one binary search per wave over the offsets, scalar loads) and finds its rank by a search over the other list of its group -- neighbours
// in a list search the same list and end in neighbouring places, so the 12 bytes a row writes land next to its neighbours' except where a
// row of the other list falls between them.  No lane waits for another and only a row number is broadcast, so a group's lists may span any number of
// tiles and waves.
#pragma once
#ifndef BMQ_WAVE_EMU // (tools/emu/delivery_emu.cpp compiles this file with g++ against the wave64 emulator)
#include <hip/hip_runtime.h>
#endif

#include "bmq_delivery_core.h"

namespace bmq {

constexpr int DL_BLOCK = 256;

__global__ __launch_bounds__(DL_BLOCK) void k_dl_scatter(FanoutState st, DeliveryPlan P) {
    const uint32_t g = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (g < P.n_norm) dl_scatter_one(st, P, g);
}
__global__ __launch_bounds__(DL_BLOCK) void k_dl_map(DistIndexMut ix, FanoutState st, DeliveryPlan P) {
    const uint32_t j = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (j < P.n_sgroups) dl_map_one(ix, st, P, j);
}
__global__ __launch_bounds__(DL_BLOCK) void k_dl_assign(DeliveryPlan P) {
    const uint32_t j = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (j < P.n_sgroups) dl_assign_one(P, j);
}
__global__ __launch_bounds__(DL_BLOCK) void k_dl_count(DeliveryPlan P) {
    const uint32_t g = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (g < P.n_groups) dl_count_one(P, g);
}
// n: max(rows, groups + 1) -- the lanes in front write the group offsets as well.  The group of the wave's first row is found once, from a
// wave-uniform row number (scalar loads); the lanes only check that their row lies in it
#ifdef BMQ_WAVE_EMU
#define DL_WAVE_UNIFORM(x) (x) // (every lane of the emulator computes the same value: nothing to broadcast)
#else
#define DL_WAVE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#endif
__global__ __launch_bounds__(DL_BLOCK) void k_dl_merge(DeliveryPlan P, uint32_t n) {
    const uint32_t i = blockIdx.x * DL_BLOCK + threadIdx.x;
    const DeliveryHint hint = dl_hint(P, DL_WAVE_UNIFORM(i & ~63u));
    if (i < n) dl_merge_one(P, i, hint);
}

} // namespace bmq
