// bmq_retain_snap_kernels.h -- the snapshot of the retained-topic index as gfx950 kernels: the BMQ_HD functions of
// bmq_retain_snap_core.h, launched by DevExec::rs_* (bmq_exec_dev.h); the scans between them are the hipCUB scans the builder uses.
// A snapshot is tens of MB and runs once per generation change, under the engine lock: the kernels must not be slow, they need not be
// tuned.  Shapes:
//   * k_rs_gather: a wave owns RS_WAVE_BYTES contiguous bytes of the output.  It searches the offsets once for the items its slice begins
//     and ends in (the same addresses in every lane: one fetch per step), then its lanes take the slice's 16-byte chunks side by side --
//     a lane searches only the slice's items for its chunk's first, loads 16 bytes where the source is aligned (always, while no id in front
//     is dead: the key store and the snapshot are packed alike) and stores 16 bytes; the last chunk of the output has a byte tail;
//   * k_rs_items / k_rs_tenants: a lane per overlay item / overlay node, a byte loop up the ONode chain (the shape of k_r_topic_write);
//   * k_rs_lens: a lane per selected id; the topic bytes and the number of bulk-loaded ids are summed per wave, one atomic each.
// Resource usage of every kernel: profiles/retain_generation/kernel_resources.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "bmq_retain_snap_core.h"

namespace bmq {

constexpr int RSK = 256;                      // lanes per workgroup
constexpr uint32_t RS_WAVE_CHUNKS = 4 * 64;   // 16-byte chunks per wave: 4 KB of output
constexpr uint32_t RS_WAVE_BYTES = 16 * RS_WAVE_CHUNKS;

__global__ __launch_bounds__(RSK) void k_rs_lens(RetainMut m, RetainKeyStore ks, RsArgs A) {
    const uint32_t i = blockIdx.x * RSK + threadIdx.x;
    bool bulk = false;
    unsigned long long len = 0;
    if (i < A.S.n) len = rs_len_one(m, ks, A, i, &bulk);
    const unsigned long long n_bulk = (unsigned long long)__popcll(__ballot(bulk));
    for (int d = 32; d > 0; d >>= 1) len += __shfl_xor(len, d, 64);
    if ((threadIdx.x & 63u) == 0) {
        if (len) atomicAdd(A.totals, len);
        if (n_bulk) atomicAdd(A.totals + 1, n_bulk);
    }
}
__global__ __launch_bounds__(RSK) void k_rs_tenant_lens(RetainMut m, RsArgs A) {
    const uint32_t i = blockIdx.x * RSK + threadIdx.x;
    if (i < A.ov_nodes) rs_tenant_len_one(m, A, i);
}
__global__ __launch_bounds__(64) void k_rs_totals(RsArgs A) {
    if (threadIdx.x == 0 && blockIdx.x == 0) rs_totals_one(A);
}
__global__ __launch_bounds__(RSK) void k_rs_tenants(RetainMut m, RsArgs A) {
    const uint32_t i = blockIdx.x * RSK + threadIdx.x;
    if (i < A.ov_nodes) rs_tenant_write_one(m, A, i);
}
__global__ __launch_bounds__(64) void k_rs_items(RetainMut m, RsArgs A) {
    const uint32_t i = A.n_bulk + blockIdx.x * 64 + threadIdx.x;
    if (i < A.S.n) rs_item_write_one(m, A, i);
}
template <class SO> __global__ __launch_bounds__(RSK) void k_rs_gather(RsGather<SO> G) {
    const unsigned long long wave = (unsigned long long)blockIdx.x * (RSK / 64) + (unsigned long long)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long begin = wave * RS_WAVE_BYTES;
    if (begin >= G.bytes) return;
    const unsigned long long last = begin + RS_WAVE_BYTES <= G.bytes ? begin + RS_WAVE_BYTES - 1 : G.bytes - 1; // the slice's last byte
    const uint32_t lo = rs_item_at(G, begin, 0u, G.n), hi = rs_item_at(G, last, lo, G.n) + 1u;
    const unsigned long long c0 = wave * RS_WAVE_CHUNKS, c_end = (G.bytes + 15) / 16;
    for (uint32_t k = threadIdx.x & 63u; k < RS_WAVE_CHUNKS; k += 64) {
        const unsigned long long c = c0 + k;
        if (c < c_end) rs_gather_chunk(G, c, lo, hi);
    }
}
__global__ __launch_bounds__(RSK) void k_rs_used(const uint32_t* item_tenant, uint32_t* used, uint32_t n) {
    const uint32_t i = blockIdx.x * RSK + threadIdx.x;
    if (i < n) rs_used_one(item_tenant, used, i);
}
__global__ __launch_bounds__(RSK) void k_rs_remap(const uint32_t* item_tenant, const uint32_t* rank_of, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * RSK + threadIdx.x;
    if (i < n) rs_remap_one(item_tenant, rank_of, out, i);
}
__global__ __launch_bounds__(RSK) void k_rs_perm_lens(RsNext N) {
    const uint32_t r = blockIdx.x * RSK + threadIdx.x;
    if (r < N.n_topics) rs_perm_len_one(N, r);
}
__global__ __launch_bounds__(RSK) void k_rs_next(RsNext N) {
    const uint32_t r = blockIdx.x * RSK + threadIdx.x;
    if (r < N.n_topics) rs_next_one(N, r);
}

} // namespace bmq
