// bmq_retain_build_kernels.h -- the bulk load of the retained-topic index as gfx950 kernels: one lane per item / rank / node / table
// word / posting / run / tenant of the BMQ_HD functions of bmq_retain_build_core.h (what each stage does is said there; DevExec::rb_*
// in bmq_exec_dev.h launches them, the sorts and scans between them are hipCUB device primitives).  The lanes are independent: pointer
// arithmetic over flat arrays, byte compares of short strings, CAS claims of table entries -- bound by memory latency, occupancy comes
// from the number of items.  No kernel here waits for another lane: a claim either wins or moves on.  Resource usage of every kernel:
// profiles/retain_build/kernel_resources.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "bmq_retain_build_core.h"

namespace bmq {

constexpr int RBK = 256; // lanes per workgroup

#define BMQ_RB_KERNEL(name, fn, count)                                                 \
    __global__ __launch_bounds__(RBK) void name(RbArgs B) {                            \
        const uint32_t i = blockIdx.x * RBK + threadIdx.x;                             \
        if (i < (count)) fn(B, i);                                                     \
    }
BMQ_RB_KERNEL(k_rb_keep, rb_keep_one, B.n_items)
BMQ_RB_KERNEL(k_rb_rank, rb_rank_one, B.n_items)
BMQ_RB_KERNEL(k_rb_shape, rb_shape_one, B.n_topics)
BMQ_RB_KERNEL(k_rb_count, rb_count_one, B.n_tenants)
BMQ_RB_KERNEL(k_rb_intern, rb_intern_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_owner, rb_owner_one, B.own_mask + 1u)
BMQ_RB_KERNEL(k_rb_place, rb_place_one, B.own_mask + 1u)
BMQ_RB_KERNEL(k_rb_token, rb_token_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_edge, rb_edge_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_edge_overflow, rb_edge_overflow_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_post_flag, rb_post_flag_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_post_emit, rb_post_emit_one, B.n_nodes)
BMQ_RB_KERNEL(k_rb_post_gp, rb_post_gp_one, B.n_posts)
BMQ_RB_KERNEL(k_rb_post_write, rb_post_write_one, B.n_posts)
BMQ_RB_KERNEL(k_rb_post_tenant, rb_post_tenant_one, B.n_tenants)
BMQ_RB_KERNEL(k_rb_run_start, rb_run_start_one, B.n_posts)
BMQ_RB_KERNEL(k_rb_gp, rb_gp_one, B.n_runs)
BMQ_RB_KERNEL(k_rb_gp_overflow, rb_gp_overflow_one, B.n_runs)
BMQ_RB_KERNEL(k_rb_tenant, rb_tenant_one, B.n_tenants)
#undef BMQ_RB_KERNEL

__global__ __launch_bounds__(RBK) void k_rb_iota(uint32_t* p, uint32_t n) {
    const uint32_t i = blockIdx.x * RBK + threadIdx.x;
    if (i < n) p[i] = i;
}
// table entries of 16 bytes whose first word NONE says "free" (REdge, RGp)
__global__ __launch_bounds__(RBK) void k_rb_fill16(uint4* p, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * RBK + threadIdx.x;
    if (i < n) p[i] = make_uint4(NONE, 0u, 0u, 0u);
}
__global__ __launch_bounds__(RBK) void k_rb_head(RbArgs B, uint32_t d) {
    const uint32_t r = blockIdx.x * RBK + threadIdx.x;
    if (r < B.n_topics) rb_head_one(B, r, d);
}
__global__ __launch_bounds__(RBK) void k_rb_root(RbArgs B, const uint32_t* S1) {
    const uint32_t t = blockIdx.x * RBK + threadIdx.x;
    if (t < B.n_tenants) rb_root_one(B, t, S1);
}
__global__ __launch_bounds__(RBK) void k_rb_emit(RbArgs B, uint32_t d, const uint32_t* Sp, const uint32_t* Sc, const uint32_t* Sn) {
    const uint32_t r = blockIdx.x * RBK + threadIdx.x;
    if (r < B.n_topics) rb_emit_one(B, r, d, Sp, Sc, Sn);
}
__global__ __launch_bounds__(RBK) void k_rb_close(RbArgs B, uint32_t d, const uint32_t* Sc, const uint32_t* Sn) {
    const uint32_t r = blockIdx.x * RBK + threadIdx.x;
    if (r < B.n_topics) rb_close_one(B, r, d, Sc, Sn);
}
__global__ __launch_bounds__(RBK) void k_rb_advance(RbArgs B, const uint32_t* Sc) {
    const uint32_t t = blockIdx.x * RBK + threadIdx.x;
    if (t < B.n_tenants) rb_advance_one(B, t, Sc);
}

} // namespace bmq
