// bmq_exec_dev.h -- DevExec: the builder functions of bmq_build_core.h as gfx950 kernels on the engine's HIP stream, over
// HBM-resident arrays (see bmq_dist_index.h for the Exec concept).  One lane per route key / directory slot / trie slot:
// the work is pointer chasing with lock-free CAS claims, bound by memory latency -- occupancy comes from the number of keys
// in a batch (100 k ops = 1563 waves; a 10 M-key bulk load = 156 k waves), not from anything clever inside a lane.
// The grouping sort and the tenant-run scan are rocPRIM/hipCUB device primitives (radix sort of 42-bit targets, prefix sum).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bmq_build_core.h"
#include "bmq_census_kernels.h"
#include "bmq_delivery_kernels.h"
#include "bmq_fanout_core.h"
#include "bmq_fanout_kernels.h"
#include "bmq_order_kernels.h"
#include "bmq_prefix_kernels.h"
#include "bmq_caps_kernels.h"
#include "bmq_gate_kernels.h"
#include "bmq_retain_build_kernels.h"
#include "bmq_retain_core.h"
#include "bmq_retain_snap_kernels.h"
#include "bmq_rplan_kernels.h"
#include "bmq_share_kernels.h"

namespace bmq {

constexpr int BK = 64; // lanes per builder workgroup: one wave, independent lanes

__global__ __launch_bounds__(256) void k_b_fill_slots(TrieSlot* p, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        uint4* q = reinterpret_cast<uint4*>(p + i);
        q[0] = make_uint4(NONE, 0u, 0u, 0u);
        q[1] = make_uint4(0u, 0u, NONE, 0u);
    }
}
__global__ __launch_bounds__(256) void k_b_iota(uint32_t* p, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = i;
}
__global__ __launch_bounds__(BK) void k_b_prepare(DistIndexMut ix, OpBatch ob) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) prepare_one(ix, ob, i);
}
__global__ __launch_bounds__(BK) void k_b_prepare_check(DistIndexMut ix, OpBatch ob, uint32_t n_dir) {
    if (ix.bc->gate) return; // (an earlier stage of the batch handed over to the host: BuildCounters.gate)
    const uint32_t d = blockIdx.x * BK + threadIdx.x;
    if (d < n_dir) prepare_check_one(ix, ob, d);
}
// closes the gate behind a stage that left work for the host
__global__ void k_b_gate(BuildCounters* bc, uint32_t stage) {
    if (threadIdx.x || blockIdx.x || bc->gate) return;
    if (bc->err || bc->n_unknown || bc->n_grow || bc->n_deferred) bc->gate = stage;
}
__global__ __launch_bounds__(BK) void k_b_bulk_prepare(DistIndexMut ix, OpBatch ob) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) bulk_prepare_one(ix, ob, i);
}
__global__ __launch_bounds__(BK) void k_b_bulk_tenants(DistIndexMut ix, OpBatch ob, const uint32_t* scan) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) bulk_tenants_one(ix, ob, i, scan);
}
__global__ __launch_bounds__(BK) void k_b_bulk_counts(OpBatch ob, uint32_t n_ten, const uint32_t* nn_incl) {
    const uint32_t t = blockIdx.x * BK + threadIdx.x;
    if (t < n_ten) bulk_counts_one(ob, t, n_ten, nn_incl);
}
__global__ __launch_bounds__(BK) void k_b_locate(DistIndexMut ix, OpBatch ob, uint32_t phase) {
    if (ix.bc->gate) return;
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) locate_one(ix, ob, i, phase);
}
__global__ __launch_bounds__(BK) void k_b_group(DistIndexMut ix, OpBatch ob) {
    if (ix.bc->gate) return;
    const uint32_t p = blockIdx.x * BK + threadIdx.x;
    if (p < ob.n) group_one(ix, ob, p);
}
__global__ __launch_bounds__(BK) void k_b_rehash(DistIndexMut ix, uint32_t old_base, uint32_t old_slots, uint32_t new_base, uint32_t new_buckets, uint32_t pass, uint32_t d) {
    const uint32_t s = blockIdx.x * BK + threadIdx.x;
    if (s < old_slots) rehash_one(ix, old_base, new_base, new_buckets, s, pass, d);
}
__global__ __launch_bounds__(BK) void k_b_tail_count(DistIndexMut ix, TailPass tp, uint32_t n_slots) {
    const uint32_t g = blockIdx.x * BK + threadIdx.x;
    if (g < n_slots) tail_count_one(ix, tp, g);
}
__global__ __launch_bounds__(BK) void k_b_tail_place(DistIndexMut ix, TailPass tp, uint32_t n_slots) {
    const uint32_t g = blockIdx.x * BK + threadIdx.x;
    if (g < n_slots) tail_place_one(ix, tp, g);
}
__global__ __launch_bounds__(BK) void k_b_dict_rehash(const DictSlot* old, uint32_t old_slots, DistIndexMut ix) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < old_slots) dict_rehash_one(old, i, ix);
}
__global__ __launch_bounds__(64) void k_b_find(DistIndexMut ix, const uint8_t* q, uint32_t tenant_len, uint32_t filter_len, uint32_t* out, uint32_t cap) {
    if (threadIdx.x == 0 && blockIdx.x == 0) find_copy(ix, q, tenant_len, filter_len, out, cap);
}
// Route keys -> route ids (find_key_one, bmq_build_core.h): one lane per key, laid out as k_b_locate lays its ops out -- the walk is a
// chain of dependent probes per key, bound by memory latency, and the occupancy comes from the number of keys.  The keys lie in a device
// buffer given as (base, references): the upload of a bmq_routes_find call, or the key pool of another generation of the index through its
// own kref entries (Share::carry).  Read-only on the index, no LDS, no cross-lane traffic but the count of malformed keys: a ballot per
// round, kept in a register, ONE atomic per wave and launch.  A bounded grid that strides (FIND_BLOCKS one-wave workgroups at most: sixteen
// per CU).
constexpr uint32_t FIND_BLOCKS = 4096;
__global__ __launch_bounds__(BK) void k_b_find_keys(DistIndexMut ix, KeySource ks, uint32_t n, uint32_t* out, uint32_t* n_bad) {
    uint32_t bad = 0; // the wave's (the same in every lane)
    for (unsigned long long base = (unsigned long long)blockIdx.x * BK; base < n; base += (unsigned long long)gridDim.x * BK) {
        const unsigned long long i = base + threadIdx.x;
        const bool b = i < n ? find_keys_one(ix, ks, (uint32_t)i, out) : false;
        bad += (uint32_t)__popcll(__ballot(b));
    }
    if (threadIdx.x == 0 && bad != 0) atomicAdd(n_bad, bad);
}
__global__ __launch_bounds__(256) void k_b_gather_refs(DistIndexMut ix, const uint32_t* ids, uint32_t n, uint32_t id_end, unsigned long long* out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) gather_ref_one(ix, ids, i, id_end, out);
}
__global__ __launch_bounds__(BK) void k_b_gather_bytes(DistIndexMut ix, const unsigned long long* refs, const uint64_t* offs, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < n) gather_bytes_one(ix, refs, offs, i, out);
}

// The boundary predicate over a chunk of key references (key_in_boundary, bmq_build_core.h): one lane per reference.  References outside
// lose their length bits in place; the chunk's inside keys and their bytes are added to ctr[0] / ctr[1].
//   - The boundary is uniform for the launch: the first BND_LDS bytes of each present key are staged in LDS once per workgroup, so a
//     lane's compare reads the boundary from LDS (every active lane of a wave is at the same step: a broadcast), never from global memory.
//     A longer boundary key is read where it lies (a uniform address too; no route key of the reference's schema needs it).
//   - Ids are handed out in append order of the key pool, so the 64 keys of a wave are neighbours there: their first words share lines.
//   - Counters: ballot + popcount for the keys, a cross-lane sum for the bytes, then ONE atomic per wave and counter -- and at most
//     4 * BND_BLOCKS waves per launch, so a 10 M-id pass adds 16 k times to the two words, not 313 k times (one hot word serialises in
//     the L2 atomic unit: bmq_build_core.h, N_CTR_LANES).
constexpr uint32_t BND_LDS = 256;
constexpr uint32_t BND_BLOCKS = 2048; // 256 CUs x 8 workgroups of 256 lanes
__global__ __launch_bounds__(256) void k_b_boundary(unsigned long long* refs, uint32_t n, const uint8_t* kpool, KeyBoundary b, unsigned long long* ctr) {
    __shared__ uint8_t s_key[2][BND_LDS];
    if ((b.flags & 1u) && b.start_len <= BND_LDS) {
        for (uint32_t p = threadIdx.x; p < b.start_len; p += 256) s_key[0][p] = b.start[p];
    }
    if ((b.flags & 2u) && b.end_len <= BND_LDS) {
        for (uint32_t p = threadIdx.x; p < b.end_len; p += 256) s_key[1][p] = b.end[p];
    }
    __syncthreads();
    if ((b.flags & 1u) && b.start_len <= BND_LDS) b.start = s_key[0];
    if ((b.flags & 2u) && b.end_len <= BND_LDS) b.end = s_key[1];
    // a bounded grid that strides over the chunk (BND_BLOCKS workgroups at most): a wave keeps its sums in registers and adds them once
    unsigned long long keys = 0, bytes = 0; // keys: the wave's (the same in every lane); bytes: this lane's until the cross-lane sum
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < n; base += (unsigned long long)gridDim.x * 256) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long len = i < n ? boundary_filter_one(kpool, refs, (uint32_t)i, b) : 0ull;
        keys += (unsigned long long)__popcll(__ballot(len != 0));
        bytes += len;
    }
    for (int d = 32; d > 0; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
    if ((threadIdx.x & 63u) == 0 && keys != 0) {
        atomicAdd(ctr, keys);
        atomicAdd(ctr + 1, bytes);
    }
}

// fan-out grouping (bmq_fanout_core.h): one lane per (topic, route) pair
__global__ __launch_bounds__(256) void k_fo_fill(DistIndexMut ix, FanoutState st, FanoutBatch b) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < b.total) fo_fill_one(ix, st, b, i);
}
__global__ __launch_bounds__(256) void k_fo_verify(DistIndexMut ix, FanoutState st, FanoutBatch b) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < b.total) fo_verify_one(ix, st, b, i);
}
__global__ __launch_bounds__(256) void k_fo_keys(DistIndexMut ix, FanoutState st, FanoutBatch b) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < b.total) fo_key_one(ix, st, b, i);
}
__global__ __launch_bounds__(256) void k_fo_emit(FanoutBatch b) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < b.total) fo_emit_one(b, j);
}
__global__ __launch_bounds__(256) void k_fo_groups(FanoutState st, FanoutBatch b) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < b.total) fo_group_one(st, b, j);
}

// retain direction: mutation of the retained-topic index (bmq_retain_core.h), one lane per op / per id
__global__ __launch_bounds__(BK) void k_r_locate(RetainMut m, RetainOps ob, uint32_t phase) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) rlocate_one(m, ob, i, phase);
}
__global__ __launch_bounds__(BK) void k_r_commit(RetainMut m, RetainOps ob) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < ob.n) rcommit_one(m, ob, i);
}
// dead ids in front of every 64-id word: ONE workgroup (a million ids are 16 k words; 100 M ids 1.6 M words = 1.5 k per thread)
__global__ __launch_bounds__(1024) void k_r_rank(const unsigned long long* bits, uint32_t* rank, uint32_t n_words) {
    __shared__ uint32_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n_words + 1023) / 1024, lo = min(n_words, tid * per), hi = min(n_words, lo + per);
    uint32_t s = 0;
    for (uint32_t w = lo; w < hi; w++) s += (uint32_t)__popcll(bits[w]);
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t run = part[tid] - s;
    for (uint32_t w = lo; w < hi; w++) {
        rank[w] = run;
        run += (uint32_t)__popcll(bits[w]);
    }
    if (tid == 1023) rank[n_words] = part[1023];
}
__global__ __launch_bounds__(256) void k_r_rehash(RetainMut m, uint32_t n_nodes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_nodes) ov_rehash_one(m, i);
}
__global__ __launch_bounds__(BK) void k_r_topic_len(RetainMut m, const uint32_t* ids, uint32_t n, uint32_t* lens) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < n) ov_topic_len_one(m, ids, i, lens);
}
__global__ __launch_bounds__(BK) void k_r_topic_write(RetainMut m, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < n) ov_topic_write_one(m, ids, i, offs, out);
}
__global__ __launch_bounds__(256) void k_r_gc_flags(RetainMut m, GcQuery q, uint8_t* flags) {
    const uint32_t id = blockIdx.x * 256 + threadIdx.x;
    if (id < q.n_ids) flags[id] = (uint8_t)gc_flag_one(m, q, id);
}
__global__ __launch_bounds__(256) void k_r_remove_ids(RetainMut m, const uint32_t* ids, uint32_t n, uint32_t n_ids) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) remove_id_one(m, ids, i, n_ids);
}
__global__ __launch_bounds__(BK) void k_r_census_bulk(RetainMut m, const uint32_t* ranges, uint32_t n_tenants, uint32_t* out) {
    const uint32_t t = blockIdx.x * BK + threadIdx.x;
    if (t < n_tenants) census_bulk_one(m, ranges, t, out);
}
__global__ __launch_bounds__(256) void k_r_census_pick(const unsigned long long* table, uint32_t n, unsigned long long* list, uint32_t* count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) census_pick_one(table, i, list, count);
}
__global__ __launch_bounds__(BK) void k_r_node_len(RetainMut m, const uint32_t* nodes, uint32_t n, uint32_t* lens) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < n) ov_node_len_one(m, nodes, i, lens);
}
__global__ __launch_bounds__(BK) void k_r_node_write(RetainMut m, const uint32_t* nodes, uint32_t n, const unsigned long long* offs, uint8_t* out) {
    const uint32_t i = blockIdx.x * BK + threadIdx.x;
    if (i < n) ov_node_write_one(m, nodes, i, offs, out);
}
// id -> retainMessageKey (key_len_one / key_write_one, bmq_retain_core.h): one lane per id.  lens[n] = 0 is the scan's last input.  A lane
// composes its whole key -- header, LevelHash bytes, escaped topic -- byte by byte at out + offs[i]: keys are 10-300 bytes at arbitrary byte
// offsets, the level hashes are a serial walk over the same bytes, and neighbouring lanes write neighbouring keys, so the partial lines of a
// wave meet in L2 before they leave for HBM (shape, measurements and resource usage: profiles/retain_keys/README.md).
__global__ __launch_bounds__(256) void k_r_key_len(RetainMut m, RetainKeyStore ks, const uint32_t* ids, uint32_t n, unsigned long long* lens) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) lens[i] = key_len_one(m, ks, ids[i]);
    else if (i == n) lens[i] = 0ull;
}
__global__ __launch_bounds__(256) void k_r_key_write(RetainMut m, RetainKeyStore ks, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) key_write_one(m, ks, ids[i], out + offs[i], offs[i + 1] - offs[i]);
}
// The boundary predicate over the retained-topic ids (retain_key_in_boundary, bmq_retain_core.h): one lane per id of [0, n_ids), in the
// launch shape of k_b_boundary -- the first BND_LDS bytes of each present boundary key staged in LDS per workgroup (a longer key is read
// where it lies: a uniform address), a bounded grid that strides over the ids, ballot + popcount for the topics and a cross-lane sum for
// the key bytes, ONE atomic per wave and counter.  ctr[0] += topics inside, ctr[1] += their key bytes (want_bytes: the lengths cost a second
// walk over the topic, so they are computed only when asked for); flags (may be null) [id] = 1 inside / 0 for the select that lists the ids.
// Neighbouring lanes hold neighbouring ranks: of one tenant mostly, so the head compare reads the same tenant bytes (a broadcast) and a
// wave whose tenant differs from the boundary key's is done after it; only the ids of the boundary key's own tenant walk their topic.
__global__ __launch_bounds__(256) void k_r_boundary(RetainMut m, RetainKeyStore ks, uint32_t n_ids, KeyBoundary b, uint8_t* flags, uint32_t want_bytes,
                                                    unsigned long long* ctr) {
    __shared__ uint8_t s_key[2][BND_LDS];
    if ((b.flags & 1u) && b.start_len <= BND_LDS) {
        for (uint32_t p = threadIdx.x; p < b.start_len; p += 256) s_key[0][p] = b.start[p];
    }
    if ((b.flags & 2u) && b.end_len <= BND_LDS) {
        for (uint32_t p = threadIdx.x; p < b.end_len; p += 256) s_key[1][p] = b.end[p];
    }
    __syncthreads();
    if ((b.flags & 1u) && b.start_len <= BND_LDS) b.start = s_key[0];
    if ((b.flags & 2u) && b.end_len <= BND_LDS) b.end = s_key[1];
    unsigned long long topics = 0, bytes = 0; // topics: the wave's (the same in every lane); bytes: this lane's until the cross-lane sum
    for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < n_ids; base += (unsigned long long)gridDim.x * 256) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long len = i < n_ids ? boundary_id_one(m, ks, (uint32_t)i, b, flags, want_bytes) : 0ull;
        topics += (unsigned long long)__popcll(__ballot(len != 0));
        bytes += want_bytes ? len : 0ull;
    }
    for (int d = 32; d > 0; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
    if ((threadIdx.x & 63u) == 0 && topics != 0) {
        atomicAdd(ctr, topics);
        atomicAdd(ctr + 1, bytes);
    }
}
__global__ __launch_bounds__(64) void k_r_find_tenant(RetainMut m, const uint8_t* name, uint32_t len, uint32_t* out) {
    if (threadIdx.x || blockIdx.x) return;
    LevelScan lv;
    unsigned long long pos = 0;
    lv.start = 0;
    scan_level_bytes<0u>(name, pos, len, lv.h, lv.inl, lv.len);
    out[0] = ov_find(m.onodes, m.oedges, m.oedge_mask, m.opool, 0u, lv.h.h1, lv.h.h2, lv.len, name, 0);
}

struct DevExec {
    std::string err;
    int device = -1;
    hipStream_t stream = nullptr;
    void* tmp = nullptr; // hipCUB temporary storage
    size_t tmp_cap = 0;

    bool ck(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        err = std::string(what) + ": " + hipGetErrorString(e);
        return false;
    }
#define BMQ_X(expr) ck((expr), #expr)
    bool launched() { return BMQ_X(hipGetLastError()); }

    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes + 64) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return p;
    }
    void release(void* p) {
        if (p) (void)hipFree(p);
    }
    ~DevExec() {
        release(tmp);
        if (pinned) (void)hipHostFree(pinned);
        if (ev_up) (void)hipEventDestroy(ev_up);
        if (ev_back) (void)hipEventDestroy(ev_back);
        for (auto& m : marks)
            if (m) (void)hipEventDestroy(m);
    }
    bool sync() { return BMQ_X(hipStreamSynchronize(stream)); }
    bool copy_in_async(void* d, const void* s, size_t n) { return n == 0 || BMQ_X(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, stream)); }
    // an apply batch's ops: uploaded on `upload_stream` (the engine's copy stream, if it has one) -- beside whatever `stream` still runs --,
    // `stream` waits for them (uploads_done); its counters come back into page-locked memory behind an event (read_back_async / _wait)
    hipStream_t upload_stream = nullptr;
    hipEvent_t ev_up = nullptr, ev_back = nullptr;
    void* pinned = nullptr;
    size_t pinned_cap = 0;
    bool upload_async(void* d, const void* s, size_t n) {
        return n == 0 || BMQ_X(hipMemcpyAsync(d, s, n, hipMemcpyDefault, upload_stream ? upload_stream : stream)); // (s: host or device memory)
    }
    bool uploads_done() {
        if (!upload_stream) return true;
        if (!ev_up && !BMQ_X(hipEventCreateWithFlags(&ev_up, hipEventDisableTiming))) return false;
        return BMQ_X(hipEventRecord(ev_up, upload_stream)) && BMQ_X(hipStreamWaitEvent(stream, ev_up, 0));
    }
    bool read_back_async(void* /*host*/, const void* dev, size_t n) {
        if (pinned_cap < n) {
            if (pinned) (void)hipHostFree(pinned);
            pinned = nullptr, pinned_cap = 0;
            if (!BMQ_X(hipHostMalloc(&pinned, n, hipHostMallocDefault))) return false;
            pinned_cap = n;
        }
        if (!ev_back && !BMQ_X(hipEventCreateWithFlags(&ev_back, hipEventDisableTiming))) return false;
        return BMQ_X(hipMemcpyAsync(pinned, dev, n, hipMemcpyDeviceToHost, stream)) && BMQ_X(hipEventRecord(ev_back, stream));
    }
    bool read_back_wait(void* host, size_t n) {
        if (!BMQ_X(hipEventSynchronize(ev_back))) return false;
        memcpy(host, pinned, n);
        return true;
    }
    bool copy_in(void* d, const void* s, size_t n) { return copy_in_async(d, s, n) && sync(); }
    bool copy_out(void* d, const void* s, size_t n) { return (n == 0 || BMQ_X(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, stream))) && sync(); }
    bool copy(void* d, const void* s, size_t n) { return n == 0 || BMQ_X(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream)); }
    bool zero(void* p, size_t n) { return n == 0 || BMQ_X(hipMemsetAsync(p, 0, n, stream)); }
    static dim3 grid(unsigned long long n, unsigned b) { return dim3((unsigned)((n + b - 1) / b)); }

    bool fill_slots(TrieSlot* p, uint64_t n) {
        // at most 2^32 slots in the table, 256 per block
        for (uint64_t o = 0; o < n; o += (1ull << 31)) {
            const uint64_t m = std::min<uint64_t>(n - o, 1ull << 31);
            hipLaunchKernelGGL(k_b_fill_slots, grid(m, 256), dim3(256), 0, stream, p + o, (unsigned long long)m);
        }
        return launched();
    }
    bool prepare(const DistIndexMut& ix, const OpBatch& ob) {
        hipLaunchKernelGGL(k_b_prepare, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob);
        return launched();
    }
    static constexpr bool gated = true; // the stages of an apply batch can run back to back behind BuildCounters.gate
    bool gate(BuildCounters* bc, uint32_t stage) {
        hipLaunchKernelGGL(k_b_gate, dim3(1), dim3(1), 0, stream, bc, stage);
        return launched();
    }
    bool prepare_check(const DistIndexMut& ix, const OpBatch& ob, uint32_t n_dir) {
        hipLaunchKernelGGL(k_b_prepare_check, grid(n_dir, BK), dim3(BK), 0, stream, ix, ob, n_dir);
        return launched();
    }
    bool bulk_prepare(const DistIndexMut& ix, const OpBatch& ob) {
        hipLaunchKernelGGL(k_b_bulk_prepare, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob);
        return launched();
    }
    bool ensure_tmp(size_t bytes) {
        if (bytes <= tmp_cap) return true;
        if (!sync()) return false;
        release(tmp);
        tmp = alloc(bytes + bytes / 4);
        tmp_cap = tmp ? bytes + bytes / 4 : 0;
        if (!tmp) err = "out of device memory (sort scratch)";
        return tmp != nullptr;
    }
    bool scan_flags(const uint32_t* in, uint32_t* out, uint32_t n) { // inclusive
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceScan::InclusiveSum(nullptr, bytes, in, out, (int)n, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceScan::InclusiveSum(tmp, bytes, in, out, (int)n, stream));
    }
    bool bulk_tenants(const DistIndexMut& ix, const OpBatch& ob, const uint32_t* scan) {
        hipLaunchKernelGGL(k_b_bulk_tenants, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob, scan);
        return launched();
    }
    bool bulk_counts(const OpBatch& ob, uint32_t n_ten, const uint32_t* nn_incl) {
        hipLaunchKernelGGL(k_b_bulk_counts, grid(n_ten, BK), dim3(BK), 0, stream, ob, n_ten, nn_incl);
        return launched();
    }
    bool locate(const DistIndexMut& ix, const OpBatch& ob) {
        if (!ob.op) {
            hipLaunchKernelGGL(k_b_locate, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob, 2u);
            return launched();
        }
        hipLaunchKernelGGL(k_b_locate, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob, 3u); // every op; a delete that finds no filter is marked
        hipLaunchKernelGGL(k_b_locate, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob, 4u); // the marked deletes, behind every put of the batch
        return launched();
    }
    bool sort_targets(const OpBatch& ob) { // stable: ops on one target stay in op order.  Values = op indices.
        uint32_t* iota = ob.unknown_list; // free again after prepare
        hipLaunchKernelGGL(k_b_iota, grid(ob.n, 256), dim3(256), 0, stream, iota, ob.n);
        if (!launched()) return false;
        size_t bytes = 0;
        const int end_bit = (int)TARGET_KIND_SHIFT + 2;
        if (!BMQ_X(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, ob.target, ob.sorted_target, iota, ob.order, (int)ob.n, 0, end_bit, stream)))
            return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, ob.target, ob.sorted_target, iota, ob.order, (int)ob.n, 0, end_bit, stream));
    }
    bool group(const DistIndexMut& ix, const OpBatch& ob) {
        hipLaunchKernelGGL(k_b_group, grid(ob.n, BK), dim3(BK), 0, stream, ix, ob);
        return launched();
    }
    bool rehash(const DistIndexMut& ix, uint32_t old_base, uint32_t old_slots, uint32_t new_base, uint32_t new_buckets, uint32_t d) {
        hipLaunchKernelGGL(k_b_rehash, grid(old_slots, BK), dim3(BK), 0, stream, ix, old_base, old_slots, new_base, new_buckets, 0u, d);
        hipLaunchKernelGGL(k_b_rehash, grid(old_slots, BK), dim3(BK), 0, stream, ix, old_base, old_slots, new_base, new_buckets, 1u, d); // ('+' children beside their parents)
        return launched();
    }
    bool tails(const DistIndexMut& ix, const TailPass& tp, uint32_t n_slots) {
        hipLaunchKernelGGL(k_b_tail_count, grid(n_slots, BK), dim3(BK), 0, stream, ix, tp, n_slots);
        hipLaunchKernelGGL(k_b_tail_place, grid(n_slots, BK), dim3(BK), 0, stream, ix, tp, n_slots);
        return launched();
    }
    bool dict_rehash(const DictSlot* old, uint32_t old_slots, const DistIndexMut& ix) {
        hipLaunchKernelGGL(k_b_dict_rehash, grid(old_slots, BK), dim3(BK), 0, stream, old, old_slots, ix);
        return launched();
    }
    bool find(const DistIndexMut& ix, const uint8_t* q, uint32_t tenant_len, uint32_t filter_len, uint32_t* out, uint32_t cap) {
        hipLaunchKernelGGL(k_b_find, dim3(1), dim3(64), 0, stream, ix, q, tenant_len, filter_len, out, cap);
        return launched();
    }
    // out[i] = id of the live route whose key is key i of `ks`, NONE if there is none; *n_bad += malformed keys (the caller zeroes it)
    bool find_keys(const DistIndexMut& ix, const KeySource& ks, uint32_t n, uint32_t* out, uint32_t* n_bad) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_b_find_keys, dim3((unsigned)std::min<unsigned long long>(((unsigned long long)n + BK - 1) / BK, FIND_BLOCKS)), dim3(BK), 0, stream, ix, ks, n, out, n_bad);
        return launched();
    }
    // ---- key-ordered window (bmq_order_core.h, bmq_order_kernels.h): bounded grids that stride ----
    static dim3 o_grid(uint32_t n) { return dim3((unsigned)std::min<unsigned long long>(((unsigned long long)n + ORD_BLOCK - 1) / ORD_BLOCK, ORD_BLOCKS)); }
    bool o_flag(const DistIndexMut& ix, uint32_t n_ids, const OrderCursor& c, uint32_t* cand, uint32_t* n_cand) {
        if (n_ids == 0) return true;
        hipLaunchKernelGGL(k_o_flag, o_grid(n_ids), dim3(ORD_BLOCK), 0, stream, ix, n_ids, c, cand, n_cand);
        return launched();
    }
    bool o_pivots(const DistIndexMut& ix, const uint32_t* list, uint32_t stride, uint32_t P, uint32_t* piv) {
        hipLaunchKernelGGL(k_o_pivots, dim3(P), dim3(64), 0, stream, ix, list, stride, P, piv);
        return launched();
    }
    bool o_bucket(const DistIndexMut& ix, const uint32_t* list, uint32_t n, const uint32_t* piv, uint32_t P, uint16_t* bins, uint32_t* hist) {
        hipLaunchKernelGGL(k_o_bucket, o_grid(n), dim3(ORD_BLOCK), 0, stream, ix, list, n, piv, P, bins, hist);
        return launched();
    }
    bool o_scatter(const uint32_t* list, const uint16_t* bins, uint32_t n, const uint32_t* base, uint32_t* cursor, uint32_t* dst) {
        hipLaunchKernelGGL(k_o_scatter, o_grid(n), dim3(ORD_BLOCK), 0, stream, list, bins, n, base, cursor, dst);
        return launched();
    }
    bool o_leaves(const DistIndexMut& ix, const uint32_t* list0, const uint32_t* list1, const OrderLeaf* leaves, uint32_t n_leaves, uint32_t* out) {
        if (n_leaves == 0) return true;
        hipLaunchKernelGGL(k_o_leaves, dim3(n_leaves * ORDER_BUCKET_MAX), dim3(64), 0, stream, ix, list0, list1, leaves, out);
        return launched();
    }
    // ---- fan-out grouping (bmq_fanout.h) ----
    bool fill_bytes(void* p, int byte, size_t n) { return n == 0 || BMQ_X(hipMemsetAsync(p, byte, n, stream)); }
    bool fo_fill(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        hipLaunchKernelGGL(k_fo_fill, grid(b.total, 256), dim3(256), 0, stream, ix, st, b);
        return launched();
    }
    bool fo_verify(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        hipLaunchKernelGGL(k_fo_verify, grid(b.total, 256), dim3(256), 0, stream, ix, st, b);
        return launched();
    }
    bool fo_keys(const DistIndexMut& ix, const FanoutState& st, const FanoutBatch& b) {
        hipLaunchKernelGGL(k_fo_keys, grid(b.total, 256), dim3(256), 0, stream, ix, st, b);
        return launched();
    }
    bool sort_pairs32(const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, int end_bit) {
        size_t bytes = 0; // LSD radix sort: stable
        if (!BMQ_X(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit, stream));
    }
    bool fo_emit(const FanoutBatch& b) {
        hipLaunchKernelGGL(k_fo_emit, grid(b.total, 256), dim3(256), 0, stream, b);
        return launched();
    }
    bool fo_groups(const FanoutState& st, const FanoutBatch& b) {
        hipLaunchKernelGGL(k_fo_groups, grid(b.total, 256), dim3(256), 0, stream, st, b);
        return launched();
    }
    bool gather_refs(const DistIndexMut& ix, const uint32_t* ids, uint32_t n, uint32_t id_end, unsigned long long* out) {
        hipLaunchKernelGGL(k_b_gather_refs, grid(n, 256), dim3(256), 0, stream, ix, ids, n, id_end, out);
        return launched();
    }
    bool gather_bytes(const DistIndexMut& ix, const unsigned long long* refs, const uint64_t* offs, uint32_t n, uint8_t* out) {
        hipLaunchKernelGGL(k_b_gather_bytes, grid(n, BK), dim3(BK), 0, stream, ix, refs, offs, n, out);
        return launched();
    }
    // refs[0, n): references outside `b` lose their length bits; ctr[0] += keys inside, ctr[1] += their bytes (b's keys: exec memory)
    bool boundary_filter(unsigned long long* refs, uint32_t n, const uint8_t* kpool, const KeyBoundary& b, unsigned long long* ctr) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_b_boundary, dim3(std::min((n + 255u) / 256u, BND_BLOCKS)), dim3(256), 0, stream, refs, n, kpool, b, ctr);
        return launched();
    }
    // table[4 * directory slot ..] += live keys of kref[0, n) inside `b` per flag, and their bytes (k_b_census, bmq_census_kernels.h; b's keys: exec memory)
    bool census(const DistIndexMut& ix, uint32_t n, const KeyBoundary& b, unsigned long long* table) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_b_census, dim3(census_grid(n)), dim3(CENSUS_WAVES * 64), 0, stream, ix, n, b, table);
        return launched();
    }
    // table[4 * table slot ..] += live keys of kref[0, n) per flag, and their bytes, under the deepest prefix of T each has (k_b_prefix_census,
    // bmq_prefix_kernels.h; T's arrays: exec memory)
    bool prefix_census(const DistIndexMut& ix, uint32_t n, const PrefixTable& T, unsigned long long* table) {
        if (n == 0 || T.n == 0) return true;
        hipLaunchKernelGGL(k_b_prefix_census, dim3(census_grid(n)), dim3(CENSUS_WAVES * 64), 0, stream, ix, n, T, table);
        return launched();
    }
    // ---- fan-out grouping, fast path (bmq_fanout_kernels.h): counting sort that carries its payload ----
    static constexpr bool has_fanout_fast = true;
    bool fo_dense(const FanoutState& st, uint16_t* dense, uint32_t* n_used) {
        hipLaunchKernelGGL(k_fo_dense, dim3(1), dim3(1024), 0, stream, st.gt_hash, st.gt_cap, dense, n_used);
        return launched();
    }
    bool fo_fast(const DistIndexMut& ix, const FanoutState& st, const FanoutFast& f) {
        const dim3 grid((f.n_tiles + FO_WAVES - 1) / FO_WAVES), block(FO_WAVES * 64);
        static const bool timing = bmq_env("BMQ_TIMING") != nullptr; // profiling experiments only: per-kernel HIP-event times on stderr
        hipEvent_t ev[5] = {};
        if (timing)
            for (auto& e : ev) (void)hipEventCreate(&e);
        if (timing) (void)hipEventRecord(ev[0], stream);
        hipLaunchKernelGGL(k_fo_hist, grid, block, 0, stream, ix, st, f);
        if (!launched()) return false;
        if (timing) (void)hipEventRecord(ev[1], stream);
        const int n = (int)((size_t)f.n_bins * f.n_tiles) + 1; // + the end mark
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, f.hist, f.hist, n, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        if (!BMQ_X(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, f.hist, f.hist, n, stream))) return false;
        if (timing) (void)hipEventRecord(ev[2], stream);
        hipLaunchKernelGGL(k_fo_scatter, dim3((f.n_tiles + FO_SC_WAVES - 1) / FO_SC_WAVES), dim3(FO_SC_WAVES * 64), FO_SC_WAVES * fo_scatter_lds(f.n_bins, f.tile),
                           stream, f);
        if (timing) (void)hipEventRecord(ev[3], stream);
        hipLaunchKernelGGL(k_fo_groups2, dim3(1), dim3(1024), 0, stream, st, f);
        if (timing) {
            (void)hipEventRecord(ev[4], stream);
            (void)hipEventSynchronize(ev[4]);
            float t[4] = {0, 0, 0, 0};
            for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&t[i], ev[i], ev[i + 1]);
            fprintf(stderr, "[bmq] fan-out grouping (%u pairs, %u keys, %u tiles): hist %.3f ms, scan %.3f, scatter %.3f, groups %.3f\n", f.total, f.n_bins,
                    f.n_tiles, t[0], t[1], t[2], t[3]);
            for (auto& e : ev) (void)hipEventDestroy(e);
        }
        return launched();
    }
    // ---- optional HIP-event marks between the steps of a pipeline (bmq_set_kernel_timing) ----
    bool marks_on = false;
    hipEvent_t marks[24] = {}; // 0 .. 7: the resolve and the carry of bmq_share.h, 8 .. 12: the delivery plan, 13 .. 16: the fan-out caps, 17 .. 20: the fan-out gate
    void mark(int i) {
        if (!marks_on) return;
        if (!marks[i] && hipEventCreate(&marks[i]) != hipSuccess) return;
        (void)hipEventRecord(marks[i], stream);
    }
    float mark_ms(int a, int b) { // after a sync of the stream
        float t = 0;
        if (!marks_on || !marks[a] || !marks[b] || hipEventElapsedTime(&t, marks[a], marks[b]) != hipSuccess) return 0;
        return t;
    }
    // ---- receivers of shared subscriptions (bmq_share.h; kernels: bmq_share_kernels.h) ----
    bool sh_count(const DistIndexMut& ix, const ShareTables& T, const ShareBatch& b) {
        hipLaunchKernelGGL(k_sh_count, grid(b.n_pairs, SH_BLOCK), dim3(SH_BLOCK), 0, stream, ix, T, b);
        return launched();
    }
    bool sh_rows(const ShareTables& T, const ShareBatch& b) {
        hipLaunchKernelGGL(k_sh_rows, grid(b.n_rows, SH_BLOCK), dim3(SH_BLOCK), 0, stream, T, b);
        return launched();
    }
    // width: lanes per row (8, 16 or 64); at most 2^24 rows per launch, so that a launch stays below 2^32 threads
    bool sh_resolve(const ShareTables& T, const ShareBatch& b, uint32_t width) {
        const uint32_t chunk = 1u << 24;
        for (uint32_t row0 = 0; row0 < b.n_rows; row0 += chunk) {
            const uint32_t n = std::min(chunk, b.n_rows - row0);
            const dim3 g = grid((unsigned long long)n * width, SH_BLOCK);
            if (width == 8) hipLaunchKernelGGL(k_sh_resolve<8>, g, dim3(SH_BLOCK), 0, stream, T, b, row0, n);
            else if (width == 16) hipLaunchKernelGGL(k_sh_resolve<16>, g, dim3(SH_BLOCK), 0, stream, T, b, row0, n);
            else hipLaunchKernelGGL(k_sh_resolve<64>, g, dim3(SH_BLOCK), 0, stream, T, b, row0, n);
        }
        return launched();
    }
    bool sh_heads(const ShareBatch& b, bool emit) {
        hipLaunchKernelGGL(k_sh_heads, grid(b.n_rows, SH_BLOCK), dim3(SH_BLOCK), 0, stream, b, emit ? 1 : 0);
        return launched();
    }
    bool sh_groups(const ShareTables& T, const ShareBatch& b) {
        hipLaunchKernelGGL(k_sh_groups, grid(b.n_rows, SH_BLOCK), dim3(SH_BLOCK), 0, stream, T, b);
        return launched();
    }
    // ---- the delivery plan (bmq_delivery.h) ----
    bool dl_map(const DistIndexMut& ix, const FanoutState& st, const DeliveryPlan& P) { // slot_group[] is filled with DL_NONE before
        if (P.n_norm) hipLaunchKernelGGL(k_dl_scatter, grid(P.n_norm, DL_BLOCK), dim3(DL_BLOCK), 0, stream, st, P);
        hipLaunchKernelGGL(k_dl_map, grid(P.n_sgroups, DL_BLOCK), dim3(DL_BLOCK), 0, stream, ix, st, P);
        return launched();
    }
    bool dl_assign(const DeliveryPlan& P) {
        hipLaunchKernelGGL(k_dl_assign, grid(P.n_sgroups, DL_BLOCK), dim3(DL_BLOCK), 0, stream, P);
        return launched();
    }
    bool dl_count(const DeliveryPlan& P) {
        hipLaunchKernelGGL(k_dl_count, grid(P.n_groups, DL_BLOCK), dim3(DL_BLOCK), 0, stream, P);
        return launched();
    }
    bool dl_merge(const DeliveryPlan& P) {
        const uint32_t n = std::max(P.n_rows, P.n_groups + 1);
        hipLaunchKernelGGL(k_dl_merge, grid(n, DL_BLOCK), dim3(DL_BLOCK), 0, stream, P, n);
        return launched();
    }
    // ---- the fan-out caps over a match CSR (bmq_caps.h; kernels: bmq_caps_kernels.h) ----
    static dim3 caps_grid(unsigned long long n) { return dim3((unsigned)std::min<unsigned long long>((n + CAPS_BLOCK - 1) / CAPS_BLOCK, CAPS_BLOCKS)); }
    bool caps_classify(const DistIndexMut& ix, const CapsBatch& b) { // row_cnt[] and ctr[] are zeroed before
        if (b.total == 0) return true;
        hipLaunchKernelGGL(k_caps_classify, caps_grid(b.total), dim3(CAPS_BLOCK), 0, stream, ix, b);
        return launched();
    }
    bool caps_rows(const CapsBatch& b) {
        if (b.n_rows == 0) return true;
        hipLaunchKernelGGL(k_caps_rows, caps_grid(b.n_rows), dim3(CAPS_BLOCK), 0, stream, b);
        return launched();
    }
    bool caps_list(const CapsBatch& b) { // behind the inclusive scan of ev_cnt[]
        if (b.total == 0) return true;
        hipLaunchKernelGGL(k_caps_list, caps_grid(b.total), dim3(CAPS_BLOCK), 0, stream, b);
        return launched();
    }
    bool caps_rank(const DistIndexMut& ix, const CapsBatch& b, uint32_t n_work) {
        if (n_work == 0) return true;
        hipLaunchKernelGGL(k_caps_rank, grid(n_work, CAPS_BLOCK / 64), dim3(CAPS_BLOCK), 0, stream, ix, b, n_work);
        return launched();
    }
    bool caps_write(const CapsBatch& b) { // behind the inclusive scan of keep[]
        const uint32_t n = std::max(b.total, b.n_rows + 1);
        hipLaunchKernelGGL(k_caps_write, caps_grid(n), dim3(CAPS_BLOCK), 0, stream, b, n);
        return launched();
    }
    // ---- the submit-time fan-out gate over a match CSR (bmq_gate.h; kernels: bmq_gate_kernels.h) ----
    bool gate_classify(const DistIndexMut& ix, const GateBatch& b) { // row_cnt[], ctr[] and the meters are zeroed before
        if (b.c.total == 0) return true;
        hipLaunchKernelGGL(k_gate_classify, caps_grid(b.c.total), dim3(CAPS_BLOCK), 0, stream, ix, b);
        return launched();
    }
    bool gate_rows(const GateBatch& b) {
        if (b.c.n_rows == 0) return true;
        hipLaunchKernelGGL(k_gate_rows, caps_grid(b.c.n_rows), dim3(CAPS_BLOCK), 0, stream, b);
        return launched();
    }
    bool gate_list(const GateBatch& b) {
        if (b.c.total == 0) return true;
        hipLaunchKernelGGL(k_gate_list, caps_grid(b.c.total), dim3(CAPS_BLOCK), 0, stream, b);
        return launched();
    }
    bool gate_rank(const DistIndexMut& ix, const GateBatch& b, uint32_t n_work) {
        if (n_work == 0) return true;
        hipLaunchKernelGGL(k_gate_rank, grid(n_work, CAPS_BLOCK / 64), dim3(CAPS_BLOCK), 0, stream, ix, b, n_work);
        return launched();
    }
    bool gate_write(const GateBatch& b, bool rows) { // behind the inclusive scan of keep[]; without `rows` only flags, kept counts and meters
        const uint32_t n = std::max(rows ? std::max(b.c.total, b.c.n_rows + 1) : b.c.n_rows, b.n_gate);
        if (n == 0) return true;
        hipLaunchKernelGGL(k_gate_write, caps_grid(n), dim3(CAPS_BLOCK), 0, stream, b, n, rows ? 1u : 0u);
        return launched();
    }
    bool sh_rekey(uint32_t* slot_of, uint32_t id_cap, const uint32_t* new_id, const uint32_t* slot, uint32_t n) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_sh_rekey, grid(n, SH_BLOCK), dim3(SH_BLOCK), 0, stream, slot_of, id_cap, new_id, slot, n);
        return launched();
    }
    // ---- retain direction (bmq_retain_core.h) ----
    bool r_locate(const RetainMut& m, const RetainOps& ob) {
        hipLaunchKernelGGL(k_r_locate, grid(ob.n, BK), dim3(BK), 0, stream, m, ob, 0u); // the adds: overlay nodes come into being
        hipLaunchKernelGGL(k_r_locate, grid(ob.n, BK), dim3(BK), 0, stream, m, ob, 1u); // the removes: they find them
        return launched();
    }
    bool r_commit(const RetainMut& m, const RetainOps& ob) {
        hipLaunchKernelGGL(k_r_commit, grid(ob.n, BK), dim3(BK), 0, stream, m, ob);
        return launched();
    }
    bool r_rank(const RetainMut& m, uint32_t n_words) {
        hipLaunchKernelGGL(k_r_rank, dim3(1), dim3(1024), 0, stream, m.dead_bits, m.dead_rank, n_words);
        return launched();
    }
    bool r_rehash(const RetainMut& m, uint32_t n_nodes) {
        hipLaunchKernelGGL(k_r_rehash, grid(n_nodes, 256), dim3(256), 0, stream, m, n_nodes);
        return launched();
    }
    bool r_topic_lens(const RetainMut& m, const uint32_t* ids, uint32_t n, uint32_t* lens) {
        hipLaunchKernelGGL(k_r_topic_len, grid(n, BK), dim3(BK), 0, stream, m, ids, n, lens);
        return launched();
    }
    bool r_topic_write(const RetainMut& m, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        hipLaunchKernelGGL(k_r_topic_write, grid(n, BK), dim3(BK), 0, stream, m, ids, n, offs, out);
        return launched();
    }
    // ids (ascending) gc_flag_one accepts -> out_ids[0 .. *out_count); flags: scratch of q.n_ids bytes
    bool r_gc_select(const RetainMut& m, const GcQuery& q, uint8_t* flags, uint32_t* out_ids, uint32_t* out_count) {
        if (q.n_ids == 0) return zero(out_count, sizeof(uint32_t));
        hipLaunchKernelGGL(k_r_gc_flags, grid(q.n_ids, 256), dim3(256), 0, stream, m, q, flags);
        if (!launched()) return false;
        return r_flagged_ids(flags, q.n_ids, out_ids, out_count);
    }
    // the ids of [0, n) whose flag byte is set, ascending -> out_ids[0 .. *out_count)
    bool r_flagged_ids(const uint8_t* flags, uint32_t n, uint32_t* out_ids, uint32_t* out_count) {
        hipcub::CountingInputIterator<uint32_t> iota(0u);
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceSelect::Flagged(nullptr, bytes, iota, flags, out_ids, out_count, (int)n, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceSelect::Flagged(tmp, bytes, iota, flags, out_ids, out_count, (int)n, stream));
    }
    // ctr[0] += live ids of [0, n_ids) whose key lies inside `b`, ctr[1] += their key bytes if want_bytes; flags (may be null) [id] = inside
    // (k_r_boundary; b's keys: exec memory)
    bool r_boundary(const RetainMut& m, const RetainKeyStore& ks, uint32_t n_ids, const KeyBoundary& b, uint8_t* flags, bool want_bytes, unsigned long long* ctr) {
        if (n_ids == 0) return true;
        hipLaunchKernelGGL(k_r_boundary, dim3(std::min((n_ids + 255u) / 256u, BND_BLOCKS)), dim3(256), 0, stream, m, ks, n_ids, b, flags, want_bytes ? 1u : 0u, ctr);
        return launched();
    }
    bool r_remove_ids(const RetainMut& m, const uint32_t* ids, uint32_t n, uint32_t n_ids) {
        hipLaunchKernelGGL(k_r_remove_ids, grid(n, 256), dim3(256), 0, stream, m, ids, n, n_ids);
        return launched();
    }
    // out[t] = live topics of the bulk-loaded rank range ranges[2 t .. 2 t + 1]
    bool r_census_bulk(const RetainMut& m, const uint32_t* ranges, uint32_t n_tenants, uint32_t* out) {
        if (n_tenants == 0) return true;
        hipLaunchKernelGGL(k_r_census_bulk, grid(n_tenants, BK), dim3(BK), 0, stream, m, ranges, n_tenants, out);
        return launched();
    }
    // table[tenant node] += retained topics among the ids [m.base_n, n_ids) (k_r_census, bmq_census_kernels.h)
    bool r_census(const RetainMut& m, uint32_t n_ids, unsigned long long* table) {
        if (n_ids <= m.base_n) return true;
        hipLaunchKernelGGL(k_r_census, dim3(census_grid(n_ids - m.base_n)), dim3(CENSUS_WAVES * 64), 0, stream, m, n_ids, table);
        return launched();
    }
    bool r_census_pick(const unsigned long long* table, uint32_t n, unsigned long long* list, uint32_t* count) {
        hipLaunchKernelGGL(k_r_census_pick, grid(n, 256), dim3(256), 0, stream, table, n, list, count);
        return launched();
    }
    bool r_node_lens(const RetainMut& m, const uint32_t* nodes, uint32_t n, uint32_t* lens) {
        hipLaunchKernelGGL(k_r_node_len, grid(n, BK), dim3(BK), 0, stream, m, nodes, n, lens);
        return launched();
    }
    bool r_node_write(const RetainMut& m, const uint32_t* nodes, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        hipLaunchKernelGGL(k_r_node_write, grid(n, BK), dim3(BK), 0, stream, m, nodes, n, offs, out);
        return launched();
    }
    // ---- bulk load of the retained-topic index (bmq_retain_build_kernels.h): one call per stage, in the order of RetainBuild::build ----
    bool rb_sort_items(const RbArgs& B) { // a merge sort with the comparator over the packed strings; stable: of equal items the last one stays the last
        if (B.n_items == 0) return true;
        hipLaunchKernelGGL(k_rb_iota, grid(B.n_items, RBK), dim3(RBK), 0, stream, B.idx, B.n_items);
        if (!launched()) return false;
        const RbItemLess less{B.topics, B.topic_off, B.item_tenant};
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceMergeSort::StableSortKeys(nullptr, bytes, B.idx, (int)B.n_items, less, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceMergeSort::StableSortKeys(tmp, bytes, B.idx, (int)B.n_items, less, stream));
    }
    bool rb_fill16(void* p, uint64_t n) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_rb_fill16, grid(n, RBK), dim3(RBK), 0, stream, (uint4*)p, (unsigned long long)n);
        return launched();
    }
    bool rb_iota(uint32_t* p, uint32_t n) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_rb_iota, grid(n, RBK), dim3(RBK), 0, stream, p, n);
        return launched();
    }
    bool sort_pairs64(const unsigned long long* keys_in, unsigned long long* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n) {
        size_t bytes = 0; // LSD radix sort: stable
        if (!BMQ_X(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 64, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, 64, stream));
    }
    bool rb_keep(const RbArgs& B) {
        if (B.n_items == 0) return true;
        hipLaunchKernelGGL(k_rb_keep, grid(B.n_items, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_rank(const RbArgs& B) {
        if (B.n_items == 0) return true;
        hipLaunchKernelGGL(k_rb_rank, grid(B.n_items, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_shape(const RbArgs& B) {
        if (B.n_topics == 0) return true;
        hipLaunchKernelGGL(k_rb_shape, grid(B.n_topics, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_count(const RbArgs& B) {
        if (B.n_tenants == 0) return true;
        hipLaunchKernelGGL(k_rb_count, grid(B.n_tenants, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_intern(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_intern, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_owner(const RbArgs& B) {
        hipLaunchKernelGGL(k_rb_owner, grid(B.own_mask + 1u, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_place(const RbArgs& B) {
        hipLaunchKernelGGL(k_rb_place, grid(B.own_mask + 1u, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_token(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_token, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_edge(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_edge, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_edge_overflow(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_edge_overflow, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_post_flag(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_post_flag, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_post_emit(const RbArgs& B) {
        if (B.n_nodes == 0) return true;
        hipLaunchKernelGGL(k_rb_post_emit, grid(B.n_nodes, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_post_gp(const RbArgs& B) {
        if (B.n_posts == 0) return true;
        hipLaunchKernelGGL(k_rb_post_gp, grid(B.n_posts, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_post_write(const RbArgs& B) {
        if (B.n_posts == 0) return true;
        hipLaunchKernelGGL(k_rb_post_write, grid(B.n_posts, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_post_tenant(const RbArgs& B) {
        if (B.n_tenants == 0) return true;
        hipLaunchKernelGGL(k_rb_post_tenant, grid(B.n_tenants, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_run_start(const RbArgs& B) {
        if (B.n_posts == 0) return true;
        hipLaunchKernelGGL(k_rb_run_start, grid(B.n_posts, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_gp(const RbArgs& B) {
        if (B.n_runs == 0) return true;
        hipLaunchKernelGGL(k_rb_gp, grid(B.n_runs, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_gp_overflow(const RbArgs& B) {
        if (B.n_runs == 0) return true;
        hipLaunchKernelGGL(k_rb_gp_overflow, grid(B.n_runs, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_tenant(const RbArgs& B) {
        if (B.n_tenants == 0) return true;
        hipLaunchKernelGGL(k_rb_tenant, grid(B.n_tenants, RBK), dim3(RBK), 0, stream, B);
        return launched();
    }
    bool rb_head(const RbArgs& B, uint32_t d) {
        hipLaunchKernelGGL(k_rb_head, grid(B.n_topics, RBK), dim3(RBK), 0, stream, B, d);
        return launched();
    }
    bool rb_root(const RbArgs& B, const uint32_t* S1) {
        hipLaunchKernelGGL(k_rb_root, grid(B.n_tenants, RBK), dim3(RBK), 0, stream, B, S1);
        return launched();
    }
    bool rb_emit(const RbArgs& B, uint32_t d, const uint32_t* Sp, const uint32_t* Sc, const uint32_t* Sn) {
        hipLaunchKernelGGL(k_rb_emit, grid(B.n_topics, RBK), dim3(RBK), 0, stream, B, d, Sp, Sc, Sn);
        return launched();
    }
    bool rb_close(const RbArgs& B, uint32_t d, const uint32_t* Sc, const uint32_t* Sn) {
        hipLaunchKernelGGL(k_rb_close, grid(B.n_topics, RBK), dim3(RBK), 0, stream, B, d, Sc, Sn);
        return launched();
    }
    bool rb_advance(const RbArgs& B, const uint32_t* Sc) {
        hipLaunchKernelGGL(k_rb_advance, grid(B.n_tenants, RBK), dim3(RBK), 0, stream, B, Sc);
        return launched();
    }
    bool r_find_tenant(const RetainMut& m, const uint8_t* name, uint32_t len, uint32_t* out) {
        hipLaunchKernelGGL(k_r_find_tenant, dim3(1), dim3(64), 0, stream, m, name, len, out);
        return launched();
    }
    // lens[0 .. n] = key lengths of ids[0, n) and a closing 0, offs[0 .. n] = their exclusive 64-bit sums (offs[n] = all key bytes)
    bool r_key_offsets(const RetainMut& m, const RetainKeyStore& ks, const uint32_t* ids, uint32_t n, unsigned long long* lens, unsigned long long* offs) {
        hipLaunchKernelGGL(k_r_key_len, grid((unsigned long long)n + 1, 256), dim3(256), 0, stream, m, ks, ids, n, lens);
        if (!launched()) return false;
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, lens, offs, (int)n + 1, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, lens, offs, (int)n + 1, stream));
    }
    bool r_key_write(const RetainMut& m, const RetainKeyStore& ks, const uint32_t* ids, uint32_t n, const unsigned long long* offs, uint8_t* out) {
        hipLaunchKernelGGL(k_r_key_write, grid(n, 256), dim3(256), 0, stream, m, ks, ids, n, offs, out);
        return launched();
    }
    // ---- the plan of a batch of retain ops (bmq_rplan_kernels.h): find, group, classify, the 64-bit scan of the key lengths; then the keys ----
    bool rp_plan(const RetainMut& m, const RplanBatch& b, bool have_index, unsigned long long* offs) {
        hipLaunchKernelGGL(k_rp_find, grid(b.n, 64), dim3(64), 0, stream, m, b, have_index ? 1u : 0u);
        hipLaunchKernelGGL(k_rp_group, grid(b.n, RPK), dim3(RPK), 0, stream, b, b.table_mask);
        hipLaunchKernelGGL(k_rp_classify, grid((unsigned long long)b.n + 1, RPK), dim3(RPK), 0, stream, b);
        if (!launched()) return false;
        size_t bytes = 0;
        if (!BMQ_X(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, b.key_len, offs, (int)b.n + 1, stream))) return false;
        if (!ensure_tmp(bytes)) return false;
        return BMQ_X(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, b.key_len, offs, (int)b.n + 1, stream));
    }
    bool rp_key_write(const RplanBatch& b, const unsigned long long* offs, uint8_t* out) {
        hipLaunchKernelGGL(k_rp_key_write, grid(b.n, RPK), dim3(RPK), 0, stream, b, offs, out);
        return launched();
    }
    // ---- snapshot of the retained-topic index and the next generation's per-id arrays (bmq_retain_snap_kernels.h) ----
    bool rs_lens(const RetainMut& m, const RetainKeyStore& ks, const RsArgs& A) { // A.totals[0] += topic bytes, [1] += bulk-loaded ids
        if (A.S.n == 0) return true;
        hipLaunchKernelGGL(k_rs_lens, grid(A.S.n, RSK), dim3(RSK), 0, stream, m, ks, A);
        return launched();
    }
    bool rs_tenant_lens(const RetainMut& m, const RsArgs& A) {
        if (A.ov_nodes == 0) return true;
        hipLaunchKernelGGL(k_rs_tenant_lens, grid(A.ov_nodes, RSK), dim3(RSK), 0, stream, m, A);
        return launched();
    }
    bool rs_totals(const RsArgs& A) {
        hipLaunchKernelGGL(k_rs_totals, dim3(1), dim3(64), 0, stream, A);
        return launched();
    }
    bool rs_tenants(const RetainMut& m, const RsArgs& A) {
        if (A.ov_nodes == 0) return true;
        hipLaunchKernelGGL(k_rs_tenants, grid(A.ov_nodes, RSK), dim3(RSK), 0, stream, m, A);
        return launched();
    }
    bool rs_items(const RetainMut& m, const RsArgs& A) { // the overlay items [A.n_bulk, A.S.n)
        if (A.S.n <= A.n_bulk) return true;
        hipLaunchKernelGGL(k_rs_items, grid(A.S.n - A.n_bulk, 64), dim3(64), 0, stream, m, A);
        return launched();
    }
    template <class SO> bool rs_gather(const RsGather<SO>& G) {
        if (G.n == 0 || G.bytes == 0) return true;
        const unsigned long long waves = (G.bytes + RS_WAVE_BYTES - 1) / RS_WAVE_BYTES;
        hipLaunchKernelGGL(k_rs_gather<SO>, grid(waves, RSK / 64), dim3(RSK), 0, stream, G);
        return launched();
    }
    bool rs_used(const uint32_t* item_tenant, uint32_t n, uint32_t* used) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_rs_used, grid(n, RSK), dim3(RSK), 0, stream, item_tenant, used, n);
        return launched();
    }
    bool rs_remap(const uint32_t* item_tenant, const uint32_t* rank_of, uint32_t* out, uint32_t n) {
        if (n == 0) return true;
        hipLaunchKernelGGL(k_rs_remap, grid(n, RSK), dim3(RSK), 0, stream, item_tenant, rank_of, out, n);
        return launched();
    }
    bool rs_perm_lens(const RsNext& N) {
        if (N.n_topics == 0) return true;
        hipLaunchKernelGGL(k_rs_perm_lens, grid(N.n_topics, RSK), dim3(RSK), 0, stream, N);
        return launched();
    }
    bool rs_next(const RsNext& N) {
        if (N.n_topics == 0) return true;
        hipLaunchKernelGGL(k_rs_next, grid(N.n_topics, RSK), dim3(RSK), 0, stream, N);
        return launched();
    }
#undef BMQ_X
};

} // namespace bmq
