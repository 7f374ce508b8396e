// bmq_range_engine.inc -- bmq_range_lookup: TenantRangeLookupCache.lookup for a batch of topics (SURVEY.md 8f-2), one lane per
// topic running range_lookup_one of bmq_range_core.h.  Included at the end of bmq_engine.hip.
namespace bmq {
__global__ __launch_bounds__(64) void k_range_lookup(const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics, const uint32_t* topic_off,
                                                     uint32_t n_topics, const uint8_t* kind, const uint8_t* first, const uint32_t* first_off,
                                                     const uint8_t* last, const uint32_t* last_off, uint32_t n_cand, uint8_t* keep) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_topics) return;
    range_lookup_one(tenant, tenant_len, topics, topic_off[i], topic_off[i + 1], kind, first, first_off, last, last_off, n_cand,
                     keep + (size_t)i * n_cand);
}
} // namespace bmq

extern "C" int bmq_range_lookup(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics, const uint32_t* topic_off,
                                uint32_t n_topics, const uint8_t* cand_kind, const uint8_t* first, const uint32_t* first_off, const uint8_t* last,
                                const uint32_t* last_off, uint32_t n_cand, uint8_t* out_keep) {
    if (!e) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (n_topics == 0 || n_cand == 0) return BMQ_OK;
    if (!topics || !topic_off || !cand_kind || !first_off || !last_off || !out_keep || (tenant_len && !tenant))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    HIPCHK(e, hipSetDevice(e->device));
    const size_t tb = topic_off[n_topics], fb = first_off[n_cand], lb = last_off[n_cand];
    // staging: [tenant | topics | topic_off | kind | first | first_off | last | last_off | keep]
    Stage st;
    const size_t o_ten = st.take(tenant_len + 16), o_top = st.take(tb + 16), o_toff = st.take(4 * ((size_t)n_topics + 1)), o_kind = st.take(n_cand), o_first = st.take(fb + 16),
                 o_foff = st.take(4 * ((size_t)n_cand + 1)), o_last = st.take(lb + 16), o_loff = st.take(4 * ((size_t)n_cand + 1)), o_keep = st.take((size_t)n_topics * n_cand);
    if (int rc_b = stage_ensure(e, e->range_buf, st.end)) return rc_b;
    uint8_t* d = e->range_buf.as<uint8_t>();
    hipStream_t s = e->stream;
    if (int rc_u = stage_up(e, {{d + o_ten, tenant, tenant_len}, {d + o_top, topics, tb}, {d + o_toff, topic_off, 4 * ((size_t)n_topics + 1)}, {d + o_kind, cand_kind, n_cand},
                                {d + o_first, first, fb}, {d + o_foff, first_off, 4 * ((size_t)n_cand + 1)}, {d + o_last, last, lb}, {d + o_loff, last_off, 4 * ((size_t)n_cand + 1)}}))
        return rc_u;
    hipLaunchKernelGGL(bmq::k_range_lookup, dim3((n_topics + 63) / 64), dim3(64), 0, s, d + o_ten, tenant_len, d + o_top, (const uint32_t*)(d + o_toff),
                       n_topics, d + o_kind, d + o_first, (const uint32_t*)(d + o_foff), d + o_last, (const uint32_t*)(d + o_loff), n_cand, d + o_keep);
    HIPCHK(e, hipGetLastError());
    if (int rc_d = stage_down(e, {{out_keep, d + o_keep, (size_t)n_topics * n_cand}})) return rc_d;
    HIPCHK(e, hipStreamSynchronize(s));
    return BMQ_OK;
}
