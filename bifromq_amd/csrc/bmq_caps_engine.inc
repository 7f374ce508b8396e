// bmq_caps_engine.inc -- bmq_routes_cap_batch / bmq_routes_cap_dev: the fan-out caps of MatchedRoutes over a whole match CSR
// (bmq_caps_core.h says what they replace in the reference).  Included at the end of bmq_engine.hip; bmq_delivery_wait_capped
// (bmq_delivery_engine.inc) runs caps_run in front of the plan.
namespace {
int caps_check_table(bmq_engine* e, const int32_t* max_pf, const int32_t* max_gf, uint32_t n_caps) {
    for (uint32_t t = 0; t < n_caps; t++)
        if (max_pf[t] < 0 || max_gf[t] < 0) return set_err(e, BMQ_E_INVAL, "negative fan-out cap");
    return BMQ_OK;
}
// one run over exec memory (h_pf / h_gf: the table on the host, checked); out_info is filled whatever the outcome of the capacity
int caps_run(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, const uint32_t* row_caps, const int32_t* max_pf,
             const int32_t* max_gf, uint32_t n_caps, const int32_t* h_pf, const int32_t* h_gf, uint32_t* out_row_ptr, uint32_t* out_ids, uint64_t out_cap,
             uint32_t* out_class_counts, int32_t* out_events, uint32_t events_cap, CapsResult& r, bmq_caps_info* out_info) {
    const int rc = with_control(e, e->hcp, e->dcp, [&](auto& cp, auto& ix) {
        out_info->generation = ix.generation;
        return cp.run(ix, row_ptr, ids, n_rows, total, row_caps, max_pf, max_gf, n_caps, h_pf, h_gf, out_row_ptr, out_ids, out_cap, out_class_counts, out_events, events_cap, r)
                   ? (int)BMQ_OK
                   : index_error(e, cp.error, cp.invalid);
    });
    if (rc) return rc;
    out_info->n_in = r.n_in;
    out_info->n_kept = r.n_kept;
    out_info->n_rows_classified = r.n_rows_classified;
    out_info->n_rows_ranked = r.n_rows_ranked;
    out_info->n_rows_fallback = r.n_rows_fallback;
    out_info->n_events = r.n_events;
    out_info->ms_classify = r.ms_classify;
    out_info->ms_rank = r.ms_rank;
    out_info->ms_write = r.ms_write;
    return BMQ_OK;
}
int caps_nospace(bmq_engine* e) { return set_err(e, BMQ_E_NOSPACE, "out_route_ids too small: see info.n_kept"); }
} // namespace

extern "C" int bmq_routes_cap_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_rows, uint64_t total,
                                  const uint32_t* d_row_caps, const int32_t* d_max_pf, const int32_t* d_max_gf, uint32_t n_caps, uint32_t* d_out_row_ptr,
                                  uint32_t* d_out_route_ids, uint64_t out_cap, uint32_t* d_out_class_counts, int32_t* d_out_events, uint32_t events_cap,
                                  uint32_t* out_n_events, bmq_caps_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (out_n_events) *out_n_events = 0;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (!d_row_ptr || !d_out_row_ptr || (total && (!d_route_ids || !d_out_route_ids)) || (n_caps && (!d_max_pf || !d_max_gf)))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (total >= 0x7FFFFFF0ull || n_rows >= 0x3FFFFFF0u) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    HIPCHK(e, hipSetDevice(e->device));
    *out_info = bmq_caps_info{};
    std::vector<int32_t> h_pf(n_caps), h_gf(n_caps); // the table is small (an entry per tenant): its caps are checked, and the fallback reads them, on the host
    if (n_caps) {
        HIPCHK(e, hipMemcpyAsync(h_pf.data(), d_max_pf, 4 * (size_t)n_caps, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(h_gf.data(), d_max_gf, 4 * (size_t)n_caps, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    if (int rc_t = caps_check_table(e, h_pf.data(), h_gf.data(), n_caps)) return rc_t;
    CapsResult r;
    const int rc = caps_run(e, d_row_ptr, d_route_ids, n_rows, (uint32_t)total, d_row_caps, d_max_pf, d_max_gf, n_caps, h_pf.data(), h_gf.data(), d_out_row_ptr,
                            d_out_route_ids, out_cap, d_out_class_counts, d_out_events, events_cap, r, out_info);
    if (rc) return rc;
    if (out_n_events) *out_n_events = r.n_events;
    return r.overflow ? caps_nospace(e) : BMQ_OK;
}

extern "C" int bmq_routes_cap_batch(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_rows, const uint32_t* row_caps,
                                    const int32_t* max_pf, const int32_t* max_gf, uint32_t n_caps, uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_cap,
                                    uint32_t* out_class_counts, int32_t* out_events, uint32_t events_cap, uint32_t* out_n_events, bmq_caps_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (out_n_events) *out_n_events = 0;
    if (!row_ptr || !out_row_ptr || (n_caps && (!max_pf || !max_gf))) return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_c = check_csr(e, row_ptr, n_rows, 0x3FFFFFF0u)) return rc_c;
    const uint32_t total = row_ptr[n_rows];
    if (total && (!route_ids || !out_route_ids)) return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_t = caps_check_table(e, max_pf, max_gf, n_caps)) return rc_t;
    for (uint32_t i = 0; i < n_rows; i++)
        if ((row_caps ? row_caps[i] : 0u) >= n_caps) return set_err(e, BMQ_E_INVAL, "row_caps: an index outside the caps table");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "bmq_rebuild has not been called");
    *out_info = bmq_caps_info{};
    CapsResult r;
    if (e->device < 0) { // host-only engine: the same per-item functions on host threads, straight on the caller's buffers
        const int rc = caps_run(e, row_ptr, route_ids, n_rows, total, row_caps, max_pf, max_gf, n_caps, max_pf, max_gf, out_row_ptr, out_route_ids, out_cap, out_class_counts,
                                out_events, out_events ? events_cap : 0u, r, out_info);
        if (rc) return rc;
        if (out_n_events) *out_n_events = r.n_events;
        return r.overflow ? caps_nospace(e) : BMQ_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    // staging: [row_ptr | ids | row_caps | max_pf | max_gf | out_row_ptr | out_ids | class counts | events]
    Stage st;
    const uint32_t ev_cap = out_events ? events_cap : 0u;
    const size_t ids_cap = (size_t)std::min<uint64_t>(out_cap, total);
    const size_t row_ptr4 = 4 * ((size_t)n_rows + 1), rc4 = row_caps ? 4 * (size_t)n_rows : 0, tab4 = 4 * (size_t)n_caps, cc8 = out_class_counts ? 8 * (size_t)n_rows : 0;
    const size_t o_row = st.take(row_ptr4), o_ids = st.take(4 * (size_t)total), o_rc = st.take(rc4), o_pf = st.take(tab4), o_gf = st.take(tab4), o_orow = st.take(row_ptr4),
                 o_oids = st.take(4 * ids_cap), o_cc = st.take(cc8), o_ev = st.take(16 * (size_t)ev_cap);
    if (int rc_b = stage_ensure(e, e->caps_buf, st.end + 16)) return rc_b;
    uint8_t* d = e->caps_buf.as<uint8_t>();
    if (int rc_u = stage_up(e, {{d + o_row, row_ptr, row_ptr4}, {d + o_ids, route_ids, 4 * (size_t)total}, {d + o_rc, row_caps, rc4}, {d + o_pf, max_pf, tab4}, {d + o_gf, max_gf, tab4}}))
        return rc_u;
    const int rc = caps_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_rows, total, row_caps ? (const uint32_t*)(d + o_rc) : nullptr,
                            (const int32_t*)(d + o_pf), (const int32_t*)(d + o_gf), n_caps, max_pf, max_gf, (uint32_t*)(d + o_orow), (uint32_t*)(d + o_oids), ids_cap,
                            out_class_counts ? (uint32_t*)(d + o_cc) : nullptr, ev_cap ? (int32_t*)(d + o_ev) : nullptr, ev_cap, r, out_info);
    if (rc) return rc;
    if (out_n_events) *out_n_events = r.n_events;
    const size_t fits = r.overflow ? 0 : 1; // (rows that do not fit were not written)
    if (int rc_d = stage_down(e, {{out_events, d + o_ev, 16 * std::min<size_t>(r.n_events, ev_cap)}, {out_row_ptr, d + o_orow, fits * row_ptr4},
                                  {out_route_ids, d + o_oids, fits * 4 * (size_t)r.n_kept}, {out_class_counts, d + o_cc, fits * cc8}}))
        return rc_d;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return r.overflow ? caps_nospace(e) : BMQ_OK;
}
