// bmq_gate_engine.inc -- bmq_routes_gate_batch / bmq_routes_gate_dev: the submit-time fan-out gate of DeliverExecutorGroup.submit over a
// whole match CSR (bmq_gate_core.h says what it replaces in the reference).  Included at the end of bmq_engine.hip; bmq_delivery_wait_gated
// (bmq_delivery_engine.inc) runs caps_run, then gate_run, in front of the plan.
namespace {
int gate_check_table(bmq_engine* e, const int32_t* max_pf, const int32_t* max_gf, const int64_t* max_pb, const uint8_t* bw, uint32_t n_gate) {
    for (uint32_t t = 0; t < n_gate; t++) {
        if (max_pf[t] < 0 || max_gf[t] < 0 || max_pb[t] < 0) return set_err(e, BMQ_E_INVAL, "negative fan-out limit");
        if (bw[t] > 3) return set_err(e, BMQ_E_INVAL, "bandwidth: bits above 1 are not defined");
    }
    return BMQ_OK;
}
// one run over exec memory; out_info is filled whatever the outcome of the capacity
int gate_run(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, const uint32_t* pack_bytes, const uint32_t* row_gate, const GateTable& T,
             uint32_t inline_threshold, uint32_t* out_row_ptr, uint32_t* out_ids, uint64_t out_cap, uint32_t* out_flags, uint32_t* out_class_counts, uint64_t* out_meter_bytes,
             uint32_t* out_meter_records, GateResult& r, bmq_gate_info* out_info) {
    const int rc = with_control(e, e->hgt, e->dgt, [&](auto& gt, auto& ix) {
        out_info->generation = ix.generation;
        return gt.run(ix, row_ptr, ids, n_rows, total, pack_bytes, row_gate, T, inline_threshold, out_row_ptr, out_ids, out_cap, out_flags, out_class_counts, out_meter_bytes,
                      out_meter_records, r)
                   ? (int)BMQ_OK
                   : index_error(e, gt.error, gt.invalid);
    });
    if (rc) return rc;
    out_info->n_in = r.n_in;
    out_info->n_kept = r.n_kept;
    out_info->n_rows_single = r.n_rows_single;
    out_info->n_rows_gated = r.n_rows_gated;
    out_info->n_rows_flagged = r.n_rows_flagged;
    out_info->n_rows_ranked = r.n_rows_ranked;
    out_info->n_rows_fallback = r.n_rows_fallback;
    out_info->ms_classify = r.ms_classify;
    out_info->ms_rank = r.ms_rank;
    out_info->ms_write = r.ms_write;
    return BMQ_OK;
}
int gate_nospace(bmq_engine* e) { return set_err(e, BMQ_E_NOSPACE, "out_route_ids too small: see info.n_kept"); }
} // namespace

extern "C" int bmq_routes_gate_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_rows, uint64_t total, const uint32_t* d_pack_bytes,
                                   const uint32_t* d_row_gate, const int32_t* d_max_pf, const int32_t* d_max_gf, const int64_t* d_max_pb, const uint8_t* d_bandwidth,
                                   uint32_t n_gate, uint32_t inline_threshold, uint32_t* d_out_row_ptr, uint32_t* d_out_route_ids, uint64_t out_cap, uint32_t* d_out_row_flags,
                                   uint32_t* d_out_class_counts, uint64_t* d_out_meter_bytes, uint32_t* d_out_meter_records, bmq_gate_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (!d_row_ptr || !d_out_row_ptr || (total && (!d_route_ids || !d_out_route_ids)) || (n_rows && (!d_pack_bytes || !d_out_row_flags)) ||
        (n_gate && (!d_max_pf || !d_max_gf || !d_max_pb || !d_bandwidth || !d_out_meter_bytes || !d_out_meter_records)))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (total >= 0x7FFFFFF0ull || n_rows >= 0x3FFFFFF0u) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    HIPCHK(e, hipSetDevice(e->device));
    *out_info = bmq_gate_info{};
    std::vector<int32_t> h_pf(n_gate), h_gf(n_gate); // the table is small (an entry per tenant): it is checked on the host
    std::vector<int64_t> h_pb(n_gate);
    std::vector<uint8_t> h_bw(n_gate);
    if (n_gate) {
        HIPCHK(e, hipMemcpyAsync(h_pf.data(), d_max_pf, 4 * (size_t)n_gate, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(h_gf.data(), d_max_gf, 4 * (size_t)n_gate, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(h_pb.data(), d_max_pb, 8 * (size_t)n_gate, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(h_bw.data(), d_bandwidth, (size_t)n_gate, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    if (int rc_t = gate_check_table(e, h_pf.data(), h_gf.data(), h_pb.data(), h_bw.data(), n_gate)) return rc_t;
    GateTable T;
    T.max_pf = d_max_pf, T.max_gf = d_max_gf, T.max_pb = d_max_pb, T.bw = d_bandwidth, T.n_gate = n_gate;
    GateResult r;
    const int rc = gate_run(e, d_row_ptr, d_route_ids, n_rows, (uint32_t)total, d_pack_bytes, d_row_gate, T, inline_threshold, d_out_row_ptr, d_out_route_ids, out_cap,
                            d_out_row_flags, d_out_class_counts, d_out_meter_bytes, d_out_meter_records, r, out_info);
    if (rc) return rc;
    return r.overflow ? gate_nospace(e) : BMQ_OK;
}

extern "C" int bmq_routes_gate_batch(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_rows, const uint32_t* pack_bytes, const uint32_t* row_gate,
                                     const int32_t* max_pf, const int32_t* max_gf, const int64_t* max_pb, const uint8_t* bandwidth, uint32_t n_gate, uint32_t inline_threshold,
                                     uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_cap, uint32_t* out_row_flags, uint32_t* out_class_counts,
                                     uint64_t* out_meter_bytes, uint32_t* out_meter_records, bmq_gate_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (!row_ptr || !out_row_ptr || (n_rows && (!pack_bytes || !out_row_flags)) ||
        (n_gate && (!max_pf || !max_gf || !max_pb || !bandwidth || !out_meter_bytes || !out_meter_records)))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_c = check_csr(e, row_ptr, n_rows, 0x3FFFFFF0u)) return rc_c;
    const uint32_t total = row_ptr[n_rows];
    if (total && (!route_ids || !out_route_ids)) return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_t = gate_check_table(e, max_pf, max_gf, max_pb, bandwidth, n_gate)) return rc_t;
    for (uint32_t i = 0; i < n_rows; i++)
        if ((row_gate ? row_gate[i] : 0u) >= n_gate) return set_err(e, BMQ_E_INVAL, "row_gate: an index outside the gate table");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "bmq_rebuild has not been called");
    *out_info = bmq_gate_info{};
    GateResult r;
    GateTable T;
    T.n_gate = n_gate;
    if (e->device < 0) { // host-only engine: the same per-item functions on host threads, straight on the caller's buffers
        T.max_pf = max_pf, T.max_gf = max_gf, T.max_pb = max_pb, T.bw = bandwidth;
        const int rc = gate_run(e, row_ptr, route_ids, n_rows, total, pack_bytes, row_gate, T, inline_threshold, out_row_ptr, out_route_ids, out_cap, out_row_flags,
                                out_class_counts, out_meter_bytes, out_meter_records, r, out_info);
        if (rc) return rc;
        return r.overflow ? gate_nospace(e) : BMQ_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    // staging: [max_pb | meter bytes | row_ptr | ids | pack_bytes | row_gate | max_pf | max_gf | bandwidth | out_row_ptr | out_ids | flags | kept counts | meter records]
    Stage st;
    const size_t ids_cap = (size_t)std::min<uint64_t>(out_cap, total);
    const size_t row_ptr4 = 4 * ((size_t)n_rows + 1), rows4 = 4 * (size_t)n_rows, rg4 = row_gate ? rows4 : 0, tab4 = 4 * (size_t)n_gate, tab8 = 8 * (size_t)n_gate,
                 cc12 = out_class_counts ? 12 * (size_t)n_rows : 0;
    const size_t o_pb = st.take(tab8), o_mb = st.take(tab8), o_row = st.take(row_ptr4), o_ids = st.take(4 * (size_t)total), o_pk = st.take(rows4), o_rg = st.take(rg4), o_pf = st.take(tab4),
                 o_gf = st.take(tab4), o_bw = st.take(n_gate), o_orow = st.take(row_ptr4), o_oids = st.take(4 * ids_cap), o_fl = st.take(rows4), o_cc = st.take(cc12), o_mr = st.take(tab4);
    if (int rc_b = stage_ensure(e, e->gate_buf, st.end + 16)) return rc_b;
    uint8_t* d = e->gate_buf.as<uint8_t>();
    if (int rc_u = stage_up(e, {{d + o_row, row_ptr, row_ptr4}, {d + o_ids, route_ids, 4 * (size_t)total}, {d + o_pk, pack_bytes, rows4}, {d + o_rg, row_gate, rg4}, {d + o_pf, max_pf, tab4},
                                {d + o_gf, max_gf, tab4}, {d + o_pb, max_pb, tab8}, {d + o_bw, bandwidth, n_gate}}))
        return rc_u;
    T.max_pf = (const int32_t*)(d + o_pf), T.max_gf = (const int32_t*)(d + o_gf), T.max_pb = (const int64_t*)(d + o_pb), T.bw = d + o_bw;
    const int rc = gate_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_rows, total, (const uint32_t*)(d + o_pk),
                            row_gate ? (const uint32_t*)(d + o_rg) : nullptr, T, inline_threshold, (uint32_t*)(d + o_orow), (uint32_t*)(d + o_oids), ids_cap,
                            (uint32_t*)(d + o_fl), out_class_counts ? (uint32_t*)(d + o_cc) : nullptr, (uint64_t*)(d + o_mb), (uint32_t*)(d + o_mr), r, out_info);
    if (rc) return rc;
    const size_t fits = r.overflow ? 0 : 1; // (rows that do not fit were not written)
    if (int rc_d = stage_down(e, {{out_row_flags, d + o_fl, rows4}, {out_class_counts, d + o_cc, cc12}, {out_meter_bytes, d + o_mb, tab8}, {out_meter_records, d + o_mr, tab4},
                                  {out_row_ptr, d + o_orow, fits * row_ptr4}, {out_route_ids, d + o_oids, fits * 4 * (size_t)r.n_kept}}))
        return rc_d;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return r.overflow ? gate_nospace(e) : BMQ_OK;
}
