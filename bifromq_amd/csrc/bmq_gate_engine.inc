// bmq_gate_engine.inc -- bmq_routes_gate_batch / bmq_routes_gate_dev / bmq_delivery_wait_gated: the submit-time fan-out gate of
// DeliverExecutorGroup.submit over a whole match CSR (bmq_gate_core.h says what it replaces in the reference).  Included at the end of
// bmq_engine.hip, behind bmq_caps_engine.inc (the gated wait runs caps_run, then the gate, then delivery_run).
namespace {
// the engine's Gate over whichever executor it has, created by the first call.  A buffer that grows is freed first, and a free waits for
// every stream of the device: the persistent matcher leaves before.
template <class F> int with_gate(bmq_engine* e, F&& f) {
    if (e->device < 0) {
        if (!e->hgt) e->hgt = std::make_unique<Gate<HostExec>>(e->hx);
        return f(*e->hgt, *e->hix);
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->dgt) {
        e->dgt = std::make_unique<Gate<DevExec>>(e->dx);
        e->dgt->before_free = [e] { poller_stop_locked(e); };
    }
    e->dx.marks_on = e->kernel_events;
    return f(*e->dgt, *e->dix);
}
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
    const int rc = with_gate(e, [&](auto& gt, auto& ix) {
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
// offsets of 16-byte aligned pieces of a staging buffer
struct GateTake {
    size_t o = 0;
    size_t operator()(size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) & ~(size_t)15;
        return at;
    }
};
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
    if (row_ptr[0] != 0) return set_err(e, BMQ_E_INVAL, "row_ptr[0] != 0");
    for (uint32_t i = 0; i < n_rows; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return set_err(e, BMQ_E_INVAL, "row_ptr not ascending");
    const uint32_t total = row_ptr[n_rows];
    if (total >= 0x7FFFFFF0u || n_rows >= 0x3FFFFFF0u) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
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
    GateTake take;
    const size_t ids_cap = (size_t)std::min<uint64_t>(out_cap, total);
    const size_t o_pb = take(8 * (size_t)n_gate), o_mb = take(8 * (size_t)n_gate), o_row = take(4 * ((size_t)n_rows + 1)), o_ids = take(4 * (size_t)total),
                 o_pk = take(4 * (size_t)n_rows), o_rg = take(row_gate ? 4 * (size_t)n_rows : 0), o_pf = take(4 * (size_t)n_gate), o_gf = take(4 * (size_t)n_gate),
                 o_bw = take(n_gate), o_orow = take(4 * ((size_t)n_rows + 1)), o_oids = take(4 * ids_cap), o_fl = take(4 * (size_t)n_rows),
                 o_cc = take(out_class_counts ? 12 * (size_t)n_rows : 0), o_mr = take(4 * (size_t)n_gate);
    if (take.o + 16 > e->gate_buf.cap) poller_stop_locked(e);
    HIPCHK(e, e->gate_buf.ensure(take.o + 16));
    uint8_t* d = e->gate_buf.as<uint8_t>();
    hipStream_t s = e->stream;
    HIPCHK(e, hipMemcpyAsync(d + o_row, row_ptr, 4 * ((size_t)n_rows + 1), hipMemcpyHostToDevice, s));
    if (total) HIPCHK(e, hipMemcpyAsync(d + o_ids, route_ids, 4 * (size_t)total, hipMemcpyHostToDevice, s));
    if (n_rows) HIPCHK(e, hipMemcpyAsync(d + o_pk, pack_bytes, 4 * (size_t)n_rows, hipMemcpyHostToDevice, s));
    if (row_gate && n_rows) HIPCHK(e, hipMemcpyAsync(d + o_rg, row_gate, 4 * (size_t)n_rows, hipMemcpyHostToDevice, s));
    if (n_gate) {
        HIPCHK(e, hipMemcpyAsync(d + o_pf, max_pf, 4 * (size_t)n_gate, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(d + o_gf, max_gf, 4 * (size_t)n_gate, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(d + o_pb, max_pb, 8 * (size_t)n_gate, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(d + o_bw, bandwidth, (size_t)n_gate, hipMemcpyHostToDevice, s));
    }
    T.max_pf = (const int32_t*)(d + o_pf), T.max_gf = (const int32_t*)(d + o_gf), T.max_pb = (const int64_t*)(d + o_pb), T.bw = d + o_bw;
    const int rc = gate_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_rows, total, (const uint32_t*)(d + o_pk),
                            row_gate ? (const uint32_t*)(d + o_rg) : nullptr, T, inline_threshold, (uint32_t*)(d + o_orow), (uint32_t*)(d + o_oids), ids_cap,
                            (uint32_t*)(d + o_fl), out_class_counts ? (uint32_t*)(d + o_cc) : nullptr, (uint64_t*)(d + o_mb), (uint32_t*)(d + o_mr), r, out_info);
    if (rc) return rc;
    if (n_rows) HIPCHK(e, hipMemcpyAsync(out_row_flags, d + o_fl, 4 * (size_t)n_rows, hipMemcpyDeviceToHost, s));
    if (out_class_counts && n_rows) HIPCHK(e, hipMemcpyAsync(out_class_counts, d + o_cc, 12 * (size_t)n_rows, hipMemcpyDeviceToHost, s));
    if (n_gate) {
        HIPCHK(e, hipMemcpyAsync(out_meter_bytes, d + o_mb, 8 * (size_t)n_gate, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipMemcpyAsync(out_meter_records, d + o_mr, 4 * (size_t)n_gate, hipMemcpyDeviceToHost, s));
    }
    if (!r.overflow) {
        HIPCHK(e, hipMemcpyAsync(out_row_ptr, d + o_orow, 4 * ((size_t)n_rows + 1), hipMemcpyDeviceToHost, s));
        if (r.n_kept) HIPCHK(e, hipMemcpyAsync(out_route_ids, d + o_oids, 4 * (size_t)r.n_kept, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    return r.overflow ? gate_nospace(e) : BMQ_OK;
}

extern "C" int bmq_delivery_wait_gated(bmq_engine* e, int ticket, const int32_t* max_pf, const int32_t* max_gf, const int64_t* max_pb, const uint8_t* bandwidth, uint32_t n_gate,
                                       const uint32_t* pack_bytes, uint32_t inline_threshold, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce,
                                       uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                                       uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total, int32_t* out_events,
                                       uint32_t events_cap, uint32_t* out_n_events, bmq_caps_info* out_caps_info, uint32_t* out_row_flags, uint64_t* out_meter_bytes,
                                       uint32_t* out_meter_records, bmq_gate_info* out_gate_info) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_info || !out_caps_info || !out_gate_info || !out_total || !sender_off || !pack_bytes || !out_row_flags ||
        (n_gate && (!max_pf || !max_gf || !max_pb || !bandwidth || !out_meter_bytes || !out_meter_records)) ||
        delivery_null_outputs(out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off))
        return BMQ_E_INVAL;
    if (out_n_events) *out_n_events = 0;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    { // refused before the wait: the ticket stays as it was
        std::lock_guard<std::mutex> g0(e->mu);
        if (int rc_t = gate_check_table(e, max_pf, max_gf, max_pb, bandwidth, n_gate)) return rc_t;
        if (S.submitted && !S.devptr && S.format == BMQ_FMT_DELIVERY && S.last.n_tenants != n_gate)
            return set_err(e, BMQ_E_INVAL, "n_gate is not the tenant count of the ticket's batch");
    }
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_DELIVERY, false, g, &total);
    if (!g.owns_lock()) return rc;
    *out_total = total;
    *out_info = bmq_delivery_info{};
    *out_caps_info = bmq_caps_info{};
    *out_gate_info = bmq_gate_info{};
    DeliveryResult r;
    CapsResult cr;
    GateResult gr;
    if (rc == BMQ_OK && total >= 0x7FFFFFF0ull) rc = set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (rc == BMQ_OK) rc = check_senders(e, sender_off, sender_hash, S.n_rows);
    if (rc == BMQ_OK) {
        // the caps over the CSR the batch left in the slot, the gate over the capped CSR, the plan of the gated CSR, all on the engine stream.
        // The capped CSR and the caps' events lie in caps_buf, the gate's table, the gated CSR, the flags and the meters in gate_buf, the
        // senders in dl_buf, the plan's outputs in the slot.
        const uint32_t n_topics = S.n_rows, n_senders = sender_off[n_topics], ev_cap = out_events ? events_cap : 0u;
        GateTake ct, gt;
        const size_t o_pf = ct(4 * (size_t)n_gate), o_gf = ct(4 * (size_t)n_gate), o_orow = ct(4 * ((size_t)n_topics + 1)), o_oids = ct(4 * (size_t)total),
                     o_ev = ct(16 * (size_t)ev_cap);
        const size_t g_pb = gt(8 * (size_t)n_gate), g_mb = gt(8 * (size_t)n_gate), g_bw = gt(n_gate), g_pk = gt(4 * (size_t)n_topics), g_orow = gt(4 * ((size_t)n_topics + 1)),
                     g_oids = gt(4 * (size_t)total), g_fl = gt(4 * (size_t)n_topics), g_mr = gt(4 * (size_t)n_gate);
        const size_t so_bytes = (4 * ((size_t)n_topics + 1) + 15) & ~(size_t)15;
        const DeliveryOut out(0, row_cap, share_cap, group_cap);
        if (so_bytes + 4 * (size_t)n_senders + 16 > e->dl_buf.cap || ct.o + 16 > e->caps_buf.cap || gt.o + 16 > e->gate_buf.cap) poller_stop_locked(e);
        if (e->dl_buf.ensure(so_bytes + 4 * (size_t)n_senders + 16) != hipSuccess || e->caps_buf.ensure(ct.o + 16) != hipSuccess || e->gate_buf.ensure(gt.o + 16) != hipSuccess ||
            S.g_pairs.ensure(out.end + 64) != hipSuccess)
            rc = set_err(e, BMQ_E_NOMEM, "out of device memory (gated delivery plan)");
        uint8_t* in = e->dl_buf.as<uint8_t>();
        uint8_t* c = e->caps_buf.as<uint8_t>();
        uint8_t* q = e->gate_buf.as<uint8_t>();
        uint8_t* d = S.g_pairs.as<uint8_t>();
        if (rc == BMQ_OK) {
            hipError_t he = hipMemcpyAsync(in, sender_off, 4 * ((size_t)n_topics + 1), hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_senders) he = hipMemcpyAsync(in + so_bytes, sender_hash, 4 * (size_t)n_senders, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(c + o_pf, max_pf, 4 * (size_t)n_gate, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(c + o_gf, max_gf, 4 * (size_t)n_gate, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(q + g_pb, max_pb, 8 * (size_t)n_gate, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(q + g_bw, bandwidth, (size_t)n_gate, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_topics) he = hipMemcpyAsync(q + g_pk, pack_bytes, 4 * (size_t)n_topics, hipMemcpyHostToDevice, e->stream);
            if (he != hipSuccess) rc = set_err(e, BMQ_E_HIP, std::string("sender upload: ") + hipGetErrorString(he));
        }
        if (rc == BMQ_OK)
            rc = caps_run(e, S.s_row_ptr.as<uint32_t>(), S.s_ids.as<uint32_t>(), n_topics, (uint32_t)total, S.s_topic_tenant.as<uint32_t>(), (const int32_t*)(c + o_pf),
                          (const int32_t*)(c + o_gf), n_gate, max_pf, max_gf, (uint32_t*)(c + o_orow), (uint32_t*)(c + o_oids), total, nullptr,
                          ev_cap ? (int32_t*)(c + o_ev) : nullptr, ev_cap, cr, out_caps_info);
        if (rc == BMQ_OK) {
            GateTable T;
            T.max_pf = (const int32_t*)(c + o_pf), T.max_gf = (const int32_t*)(c + o_gf), T.max_pb = (const int64_t*)(q + g_pb), T.bw = q + g_bw, T.n_gate = n_gate;
            rc = gate_run(e, (const uint32_t*)(c + o_orow), (const uint32_t*)(c + o_oids), n_topics, (uint32_t)cr.n_kept, (const uint32_t*)(q + g_pk),
                          S.s_topic_tenant.as<uint32_t>(), T, inline_threshold, (uint32_t*)(q + g_orow), (uint32_t*)(q + g_oids), total, (uint32_t*)(q + g_fl), nullptr,
                          (uint64_t*)(q + g_mb), (uint32_t*)(q + g_mr), gr, out_gate_info);
        }
        if (rc == BMQ_OK) {
            if (out_n_events) *out_n_events = cr.n_events;
            const size_t n_ev = std::min<size_t>(cr.n_events, ev_cap);
            hipError_t he = n_ev ? hipMemcpyAsync(out_events, c + o_ev, 16 * n_ev, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
            if (he == hipSuccess && n_topics) he = hipMemcpyAsync(out_row_flags, q + g_fl, 4 * (size_t)n_topics, hipMemcpyDeviceToHost, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(out_meter_bytes, q + g_mb, 8 * (size_t)n_gate, hipMemcpyDeviceToHost, e->stream);
            if (he == hipSuccess && n_gate) he = hipMemcpyAsync(out_meter_records, q + g_mr, 4 * (size_t)n_gate, hipMemcpyDeviceToHost, e->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
            if (he != hipSuccess) rc = set_err(e, BMQ_E_HIP, std::string("event download: ") + hipGetErrorString(he));
        }
        if (rc == BMQ_OK)
            rc = delivery_run(e, (const uint32_t*)(q + g_orow), (const uint32_t*)(q + g_oids), n_topics, (uint32_t)gr.n_kept, (const uint32_t*)in,
                              (const uint32_t*)(in + so_bytes), n_senders, nonce, (uint32_t*)(d + out.topic), (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap,
                              (uint32_t*)(d + out.sh_sender), (uint32_t*)(d + out.sh_member), share_cap, (uint32_t*)(d + out.group_off), group_cap, r, out_info);
        if (rc == BMQ_OK && !r.overflow)
            rc = download_end(e, g, delivery_download(d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, e->s_out));
    }
    ticket_release(S);
    if (rc) return rc;
    return r.overflow ? delivery_nospace(e) : BMQ_OK;
}
