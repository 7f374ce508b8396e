// bmq_caps_engine.inc -- bmq_routes_cap_batch / bmq_routes_cap_dev / bmq_delivery_wait_capped: the fan-out caps of MatchedRoutes over a
// whole match CSR (bmq_caps_core.h says what they replace in the reference).  Included at the end of bmq_engine.hip, behind
// bmq_delivery_engine.inc (the capped wait hands its CSR to delivery_run).
namespace {
// the engine's Caps over whichever executor it has, created by the first call.  A buffer that grows is freed first, and a free waits for
// every stream of the device: the persistent matcher leaves before.
template <class F> int with_caps(bmq_engine* e, F&& f) {
    if (e->device < 0) {
        if (!e->hcp) e->hcp = std::make_unique<Caps<HostExec>>(e->hx);
        return f(*e->hcp, *e->hix);
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->dcp) {
        e->dcp = std::make_unique<Caps<DevExec>>(e->dx);
        e->dcp->before_free = [e] { poller_stop_locked(e); };
    }
    e->dx.marks_on = e->kernel_events;
    return f(*e->dcp, *e->dix);
}
int caps_check_table(bmq_engine* e, const int32_t* max_pf, const int32_t* max_gf, uint32_t n_caps) {
    for (uint32_t t = 0; t < n_caps; t++)
        if (max_pf[t] < 0 || max_gf[t] < 0) return set_err(e, BMQ_E_INVAL, "negative fan-out cap");
    return BMQ_OK;
}
// one run over exec memory (h_pf / h_gf: the table on the host, checked); out_info is filled whatever the outcome of the capacity
int caps_run(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_rows, uint32_t total, const uint32_t* row_caps, const int32_t* max_pf,
             const int32_t* max_gf, uint32_t n_caps, const int32_t* h_pf, const int32_t* h_gf, uint32_t* out_row_ptr, uint32_t* out_ids, uint64_t out_cap,
             uint32_t* out_class_counts, int32_t* out_events, uint32_t events_cap, CapsResult& r, bmq_caps_info* out_info) {
    const int rc = with_caps(e, [&](auto& cp, auto& ix) {
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
    if (row_ptr[0] != 0) return set_err(e, BMQ_E_INVAL, "row_ptr[0] != 0");
    for (uint32_t i = 0; i < n_rows; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return set_err(e, BMQ_E_INVAL, "row_ptr not ascending");
    const uint32_t total = row_ptr[n_rows];
    if (total >= 0x7FFFFFF0u || n_rows >= 0x3FFFFFF0u) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
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
    size_t o = 0;
    auto take = [&](size_t words) {
        const size_t at = o;
        o += (words * 4 + 15) & ~(size_t)15;
        return at;
    };
    const uint32_t ev_cap = out_events ? events_cap : 0u;
    const size_t ids_cap = (size_t)std::min<uint64_t>(out_cap, total);
    const size_t o_row = take((size_t)n_rows + 1), o_ids = take(total), o_rc = take(row_caps ? n_rows : 0), o_pf = take(n_caps), o_gf = take(n_caps);
    const size_t o_orow = take((size_t)n_rows + 1), o_oids = take(ids_cap), o_cc = take(out_class_counts ? 2 * (size_t)n_rows : 0), o_ev = take(4 * (size_t)ev_cap);
    if (o + 16 > e->caps_buf.cap) poller_stop_locked(e);
    HIPCHK(e, e->caps_buf.ensure(o + 16));
    uint8_t* d = e->caps_buf.as<uint8_t>();
    hipStream_t s = e->stream;
    HIPCHK(e, hipMemcpyAsync(d + o_row, row_ptr, 4 * ((size_t)n_rows + 1), hipMemcpyHostToDevice, s));
    if (total) HIPCHK(e, hipMemcpyAsync(d + o_ids, route_ids, 4 * (size_t)total, hipMemcpyHostToDevice, s));
    if (row_caps && n_rows) HIPCHK(e, hipMemcpyAsync(d + o_rc, row_caps, 4 * (size_t)n_rows, hipMemcpyHostToDevice, s));
    if (n_caps) {
        HIPCHK(e, hipMemcpyAsync(d + o_pf, max_pf, 4 * (size_t)n_caps, hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(d + o_gf, max_gf, 4 * (size_t)n_caps, hipMemcpyHostToDevice, s));
    }
    const int rc = caps_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_rows, total, row_caps ? (const uint32_t*)(d + o_rc) : nullptr,
                            (const int32_t*)(d + o_pf), (const int32_t*)(d + o_gf), n_caps, max_pf, max_gf, (uint32_t*)(d + o_orow), (uint32_t*)(d + o_oids), ids_cap,
                            out_class_counts ? (uint32_t*)(d + o_cc) : nullptr, ev_cap ? (int32_t*)(d + o_ev) : nullptr, ev_cap, r, out_info);
    if (rc) return rc;
    if (out_n_events) *out_n_events = r.n_events;
    const size_t n_ev = std::min<size_t>(r.n_events, ev_cap);
    if (n_ev) HIPCHK(e, hipMemcpyAsync(out_events, d + o_ev, 16 * n_ev, hipMemcpyDeviceToHost, s));
    if (!r.overflow) {
        HIPCHK(e, hipMemcpyAsync(out_row_ptr, d + o_orow, 4 * ((size_t)n_rows + 1), hipMemcpyDeviceToHost, s));
        if (r.n_kept) HIPCHK(e, hipMemcpyAsync(out_route_ids, d + o_oids, 4 * (size_t)r.n_kept, hipMemcpyDeviceToHost, s));
        if (out_class_counts && n_rows) HIPCHK(e, hipMemcpyAsync(out_class_counts, d + o_cc, 8 * (size_t)n_rows, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    return r.overflow ? caps_nospace(e) : BMQ_OK;
}

extern "C" int bmq_delivery_wait_capped(bmq_engine* e, int ticket, const int32_t* max_pf, const int32_t* max_gf, uint32_t n_caps, const uint32_t* sender_off,
                                        const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap,
                                        uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap,
                                        bmq_delivery_info* out_info, uint64_t* out_total, int32_t* out_events, uint32_t events_cap, uint32_t* out_n_events,
                                        bmq_caps_info* out_caps_info) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_info || !out_caps_info || !out_total || !sender_off || (n_caps && (!max_pf || !max_gf)) ||
        delivery_null_outputs(out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off))
        return BMQ_E_INVAL;
    if (out_n_events) *out_n_events = 0;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    { // refused before the wait: the ticket stays as it was
        std::lock_guard<std::mutex> g0(e->mu);
        if (int rc_t = caps_check_table(e, max_pf, max_gf, n_caps)) return rc_t;
        if (S.submitted && !S.devptr && S.format == BMQ_FMT_DELIVERY && S.last.n_tenants != n_caps)
            return set_err(e, BMQ_E_INVAL, "n_caps is not the tenant count of the ticket's batch");
    }
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_DELIVERY, false, g, &total);
    if (!g.owns_lock()) return rc;
    *out_total = total;
    *out_info = bmq_delivery_info{};
    *out_caps_info = bmq_caps_info{};
    DeliveryResult r;
    CapsResult cr;
    if (rc == BMQ_OK && total >= 0x7FFFFFF0ull) rc = set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (rc == BMQ_OK) rc = check_senders(e, sender_off, sender_hash, S.n_rows);
    if (rc == BMQ_OK) {
        // the caps over the CSR the batch left in the slot, then the plan of the capped CSR, both on the engine stream; the caps table and the
        // senders are staged in front of them, the capped CSR and the events lie in the engine's buffer, the plan's outputs in the slot
        const uint32_t n_topics = S.n_rows, n_senders = sender_off[n_topics], ev_cap = out_events ? events_cap : 0u;
        size_t o = 0;
        auto take = [&](size_t words) {
            const size_t at = o;
            o += (words * 4 + 15) & ~(size_t)15;
            return at;
        };
        const size_t o_pf = take(n_caps), o_gf = take(n_caps), o_orow = take((size_t)n_topics + 1), o_oids = take((size_t)total), o_ev = take(4 * (size_t)ev_cap);
        const size_t so_bytes = (4 * ((size_t)n_topics + 1) + 15) & ~(size_t)15;
        const DeliveryOut out(0, row_cap, share_cap, group_cap);
        if (so_bytes + 4 * (size_t)n_senders + 16 > e->dl_buf.cap || o + 16 > e->caps_buf.cap) poller_stop_locked(e);
        if (e->dl_buf.ensure(so_bytes + 4 * (size_t)n_senders + 16) != hipSuccess || e->caps_buf.ensure(o + 16) != hipSuccess || S.g_pairs.ensure(out.end + 64) != hipSuccess)
            rc = set_err(e, BMQ_E_NOMEM, "out of device memory (capped delivery plan)");
        uint8_t* in = e->dl_buf.as<uint8_t>();
        uint8_t* c = e->caps_buf.as<uint8_t>();
        uint8_t* d = S.g_pairs.as<uint8_t>();
        if (rc == BMQ_OK) {
            hipError_t he = hipMemcpyAsync(in, sender_off, 4 * ((size_t)n_topics + 1), hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_senders) he = hipMemcpyAsync(in + so_bytes, sender_hash, 4 * (size_t)n_senders, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_caps) he = hipMemcpyAsync(c + o_pf, max_pf, 4 * (size_t)n_caps, hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_caps) he = hipMemcpyAsync(c + o_gf, max_gf, 4 * (size_t)n_caps, hipMemcpyHostToDevice, e->stream);
            if (he != hipSuccess) rc = set_err(e, BMQ_E_HIP, std::string("sender upload: ") + hipGetErrorString(he));
        }
        if (rc == BMQ_OK)
            rc = caps_run(e, S.s_row_ptr.as<uint32_t>(), S.s_ids.as<uint32_t>(), n_topics, (uint32_t)total, S.s_topic_tenant.as<uint32_t>(), (const int32_t*)(c + o_pf),
                          (const int32_t*)(c + o_gf), n_caps, max_pf, max_gf, (uint32_t*)(c + o_orow), (uint32_t*)(c + o_oids), total, nullptr,
                          ev_cap ? (int32_t*)(c + o_ev) : nullptr, ev_cap, cr, out_caps_info);
        if (rc == BMQ_OK) {
            if (out_n_events) *out_n_events = cr.n_events;
            const size_t n_ev = std::min<size_t>(cr.n_events, ev_cap);
            hipError_t he = n_ev ? hipMemcpyAsync(out_events, c + o_ev, 16 * n_ev, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
            if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
            if (he != hipSuccess) rc = set_err(e, BMQ_E_HIP, std::string("event download: ") + hipGetErrorString(he));
        }
        if (rc == BMQ_OK)
            rc = delivery_run(e, (const uint32_t*)(c + o_orow), (const uint32_t*)(c + o_oids), n_topics, (uint32_t)cr.n_kept, (const uint32_t*)in,
                              (const uint32_t*)(in + so_bytes), n_senders, nonce, (uint32_t*)(d + out.topic), (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap,
                              (uint32_t*)(d + out.sh_sender), (uint32_t*)(d + out.sh_member), share_cap, (uint32_t*)(d + out.group_off), group_cap, r, out_info);
        if (rc == BMQ_OK && !r.overflow)
            rc = download_end(e, g, delivery_download(d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, e->s_out));
    }
    ticket_release(S);
    if (rc) return rc;
    return r.overflow ? delivery_nospace(e) : BMQ_OK;
}
