// bmq_order_engine.inc -- bmq_routes_window / bmq_routes_gc_sweep / bmq_routes_window_info_get: reads of the route keys in key order
// (DistIndex::window, bmq_order_core.h) and the dist worker's GC sweep over them (DW/DistWorkerCoProc.java:554-701).  Included at the end
// of bmq_engine.hip.
namespace {
// one window of the serving generation under e->mu; the cursor is key bytes, or (by_id) the key of a live route
int order_window(bmq_engine* e, const uint8_t* lo, uint32_t lo_len, bool has_lo, bool exclusive, bool by_id, uint32_t lo_id, uint32_t max_routes,
                 uint32_t* out_ids, uint32_t& n, uint32_t& more) {
    const bool ok = with_index(e, [&](auto& ix) {
        // the scratch grows rarely; a free waits for every stream of the device, so the persistent matcher leaves first then
        if (e->device >= 0 && !ix.window_fits(lo_len)) poller_stop_locked(e);
        const bool r = ix.window(lo, lo_len, has_lo, exclusive, by_id, lo_id, max_routes, out_ids, n, more, e->order_stats);
        if (!r) e->err = ix.error;
        return r;
    });
    return ok ? BMQ_OK : index_error(e, e->err, false);
}
} // namespace

extern "C" int bmq_routes_window(const bmq_engine* ce, const uint8_t* lo, uint32_t lo_len, uint32_t lo_exclusive, uint32_t max_routes, uint32_t* out_route_ids,
                                 uint32_t* out_n, uint32_t* out_more) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out_n || (max_routes && !out_route_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (max_routes > BMQ_WINDOW_MAX) return set_err(e, BMQ_E_INVAL, "more than BMQ_WINDOW_MAX routes asked for");
    if (lo && lo_len >= (1u << 24)) return set_err(e, BMQ_E_INVAL, "cursor key of 16 MiB or more");
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n = 0, more = 0;
    if (int rc = order_window(e, lo, lo ? lo_len : 0u, lo != nullptr, lo && lo_exclusive, false, 0, max_routes, out_route_ids, n, more)) return rc;
    e->order_last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out_n = n;
    if (out_more) *out_more = more;
    return BMQ_OK;
}

extern "C" int bmq_routes_gc_sweep(const bmq_engine* ce, const uint8_t* start_key, uint32_t start_len, uint32_t step_hint, uint32_t scan_quota,
                                   uint32_t* out_route_ids, uint32_t cap, bmq_gc_sweep_reply* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out || (cap && !out_route_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (DistIndex<HostExec>::sweep_keys_needed(step_hint, scan_quota) > 16ull * BMQ_WINDOW_MAX) return set_err(e, BMQ_E_INVAL, "a sweep of more than 16 windows per phase");
    if (start_key && start_len >= (1u << 24)) return set_err(e, BMQ_E_INVAL, "start key of 16 MiB or more");
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(*out);
    out->epoch = e->epoch;
    uint64_t inspected = 0;
    bool wrapped = false;
    uint32_t next = NONE;
    const bool ok = with_index(e, [&](auto& ix) {
        // the scratch grows rarely; a free waits for every stream of the device, so the persistent matcher leaves first then
        if (e->device >= 0 && !ix.window_fits(start_key ? start_len : 0u)) poller_stop_locked(e);
        typename std::decay_t<decltype(ix)>::SweepResult r;
        const bool done = ix.gc_sweep(start_key, start_key ? start_len : 0u, start_key != nullptr, step_hint, scan_quota, out_route_ids, cap, r, e->order_stats);
        if (!done) e->err = ix.error;
        inspected = r.inspected, wrapped = r.wrapped, next = r.has_next ? r.next_id : NONE;
        return done;
    });
    if (!ok) return index_error(e, e->err, false);
    e->order_last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    out->inspected = (uint32_t)inspected;
    out->wrapped = wrapped ? 1u : 0u;
    out->has_next = next != NONE ? 1u : 0u;
    out->next_route_id = next != NONE ? next : 0u;
    if (inspected > cap) return set_err(e, BMQ_E_NOSPACE, "out_route_ids too small: see reply.inspected");
    return BMQ_OK;
}

extern "C" int bmq_routes_window_info_get(const bmq_engine* ce, bmq_window_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(*out);
    out->window_max = BMQ_WINDOW_MAX;
    out->bucket_max = ORDER_BUCKET_MAX;
    const OrderStats& s = e->order_stats;
    out->n_calls = s.n_calls, out->n_candidates = s.n_candidates, out->n_rounds = s.n_rounds, out->n_bucket_sorts = s.n_bucket_sorts;
    out->max_bucket = s.max_bucket, out->n_rebucketed = s.n_rebucketed;
    out->last_ms = e->order_last_ms;
    return BMQ_OK;
}
