// bmq_delivery_engine.inc -- bmq_delivery_plan / bmq_delivery_plan_dev / bmq_delivery_wait: the delivery plan of a match batch
// (bmq_delivery_core.h says what it replaces in the reference).  Included at the end of bmq_engine.hip, behind bmq_share_engine.inc.
namespace {
// the engine's Delivery over whichever executor it has, with the Fanout and the Share it composes (all created by the first call).  A
// buffer that grows is freed first, and a free waits for every stream of the device: the persistent matcher leaves before.
template <class F> int with_delivery(bmq_engine* e, F&& f) {
    return with_share(e, [&](auto& sh, auto& ix) {
        if constexpr (std::is_same_v<std::decay_t<decltype(ix)>, DistIndex<HostExec>>) {
            if (!e->hfo) e->hfo = std::make_unique<Fanout<HostExec>>(e->hx, *e->hix);
            if (!e->hdl) e->hdl = std::make_unique<Delivery<HostExec>>(e->hx);
            return f(*e->hdl, *e->hfo, sh, ix);
        } else {
            if (!e->dfo) e->dfo = std::make_unique<Fanout<DevExec>>(e->dx, *e->dix);
            if (!e->ddl) {
                e->ddl = std::make_unique<Delivery<DevExec>>(e->dx);
                e->ddl->before_free = [e] { poller_stop_locked(e); };
            }
            return f(*e->ddl, *e->dfo, sh, ix);
        }
    });
}
// one plan over exec memory; out_info is filled whatever the outcome of the capacities
int delivery_run(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* ids, uint32_t n_topics, uint32_t total, const uint32_t* sender_off,
                 const uint32_t* sender_hash, uint32_t n_senders, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap,
                 uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, DeliveryResult& r,
                 bmq_delivery_info* out_info) {
    const int rc = with_delivery(e, [&](auto& dl, auto& fo, auto& sh, auto& ix) {
        out_info->generation = ix.generation;
        return dl.plan(fo, sh, ix, row_ptr, ids, n_topics, total, sender_off, sender_hash, n_senders, nonce, out_topic, out_route, out_aux, row_cap, out_share_sender,
                       out_share_member, share_cap, out_group_off, group_cap, r)
                   ? (int)BMQ_OK
                   : index_error(e, dl.error, dl.invalid);
    });
    if (rc) return rc;
    out_info->n_rows = r.n_rows;
    out_info->n_share_rows = r.n_share_rows;
    out_info->n_groups = r.n_groups;
    out_info->n_merged_groups = r.n_merged_groups;
    out_info->n_share_only_groups = r.n_share_only_groups;
    out_info->special = r.special;
    out_info->ms_group = r.ms_group;
    out_info->ms_resolve = r.ms_resolve;
    out_info->ms_map = r.ms_map;
    out_info->ms_merge = r.ms_merge;
    return BMQ_OK;
}
int delivery_nospace(bmq_engine* e) { return set_err(e, BMQ_E_NOSPACE, "row buffers, share buffers or group table too small"); }
int check_senders(bmq_engine* e, const uint32_t* sender_off, const int32_t* sender_hash, uint32_t n_topics) {
    if (sender_off[0] != 0) return set_err(e, BMQ_E_INVAL, "sender_off[0] != 0");
    for (uint32_t t = 0; t < n_topics; t++)
        if (sender_off[t + 1] < sender_off[t]) return set_err(e, BMQ_E_INVAL, "sender_off not ascending");
    if (sender_off[n_topics] && !sender_hash) return set_err(e, BMQ_E_INVAL, "null pointer");
    return BMQ_OK;
}
// where the outputs of a plan lie in one device buffer
struct DeliveryOut {
    size_t topic, route, aux, sh_sender, sh_member, group_off, end;
    DeliveryOut(size_t at, uint32_t row_cap, uint32_t share_cap, uint32_t group_cap) {
        auto take = [&](size_t words) {
            const size_t o = at;
            at += (words * 4 + 15) & ~(size_t)15;
            return o;
        };
        topic = take(row_cap), route = take(row_cap), aux = take(row_cap), sh_sender = take(share_cap), sh_member = take(share_cap);
        group_off = take((size_t)group_cap + 1);
        end = at;
    }
};
// the caller's arrays from the device buffer, on stream `s`
hipError_t delivery_download(const uint8_t* d, const DeliveryOut& o, const DeliveryResult& r, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux,
                             uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t* out_group_off, hipStream_t s) {
    hipError_t he = hipMemcpyAsync(out_group_off, d + o.group_off, 4 * ((size_t)r.n_groups + 1), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && r.n_rows) he = hipMemcpyAsync(out_topic, d + o.topic, 4 * (size_t)r.n_rows, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && r.n_rows) he = hipMemcpyAsync(out_route, d + o.route, 4 * (size_t)r.n_rows, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && r.n_rows) he = hipMemcpyAsync(out_aux, d + o.aux, 4 * (size_t)r.n_rows, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && r.n_share_rows) he = hipMemcpyAsync(out_share_sender, d + o.sh_sender, 4 * (size_t)r.n_share_rows, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess && r.n_share_rows) he = hipMemcpyAsync(out_share_member, d + o.sh_member, 4 * (size_t)r.n_share_rows, hipMemcpyDeviceToHost, s);
    return he;
}
bool delivery_null_outputs(uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                           uint32_t share_cap, uint32_t* out_group_off) {
    return !out_group_off || (row_cap && (!out_topic || !out_route || !out_aux)) || (share_cap && (!out_share_sender || !out_share_member));
}
} // namespace

extern "C" int bmq_delivery_plan_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_topics, uint64_t total,
                                     const uint32_t* d_sender_off, const int32_t* d_sender_hash, uint32_t n_senders, uint64_t nonce, uint32_t* d_out_topic,
                                     uint32_t* d_out_route, uint32_t* d_out_aux, uint32_t row_cap, uint32_t* d_out_share_sender, uint32_t* d_out_share_member,
                                     uint32_t share_cap, uint32_t* d_out_group_off, uint32_t group_cap, bmq_delivery_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (!d_row_ptr || !d_sender_off || (total && !d_route_ids) || (n_senders && !d_sender_hash) ||
        delivery_null_outputs(d_out_topic, d_out_route, d_out_aux, row_cap, d_out_share_sender, d_out_share_member, share_cap, d_out_group_off))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (total >= 0x7FFFFFF0ull) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    *out_info = bmq_delivery_info{};
    DeliveryResult r;
    const int rc = delivery_run(e, d_row_ptr, d_route_ids, n_topics, (uint32_t)total, d_sender_off, (const uint32_t*)d_sender_hash, n_senders, nonce, d_out_topic,
                                d_out_route, d_out_aux, row_cap, d_out_share_sender, d_out_share_member, share_cap, d_out_group_off, group_cap, r, out_info);
    if (rc) return rc;
    return r.overflow ? delivery_nospace(e) : BMQ_OK;
}

extern "C" int bmq_delivery_plan(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_topics, const uint32_t* sender_off,
                                 const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap,
                                 uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap,
                                 bmq_delivery_info* out_info) {
    if (!e || !out_info) return BMQ_E_INVAL;
    if (!row_ptr || !sender_off || delivery_null_outputs(out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (row_ptr[0] != 0) return set_err(e, BMQ_E_INVAL, "row_ptr[0] != 0");
    for (uint32_t i = 0; i < n_topics; i++)
        if (row_ptr[i + 1] < row_ptr[i]) return set_err(e, BMQ_E_INVAL, "row_ptr not ascending");
    const uint32_t total = row_ptr[n_topics];
    if (total >= 0x7FFFFFF0u) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (total && !route_ids) return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_s = check_senders(e, sender_off, sender_hash, n_topics)) return rc_s;
    const uint32_t n_senders = sender_off[n_topics];
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    *out_info = bmq_delivery_info{};
    DeliveryResult r;
    if (e->device < 0) { // host-only engine: the same per-item functions on host threads, straight on the caller's buffers
        const int rc = delivery_run(e, row_ptr, route_ids, n_topics, total, sender_off, (const uint32_t*)sender_hash, n_senders, nonce, out_topic, out_route, out_aux,
                                    row_cap, out_share_sender, out_share_member, share_cap, out_group_off, group_cap, r, out_info);
        if (rc) return rc;
        return r.overflow ? delivery_nospace(e) : BMQ_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    // staging: [row_ptr | ids | sender_off | sender_hash | the outputs]
    size_t o = 0;
    auto take = [&](size_t words) {
        const size_t at = o;
        o += (words * 4 + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_row = take((size_t)n_topics + 1), o_ids = take(total), o_so = take((size_t)n_topics + 1), o_sh = take(n_senders);
    const DeliveryOut out(o, row_cap, share_cap, group_cap);
    if (out.end + 16 > e->dl_buf.cap) poller_stop_locked(e);
    HIPCHK(e, e->dl_buf.ensure(out.end + 16));
    uint8_t* d = e->dl_buf.as<uint8_t>();
    hipStream_t s = e->stream;
    HIPCHK(e, hipMemcpyAsync(d + o_row, row_ptr, 4 * ((size_t)n_topics + 1), hipMemcpyHostToDevice, s));
    if (total) HIPCHK(e, hipMemcpyAsync(d + o_ids, route_ids, 4 * (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(d + o_so, sender_off, 4 * ((size_t)n_topics + 1), hipMemcpyHostToDevice, s));
    if (n_senders) HIPCHK(e, hipMemcpyAsync(d + o_sh, sender_hash, 4 * (size_t)n_senders, hipMemcpyHostToDevice, s));
    const int rc = delivery_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_topics, total, (const uint32_t*)(d + o_so), (const uint32_t*)(d + o_sh),
                                n_senders, nonce, (uint32_t*)(d + out.topic), (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap, (uint32_t*)(d + out.sh_sender),
                                (uint32_t*)(d + out.sh_member), share_cap, (uint32_t*)(d + out.group_off), group_cap, r, out_info);
    if (rc) return rc;
    if (r.overflow) return delivery_nospace(e);
    HIPCHK(e, delivery_download(d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return BMQ_OK;
}

extern "C" int bmq_delivery_wait(bmq_engine* e, int ticket, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic,
                                       uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                                       uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_info || !out_total || !sender_off ||
        delivery_null_outputs(out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off))
        return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_DELIVERY, false, g, &total);
    if (!g.owns_lock()) return rc; // refused before the wait: the ticket stays as it was
    *out_total = total;
    *out_info = bmq_delivery_info{};
    DeliveryResult r;
    if (rc == BMQ_OK && total >= 0x7FFFFFF0ull) rc = set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (rc == BMQ_OK) rc = check_senders(e, sender_off, sender_hash, S.n_rows);
    if (rc == BMQ_OK) {
        // the plan of the CSR the batch left in the slot, on the engine stream (bmq_delivery.h: returns when the rows are complete); the
        // senders are staged in front of it, the outputs lie in the slot until the download on the copy-out stream is over
        const uint32_t n_topics = S.n_rows, n_senders = sender_off[n_topics];
        const size_t so_bytes = (4 * ((size_t)n_topics + 1) + 15) & ~(size_t)15;
        const DeliveryOut out(0, row_cap, share_cap, group_cap);
        if (so_bytes + 4 * (size_t)n_senders + 16 > e->dl_buf.cap) poller_stop_locked(e);
        if (e->dl_buf.ensure(so_bytes + 4 * (size_t)n_senders + 16) != hipSuccess || S.g_pairs.ensure(out.end + 64) != hipSuccess)
            rc = set_err(e, BMQ_E_NOMEM, "out of device memory (delivery plan)");
        uint8_t* in = e->dl_buf.as<uint8_t>();
        uint8_t* d = S.g_pairs.as<uint8_t>();
        if (rc == BMQ_OK) {
            hipError_t he = hipMemcpyAsync(in, sender_off, 4 * ((size_t)n_topics + 1), hipMemcpyHostToDevice, e->stream);
            if (he == hipSuccess && n_senders) he = hipMemcpyAsync(in + so_bytes, sender_hash, 4 * (size_t)n_senders, hipMemcpyHostToDevice, e->stream);
            if (he != hipSuccess) rc = set_err(e, BMQ_E_HIP, std::string("sender upload: ") + hipGetErrorString(he));
        }
        if (rc == BMQ_OK)
            rc = delivery_run(e, S.s_row_ptr.as<uint32_t>(), S.s_ids.as<uint32_t>(), n_topics, (uint32_t)total, (const uint32_t*)in, (const uint32_t*)(in + so_bytes),
                              n_senders, nonce, (uint32_t*)(d + out.topic), (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap, (uint32_t*)(d + out.sh_sender),
                              (uint32_t*)(d + out.sh_member), share_cap, (uint32_t*)(d + out.group_off), group_cap, r, out_info);
        if (rc == BMQ_OK && !r.overflow)
            rc = download_end(e, g, delivery_download(d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, e->s_out));
    }
    ticket_release(S);
    if (rc) return rc;
    return r.overflow ? delivery_nospace(e) : BMQ_OK;
}
