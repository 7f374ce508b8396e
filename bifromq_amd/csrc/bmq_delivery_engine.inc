// bmq_delivery_engine.inc -- bmq_delivery_plan / bmq_delivery_plan_dev / bmq_delivery_wait[_capped / _gated]: the delivery plan of a match
// batch (bmq_delivery_core.h says what it replaces in the reference).  Included at the end of bmq_engine.hip, behind bmq_share_engine.inc and
// behind bmq_caps_engine.inc / bmq_gate_engine.inc (the waits run caps_run and gate_run in front of the plan).
namespace {
// the engine's Delivery over whichever executor it has, with the Fanout and the Share it composes (all created by the first call).  A
// buffer that grows is freed first, and a free waits for every stream of the device: the persistent matcher leaves before.
template <class F> int with_delivery(bmq_engine* e, F&& f) {
    return with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
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
// where the outputs of a plan lie in one device buffer, behind what `st` holds already
struct DeliveryOut {
    size_t topic, route, aux, sh_sender, sh_member, group_off, end;
    DeliveryOut(Stage st, uint32_t row_cap, uint32_t share_cap, uint32_t group_cap) {
        topic = st.take(4 * (size_t)row_cap), route = st.take(4 * (size_t)row_cap), aux = st.take(4 * (size_t)row_cap);
        sh_sender = st.take(4 * (size_t)share_cap), sh_member = st.take(4 * (size_t)share_cap), group_off = st.take(4 * ((size_t)group_cap + 1));
        end = st.end;
    }
};
// the caller's arrays from the device buffer, on stream `s`
int delivery_download(bmq_engine* e, const uint8_t* d, const DeliveryOut& o, const DeliveryResult& r, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux,
                      uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t* out_group_off, hipStream_t s) {
    const size_t rows = 4 * (size_t)r.n_rows, share_rows = 4 * (size_t)r.n_share_rows;
    return stage_down(e, {{out_group_off, d + o.group_off, 4 * ((size_t)r.n_groups + 1)}, {out_topic, d + o.topic, rows}, {out_route, d + o.route, rows}, {out_aux, d + o.aux, rows},
                          {out_share_sender, d + o.sh_sender, share_rows}, {out_share_member, d + o.sh_member, share_rows}}, s);
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
    if (int rc_c = check_csr(e, row_ptr, n_topics)) return rc_c;
    const uint32_t total = row_ptr[n_topics];
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
    Stage st;
    const size_t o_row = st.take(4 * ((size_t)n_topics + 1)), o_ids = st.take(4 * (size_t)total), o_so = st.take(4 * ((size_t)n_topics + 1)), o_sh = st.take(4 * (size_t)n_senders);
    const DeliveryOut out(st, row_cap, share_cap, group_cap);
    if (int rc_b = stage_ensure(e, e->dl_buf, out.end + 16)) return rc_b;
    uint8_t* d = e->dl_buf.as<uint8_t>();
    if (int rc_u = stage_up(e, {{d + o_row, row_ptr, 4 * ((size_t)n_topics + 1)}, {d + o_ids, route_ids, 4 * (size_t)total}, {d + o_so, sender_off, 4 * ((size_t)n_topics + 1)},
                                {d + o_sh, sender_hash, 4 * (size_t)n_senders}}))
        return rc_u;
    const int rc = delivery_run(e, (const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_topics, total, (const uint32_t*)(d + o_so), (const uint32_t*)(d + o_sh),
                                n_senders, nonce, (uint32_t*)(d + out.topic), (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap, (uint32_t*)(d + out.sh_sender),
                                (uint32_t*)(d + out.sh_member), share_cap, (uint32_t*)(d + out.group_off), group_cap, r, out_info);
    if (rc) return rc;
    if (r.overflow) return delivery_nospace(e);
    if (int rc_d = delivery_download(e, d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, e->stream)) return rc_d;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return BMQ_OK;
}

// ---- the wait of a FMT_DELIVERY ticket: the plan of the CSR the batch left in the slot, with the caps and the gate in front of it where
// the caller asks for them.  A stage is its inputs and outputs; a gate stage comes with a caps stage (max_pf / max_gf of its table are that one's).
namespace {
struct WaitCaps {
    const int32_t *max_pf = nullptr, *max_gf = nullptr;
    uint32_t n = 0; // entries of the table: one per tenant of the batch
    int32_t* out_events = nullptr;
    uint32_t events_cap = 0;
    uint32_t* out_n_events = nullptr;
    bmq_caps_info* out_info = nullptr;
};
struct WaitGate {
    const int64_t* max_pb = nullptr;
    const uint8_t* bandwidth = nullptr;
    const uint32_t* pack_bytes = nullptr;
    uint32_t inline_threshold = 0;
    uint32_t* out_row_flags = nullptr;
    uint64_t* out_meter_bytes = nullptr;
    uint32_t* out_meter_records = nullptr;
    bmq_gate_info* out_info = nullptr;
};
// Everything on the engine stream: the senders (dl_buf) and the tables up; the caps over the slot's CSR -> the capped CSR and the events
// in caps_buf; the gate over that -> its table, the gated CSR, the flags and the meters in gate_buf; what the stages report down; the plan of
// whichever CSR is last -> the slot's g_pairs, where it lies until the download on the copy-out stream is over.
int delivery_wait(bmq_engine* e, int ticket, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route,
                  uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap,
                  bmq_delivery_info* out_info, uint64_t* out_total, const WaitCaps* caps, const WaitGate* gate) {
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (gate && !caps) return set_err(e, BMQ_E_INVAL, "a gate stage without a caps stage");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    if (caps) { // refused before the wait: the ticket stays as it was
        std::lock_guard<std::mutex> g0(e->mu);
        if (int rc_t = gate ? gate_check_table(e, caps->max_pf, caps->max_gf, gate->max_pb, gate->bandwidth, caps->n) : caps_check_table(e, caps->max_pf, caps->max_gf, caps->n))
            return rc_t;
        if (S.submitted && !S.devptr && S.format == BMQ_FMT_DELIVERY && S.last.n_tenants != caps->n)
            return set_err(e, BMQ_E_INVAL, std::string(gate ? "n_gate" : "n_caps") + " is not the tenant count of the ticket's batch");
    }
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_DELIVERY, false, g, &total);
    if (!g.owns_lock()) return rc; // refused before the wait: the ticket stays as it was
    *out_total = total;
    *out_info = bmq_delivery_info{};
    if (caps) *caps->out_info = bmq_caps_info{};
    if (gate) *gate->out_info = bmq_gate_info{};
    DeliveryResult r;
    if (rc == BMQ_OK && total >= 0x7FFFFFF0ull) rc = set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (rc == BMQ_OK) rc = check_senders(e, sender_off, sender_hash, S.n_rows);
    if (rc == BMQ_OK) rc = [&]() -> int {
        const uint32_t n_topics = S.n_rows, n_senders = sender_off[n_topics], n_tab = caps ? caps->n : 0u, ev_cap = caps && caps->out_events ? caps->events_cap : 0u;
        const size_t tab4 = 4 * (size_t)n_tab, tab8 = 8 * (size_t)n_tab, rows4 = 4 * (size_t)n_topics, row_ptr4 = rows4 + 4, ids4 = 4 * (size_t)total;
        Stage is, cs, gs;
        const size_t i_off = is.take(row_ptr4), i_hash = is.take(4 * (size_t)n_senders);
        size_t o_pf = 0, o_gf = 0, o_orow = 0, o_oids = 0, o_ev = 0, g_pb = 0, g_mb = 0, g_bw = 0, g_pk = 0, g_orow = 0, g_oids = 0, g_fl = 0, g_mr = 0;
        if (caps) o_pf = cs.take(tab4), o_gf = cs.take(tab4), o_orow = cs.take(row_ptr4), o_oids = cs.take(ids4), o_ev = cs.take(16 * (size_t)ev_cap);
        if (gate)
            g_pb = gs.take(tab8), g_mb = gs.take(tab8), g_bw = gs.take(n_tab), g_pk = gs.take(rows4), g_orow = gs.take(row_ptr4), g_oids = gs.take(ids4), g_fl = gs.take(rows4),
            g_mr = gs.take(tab4);
        const DeliveryOut out(Stage{}, row_cap, share_cap, group_cap);
        if (stage_ensure(e, e->dl_buf, is.end + 16) || (caps && stage_ensure(e, e->caps_buf, cs.end + 16)) || (gate && stage_ensure(e, e->gate_buf, gs.end + 16)) ||
            S.g_pairs.ensure(out.end + 64) != hipSuccess)
            return set_err(e, BMQ_E_NOMEM, std::string("out of device memory (") + (gate ? "gated " : caps ? "capped " : "") + "delivery plan)");
        uint8_t *in = e->dl_buf.as<uint8_t>(), *c = e->caps_buf.as<uint8_t>(), *q = e->gate_buf.as<uint8_t>(), *d = S.g_pairs.as<uint8_t>(); // (c, q: used by their stage only)
        if (int rc_u = stage_up(e, {{in + i_off, sender_off, row_ptr4}, {in + i_hash, sender_hash, 4 * (size_t)n_senders}})) return rc_u;
        if (caps)
            if (int rc_u = stage_up(e, {{c + o_pf, caps->max_pf, tab4}, {c + o_gf, caps->max_gf, tab4}})) return rc_u;
        if (gate)
            if (int rc_u = stage_up(e, {{q + g_pb, gate->max_pb, tab8}, {q + g_bw, gate->bandwidth, n_tab}, {q + g_pk, gate->pack_bytes, rows4}})) return rc_u;
        // the CSR the next step reads
        const uint32_t *row_ptr = S.s_row_ptr.as<uint32_t>(), *ids = S.s_ids.as<uint32_t>(), *tenant_of = S.s_topic_tenant.as<uint32_t>();
        uint32_t n_ids = (uint32_t)total, n_events = 0;
        if (caps) {
            CapsResult cr;
            if (int rc_c = caps_run(e, row_ptr, ids, n_topics, n_ids, tenant_of, (const int32_t*)(c + o_pf), (const int32_t*)(c + o_gf), n_tab, caps->max_pf, caps->max_gf,
                                    (uint32_t*)(c + o_orow), (uint32_t*)(c + o_oids), total, nullptr, ev_cap ? (int32_t*)(c + o_ev) : nullptr, ev_cap, cr, caps->out_info))
                return rc_c;
            row_ptr = (const uint32_t*)(c + o_orow), ids = (const uint32_t*)(c + o_oids), n_ids = (uint32_t)cr.n_kept, n_events = cr.n_events;
        }
        if (gate) {
            GateTable T;
            T.max_pf = (const int32_t*)(c + o_pf), T.max_gf = (const int32_t*)(c + o_gf), T.max_pb = (const int64_t*)(q + g_pb), T.bw = q + g_bw, T.n_gate = n_tab;
            GateResult gr;
            if (int rc_g = gate_run(e, row_ptr, ids, n_topics, n_ids, (const uint32_t*)(q + g_pk), tenant_of, T, gate->inline_threshold, (uint32_t*)(q + g_orow), (uint32_t*)(q + g_oids),
                                    total, (uint32_t*)(q + g_fl), nullptr, (uint64_t*)(q + g_mb), (uint32_t*)(q + g_mr), gr, gate->out_info))
                return rc_g;
            row_ptr = (const uint32_t*)(q + g_orow), ids = (const uint32_t*)(q + g_oids), n_ids = (uint32_t)gr.n_kept;
        }
        if (caps) { // what the stages report: the events, the flags and the meters
            if (caps->out_n_events) *caps->out_n_events = n_events;
            if (int rc_d = stage_down(e, {{caps->out_events, c + o_ev, 16 * std::min<size_t>(n_events, ev_cap)}})) return rc_d;
            if (gate)
                if (int rc_d = stage_down(e, {{gate->out_row_flags, q + g_fl, rows4}, {gate->out_meter_bytes, q + g_mb, tab8}, {gate->out_meter_records, q + g_mr, tab4}})) return rc_d;
            HIPCHK(e, hipStreamSynchronize(e->stream));
        }
        if (int rc_p = delivery_run(e, row_ptr, ids, n_topics, n_ids, (const uint32_t*)(in + i_off), (const uint32_t*)(in + i_hash), n_senders, nonce, (uint32_t*)(d + out.topic),
                                    (uint32_t*)(d + out.route), (uint32_t*)(d + out.aux), row_cap, (uint32_t*)(d + out.sh_sender), (uint32_t*)(d + out.sh_member), share_cap,
                                    (uint32_t*)(d + out.group_off), group_cap, r, out_info))
            return rc_p;
        if (r.overflow) return BMQ_OK;
        if (int rc_d = delivery_download(e, d, out, r, out_topic, out_route, out_aux, out_share_sender, out_share_member, out_group_off, e->s_out)) return rc_d;
        return download_end(e, g, hipSuccess);
    }();
    ticket_release(S);
    if (rc) return rc;
    return r.overflow ? delivery_nospace(e) : BMQ_OK;
}
} // namespace

extern "C" int bmq_delivery_wait(bmq_engine* e, int ticket, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic,
                                 uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                                 uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_info || !out_total || !sender_off ||
        delivery_null_outputs(out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off))
        return BMQ_E_INVAL;
    return delivery_wait(e, ticket, sender_off, sender_hash, nonce, out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off, group_cap,
                         out_info, out_total, nullptr, nullptr);
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
    const WaitCaps caps{max_pf, max_gf, n_caps, out_events, events_cap, out_n_events, out_caps_info};
    return delivery_wait(e, ticket, sender_off, sender_hash, nonce, out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off, group_cap,
                         out_info, out_total, &caps, nullptr);
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
    const WaitCaps caps{max_pf, max_gf, n_gate, out_events, events_cap, out_n_events, out_caps_info};
    const WaitGate gate{max_pb, bandwidth, pack_bytes, inline_threshold, out_row_flags, out_meter_bytes, out_meter_records, out_gate_info};
    return delivery_wait(e, ticket, sender_off, sender_hash, nonce, out_topic, out_route, out_aux, row_cap, out_share_sender, out_share_member, share_cap, out_group_off, group_cap,
                         out_info, out_total, &caps, &gate);
}
