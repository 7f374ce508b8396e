// bmq_fanout_engine.inc -- bmq_fanout_group / bmq_fanout_group_dev / bmq_fanout_info_get: the segmented sort of a match CSR by DelivererKey (SURVEY.md 8f-4;
// bmq_fanout_core.h says what it replaces in the reference).  Included at the end of bmq_engine.hip.
namespace {
int fanout_result(bmq_engine* e, const FanoutResult& r, uint32_t* out_n_groups, uint32_t* out_special) {
    if (out_n_groups) *out_n_groups = r.n_groups;
    if (out_special) *out_special = r.special;
    return r.group_overflow ? set_err(e, BMQ_E_NOSPACE, "group table too small") : BMQ_OK;
}
} // namespace

extern "C" int bmq_fanout_group_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_topics, uint64_t total,
                                    uint32_t* d_out_topic, uint32_t* d_out_route, uint32_t* d_out_group_off, uint32_t* d_out_group_rep,
                                    uint32_t group_cap, uint32_t* out_n_groups, uint32_t* out_special) {
    if (!e) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (!d_row_ptr || !d_out_group_off || (total && (!d_route_ids || !d_out_topic || !d_out_route)) || (group_cap && !d_out_group_rep))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (total >= 0x7FFFFFF0ull) return set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->dfo) e->dfo = std::make_unique<Fanout<DevExec>>(e->dx, *e->dix);
    FanoutResult r;
    if (!e->dfo->group(d_row_ptr, d_route_ids, n_topics, (uint32_t)total, d_out_topic, d_out_route, d_out_group_off, d_out_group_rep, group_cap, r))
        return index_error(e, e->dfo->error, false);
    return fanout_result(e, r, out_n_groups, out_special);
}

extern "C" int bmq_fanout_group(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_topics, uint32_t* out_topic,
                                uint32_t* out_route, uint64_t pair_cap, uint32_t* out_group_off, uint32_t* out_group_rep, uint32_t group_cap,
                                uint32_t* out_n_groups, uint32_t* out_special) {
    if (!e || !row_ptr || !out_group_off || (group_cap && !out_group_rep)) return BMQ_E_INVAL;
    if (int rc_c = check_csr(e, row_ptr, n_topics)) return rc_c;
    const uint32_t total = row_ptr[n_topics];
    if (total > pair_cap || (total && (!route_ids || !out_topic || !out_route))) return set_err(e, BMQ_E_NOSPACE, "pair buffers too small");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    FanoutResult r;
    if (e->device < 0) { // host-only engine: the same per-pair functions on host threads, straight on the caller's buffers
        if (!e->hfo) e->hfo = std::make_unique<Fanout<HostExec>>(e->hx, *e->hix);
        if (!e->hfo->group(row_ptr, route_ids, n_topics, total, out_topic, out_route, out_group_off, out_group_rep, group_cap, r))
            return index_error(e, e->hfo->error, false);
        return fanout_result(e, r, out_n_groups, out_special);
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->dfo) e->dfo = std::make_unique<Fanout<DevExec>>(e->dx, *e->dix);
    // staging: [row_ptr | ids | out_topic | out_route | group_off | group_rep]
    Stage st;
    const size_t o_row = st.take(4 * ((size_t)n_topics + 1)), o_ids = st.take(4 * (size_t)total), o_ot = st.take(4 * (size_t)total), o_or = st.take(4 * (size_t)total),
                 o_go = st.take(4 * ((size_t)group_cap + 1)), o_gr = st.take(4 * (size_t)group_cap);
    if (int rc_b = stage_ensure(e, e->fo_buf, st.end + 16)) return rc_b;
    uint8_t* d = e->fo_buf.as<uint8_t>();
    if (int rc_u = stage_up(e, {{d + o_row, row_ptr, 4 * ((size_t)n_topics + 1)}, {d + o_ids, route_ids, 4 * (size_t)total}})) return rc_u;
    if (!e->dfo->group((const uint32_t*)(d + o_row), (const uint32_t*)(d + o_ids), n_topics, total, (uint32_t*)(d + o_ot), (uint32_t*)(d + o_or),
                       (uint32_t*)(d + o_go), (uint32_t*)(d + o_gr), group_cap, r))
        return index_error(e, e->dfo->error, false);
    const size_t fits = r.group_overflow ? 0 : 1; // (a group table that is too small is not copied)
    if (int rc_d = stage_down(e, {{out_topic, d + o_ot, 4 * (size_t)total}, {out_route, d + o_or, 4 * (size_t)total},
                                  {out_group_off, d + o_go, fits * 4 * ((size_t)r.n_groups + 1)}, {out_group_rep, d + o_gr, fits * 4 * (size_t)r.n_groups}}))
        return rc_d;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return fanout_result(e, r, out_n_groups, out_special);
}

extern "C" int bmq_fanout_info_get(const bmq_engine* ce, bmq_fanout_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    memset(out, 0, sizeof(*out));
    auto fill = [&](const auto& fo) {
        if (fo.state_generation() == ~0ull) return; // created, never grouped
        out->n_fast_calls = fo.ctr.n_fast;
        out->n_generic_calls = fo.ctr.n_generic;
        out->n_refill_calls = fo.ctr.n_refill;
        out->n_table_grows = fo.ctr.n_grow;
        out->n_table_reseeds = fo.ctr.n_reseed;
        out->n_keys = fo.keys_mapped();
        out->table_slots = fo.table_slots();
        out->generation = fo.state_generation();
    };
    if (e->dfo) fill(*e->dfo);
    else if (e->hfo) fill(*e->hfo);
    return BMQ_OK;
}
