// bmq_share_engine.inc -- bmq_share_members_apply / bmq_share_resolve / bmq_share_resolve_dev / bmq_share_member / bmq_share_info_get: the
// receivers of shared subscriptions (bmq_share_core.h says what they replace in the reference).  Included at the end of bmq_engine.hip.
namespace {
template <class S> int share_error(bmq_engine* e, const S& s) { return index_error(e, s.error, s.invalid); }
int share_result(bmq_engine* e, const ShareResult& r, uint32_t* out_n_rows, uint32_t* out_n_groups, uint32_t* out_special) {
    if (out_n_rows) *out_n_rows = r.n_rows;
    if (out_n_groups) *out_n_groups = r.n_groups;
    if (out_special) *out_special = r.special;
    return r.overflow ? set_err(e, BMQ_E_NOSPACE, "row buffers or group table too small") : BMQ_OK;
}
} // namespace

// ---- bmq_config.share_carry = 1: called by bmq_compact / bmq_compact_swap under the locks they hold, with the poller stopped.  A carry that
// fails drops every table and leaves its message in the error string; the generation change goes on.
namespace {
DistIndex<DevExec>& next_generation(bmq_engine* e, DistIndex<DevExec>&) { return *e->cmp.next_d; }
DistIndex<HostExec>& next_generation(bmq_engine* e, DistIndex<HostExec>&) { return *e->cmp.next_h; }
} // namespace
static void share_carry_prepare(bmq_engine* e, bool copy_bytes) {
    (void)with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
        if (!sh.carry_prepare(ix, copy_bytes)) e->err = sh.error;
        return 0;
    });
}
static void share_carry_finish(bmq_engine* e, bool changed) {
    (void)with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
        if (!changed) sh.carry_cancel();
        else if (!sh.carry_finish(ix)) e->err = sh.error;
        return 0;
    });
}
static void share_carry_swap(bmq_engine* e) {
    (void)with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
        if (!sh.carry_prepare(ix, false) || !sh.carry_finish(next_generation(e, ix))) e->err = sh.error;
        return 0;
    });
}

extern "C" int bmq_share_carry_info_get(const bmq_engine* ce, bmq_share_carry_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    memset(out, 0, sizeof(*out));
    return with_control(e, e->hsh, e->dsh, [&](auto& sh, auto&) {
        const auto& ci = sh.carry_info;
        out->from_generation = ci.from_generation;
        out->to_generation = ci.to_generation;
        out->n_carried = ci.n_carried;
        out->n_dropped = ci.n_dropped;
        out->n_members_carried = ci.n_members_carried;
        out->ms_gather = ci.ms_gather;
        out->ms_find = ci.ms_find;
        out->ms_rekey = ci.ms_rekey;
        out->status = ci.status;
        return (int)BMQ_OK;
    });
}

extern "C" int bmq_share_members_apply(bmq_engine* e, const uint32_t* route_ids, uint32_t n, const uint32_t* member_off, const uint8_t* urls,
                                       const uint32_t* url_off) {
    if (!e) return BMQ_E_INVAL;
    if (n && (!route_ids || !member_off || !url_off || (member_off[n] && !urls))) return set_err(e, BMQ_E_INVAL, "null pointer");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    if (e->device >= 0) poller_stop_locked(e); // (the mutation path allocates and frees)
    return with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) { return sh.apply(ix, route_ids, n, member_off, urls, url_off) ? (int)BMQ_OK : share_error(e, sh); });
}

extern "C" int bmq_share_resolve_dev(bmq_engine* e, const uint32_t* d_pair_topic, const uint32_t* d_pair_route, uint32_t n_pairs,
                                     const uint32_t* d_sender_off, const int32_t* d_sender_hash, uint32_t n_topics, uint32_t n_senders, uint64_t nonce,
                                     uint32_t* d_out_pair, uint32_t* d_out_sender, uint32_t* d_out_member, uint32_t row_cap, uint32_t* d_out_group_off,
                                     uint32_t group_cap, uint32_t* out_n_rows, uint32_t* out_n_groups, uint32_t* out_special) {
    if (!e) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    if (!d_out_group_off || !d_sender_off || (n_pairs && (!d_pair_topic || !d_pair_route)) || (n_senders && !d_sender_hash) ||
        (row_cap && (!d_out_pair || !d_out_sender || !d_out_member)))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    ShareResult r;
    const int rc = with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
        return sh.resolve(ix, d_pair_topic, d_pair_route, n_pairs, d_sender_off, (const uint32_t*)d_sender_hash, n_topics, n_senders, nonce, d_out_pair,
                          d_out_sender, d_out_member, row_cap, d_out_group_off, group_cap, r)
                   ? (int)BMQ_OK
                   : share_error(e, sh);
    });
    return rc ? rc : share_result(e, r, out_n_rows, out_n_groups, out_special);
}

extern "C" int bmq_share_resolve(bmq_engine* e, const uint32_t* pair_topic, const uint32_t* pair_route, uint32_t n_pairs, const uint32_t* sender_off,
                                 const int32_t* sender_hash, uint32_t n_topics, uint64_t nonce, uint32_t* out_pair, uint32_t* out_sender,
                                 uint32_t* out_member, uint32_t row_cap, uint32_t* out_group_off, uint32_t group_cap, uint32_t* out_n_rows,
                                 uint32_t* out_n_groups, uint32_t* out_special) {
    if (!e) return BMQ_E_INVAL;
    if (!out_group_off || !sender_off || (n_pairs && (!pair_topic || !pair_route)) || (row_cap && (!out_pair || !out_sender || !out_member)))
        return set_err(e, BMQ_E_INVAL, "null pointer");
    if (int rc_s = check_senders(e, sender_off, sender_hash, n_topics)) return rc_s;
    const uint32_t n_senders = sender_off[n_topics];
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    ShareResult r;
    if (e->device < 0) { // host-only engine: the same per-item functions on host threads, straight on the caller's buffers
        const int rc = with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
            return sh.resolve(ix, pair_topic, pair_route, n_pairs, sender_off, (const uint32_t*)sender_hash, n_topics, n_senders, nonce, out_pair, out_sender,
                              out_member, row_cap, out_group_off, group_cap, r)
                       ? (int)BMQ_OK
                       : share_error(e, sh);
        });
        return rc ? rc : share_result(e, r, out_n_rows, out_n_groups, out_special);
    }
    HIPCHK(e, hipSetDevice(e->device));
    // staging: [pair_topic | pair_route | sender_off | sender_hash | out_pair | out_sender | out_member | group_off]
    Stage st;
    const size_t o_pt = st.take(4 * (size_t)n_pairs), o_pr = st.take(4 * (size_t)n_pairs), o_so = st.take(4 * ((size_t)n_topics + 1)), o_sh = st.take(4 * (size_t)n_senders),
                 o_op = st.take(4 * (size_t)row_cap), o_os = st.take(4 * (size_t)row_cap), o_om = st.take(4 * (size_t)row_cap), o_go = st.take(4 * ((size_t)group_cap + 1));
    if (int rc_b = stage_ensure(e, e->sh_buf, st.end + 16)) return rc_b;
    uint8_t* d = e->sh_buf.as<uint8_t>();
    if (int rc_u = stage_up(e, {{d + o_pt, pair_topic, 4 * (size_t)n_pairs}, {d + o_pr, pair_route, 4 * (size_t)n_pairs}, {d + o_so, sender_off, 4 * ((size_t)n_topics + 1)},
                                {d + o_sh, sender_hash, 4 * (size_t)n_senders}}))
        return rc_u;
    const int rc = with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) {
        return sh.resolve(ix, (const uint32_t*)(d + o_pt), (const uint32_t*)(d + o_pr), n_pairs, (const uint32_t*)(d + o_so), (const uint32_t*)(d + o_sh),
                          n_topics, n_senders, nonce, (uint32_t*)(d + o_op), (uint32_t*)(d + o_os), (uint32_t*)(d + o_om), row_cap, (uint32_t*)(d + o_go),
                          group_cap, r)
                   ? (int)BMQ_OK
                   : share_error(e, sh);
    });
    if (rc) return rc;
    if (!r.overflow)
        if (int rc_d = stage_down(e, {{out_pair, d + o_op, 4 * (size_t)r.n_rows}, {out_sender, d + o_os, 4 * (size_t)r.n_rows}, {out_member, d + o_om, 4 * (size_t)r.n_rows},
                                      {out_group_off, d + o_go, 4 * ((size_t)r.n_groups + 1)}}))
            return rc_d;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return share_result(e, r, out_n_rows, out_n_groups, out_special);
}

extern "C" int bmq_share_member(const bmq_engine* ce, uint32_t route_id, uint32_t index, uint8_t* out_url, uint32_t cap, uint32_t* out_len) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out_len || (cap && !out_url)) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open;
    if (!e->built) return set_err(e, BMQ_E_STATE, "no index");
    std::string url;
    const int rc = with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) { return sh.member(ix, route_id, index, url) ? (int)BMQ_OK : share_error(e, sh); });
    if (rc) return rc;
    *out_len = (uint32_t)url.size();
    if (url.size() > cap) return set_err(e, BMQ_E_NOSPACE, "url buffer too small");
    memcpy(out_url, url.data(), url.size());
    return BMQ_OK;
}

extern "C" int bmq_share_info_get(const bmq_engine* ce, bmq_share_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc_open = complete_apply(e)) return rc_open;
    memset(out, 0, sizeof(*out));
    ShareInfo si;
    const int rc = with_control(e, e->hsh, e->dsh, [&](auto& sh, auto& ix) { return sh.info(ix, si) ? (int)BMQ_OK : share_error(e, sh); });
    if (rc) return rc;
    out->n_tables = si.n_tables;
    out->n_members = si.n_members;
    out->n_deliverers = si.n_deliverers;
    out->device_bytes = e->device >= 0 ? si.bytes : 0;
    out->generation = si.generation;
    out->ms_count = si.ms[0];
    out->ms_rows = si.ms[1];
    out->ms_resolve = si.ms[2];
    out->ms_sort = si.ms[3];
    out->ms_group = si.ms[4];
    return BMQ_OK;
}
