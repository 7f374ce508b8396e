// bmq_formats.inc -- host-visible result formats of the asynchronous match (include/bmq.h: bmq_match_submit_fmt / bmq_match_wait_*;
// SURVEY.md 8d: "host enqueue -> results visible on host").  The id CSR of a million-topic batch is 77 MB over PCIe; what the callers of the reference's match path go on to
// do needs less:
//   COUNTS  : DistWorkerCoProc.batchDist replies with the fan-out per topic and nothing else (DW/DistWorkerCoProc.java:535-538)
//   RANGES  : the matched (begin, count) id ranges (bmq_format_kernels.h); the consumer that walks the routes expands them itself
//   GROUPED : the (topic, route) pairs regrouped by DelivererKey (bmq_fanout.h), what DeliverExecutorGroup.submit builds next
// Included at the end of bmq_engine.hip; the waits stand on its ticket_begin / download_end / ticket_release.
extern "C" int bmq_match_wait_counts(bmq_engine* e, int ticket, uint32_t* out_row_ptr, uint64_t* out_total) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_row_ptr) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_COUNTS, false, g, &total);
    if (!g.owns_lock()) return rc; // refused before the wait: the ticket stays as it was
    if (rc == BMQ_OK) {
        const hipError_t he = hipMemcpyAsync(out_row_ptr, S.s_row_ptr.p, sizeof(uint32_t) * ((size_t)S.n_rows + 1), hipMemcpyDeviceToHost, e->s_out);
        rc = download_end(e, g, he);
    }
    if (out_total) *out_total = total;
    ticket_release(S);
    return rc;
}

extern "C" int bmq_match_wait_ranges(bmq_engine* e, int ticket, uint32_t* out_row_ptr, uint32_t* out_range_ptr, bmq_id_range* out_ranges, uint64_t range_cap,
                                     uint32_t* out_side_ids, uint64_t side_cap, bmq_ranges_info* out_info) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_range_ptr || !out_info) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    static_assert(sizeof(bmq_id_range) == sizeof(MatchRange), "bmq_id_range is the device layout");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_RANGES, false, g, &total);
    if (!g.owns_lock()) return rc;
    *out_info = bmq_ranges_info{};
    out_info->n_ids = total;
    for (int attempt = 0; rc == BMQ_OK && attempt < 3; attempt++) {
        if (hipEventSynchronize(S.ev_fmt) != hipSuccess) {
            rc = set_err(e, BMQ_E_HIP, "format kernels");
            break;
        }
        const unsigned long long n_r = S.h_fsums[0], n_s = S.h_fsums[1], flags = S.h_fsums[3];
        if (flags & 2ull) {
            rc = set_err(e, BMQ_E_STATE, "range format ran on an incomplete batch");
            break;
        }
        if (!(flags & 1ull)) break;
        // the slot's own buffers were too small: they know the sizes now; only the format kernels run again (the matched ranges of the
        // batch stay in the slot until its next launch)
        S.range_cap = std::max<uint64_t>(S.range_cap, n_r + n_r / 8 + 1024);
        S.side_cap = std::max<uint64_t>(S.side_cap, n_s + n_s / 8 + 1024);
        if ((rc = complete_apply(e))) break; // (a batch handed over with bmq_routes_apply_async: the view below is read from its bookkeeping)
        BatchArgs again = S.last;
        again.ix = e->dix->view(); // (an apply since the launch may have moved the id lists to a larger buffer: offsets stay valid, pointers do not)
        if ((rc = enqueue_ranges(e, S, again))) break;
        if (attempt == 2) rc = set_err(e, BMQ_E_NOMEM, "range buffers did not converge");
    }
    bool fits = true;
    if (rc == BMQ_OK) {
        const uint64_t n_r = S.h_fsums[0], n_s = S.h_fsums[1];
        out_info->n_ranges = n_r;
        out_info->n_side_ids = n_s;
        out_info->n_overlapping_rows = S.h_fsums[2];
        fits = n_r <= range_cap && n_s <= side_cap && (n_r == 0 || out_ranges) && (n_s == 0 || out_side_ids);
        const size_t n1 = (size_t)S.n_rows + 1;
        hipError_t he = hipMemcpyAsync(out_range_ptr, S.f_ptr.p, sizeof(uint32_t) * n1, hipMemcpyDeviceToHost, e->s_out);
        if (he == hipSuccess && out_row_ptr) he = hipMemcpyAsync(out_row_ptr, S.s_row_ptr.p, sizeof(uint32_t) * n1, hipMemcpyDeviceToHost, e->s_out);
        if (he == hipSuccess && fits && n_r) he = hipMemcpyAsync(out_ranges, S.f_ranges.p, sizeof(MatchRange) * n_r, hipMemcpyDeviceToHost, e->s_out);
        if (he == hipSuccess && fits && n_s) he = hipMemcpyAsync(out_side_ids, S.f_side.p, sizeof(uint32_t) * n_s, hipMemcpyDeviceToHost, e->s_out);
        rc = download_end(e, g, he);
    }
    ticket_release(S);
    if (rc) return rc;
    return fits ? BMQ_OK : set_err(e, BMQ_E_NOSPACE, "range buffers too small");
}

extern "C" int bmq_match_wait_grouped(bmq_engine* e, int ticket, uint32_t* out_topic, uint32_t* out_route, uint64_t pair_cap, uint32_t* out_group_off,
                                      uint32_t* out_group_rep, uint32_t group_cap, uint32_t* out_n_groups, uint32_t* out_special, uint64_t* out_total) {
    if (!e || ticket < 0 || ticket >= BMQ_MAX_TICKETS || !out_group_off || !out_total || (group_cap && !out_group_rep)) return BMQ_E_INVAL;
    if (e->device < 0) return set_err(e, BMQ_E_NODEVICE, "engine is host-only");
    bmq_engine::BatchSlot& S = e->slots[1 + ticket];
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    uint64_t total = 0;
    int rc = ticket_begin(e, ticket, BMQ_FMT_GROUPED, false, g, &total);
    if (!g.owns_lock()) return rc;
    *out_total = total;
    FanoutResult r{};
    bool fits = total <= pair_cap && (total == 0 || (out_topic && out_route));
    if (rc == BMQ_OK && total >= 0x7FFFFFF0ull) rc = set_err(e, BMQ_E_RANGE, "more than 2^31 (topic, route) pairs in one batch");
    if (rc == BMQ_OK) {
        // the segmented sort of the CSR the batch left in the slot, on the engine stream (bmq_fanout.h: returns when the groups are complete)
        const size_t tw = ((size_t)total + 3) & ~(size_t)3;
        if (S.g_pairs.ensure(sizeof(uint32_t) * 2 * tw + 64) != hipSuccess || S.g_groups.ensure(sizeof(uint32_t) * (2 * (size_t)group_cap + 2) + 64) != hipSuccess)
            rc = set_err(e, BMQ_E_NOMEM, "out of device memory (grouped result)");
        uint32_t *d_topic = S.g_pairs.as<uint32_t>(), *d_route = d_topic + tw;
        uint32_t *d_off = S.g_groups.as<uint32_t>(), *d_rep = d_off + group_cap + 1;
        if (rc == BMQ_OK) {
            if (!e->dfo) e->dfo = std::make_unique<Fanout<DevExec>>(e->dx, *e->dix);
            if (!e->dfo->group(S.s_row_ptr.as<uint32_t>(), S.s_ids.as<uint32_t>(), S.n_rows, (uint32_t)total, d_topic, d_route, d_off, d_rep, group_cap, r))
                rc = index_error(e, e->dfo->error, false);
        }
        if (rc == BMQ_OK) {
            hipError_t he = hipSuccess;
            if (fits && total) {
                he = hipMemcpyAsync(out_topic, d_topic, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, e->s_out);
                if (he == hipSuccess) he = hipMemcpyAsync(out_route, d_route, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, e->s_out);
            }
            if (he == hipSuccess && !r.group_overflow) {
                he = hipMemcpyAsync(out_group_off, d_off, sizeof(uint32_t) * ((size_t)r.n_groups + 1), hipMemcpyDeviceToHost, e->s_out);
                if (he == hipSuccess && r.n_groups) he = hipMemcpyAsync(out_group_rep, d_rep, sizeof(uint32_t) * r.n_groups, hipMemcpyDeviceToHost, e->s_out);
            }
            rc = download_end(e, g, he);
        }
    }
    ticket_release(S);
    if (rc) return rc;
    if (out_n_groups) *out_n_groups = r.n_groups;
    if (out_special) *out_special = r.special;
    if (!fits) return set_err(e, BMQ_E_NOSPACE, "pair buffers too small");
    return r.group_overflow ? set_err(e, BMQ_E_NOSPACE, "group table too small") : BMQ_OK;
}
