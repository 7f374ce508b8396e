// bmq_retain_engine.inc -- retain-direction entry points of include/bmq.h (included at the end of bmq_engine.hip).
namespace {

// the engine runs on ONE executor type: f gets the serving mutable part ...
template <class F> static decltype(auto) with_retain(bmq_engine* e, F&& f) {
    if (e->drt) return f(*e->drt);
    return f(*e->hrt);
}
// f on the serving mutable part; false: its message is the engine's
template <class F> static bool retain_try(bmq_engine* e, F&& f) {
    return with_retain(e, [&](auto& rt) {
        const bool ok = f(rt);
        if (!ok) e->err = rt.error;
        return ok;
    });
}
// ... and, for the generation change: the serving builder (null under bmq_config.retain_builder = 0), the executor the next generation is
// built on, and what the compaction holds of it
template <class F> static decltype(auto) with_retain_next(bmq_engine* e, F&& f) {
    if (e->drt) return f(*e->drt, e->drb.get(), e->rbx, e->rcmp.on_dev);
    return f(*e->hrt, e->hrb.get(), e->rhx, e->rcmp.on_host);
}
static const RetainDynInfo& retain_dyn_info(bmq_engine* e) {
    return with_retain(e, [](auto& rt) -> const RetainDynInfo& { return rt.info; });
}

// An image the executor builder left in rb serves from now on: the view the walk reads (the arrays lie where it reads them already); a device
// engine lets a host-built generation's buffers go
static RetainIndexView& adopt_exec_image(bmq_engine* e, const RetainBuild<HostExec>& rb) { return rb.view(e->rhview), e->rhview; }
static RetainIndexView& adopt_exec_image(bmq_engine* e, const RetainBuild<DevExec>& rb) {
    rb.view(e->rdev.view);
    for (DevBuf* b : {&e->rdev.nodes, &e->rdev.edges, &e->rdev.posts, &e->rdev.gps, &e->rdev.tenants, &e->rdev.dict, &e->rdev.pool}) b->release();
    return e->rdev.view;
}

// the stream the next generation is built on (HostExec has none)
static int retain_build_stream(bmq_engine*, HostExec&) { return BMQ_OK; }
static int retain_build_stream(bmq_engine* e, DevExec& bx) {
    if (!e->s_build) {
        int least = 0, greatest = 0;
        HIPCHK(e, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(e, hipStreamCreateWithPriority(&e->s_build, hipStreamNonBlocking, least)); // a match batch's waves go first
        HIPCHK(e, hipEventCreateWithFlags(&e->ev_serving, hipEventDisableTiming));
    }
    bx.stream = e->s_build;
    return BMQ_OK;
}

int upload_retain(bmq_engine* e) {
    RetainIndexHost& h = e->rhost;
    if (e->rb_serving) { // built by the executor builder (bmq_retain_build.h): rhost is the catalogue
        if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
        return with_retain_next(e, [&](auto& rt, auto* rb, auto&, auto&) {
            if (!rt.reset(adopt_exec_image(e, *rb), h)) return set_err(e, e->device < 0 || e->dx.err.empty() ? BMQ_E_NOMEM : BMQ_E_HIP, rt.error);
            return (int)BMQ_OK;
        });
    }
    if (e->device < 0) { // host-only engine: the bulk-loaded arrays stay where the host builder keeps them
        RetainIndexView& v = e->rhview;
        v = RetainIndexView{};
        v.nodes = h.nodes.data();
        v.edges = h.edges.data();
        v.posts = h.posts.data();
        v.gps = h.gps.data();
        v.tenants = h.tenants.data();
        v.tenant_mask = (uint32_t)h.tenants.size() - 1;
        v.dict = h.dict.data();
        v.dict_group_mask = (uint32_t)h.dict.size() / DICT_GROUP - 1;
        v.pool = h.pool.data();
        h.full_upload = h.dict_changed = false;
        h.dirty.clear();
        if (!e->hrt->reset(v, h)) return set_err(e, BMQ_E_NOMEM, e->hrt->error);
        if (e->hrb) e->hrb->release_image(); // (an executor-built generation's)
        return BMQ_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    RetainDevice& d = e->rdev;
    int rc;
    const size_t nb = h.nodes.size() * sizeof(RNode), eb = h.edges.size() * sizeof(REdge);
    if ((rc = upload(e, d.nodes, h.nodes.data(), nb))) return rc;
    if ((rc = upload(e, d.edges, h.edges.data(), eb))) return rc;
    if ((rc = upload(e, d.posts, h.posts.data(), h.posts.size() * sizeof(REdge)))) return rc;
    if ((rc = upload(e, d.gps, h.gps.data(), h.gps.size() * sizeof(RGp)))) return rc;
    if ((rc = upload(e, d.tenants, h.tenants.data(), h.tenants.size() * sizeof(RTenantSlot)))) return rc;
    if ((rc = upload(e, d.dict, h.dict.data(), h.dict.size() * sizeof(DictSlot)))) return rc;
    if ((rc = upload(e, d.pool, h.pool.data(), h.pool.size()))) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->r_up_bytes += nb + eb + h.posts.size() * sizeof(REdge) + h.gps.size() * sizeof(RGp) + h.tenants.size() * sizeof(RTenantSlot) + h.dict.size() * sizeof(DictSlot) + h.pool.size();
    h.full_upload = false;
    h.dict_changed = false;
    h.dirty.clear();
    d.view = RetainIndexView{};
    d.view.nodes = d.nodes.as<RNode>();
    d.view.edges = d.edges.as<REdge>();
    d.view.posts = d.posts.as<REdge>();
    d.view.gps = d.gps.as<RGp>();
    d.view.tenants = d.tenants.as<RTenantSlot>();
    d.view.tenant_mask = (uint32_t)h.tenants.size() - 1;
    d.view.dict = d.dict.as<DictSlot>();
    d.view.dict_group_mask = (uint32_t)h.dict.size() / DICT_GROUP - 1;
    d.view.pool = d.pool.as<uint8_t>();
    // the mutable part starts over: every bulk-loaded id live, no overlay topics (bmq_retain_dyn.h)
    if (!e->drt->reset(d.view, h)) return set_err(e, e->dx.err.empty() ? BMQ_E_NOMEM : BMQ_E_HIP, e->drt->error);
    if (e->drb) e->drb->release_image(); // (an executor-built generation's)
    return BMQ_OK;
}


// ---- who bulk-loads (bmq_config.retain_builder) -------------------------------------------------------------------------------------------
int retain_publish(bmq_engine* e);
// what bmq_retain_build_info_get tells of a generation the HOST builder built
RetainBuildInfo host_build_info(const RetainIndexHost& h, uint64_t n_items, float ms, uint32_t fallback) {
    RetainBuildInfo b;
    b.builder = 0;
    b.fallback = fallback;
    b.n_items = n_items;
    b.n_topics = h.n_topics;
    b.n_tenants = h.order.size();
    for (const RTenantState* t : h.order) {
        b.n_nodes += t->nodes.size();
        b.n_posts += t->posts.size();
        for (const RGp& g : t->gps) b.n_gp_runs += g.gp != NONE;
        for (const std::string& p : t->topics) b.max_depth = std::max<uint32_t>(b.max_depth, 1u + (uint32_t)std::count(p.begin(), p.end(), '/'));
    }
    b.n_edges = b.n_nodes - b.n_tenants;
    b.n_tokens = h.dict_h.entries.size();
    b.ms_total = ms;
    return b;
}

int retain_load_host(bmq_engine* e, std::vector<RetainIndexHost::Item>&& items, uint32_t fallback) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n_items = items.size();
    if (!e->rhost.rebuild(std::move(items))) return set_err(e, BMQ_E_INVAL, e->rhost.error);
    e->rb_serving = false;
    const int rc = retain_publish(e); // (ends in a synchronise)
    e->rbinfo = host_build_info(e->rhost, n_items, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(), fallback);
    return rc;
}

// the executor builder over the caller's packed items; *too_deep: it declined (a topic of more than RB_MAX_DEPTH levels), nothing was changed
int retain_load_exec(bmq_engine* e, const RbInput& in, bool* too_deep) {
    *too_deep = false;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    return with_retain_next(e, [&](auto&, auto* rb, auto&, auto&) {
        if (!rb->build(in)) {
            if (!rb->too_deep) return set_err(e, retain_rc(rb->error), rb->error);
            *too_deep = true;
            return (int)BMQ_OK;
        }
        retain_catalogue(e->rhost, in, *rb);
        e->rb_serving = true;
        const int rc = retain_publish(e);
        e->rbinfo = rb->info;
        return rc;
    });
}

// a bulk load of host strings (bmq_retain_compact, bmq_retain_import into an empty engine) with the configured builder
int retain_load_items(bmq_engine* e, std::vector<RetainIndexHost::Item>&& items) {
    if (!e->drb && !e->hrb) return retain_load_host(e, std::move(items), 0);
    PackedTopics P;
    for (const auto& it : items)
        if (!P.add(it.tenant, it.topic, it.has_ts, it.ts, it.expiry)) return set_err(e, BMQ_E_RANGE, "the topics of the load exceed 4 GiB");
    P.pad();
    bool too_deep = false;
    const int rc = retain_load_exec(e, P.rb_input(), &too_deep);
    if (!too_deep) return rc;
    return retain_load_host(e, std::move(items), 1);
}

// a bulk load (rebuild / compact) has produced a new RetainIndexHost: a new generation of topic ids
int retain_publish(bmq_engine* e) {
    int rc = upload_retain(e);
    if (rc) return rc;
    e->rbuilt = true;
    e->repoch++;
    e->rgeneration++;
    return BMQ_OK;
}

// row pointers of a match(limit, now) batch: exclusive scan of kept[0 .. n] (entry n is zeroed here), the total into *total
int limit_rowptr(bmq_engine* e, uint32_t* kept, uint32_t n, uint32_t* row_ptr, unsigned long long* total, hipStream_t s) {
    HIPCHK(e, hipMemsetAsync(kept + n, 0, sizeof(uint32_t), s));
    size_t bytes = 0;
    HIPCHK(e, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, kept, row_ptr, (int)n + 1, s));
    if (!e->dx.ensure_tmp(bytes)) return set_err(e, BMQ_E_NOMEM, e->dx.err);
    HIPCHK(e, hipcub::DeviceScan::ExclusiveSum(e->dx.tmp, bytes, kept, row_ptr, (int)n + 1, s));
    hipLaunchKernelGGL(k_limit_total, dim3(1), dim3(64), 0, s, row_ptr, n, total);
    return BMQ_OK;
}

int launch_retain(bmq_engine* e, RetainArgs& r, BatchArgs& a) {
    r.ix = e->rdev.view;
    r.ix.dyn = e->drt->view(); // what bmq_retain_apply* changed since the bulk load
    r.ix.expire_at = e->drt->expire_at();
    // k_retain_walk (bmq_rwalk_kernel.h: RW_G filters per wave at a time, persistent waves) walks the bulk-loaded index.  Topics added since
    // the bulk load (the overlay trie) are matched by k_retain_overlay at the same time on a side stream, into a range list of their own.
    // Every kernel behind the walks reads both lists -- k_limit_select (match(limit, now)) since round 6.
    const bool ov_split = r.ix.dyn.ov_live != 0;
    if (e->rw_waves == 0) { // resident one-wave workgroups of the kernel on this device
        int per_cu = 0;
        hipDeviceProp_t prop;
        HIPCHK(e, hipGetDeviceProperties(&prop, e->device));
        HIPCHK(e, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_retain_walk<RW_G, false>, 64, 0));
        e->rw_waves = (uint32_t)std::max(1, per_cu) * (uint32_t)std::max(1, prop.multiProcessorCount);
        if (const char* v = bmq_env("BMQ_RW_WAVES")) e->rw_waves = std::max(1, atoi(v));
    }
    const uint32_t grid = std::max(1u, std::min<uint32_t>((r.n_filters + RW_G - 1) / RW_G, e->rw_waves)); // persistent waves: what fits the chip at once
    if (e->rgcap == 0) e->rgcap = 8192;
    if (e->rwcap == 0) e->rwcap = 1024;
    constexpr uint32_t DEEP_WAVES = 64, DEEP_MAXL = 32768; // a filter of 65535 bytes has at most 32768 levels
    const uint32_t ov_grid = std::max(1u, std::min<uint32_t>(r.n_filters, 256u * R_WAVES_PER_CU));
    HIPCHK(e, e->r_scratch.ensure(sizeof(uint2) * 2ull * e->rgcap * (ov_split ? std::max(ov_grid, DEEP_WAVES) : DEEP_WAVES)));
    r.gscratch = e->r_scratch.as<uint2>();
    r.gcap = e->rgcap;
    {
        HIPCHK(e, e->r_arena.ensure(sizeof(uint32_t) * 2ull * RW_G * e->rwcap * grid));
        // every wave holds a chunk of `pairs` (RW_CHUNK entries, one atomic per chunk): room for a few chunks per wave in every slice
        const uint64_t want = (uint64_t)N_SUB * ((grid + N_SUB - 1) / N_SUB) * 4ull * RW_CHUNK;
        if (e->cur->pair_cap < want && want < 0xFFFFFFFFull) {
            e->cur->pair_cap = want;
            HIPCHK(e, e->cur->b_pairs.ensure(sizeof(MatchRange) * e->cur->pair_cap));
        }
    }
    r.rw_arena = e->r_arena.as<uint32_t>();
    r.rw_cap = e->rwcap;
    HIPCHK(e, e->r_deep_list.ensure(sizeof(uint32_t) * std::max(r.n_filters, 1u)));
    r.deep_list = e->r_deep_list.as<uint32_t>();
    r.deep_levels = nullptr;
    r.deep_maxl = 0;
    if (e->rdeep_on) {
        HIPCHK(e, e->r_deep_levels.ensure(sizeof(uint32_t) * 6ull * (DEEP_MAXL + 1) * DEEP_WAVES));
        r.deep_levels = e->r_deep_levels.as<uint32_t>();
        r.deep_maxl = DEEP_MAXL;
    }
    e->cur->ran_rdeep = e->rdeep_on;
    a.ix = DistIndexView{};
    a.n_topics = r.n_filters;
    a.tpw_shift = 6;
    a.n_blocks = (a.n_topics + 63) / 64;
    a.pair_off = e->cur->b_pair_off.as<uint32_t>();
    a.pair_cnt = e->cur->b_pair_cnt.as<uint32_t>();
    a.route_cnt = e->cur->b_route_cnt.as<uint32_t>();
    a.pairs = e->cur->b_pairs.as<MatchRange>();
    a.pair_cap = e->cur->pair_cap;
    a.subs = e->cur->b_subs.as<SubAlloc>();
    a.super_sums = e->cur->b_super.as<unsigned long long>();
    a.blk_stats = nullptr;
    a.heavy_list = nullptr, a.heavy_cap = 0; // (k_expand's splitting of heavy blocks is the dist direction's: bmq_batch_args.h)
    a.wave_sums = e->cur->b_wave_sums.as<unsigned long long>();
    a.sort_list = e->cur->b_sort_list.as<uint32_t>();
    a.sort_cap = e->cur->sort_cap;
    a.ctr = e->cur->b_ctr.as<Counters>();
    hipStream_t s = e->stream;
    e->cur->clean = false; // this batch leaves the slot's counters behind: a dist batch after it resets them first
    HIPCHK(e, hipMemsetAsync(a.ctr, 0, sizeof(Counters), s));
    HIPCHK(e, hipMemsetAsync(a.subs, 0, sizeof(SubAlloc) * 2 * N_SUB, s));
    HIPCHK(e, hipMemsetAsync(a.super_sums, 0, sizeof(unsigned long long) * SUPER_STRIDE * ((a.n_blocks >> SUPER_SHIFT) + 1), s));
    e->cur->timed = e->kernel_events;
    HIPCHK(e, hipEventRecord(e->cur->ev[0], s));
    if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[1], s));
    RetainOvList ov{nullptr, nullptr, nullptr, nullptr};
    if (ov_split) { // the overlay's walk, beside the bulk-loaded index's: its own range list (the second half of the slot's allocators hands it out)
        e->ov_pair_cap = std::max<uint64_t>(e->ov_pair_cap, std::max<uint64_t>(1u << 16, (uint64_t)r.n_filters * 16));
        HIPCHK(e, e->r_ov_off.ensure(sizeof(uint32_t) * std::max(r.n_filters, 1u)));
        HIPCHK(e, e->r_ov_cnt.ensure(sizeof(uint32_t) * std::max(r.n_filters, 1u)));
        HIPCHK(e, e->r_ov_route.ensure(sizeof(uint32_t) * std::max(r.n_filters, 1u)));
        HIPCHK(e, e->r_ov_pairs.ensure(sizeof(MatchRange) * e->ov_pair_cap));
        if (!e->s_side) {
            HIPCHK(e, hipStreamCreateWithFlags(&e->s_side, hipStreamNonBlocking));
            HIPCHK(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
            HIPCHK(e, hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
        }
        BatchArgs ao = a;
        ao.pair_off = e->r_ov_off.as<uint32_t>();
        ao.pair_cnt = e->r_ov_cnt.as<uint32_t>();
        ao.route_cnt = e->r_ov_route.as<uint32_t>();
        ao.pairs = e->r_ov_pairs.as<MatchRange>();
        ao.pair_cap = e->ov_pair_cap;
        ao.subs = a.subs + N_SUB;
        ov = RetainOvList{ao.pair_off, ao.pair_cnt, ao.route_cnt, ao.pairs};
        HIPCHK(e, hipEventRecord(e->ev_fork, s));
        HIPCHK(e, hipStreamWaitEvent(e->s_side, e->ev_fork, 0));
        hipLaunchKernelGGL(k_retain_overlay, dim3(ov_grid), dim3(64), 0, e->s_side, r, ao);
        HIPCHK(e, hipEventRecord(e->ev_join, e->s_side));
    }
    if (r.ix.dyn.use_dead) hipLaunchKernelGGL((k_retain_walk<RW_G, true>), dim3(grid), dim3(64), 0, s, r, a);
    else hipLaunchKernelGGL((k_retain_walk<RW_G, false>), dim3(grid), dim3(64), 0, s, r, a);
    if (ov_split) HIPCHK(e, hipStreamWaitEvent(s, e->ev_join, 0));
    // filters of more than R_MAXL levels: listed by the walk, answered by the same walk with its per-level arrays in global memory --
    // in the pipeline only while batches hold such filters (retain_finish turns it on and runs the batch that found out again)
    if (e->rdeep_on) hipLaunchKernelGGL(k_retain_walk_deep, dim3(DEEP_WAVES), dim3(64), 0, s, r, a);
    hipLaunchKernelGGL(k_retain_sums, dim3(a.n_blocks), dim3(64), 0, s, a, ov);
    if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[2], s));
    if (e->rlim.active) { // RetainStoreCoProc.match(limit, now): the first `limit` live ids straight from the matched ranges
        const RetainLimit& L = e->rlim;
        if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[3], s));
        hipLaunchKernelGGL(k_limit_select, dim3(std::max(1u, std::min<uint32_t>(r.n_filters, 8192u))), dim3(64), 0, s, a, ov, L.d_limit,
                           r.ix.expire_at, (unsigned long long)L.now, r.n_filters, L.d_tmp, L.d_kept, L.d_counts);
        if (int rc = limit_rowptr(e, L.d_kept, r.n_filters, a.out_row_ptr, &a.ctr->total_ids, s)) return rc;
        hipLaunchKernelGGL(k_limit_compact, dim3((r.n_filters + 255) / 256), dim3(256), 0, s, L.d_tmp, a.out_row_ptr, r.n_filters, a.out_ids);
        if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[4], s));
    } else {
        if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[3], s));
        // bulk-loaded topics removed since the load keep their ids inside the matched ranges: the dead-aware expansion drops them
        if (r.ix.dyn.use_dead || ov_split) { // (two range lists, or ids to drop: the plain k_expand knows neither)
            hipLaunchKernelGGL(k_retain_rowptr_dyn, dim3(a.n_blocks), dim3(64), 0, s, a, ov);
            hipLaunchKernelGGL(k_retain_expand_dyn, dim3((r.n_filters + RXD_WAVES - 1) / RXD_WAVES), dim3(RXD_WAVES * 64), 0, s, a, ov, r.ix.dyn.dead_bits,
                               r.ix.dyn.dead_rank, r.ix.dyn.use_dead ? r.ix.dyn.base_n : 0u);
        }
        else hipLaunchKernelGGL(k_expand, dim3(a.n_blocks), dim3(64), 0, s, a);
        if (e->kernel_events) HIPCHK(e, hipEventRecord(e->cur->ev[4], s));
        hipLaunchKernelGGL(k_sort_rows, dim3(1024), dim3(256), 0, s, a);
    }
    HIPCHK(e, hipEventRecord(e->cur->ev[5], s));
    HIPCHK(e, hipMemcpyAsync(e->cur->h_ctr, a.ctr, sizeof(Counters), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipGetLastError());
    e->cur->last = a;
    e->cur->rlast = r;
    e->cur->pending = true;
    e->cur->pending_kind = 1;
    return BMQ_OK;
}

} // namespace

static int retain_finish(bmq_engine* e, uint64_t* out_total) {
    const auto rerun = [&] { // the same batch once more, with what this function has grown or switched on
        RetainArgs r = e->cur->rlast;
        BatchArgs a = e->cur->last;
        return launch_retain(e, r, a);
    };
    for (int attempt = 0; attempt < 16; attempt++) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        const Counters c = *e->cur->h_ctr;
        if (c.status & ST_RETAIN_DEEP) {
            e->cur->pending = false;
            return set_err(e, BMQ_E_RANGE, "a filter has more levels than a 64 KB filter can have");
        }
        if (c.slow_count && !e->cur->ran_rdeep) { // filters of more than R_MAXL levels and the deep pass was not in the pipeline: once more with it
            e->rdeep_on = true, e->rdeep_idle = 0;
            if (int rc = rerun()) return rc;
            continue;
        }
        if (e->cur->ran_rdeep && (c.slow_count ? (e->rdeep_idle = 0) : ++e->rdeep_idle) >= REPAIR_IDLE_BATCHES) e->rdeep_on = false;
        const uint32_t grow = c.status & (ST_NEED_PAIRS | ST_NEED_SPILL | ST_RETAIN_FRONT | ST_RETAIN_LIST | ST_NEED_SORTLIST);
        if (grow) {
            if (grow & ST_NEED_SPILL) { // k_retain_overlay's range list (one entry per matched overlay topic: it can be long)
                e->ov_pair_cap *= 4;
                if (e->ov_pair_cap >= 0xFFFFFFFFull) return set_err(e, BMQ_E_RANGE, "the overlay's matched-range buffer exceeds 2^32 entries");
            }
            int rc;
            if ((grow & ST_NEED_PAIRS) && (rc = grow_pairs(e, *e->cur))) return rc;
            if (grow & ST_RETAIN_FRONT) {
                if (e->rgcap >= (1u << 24)) return set_err(e, BMQ_E_RANGE, "retain frontier exceeds 16M ranges");
                e->rgcap *= 4;
            }
            if (grow & ST_RETAIN_LIST) {
                if (e->rwcap >= (1u << 22)) return set_err(e, BMQ_E_RANGE, "retain frontier list exceeds 4M nodes");
                e->rwcap *= 4;
            }
            if ((grow & ST_NEED_SORTLIST) && (rc = grow_sort_list(e, *e->cur, c.sort_count))) return rc;
            if ((rc = rerun())) return rc;
            continue;
        }
        e->cur->pending = false;
#if BMQ_RW_CLOCKS
        if (bmq_env("BMQ_DEBUG") && (atoi(bmq_env("BMQ_DEBUG")) & 64)) { // phase clocks of the last k_retain_walk launch (profiling builds only)
            unsigned long long h[24] = {0}, z[24] = {0};
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_rw_clk), sizeof(h));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rw_clk), z, sizeof(z));
            if (const char* fn = bmq_env("BMQ_RW_WAVE_FILE")) { // per-wave records for offline analysis
                std::vector<uint4> wv(16384);
                (void)hipMemcpyFromSymbol(wv.data(), HIP_SYMBOL(g_rw_wave), sizeof(uint4) * wv.size());
                if (FILE* f = fopen(fn, "wb")) {
                    fwrite(wv.data(), sizeof(uint4), std::min<size_t>(wv.size(), h[0]), f);
                    fclose(f);
                }
            }
            if (h[0])
                fprintf(stderr, "[bmq] k_retain_walk: %llu waves, %.2f groups/wave, %.1f rounds/group, %.1f units/round, cold probe loop in %.0f %% of the rounds; ticks/wave: all %.0f (slowest %llu), tokenise %.0f, fetch waits %.0f, cold loops %.0f | round segments: hand-out + unit %.0f, found + '+' (incl. cold) %.0f, emission %.0f, hand-over %.0f, reserve %.0f | inside hand-out: bulk set-up %.0f, lanes <- units %.0f, slot state %.0f, entry + tenant + addresses %.0f\n",
                        h[0], (double)h[1] / h[0], (double)h[2] / std::max(1ull, h[1]), (double)h[3] / std::max(1ull, h[2]), 100.0 * h[4] / std::max(1ull, h[2]), (double)h[5] / h[0], h[9],
                        (double)h[6] / h[0], (double)h[7] / h[0], (double)h[8] / h[0], (double)h[10] / h[0], (double)h[11] / h[0], (double)h[12] / h[0], (double)h[13] / h[0], (double)h[14] / h[0], (double)h[15] / h[0], (double)h[16] / h[0], (double)h[17] / h[0], (double)h[18] / h[0]);
        }
#endif
        bmq_stats& st = e->stats;
        st = bmq_stats{};
        st.n_topics = e->cur->rlast.n_filters;
        st.n_visit = c.n_visit;
        st.n_match = c.total_ids;
        st.n_ranges = c.n_ranges;
        st.n_sorted_rows = c.sort_count;
        st.topic_bytes = c.topic_bytes;
        (void)hipEventElapsedTime(&st.ms_total, e->cur->ev[0], e->cur->ev[5]);
        if (e->cur->timed) {
            (void)hipEventElapsedTime(&st.ms_walk, e->cur->ev[1], e->cur->ev[2]);
            (void)hipEventElapsedTime(&st.ms_expand, e->cur->ev[3], e->cur->ev[4]);
        }
        if (out_total) *out_total = c.total_ids;
        if (c.status & ST_RANGE) return set_err(e, BMQ_E_RANGE, "batch produced >= 2^32 topic ids");
        if (c.status & ST_NOSPACE) return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
        return BMQ_OK;
    }
    return set_err(e, BMQ_E_NOMEM, "scratch growth did not converge");
}

extern "C" {

int bmq_retain_rebuild_ex(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                          const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics,
                          const uint64_t* timestamp_hlc, const uint32_t* expiry_seconds) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || (n_topics && (!tenants || !tenant_off || !topic_tenant || !topics || !topic_off))) return BMQ_E_INVAL;
    if ((timestamp_hlc == nullptr) != (expiry_seconds == nullptr)) return set_err(e, BMQ_E_INVAL, "timestamps and expiry intervals come together");
    std::lock_guard<std::mutex> g(e->mu);
    for (uint32_t i = 0; i < n_topics; i++)
        if (topic_tenant[i] >= n_tenants) return set_err(e, BMQ_E_INVAL, "topic_tenant index out of range");
    if (e->cur->pending) return set_err(e, BMQ_E_STATE, "a batch is in flight: call bmq_match_finish first");
    if (e->rcmp.active) return set_err(e, BMQ_E_STATE, "a retain compaction is running: bmq_retain_compact_swap or bmq_retain_compact_abort first");
    uint32_t fallback = 0;
    if (e->drb || e->hrb) { // bmq_config.retain_builder = 1: the caller's packed items go to the executor as they are
        const RbInput in{tenants, tenant_off, n_tenants, topic_tenant, topics, topic_off, n_topics, timestamp_hlc, expiry_seconds};
        bool too_deep = false;
        const int rc = retain_load_exec(e, in, &too_deep);
        if (!too_deep) return rc;
        fallback = 1;
    }
    return retain_load_host(e, PackedTopics::items(n_topics, PackedTopics::by_table(tenants, tenant_off, topic_tenant, topics, topic_off), timestamp_hlc, expiry_seconds), fallback);
}

int bmq_retain_rebuild(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                       const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics) {
    return bmq_retain_rebuild_ex(e, tenants, tenant_off, n_tenants, topic_tenant, topics, topic_off, n_topics, nullptr, nullptr);
}

// ops the serving generation has taken enter the log of the compaction that runs beside it (under e->mu)
static void retain_log(bmq_engine::RetainCompaction& c, std::vector<bmq_engine::RetainCompaction::Op>& ops) {
    for (auto& o : ops) {
        c.log_bytes += o.tenant.size() + o.topic.size() + 48;
        c.log.push_back(std::move(o));
    }
    if (c.log_bytes > (1ull << 30)) { // (what gives way is the compaction, never the mutation)
        c.log_overflow = true;
        c.log.clear(), c.log.shrink_to_fit();
    }
}
// IRetainTopicIndex.add / remove for a batch of (tenant, topic) pairs: three kernels on the engine stream (locate, commit, rank:
// bmq_retain_core.h), behind whatever match batch is in flight and in front of every later one.  Ids are stable: a removed topic's id
// goes dead, a re-added one gets its id back, a new topic gets the next unused id.
static int retain_apply_common(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                               const uint8_t* topics, const uint32_t* topic_off, const uint8_t* op, const uint64_t* timestamp_hlc,
                               const uint32_t* expiry_seconds, uint32_t n, uint32_t* out_ids) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || (n && (!topics || !topic_off || !op || !tenants || !tenant_off || n_tenants == 0))) return BMQ_E_INVAL;
    if ((timestamp_hlc == nullptr) != (expiry_seconds == nullptr)) return set_err(e, BMQ_E_INVAL, "timestamps and expiry intervals come together");
    std::lock_guard<std::mutex> g(e->mu);
    if (n == 0) return BMQ_OK;
    for (uint32_t i = 0; i < n; i++) { // nothing is changed by a batch that holds a malformed op
        if (op[i] > 1) return set_err(e, BMQ_E_INVAL, "op must be 0 (add) or 1 (remove)");
        if (op_tenant && op_tenant[i] >= n_tenants) return set_err(e, BMQ_E_INVAL, "op_tenant index out of range");
    }
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    if (!e->rbuilt) { // the first retained message of a fresh range: start from an empty bulk load
        const int rc = retain_load_host(e, {}, 0); // (nothing to build: the host builder, whatever bmq_config.retain_builder says)
        if (rc) return rc;
    }
    const bool ok = retain_try(e, [&](auto& rt) { return rt.apply(tenants, tenant_off, n_tenants, op_tenant, topics, topic_off, op, (const unsigned long long*)timestamp_hlc, expiry_seconds, n, out_ids); });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    if (e->rcmp.active && !e->rcmp.log_overflow) { // a generation is being built beside this one: it gets the ops too, before the swap
        std::vector<bmq_engine::RetainCompaction::Op> ops(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t ti = op_tenant ? op_tenant[i] : 0u;
            ops[i] = {std::string((const char*)tenants + tenant_off[ti], tenant_off[ti + 1] - tenant_off[ti]), std::string((const char*)topics + topic_off[i], topic_off[i + 1] - topic_off[i]),
                      op[i], timestamp_hlc != nullptr, timestamp_hlc ? timestamp_hlc[i] : 0ull, expiry_seconds ? expiry_seconds[i] : 0xFFFFFFFFu};
        }
        retain_log(e->rcmp, ops);
    }
    e->repoch++;
    return BMQ_OK;
}

int bmq_retain_apply_batch(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                           const uint8_t* topics, const uint32_t* topic_off, const uint8_t* op, const uint64_t* timestamp_hlc,
                           const uint32_t* expiry_seconds, uint32_t n, uint32_t* out_topic_ids) {
    return retain_apply_common(e, tenants, tenant_off, n_tenants, op_tenant, topics, topic_off, op, timestamp_hlc, expiry_seconds, n, out_topic_ids);
}

int bmq_retain_apply_ex(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics, const uint32_t* topic_off,
                        const uint8_t* op, const uint64_t* timestamp_hlc, const uint32_t* expiry_seconds, uint32_t n) {
    const uint32_t toff[2] = {0, tenant_len};
    static const uint8_t none[1] = {0};
    return retain_apply_common(e, tenant ? tenant : none, toff, 1, nullptr, topics, topic_off, op, timestamp_hlc, expiry_seconds, n, nullptr);
}

int bmq_retain_apply(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics,
                     const uint32_t* topic_off, const uint8_t* op, uint32_t n) {
    return bmq_retain_apply_ex(e, tenant, tenant_len, topics, topic_off, op, nullptr, nullptr, n);
}

int bmq_retain_topic_info(const bmq_engine* ce, uint32_t topic_id, uint64_t* out_timestamp_hlc, uint32_t* out_expiry_seconds, uint64_t* out_expire_at_ms) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->rbuilt) return BMQ_E_INVAL;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    unsigned long long ts = 0, at = 0;
    uint32_t ex = 0;
    bool live = false;
    const bool ok = with_retain(e, [&](auto& rt) { return rt.topic_info(topic_id, ts, ex, at, live); });
    if (!ok || !live) return BMQ_E_INVAL; // never handed out, or its topic is not retained any more
    if (out_timestamp_hlc) *out_timestamp_hlc = ts;
    if (out_expiry_seconds) *out_expiry_seconds = ex;
    if (out_expire_at_ms) *out_expire_at_ms = at;
    return BMQ_OK;
}

int bmq_retain_info_get(const bmq_engine* ce, bmq_retain_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out) return BMQ_E_INVAL;
    memset(out, 0, sizeof(*out));
    out->epoch = e->repoch;
    out->generation = e->rgeneration;
    if (!e->rbuilt) return BMQ_OK;
    const RetainDynInfo& in = retain_dyn_info(e);
    out->n_topics = in.n_live;
    out->id_bound = in.id_bound;
    out->loaded_topics = in.base_n;
    out->loaded_removed = in.base_dead;
    out->added_ids = in.overlay_ids;
    out->overlay_nodes = in.overlay_nodes;
    out->n_tenants = e->rhost.n_tenants();
    return BMQ_OK;
}

int bmq_retain_build_info_get(const bmq_engine* ce, bmq_retain_build_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out) return BMQ_E_INVAL;
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->rbuilt) return set_err(e, BMQ_E_STATE, "no retained-topic index");
    const RetainBuildInfo& b = e->rbinfo;
    out->builder = b.builder;
    out->fallback = b.fallback;
    out->n_items = b.n_items;
    out->n_topics = b.n_topics;
    out->n_tenants = b.n_tenants;
    out->n_nodes = b.n_nodes;
    out->n_edges = b.n_edges;
    out->n_edge_overflows = b.n_edge_overflows;
    out->n_posts = b.n_posts;
    out->n_gp_runs = b.n_gp_runs;
    out->n_tokens = b.n_tokens;
    out->max_depth = b.max_depth;
    out->ms_total = b.ms_total;
    out->ms_sort = b.ms_sort;
    out->n_gp_overflows = (uint32_t)b.n_gp_overflows;
    return BMQ_OK;
}

// IRetainTopicIndex.findAll() (RS/index/RetainTopicIndex.java:140-143): the count; bmq_retain_live_ids lists the ids
int bmq_retain_find_all(const bmq_engine* ce, uint64_t* out_n_topics, uint64_t* out_epoch) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_n_topics) return BMQ_E_INVAL;
    *out_n_topics = e->rbuilt ? retain_dyn_info(e).n_live : 0;
    if (out_epoch) *out_epoch = e->repoch;
    return BMQ_OK;
}

// ids the query accepts, ascending (one flag kernel over the ids + a device select)
static int retain_select(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, GcQuery q, uint32_t* out_ids, uint32_t cap, uint32_t* out_n) {
    *out_n = 0;
    if (!e->rbuilt) return BMQ_OK;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    if (tenant) { // the tenant's bulk-loaded rank range, and inside it the ranks below '$' first levels
        q.has_tenant = 1;
        auto f = e->rhost.by_name.find(std::string((const char*)tenant, tenant_len));
        if (f != e->rhost.by_name.end()) {
            const RTenantState& t = *f->second;
            q.t_lo = t.id_base;
            q.t_hi = t.id_base + (uint32_t)t.topics.size();
            q.sys_lo = t.id_base + t.sys_id_lo;
            q.sys_hi = t.id_base + t.sys_id_hi;
        }
        q.t_node = NONE;
    }
    std::vector<uint32_t> ids;
    const bool ok = retain_try(e, [&](auto& rt) { return rt.select(q, tenant, tenant_len, ids); });
    if (!ok) return set_err(e, BMQ_E_HIP, e->err);
    *out_n = (uint32_t)ids.size();
    for (size_t i = 0; i < ids.size() && i < cap && out_ids; i++) out_ids[i] = ids[i];
    return ids.size() > cap ? BMQ_E_NOSPACE : BMQ_OK;
}

// The GC scan of RetainStoreCoProc (RS/RetainStoreCoProc.java:257-277): with a tenant the reference scans index.match(tenantId, "#"),
// which does not reach topics whose first level starts with '$' (RetainTopicIndex.java:60,86,99) -- neither does this; without one it
// scans findAll(): every retained topic.  override_expiry_seconds >= 0 replaces the stored interval (GCRequest.expirySeconds).
int bmq_retain_expired(const bmq_engine* ce, const uint8_t* tenant, uint32_t tenant_len, uint64_t now_ms, int64_t override_expiry_seconds,
                       uint32_t* out_ids, uint32_t cap, uint32_t* out_n) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_n) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    GcQuery q{};
    q.now = now_ms;
    q.override_expiry = override_expiry_seconds;
    q.skip_sys = 1;
    return retain_select(e, tenant, tenant_len, q, out_ids, cap, out_n);
}

int bmq_retain_live_ids(const bmq_engine* ce, const uint8_t* tenant, uint32_t tenant_len, uint32_t* out_ids, uint32_t cap, uint32_t* out_n) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_n) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    GcQuery q{};
    q.live_only = 1;
    q.override_expiry = -1;
    return retain_select(e, tenant, tenant_len, q, out_ids, cap, out_n);
}

// ids -> tenant id + topic, many at once: bulk-loaded ids from the host's copy of the load, overlay ids with ONE device gather
static int retain_topics_locked(bmq_engine* e, const uint32_t* ids, uint32_t n, std::vector<uint8_t>& bytes, std::vector<uint64_t>& off, std::vector<uint32_t>& tlen) {
    off.assign((size_t)n + 1, 0);
    tlen.assign(n, 0);
    bytes.clear();
    if (!e->rbuilt) return BMQ_OK;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const uint64_t base_n = retain_dyn_info(e).base_n;
    std::vector<uint32_t> ov_ids, ov_pos;
    for (uint32_t i = 0; i < n; i++)
        if (ids[i] >= base_n) {
            ov_ids.push_back(ids[i]);
            ov_pos.push_back(i);
        }
    std::vector<uint32_t> lens;
    std::vector<uint8_t> ov_bytes;
    if (!ov_ids.empty()) {
        const bool ok = retain_try(e, [&](auto& rt) { return rt.overlay_topics(ov_ids.data(), (uint32_t)ov_ids.size(), lens, ov_bytes); });
        if (!ok) return set_err(e, BMQ_E_HIP, e->err);
    }
    size_t k = 0, ov_off = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (ids[i] < base_n) {
            std::string_view tn, tp;
            if (e->rhost.topic(ids[i], tn, tp)) {
                bytes.insert(bytes.end(), tn.begin(), tn.end());
                bytes.insert(bytes.end(), tp.begin(), tp.end());
                tlen[i] = (uint32_t)tn.size();
            }
        } else {
            const uint32_t total = lens[2 * k + 1];
            bytes.insert(bytes.end(), ov_bytes.begin() + (long)ov_off, ov_bytes.begin() + (long)(ov_off + total));
            tlen[i] = lens[2 * k];
            ov_off += total;
            k++;
        }
        off[i + 1] = bytes.size();
    }
    return BMQ_OK;
}

int bmq_retain_topics(const bmq_engine* ce, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off, uint32_t* out_tenant_len) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_off || (n && !topic_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> tlen;
    const int rc = retain_topics_locked(e, topic_ids, n, bytes, off, tlen);
    if (rc) return rc;
    memcpy(out_off, off.data(), sizeof(uint64_t) * ((size_t)n + 1));
    if (out_tenant_len && n) memcpy(out_tenant_len, tlen.data(), sizeof(uint32_t) * n);
    if (off[n] > cap || (off[n] && !out)) return BMQ_E_NOSPACE;
    if (off[n]) memcpy(out, bytes.data(), off[n]);
    return BMQ_OK;
}

int bmq_retain_topic(const bmq_engine* ce, uint32_t topic_id, uint8_t* out, uint32_t cap, uint32_t* out_len,
                     uint32_t* out_tenant_len) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_len || !out_tenant_len) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> tlen;
    const int rc = retain_topics_locked(e, &topic_id, 1, bytes, off, tlen);
    if (rc) return rc;
    if (off[1] == 0) return BMQ_E_INVAL; // no id of this generation (a topic has at least a tenant or a level byte... or both empty: not retainable)
    *out_len = (uint32_t)off[1];
    *out_tenant_len = tlen[0];
    if (*out_len > cap) return BMQ_E_NOSPACE;
    if (out) memcpy(out, bytes.data(), off[1]);
    return BMQ_OK;
}

// liveness of ids: the dead bitmap over the ids handed out (a bit per id: 128 KB per million ids), one copy
static int retain_dead_words_locked(bmq_engine* e, std::vector<unsigned long long>& words) {
    const bool ok = retain_try(e, [&](auto& rt) { return rt.dead_words(words); });
    return ok ? BMQ_OK : set_err(e, BMQ_E_HIP, e->err);
}

int bmq_retain_message_keys(const bmq_engine* ce, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_off || (n && !topic_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    std::vector<uint64_t> koff((size_t)n + 1, 0);
    std::vector<uint8_t> keys;
    if (e->rbuilt && n) {
        std::vector<unsigned long long> dead;
        if (int rc = retain_dead_words_locked(e, dead)) return rc;
        const uint64_t bound = retain_dyn_info(e).id_bound;
        std::vector<uint32_t> live; // (positions keep their order: the keys are composed id for id below)
        for (uint32_t i = 0; i < n; i++)
            if (topic_ids[i] < bound && !((dead[topic_ids[i] >> 6] >> (topic_ids[i] & 63u)) & 1ull)) live.push_back(topic_ids[i]);
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off;
        std::vector<uint32_t> tlen;
        if (int rc = retain_topics_locked(e, live.data(), (uint32_t)live.size(), bytes, off, tlen)) return rc;
        size_t k = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (k < live.size() && topic_ids[i] < bound && !((dead[topic_ids[i] >> 6] >> (topic_ids[i] & 63u)) & 1ull)) {
                const std::string_view tn((const char*)bytes.data() + off[k], tlen[k]), tp((const char*)bytes.data() + off[k] + tlen[k], (size_t)(off[k + 1] - off[k]) - tlen[k]);
                if (off[k + 1] != off[k]) {
                    const std::string key = retain_message_key(tn, tp);
                    keys.insert(keys.end(), key.begin(), key.end());
                }
                k++;
            }
            koff[i + 1] = keys.size();
        }
    }
    memcpy(out_off, koff.data(), sizeof(uint64_t) * ((size_t)n + 1));
    if (koff[n] > cap || (koff[n] && !out)) return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
    if (koff[n]) memcpy(out, keys.data(), koff[n]);
    return BMQ_OK;
}

int bmq_retain_remove_ids(bmq_engine* e, const uint32_t* topic_ids, uint32_t n, uint64_t generation, uint64_t* out_removed) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || (n && !topic_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (out_removed) *out_removed = 0;
    if (!e->rbuilt || generation != e->rgeneration) return set_err(e, BMQ_E_STATE, "the topic ids belong to another generation of the retained-topic index");
    const uint64_t bound = retain_dyn_info(e).id_bound;
    for (uint32_t i = 0; i < n; i++) // nothing is changed by a call that holds an id nobody handed out
        if (topic_ids[i] >= bound) return set_err(e, BMQ_E_INVAL, "topic id out of range (>= bmq_retain_info.id_bound)");
    if (n == 0) return BMQ_OK;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    // a generation is being built beside this one: it gets the removals as remove ops of the topics.  The ops are made ready here (the ids
    // that are live now, once each, with their strings) and enter the log only after the removal has succeeded, as in retain_apply_common
    std::vector<bmq_engine::RetainCompaction::Op> log_ops;
    if (e->rcmp.active && !e->rcmp.log_overflow) {
        std::vector<unsigned long long> dead;
        if (int rc = retain_dead_words_locked(e, dead)) return rc;
        std::vector<uint32_t> live;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t id = topic_ids[i];
            if ((dead[id >> 6] >> (id & 63u)) & 1ull) continue;
            dead[id >> 6] |= 1ull << (id & 63u); // (a repeat inside the call is logged once)
            live.push_back(id);
        }
        std::vector<uint8_t> bytes;
        std::vector<uint64_t> off;
        std::vector<uint32_t> tlen;
        if (int rc = retain_topics_locked(e, live.data(), (uint32_t)live.size(), bytes, off, tlen)) return rc;
        for (size_t i = 0; i < live.size(); i++)
            log_ops.push_back({std::string((const char*)bytes.data() + off[i], tlen[i]), std::string((const char*)bytes.data() + off[i] + tlen[i], (size_t)(off[i + 1] - off[i]) - tlen[i]), 1, false, 0ull,
                               0xFFFFFFFFu});
    }
    uint64_t removed = 0;
    const bool ok = retain_try(e, [&](auto& rt) { return rt.remove_ids(topic_ids, n, removed); });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    if (e->rcmp.active && !e->rcmp.log_overflow) retain_log(e->rcmp, log_ops);
    if (out_removed) *out_removed = removed;
    e->repoch++;
    return BMQ_OK;
}

int bmq_retain_tenant_counts(const bmq_engine* ce, uint8_t* out_tenants, uint64_t tenants_cap, uint64_t* out_tenant_off, uint64_t* out_counts, uint32_t cap,
                             uint32_t* out_n_tenants, uint64_t* out_tenant_bytes) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    std::map<std::string, uint64_t> merged; // byte order of the tenant ids; a tenant with both parts comes out once
    if (e->rbuilt) {
        if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
        std::vector<uint32_t> ranges, bulk_live;
        for (const RTenantState* t : e->rhost.order) {
            ranges.push_back(t->id_base);
            ranges.push_back(t->id_base + (uint32_t)t->topics.size());
        }
        std::vector<std::pair<std::string, uint64_t>> ov;
        const bool ok = retain_try(e, [&](auto& rt) { return rt.tenant_counts(ranges, bulk_live, ov); });
        if (!ok) return set_err(e, BMQ_E_HIP, e->err);
        for (size_t i = 0; i < e->rhost.order.size(); i++)
            if (bulk_live[i]) merged[e->rhost.order[i]->name] += bulk_live[i];
        for (auto& o : ov) merged[o.first] += o.second;
    }
    std::vector<std::pair<std::string, std::array<uint64_t, 4>>> rows;
    for (auto& m : merged) rows.push_back({m.first, {m.second, 0, 0, 0}});
    return pack_names(e, rows, 1, out_tenants, tenants_cap, out_tenant_off, out_counts, cap, out_n_tenants, out_tenant_bytes);
}

// Maintenance: merge what bmq_retain_apply* changed into a fresh bulk load -- removed topics and their ids go, overlay topics become
// ranks again (every subtree one id range: the fast path of '+' and '#').  A new generation of ids.
// the live retained topics with their stamps, as bmq_retain_rebuild_ex takes them (under e->mu)
// ids (ascending) of the retained topics whose retainMessageKey lies inside `b`, their number and (key_bytes != null) the sum of their key
// lengths: one pass of k_r_boundary over the ids handed out (under e->mu)
static int retain_boundary_locked(bmq_engine* e, const Boundary& b, uint64_t& topics, uint64_t* key_bytes, std::vector<uint32_t>* ids) {
    topics = 0;
    if (key_bytes) *key_bytes = 0;
    if (ids) ids->clear();
    if (!e->rbuilt) return BMQ_OK;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const bool ok = retain_try(e, [&](auto& rt) {
        return rt.boundary_select(e->rhost, b.flags, (const uint8_t*)b.start.data(), (uint32_t)b.start.size(), (const uint8_t*)b.end.data(), (uint32_t)b.end.size(),
                                  topics, key_bytes, ids);
    });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    return BMQ_OK;
}

static int retain_live_items_locked(bmq_engine* e, std::vector<RetainIndexHost::Item>& items, const Boundary& bound = Boundary{}) {
    std::vector<uint32_t> ids;
    std::vector<unsigned long long> ts;
    std::vector<uint32_t> ex;
    if (bound.bounded()) { // only the topics whose key lies inside: the predicate runs where the index lives
        uint64_t n_in = 0;
        if (int rc = retain_boundary_locked(e, bound, n_in, nullptr, &ids)) return rc;
    }
    GcQuery q{};
    q.live_only = 1;
    q.override_expiry = -1;
    const bool ok = retain_try(e, [&](auto& rt) { return (bound.bounded() || rt.select(q, nullptr, 0, ids)) && rt.payload(ts, ex); });
    if (!ok) return set_err(e, BMQ_E_HIP, e->err);
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<uint32_t> tlen;
    int rc = retain_topics_locked(e, ids.data(), (uint32_t)ids.size(), bytes, off, tlen);
    if (rc) return rc;
    items = PackedTopics::items(ids.size(), PackedTopics::by_prefix(bytes.data(), off.data(), tlen.data()), (const uint64_t*)ts.data(), ex.data(), ids.data());
    return BMQ_OK;
}

// ---- retained topics: a generation change that does not stop the world (round 6) --------------------------------------------------------
// TopicLevelTrie contracts tombed branches as it goes (UTIL/index/TopicLevelTrie.java:257-384) -- this is the index that code belongs to.
// Here removed topics leave dead ids and added ones an overlay beside the bulk-loaded part (bmq_retain_dyn.h); bmq_retain_compact folds
// both back into a fresh bulk load, but under the engine lock: 2 s for 1 M topics (the host-side load).  The three calls below take the
// load out of the lock:  begin = snapshot of the live topics (tens of ms under the lock); build = the load into an index of its own, no
// lock held, matching and bmq_retain_apply* go on (what they change is logged); swap = upload + replay of the log under the lock.
// With bmq_config.retain_builder = 3 (under 1 the three calls stay as they are) the snapshot is gathered where the index lives and stays there (RetainDyn::snapshot), build runs the
// executor builder on an executor of its own and makes the next mutable part ready (retain_build_next in bmq_retain_next.h, which knows no engine: tools/retain_snapshot_check.cpp runs that very
// function under the sanitizers), swap exchanges pointers: what the two holds of the lock copy between host and executor is a handful of words
// (bmq_retain_compact_info.locked_copy_bytes).  One body per call: the executor type comes in through with_retain_next.
int bmq_retain_compact_begin(bmq_engine* e) { return bmq_retain_compact_begin_in(e, 0, nullptr, 0, nullptr, 0); }
// bytes of host <-> exec copies the retain direction has issued so far (RetainDyn::copied + the image uploads): under e->mu
static uint64_t retain_copy_meter(bmq_engine* e) { return with_retain(e, [](auto& rt) { return rt.copied; }) + e->r_up_bytes; }
static float ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
// ... for a range that SHRINKS (RetainStoreCoProc.reset(Boundary) after a split): the snapshot takes only the topics whose key lies inside
// the boundary, and the swap replays only the logged ops whose key does.  The serving generation matches and mutates over all its topics
// until the swap.
int bmq_retain_compact_begin_in(bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len) {
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> gc(e->cmp_mu);
    std::lock_guard<std::mutex> g(e->mu);
    Boundary bound;
    if (int rc = parse_boundary(e, flags, start, start_len, end, end_len, bound)) return rc;
    if (e->rcmp.active) return set_err(e, BMQ_E_STATE, "a retain compaction is running: bmq_retain_compact_swap or bmq_retain_compact_abort first");
    if (!e->rbuilt) return set_err(e, BMQ_E_STATE, "no retained-topic index");
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t meter0 = retain_copy_meter(e);
    e->rcmp = bmq_engine::RetainCompaction{};
    bmq_engine::RetainCompaction& c = e->rcmp;
    c.bound = bound;
    if (e->rb_generation) { // bmq_config.retain_builder = 3: ids, strings and stamps are gathered where the index lives and stay there
        const int rc = with_retain_next(e, [&](auto& rt, auto*, auto& bx, auto& nx) {
            if (int rc = retain_build_stream(e, bx)) return rc;
            nx.snap = std::make_unique<std::decay_t<decltype(*nx.snap)>>(rt.x);
            if (!rt.snapshot(e->rhost, bound.flags, (const uint8_t*)bound.start.data(), (uint32_t)bound.start.size(), (const uint8_t*)bound.end.data(), (uint32_t)bound.end.size(), *nx.snap)) {
                const std::string msg = rt.error;
                e->rcmp = bmq_engine::RetainCompaction{};
                return set_err(e, retain_rc(msg), msg);
            }
            c.ci.n_items = nx.snap->s.n;
            c.ci.snapshot_bytes = nx.snap->bytes;
            return (int)BMQ_OK;
        });
        if (rc) return rc;
        c.exec_snapshot = true;
        c.ci.builder = 1;
    } else {
        if (int rc = retain_live_items_locked(e, c.items, bound)) return rc;
        c.ci.n_items = c.items.size();
        for (const auto& it : c.items) c.ci.snapshot_bytes += it.tenant.size() + it.topic.size() + 12;
    }
    c.active = true;
    c.ci.state = 1;
    c.ci.locked_copy_bytes = retain_copy_meter(e) - meter0;
    c.ci.begin_ms = ms_since(t0);
    return BMQ_OK;
}

extern "C++" {
static uint8_t retain_op_of(const bmq_engine::RetainCompaction::Op& o) { return o.op; }
static uint8_t retain_op_of(const RetainIndexHost::Item&) { return 0; } // (an item is an add)
// Logged ops / items through the ordinary apply path, 65 536 at a time.  around(n, apply) runs each chunk of n: it calls apply() and hands its
// result on.  Stamps go with a chunk if one of its entries has some, or with every chunk (always_stamps).
template <class T, class Around> static int retain_apply_chunked(bmq_engine* e, const std::vector<T>& v, bool always_stamps, Around&& around) {
    for (size_t lo = 0; lo < v.size();) {
        const size_t hi = std::min(v.size(), lo + 65536);
        PackedTopics P;
        for (size_t i = lo; i < hi; i++)
            if (!P.add(v[i].tenant, v[i].topic, v[i].has_ts, v[i].ts, v[i].expiry, retain_op_of(v[i]))) return set_err(e, BMQ_E_RANGE, "the topics of the batch exceed 4 GiB");
        P.pad();
        const bool stamps = always_stamps || P.any_ts;
        const int rc = around((uint32_t)(hi - lo), [&] {
            return retain_apply_common(e, P.tenants.data(), P.tenant_off.data(), P.n_tenants(), P.item_tenant.data(), P.topics.data(), P.topic_off.data(), P.op.data(),
                                       stamps ? P.ts.data() : nullptr, stamps ? P.expiry.data() : nullptr, P.n(), nullptr);
        });
        if (rc) return rc;
        lo = hi;
    }
    return BMQ_OK;
}
} // extern "C++"

// bmq_retain_compact_build under bmq_config.retain_builder = 3 is retain_build_next (bmq_retain_next.h) on rbx (its own stream) / rhx: no engine
// lock.  tools/retain_snapshot_check.cpp runs the same function under the sanitizers.
int bmq_retain_compact_build(bmq_engine* e) {
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> gc(e->cmp_mu); // (one compaction call at a time; the engine lock is NOT held: this is the long part)
    bmq_engine::RetainCompaction& c = e->rcmp;
    bool tiny = false;
    {
        std::lock_guard<std::mutex> g(e->mu);
        if (!c.active) return set_err(e, BMQ_E_STATE, "no retain compaction is running");
        if (c.built) return BMQ_OK;
        tiny = with_retain(e, [](auto& rt) { return rt.tiny; });
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::string msg;
    const int rc = with_retain_next(e, [&](auto&, auto*, auto& bx, auto& nx) {
        if (!c.exec_snapshot) {
            nx.n_items = c.items.size();
            if (!c.next.rebuild(std::move(c.items))) return msg = c.next.error, (int)BMQ_E_INVAL;
            c.items.clear(), c.items.shrink_to_fit();
            return (int)BMQ_OK;
        }
        if constexpr (std::is_same_v<std::decay_t<decltype(bx)>, DevExec>)
            if (hipSetDevice(e->device) != hipSuccess) return msg = "hipSetDevice failed", (int)BMQ_E_HIP;
        if (const int rc = retain_build_next(nx, bx, c.next, tiny, msg)) return rc;
        nx.snap.reset(); // (the next generation holds everything it needs)
        return (int)BMQ_OK;
    });
    std::lock_guard<std::mutex> g(e->mu);
    if (rc) return set_err(e, rc, msg);
    c.ms_build = ms_since(t0);
    c.built = true;
    c.ci.state = 2;
    with_retain_next(e, [&](auto&, auto*, auto&, auto& nx) { c.ci.builder = nx.exec_built ? 1 : 0, c.ci.fallback = nx.fallback; });
    c.ci.build_ms = c.ms_build;
    return BMQ_OK;
}
int bmq_retain_compact_swap(bmq_engine* e, uint64_t* out_carried, uint64_t* out_replayed) {
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> gc(e->cmp_mu);
    uint64_t n_log = 0;
    bmq_retain_compact_info ci{};
    {
        std::lock_guard<std::mutex> g(e->mu);
        bmq_engine::RetainCompaction& c = e->rcmp;
        if (!c.active) return set_err(e, BMQ_E_STATE, "no retain compaction is running");
        if (!c.built) return set_err(e, BMQ_E_STATE, "the next generation is not built: bmq_retain_compact_build first");
        if (c.log_overflow) return set_err(e, BMQ_E_NOSPACE, "the mutation log of this retain compaction outgrew its cap (1 GiB): bmq_retain_compact_abort, then begin again");
        for (auto& sl : e->slots)
            if (sl.pending) return set_err(e, BMQ_E_STATE, "a batch is in flight: finish / wait for it first");
        if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t meter0 = retain_copy_meter(e);
        if (out_carried) *out_carried = c.next.n_topics;
        e->rhost = std::move(c.next);
        const int rc = with_retain_next(e, [&](auto& rt, auto* rb, auto&, auto& nx) {
            if (nx.exec_built) { // image, key store and mutable part change hands: no upload, no host loop over the topics
                e->rb_serving = true;
                rb->take_image(*nx.rb);
                rt.adopt(*nx.rt, adopt_exec_image(e, *rb));
                e->rbinfo = rb->info;
                e->rbuilt = true;
                e->repoch++;
                e->rgeneration++;
                return (int)BMQ_OK;
            }
            e->rb_serving = false; // (the host builder's: retain_builder = 0 or 1, or the executor builder declined)
            e->rbinfo = host_build_info(e->rhost, nx.n_items, c.ms_build, nx.fallback);
            return retain_publish(e); // upload + the mutable part starts over: a new generation of topic ids
        });
        if (rc) {
            e->rcmp = bmq_engine::RetainCompaction{};
            return rc;
        }
        n_log = c.log.size();
        ci = c.ci;
        ci.locked_copy_bytes += retain_copy_meter(e) - meter0;
        ci.swap_ms = ms_since(t0);
    }
    // what was added / removed meanwhile, in order (the ordinary apply path; nothing is logged any more: the compaction is over)
    std::vector<bmq_engine::RetainCompaction::Op> log;
    {
        std::lock_guard<std::mutex> g(e->mu);
        log.swap(e->rcmp.log);
        const Boundary bound = e->rcmp.bound;
        e->rcmp = bmq_engine::RetainCompaction{};
        if (bound.bounded()) { // the range has shrunk: an op whose key lies outside is not this range's any more (adds and removals alike)
            size_t kept = 0;
            for (size_t i = 0; i < log.size(); i++)
                if (bound.contains(retain_message_key(log[i].tenant, log[i].topic))) {
                    if (kept != i) log[kept] = std::move(log[i]);
                    kept++;
                }
            log.resize(kept);
            n_log = kept;
        }
        ci.state = 3;
        ci.replayed = n_log;
        e->rcinfo = ci;
    }
    if (int rc = retain_apply_chunked(e, log, false, [](uint32_t, auto&& apply) { return apply(); })) return rc;
    if (out_replayed) *out_replayed = n_log;
    return BMQ_OK;
}
int bmq_retain_compact_abort(bmq_engine* e) {
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> gc(e->cmp_mu);
    std::lock_guard<std::mutex> g(e->mu);
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    e->rcmp = bmq_engine::RetainCompaction{}; // (the snapshot and the next generation's buffers go with it; bmq_retain_compact_info tells of the last swap again)
    return BMQ_OK;
}
int bmq_retain_compact_info_get(const bmq_engine* ce, bmq_retain_compact_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->rcmp.active ? e->rcmp.ci : e->rcinfo;
    return BMQ_OK;
}

int bmq_retain_compact(bmq_engine* e) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->rbuilt) return BMQ_OK;
    if (e->rcmp.active) return set_err(e, BMQ_E_STATE, "a retain compaction is running: bmq_retain_compact_swap or bmq_retain_compact_abort first");
    if (e->cur->pending) return set_err(e, BMQ_E_STATE, "a batch is in flight: call bmq_match_finish first");
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    std::vector<RetainIndexHost::Item> items;
    if (int rc = retain_live_items_locked(e, items)) return rc;
    return retain_load_items(e, std::move(items));
}

// ---- the retain store's range by KV boundary: RetainStoreCoProc.reset(Boundary) without the KV scan --------------------------------------
int bmq_retain_count_in(const bmq_engine* ce, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                        uint64_t* out_topics, uint64_t* out_key_bytes) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    Boundary bound;
    if (int rc = parse_boundary(e, flags, start, start_len, end, end_len, bound)) return rc;
    uint64_t topics = 0, bytes = 0;
    if (int rc = retain_boundary_locked(e, bound, topics, out_key_bytes ? &bytes : nullptr, nullptr)) return rc;
    if (out_topics) *out_topics = topics;
    if (out_key_bytes) *out_key_bytes = bytes;
    return BMQ_OK;
}

int bmq_retain_ids_in(const bmq_engine* ce, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len, uint32_t* out_ids,
                      uint32_t cap, uint32_t* out_n) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_n) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    *out_n = 0;
    Boundary bound;
    if (int rc = parse_boundary(e, flags, start, start_len, end, end_len, bound)) return rc;
    uint64_t topics = 0;
    std::vector<uint32_t> ids;
    if (int rc = retain_boundary_locked(e, bound, topics, nullptr, &ids)) return rc;
    *out_n = (uint32_t)ids.size();
    for (size_t i = 0; i < ids.size() && i < cap && out_ids; i++) out_ids[i] = ids[i];
    return ids.size() > cap ? BMQ_E_NOSPACE : BMQ_OK;
}

// Locks: dst->api for the whole call, then ONE engine lock at a time and never nested -- dst->mu to check, src->mu for the snapshot (ids
// inside the boundary, stamps, strings: src goes on serving afterwards), dst's own locks per chunk through the ordinary apply path.
int bmq_retain_import(bmq_engine* dst, bmq_engine* src, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                      uint64_t* out_imported, uint64_t* out_replaced) {
    if (!dst || !src) return BMQ_E_INVAL;
    std::lock_guard<std::recursive_mutex> api_lock(dst->api);
    Boundary bound;
    bool dst_empty = false;
    {
        std::lock_guard<std::mutex> g(dst->mu);
        if (dst == src) return set_err(dst, BMQ_E_INVAL, "bmq_retain_import: source and destination are the same engine");
        if (int rc = parse_boundary(dst, flags, start, start_len, end, end_len, bound)) return rc;
        // the new sibling of a split: nothing to merge with, so the import is a bulk load (ranks, the fast path of '+' and '#')
        dst_empty = !dst->rbuilt || (!dst->rcmp.active && retain_dyn_info(dst).n_live == 0);
        if (dst_empty)
            for (auto& sl : dst->slots)
                if (sl.pending) return set_err(dst, BMQ_E_STATE, "a batch is in flight: finish / wait for it first");
    }
    if (out_imported) *out_imported = 0;
    if (out_replaced) *out_replaced = 0;
    std::vector<RetainIndexHost::Item> items;
    int src_rc = BMQ_OK;
    std::string src_msg;
    {
        std::lock_guard<std::mutex> g(src->mu);
        if (src->device >= 0 && hipSetDevice(src->device) != hipSuccess) src_rc = BMQ_E_HIP, src_msg = "source engine: hipSetDevice failed";
        else if (src->rbuilt && (src_rc = retain_live_items_locked(src, items, bound)) != BMQ_OK) src_msg = "source engine: " + src->err;
    }
    if (src_rc != BMQ_OK) {
        std::lock_guard<std::mutex> g(dst->mu);
        return set_err(dst, src_rc, src_msg);
    }
    if (dst_empty) {
        std::lock_guard<std::mutex> g(dst->mu);
        if (dst->device >= 0) HIPCHK(dst, hipSetDevice(dst->device));
        const uint64_t n = items.size();
        if (int rc = retain_load_items(dst, std::move(items))) return rc;
        if (out_imported) *out_imported = n;
        return BMQ_OK;
    }
    // a merge: add ops through the ordinary apply path (a compaction running on dst logs them like any apply).  A topic dst holds already
    // has its stamps replaced: counted from dst's live count around every chunk (dst->api keeps other mutators out).
    uint64_t imported = 0, replaced = 0;
    const int rc = retain_apply_chunked(dst, items, true, [&](uint32_t n, auto&& apply) {
        const uint64_t before = retain_dyn_info(dst).n_live;
        if (int rc = apply()) return rc;
        const uint64_t fresh = retain_dyn_info(dst).n_live - before;
        imported += fresh;
        replaced += n - fresh;
        return (int)BMQ_OK;
    });
    if (rc) return rc;
    if (out_imported) *out_imported = imported;
    if (out_replaced) *out_replaced = replaced;
    return BMQ_OK;
}

int bmq_retain_match_batch_dev(bmq_engine* e, const uint8_t* d_tenants, const uint32_t* d_tenant_off, uint32_t n_tenants,
                               const uint32_t* d_filter_tenant, const uint8_t* d_filters, const uint32_t* d_filter_off,
                               uint32_t n_filters, uint32_t* d_out_row_ptr, uint32_t* d_out_topic_ids, uint64_t out_capacity,
                               uint64_t* d_out_total) {
    int rc = check_retain_ready(e);
    if (rc) return rc;
    if (n_filters == 0 || !d_out_row_ptr || !d_filter_off || !d_filters || !d_filter_tenant || !d_out_total)
        return set_err(e, BMQ_E_INVAL, "null pointer or empty batch");
    ApiHold api(e);
    if (!api.owns) return set_err(e, BMQ_E_STATE, "the engine is busy with another thread's call");
    std::lock_guard<std::mutex> g(e->mu);
    if (e->cur->pending) return set_err(e, BMQ_E_STATE, "a batch is in flight: call bmq_match_finish first");
    HIPCHK(e, hipSetDevice(e->device));
    if ((rc = ensure_batch_scratch(e, *e->cur, n_tenants, n_filters))) return rc;
    RetainArgs r{};
    r.tenants = d_tenants;
    r.tenant_off = d_tenant_off;
    r.n_tenants = n_tenants;
    r.filter_tenant = d_filter_tenant;
    r.filters = d_filters;
    r.filter_off = d_filter_off;
    r.n_filters = n_filters;
    BatchArgs a{};
    bind_outputs(a, d_out_row_ptr, d_out_topic_ids, out_capacity, d_out_total);
    rc = launch_retain(e, r, a);
    if (rc == BMQ_OK) api.keep();
    return rc;
}

// host buffers in -> the complete CSR of the batch in e->cur->s_row_ptr / e->cur->s_ids (device); *total = number of ids
// d_row / d_ids: where the CSR goes (nullptr: the engine's own s_row_ptr / s_ids, grown on demand)
static int retain_match_to_scratch(bmq_engine* e, const BatchInput& in, uint64_t* total, uint32_t* d_row, uint32_t* d_ids,
                                   uint64_t d_ids_cap) {
    bmq_engine::BatchSlot& S = *e->cur;
    BatchInput d;
    int rc;
    {
        std::lock_guard<std::mutex> g(e->mu);
        HIPCHK(e, hipSetDevice(e->device));
        if ((rc = stage_input(e, S, in, e->stream, d_ids ? 0 : 16, d))) return rc;
    }
    rc = bmq_retain_match_batch_dev(e, d.tenants, d.tenant_off, d.n_tenants, d.row_tenant, d.rows, d.row_off, d.n_rows,
                                    d_row ? d_row : S.s_row_ptr.as<uint32_t>(), d_ids ? d_ids : S.s_ids.as<uint32_t>(),
                                    d_ids ? d_ids_cap : S.dev_cap, S.b_total.as<uint64_t>());
    for (int attempt = 0; rc == BMQ_OK; attempt++) { // launched: finish; the slot's id buffer too small: once more with the size it told
        rc = bmq_match_finish(e, total);
        if (rc != BMQ_E_NOSPACE || d_ids) break;
        if (attempt == 2) return set_err(e, BMQ_E_NOMEM, "device output buffer growth did not converge");
        std::lock_guard<std::mutex> g(e->mu);
        rc = regrow_ids_and_relaunch(e, S, *total, BLOCKING_REGROW);
    }
    return rc;
}

// An empty batch with somewhere to put the empty CSR needs no device work: answered here (true; *rc -- a host-only engine still says
// what it is).
static bool retain_empty_batch(bmq_engine* e, uint32_t n_filters, uint32_t* out_row_ptr, uint64_t* out_needed, int* rc) {
    if (n_filters != 0 || !out_row_ptr || !out_needed) return false;
    *out_needed = 0;
    out_row_ptr[0] = 0;
    *rc = e->device < 0 ? BMQ_E_NODEVICE : BMQ_OK;
    return true;
}

static int retain_host_args_ok(bmq_engine* e, const BatchInput& in, const uint32_t* out_row_ptr, const uint64_t* out_needed) {
    if (int rc = check_retain_ready(e)) return rc;
    if (!out_row_ptr || !out_needed) return set_err(e, BMQ_E_INVAL, "null output pointer");
    if (!in.rows || !in.row_off || !in.row_tenant || (in.n_tenants && (!in.tenants || !in.tenant_off)))
        return set_err(e, BMQ_E_INVAL, "null input pointer");
    return BMQ_OK;
}

int bmq_retain_match_batch(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                           const uint32_t* filter_tenant, const uint8_t* filters, const uint32_t* filter_off,
                           uint32_t n_filters, uint32_t* out_row_ptr, uint32_t* out_topic_ids, uint64_t out_capacity,
                           uint64_t* out_needed) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    const BatchInput in{tenants, tenant_off, n_tenants, filter_tenant, filters, filter_off, n_filters};
    int rc;
    if (!e) return BMQ_E_INVAL;
    if (retain_empty_batch(e, n_filters, out_row_ptr, out_needed, &rc)) return rc;
    if ((rc = retain_host_args_ok(e, in, out_row_ptr, out_needed))) return rc;
    uint64_t total = 0;
    rc = retain_match_to_scratch(e, in, &total, nullptr, nullptr, 0);
    *out_needed = total;
    if (rc) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    HIPCHK(e, hipMemcpy(out_row_ptr, e->cur->s_row_ptr.p, sizeof(uint32_t) * (n_filters + 1), hipMemcpyDeviceToHost));
    if (total > out_capacity || (total && !out_topic_ids)) return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
    if (total) HIPCHK(e, hipMemcpy(out_topic_ids, e->cur->s_ids.p, sizeof(uint32_t) * total, hipMemcpyDeviceToHost));
    return BMQ_OK;
}

// The device part of RetainStoreCoProc.match(limit, now) for a host batch (the arguments were checked): the kept ids into e->cur->s_lim_ids, their
// row pointers (n + 1) into *out_d_row, the match counts (n) into *out_d_counts -- all device memory, the last kernels possibly still in the
// stream.  What bmq_retain_match_limited copies out, and what bmq_retain_keys_match composes the keys of where it lies.
static int retain_limited_to_scratch(bmq_engine* e, const BatchInput& in, const uint32_t* limit, uint64_t now_ms, uint32_t** out_d_row, uint32_t** out_d_counts) {
    const uint32_t n_filters = in.n_rows;
    int rc;
    uint32_t max_lim = 0;
    for (uint32_t i = 0; i < n_filters; i++) max_lim = std::max(max_lim, limit[i]);
    uint64_t total = 0;
    uint32_t* d_limit;
    uint32_t* d_counts = nullptr;
    uint32_t* d_kept;
    {
        std::lock_guard<std::mutex> g(e->mu);
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, e->cur->s_lim.ensure(sizeof(uint32_t) * (4 * (size_t)n_filters + 4)));
        d_limit = e->cur->s_lim.as<uint32_t>();
        d_counts = d_limit + n_filters;
        d_kept = d_counts + n_filters;
        HIPCHK(e, hipMemcpyAsync(d_limit, limit, sizeof(uint32_t) * n_filters, hipMemcpyHostToDevice, e->stream));
    }
    uint32_t* d_new_row = d_kept + n_filters + 1; // (kept has n + 1 entries: the scan's last input)
    *out_d_row = d_new_row;
    *out_d_counts = d_counts;
    if (max_lim <= LIM_FAST) { // walk + select: nothing is expanded
        {
            std::lock_guard<std::mutex> g(e->mu);
            HIPCHK(e, e->cur->s_lim_tmp.ensure(sizeof(uint32_t) * (size_t)n_filters * LIM_FAST));
            HIPCHK(e, e->cur->s_lim_ids.ensure(sizeof(uint32_t) * (size_t)n_filters * std::max(1u, max_lim)));
            e->rlim = RetainLimit{true, d_limit, now_ms, e->cur->s_lim_tmp.as<uint32_t>(), d_kept, d_counts};
        }
        rc = retain_match_to_scratch(e, in, &total, d_new_row, e->cur->s_lim_ids.as<uint32_t>(), (uint64_t)n_filters * std::max(1u, max_lim));
        {
            std::lock_guard<std::mutex> g(e->mu);
            e->rlim.active = false;
        }
        if (rc) return rc;
    } else { // large limits: the complete CSR, then the first limit[i] live ids of every row
        rc = retain_match_to_scratch(e, in, &total, nullptr, nullptr, 0);
        if (rc) return rc;
        std::lock_guard<std::mutex> g(e->mu);
        HIPCHK(e, e->cur->s_lim_ids.ensure(sizeof(uint32_t) * std::max<uint64_t>(total, 1)));
        const unsigned long long* ex = e->drt->expire_at();
        hipLaunchKernelGGL(k_limit_count_live, dim3((n_filters + 255) / 256), dim3(256), 0, e->stream, e->cur->s_row_ptr.as<uint32_t>(), e->cur->s_ids.as<uint32_t>(),
                           d_limit, ex, (unsigned long long)now_ms, n_filters, d_kept, d_counts);
        if (int rc2 = limit_rowptr(e, d_kept, n_filters, d_new_row, e->cur->b_total.as<unsigned long long>(), e->stream)) return rc2;
        hipLaunchKernelGGL(k_limit_copy_live, dim3((n_filters + 255) / 256), dim3(256), 0, e->stream, e->cur->s_row_ptr.as<uint32_t>(), d_new_row,
                           e->cur->s_ids.as<uint32_t>(), ex, (unsigned long long)now_ms, n_filters, e->cur->s_lim_ids.as<uint32_t>());
        HIPCHK(e, hipGetLastError());
    }
    return BMQ_OK;
}

int bmq_retain_match_limited(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                             const uint32_t* filter_tenant, const uint8_t* filters, const uint32_t* filter_off,
                             uint32_t n_filters, const uint32_t* limit, uint64_t now_ms, uint32_t* out_row_ptr, uint32_t* out_topic_ids,
                             uint64_t out_capacity, uint64_t* out_needed, uint32_t* out_match_count) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    const BatchInput in{tenants, tenant_off, n_tenants, filter_tenant, filters, filter_off, n_filters};
    int rc;
    if (!e) return BMQ_E_INVAL;
    if (retain_empty_batch(e, n_filters, out_row_ptr, out_needed, &rc)) return rc;
    if ((rc = retain_host_args_ok(e, in, out_row_ptr, out_needed))) return rc;
    if (!limit) return set_err(e, BMQ_E_INVAL, "null limit array");
    uint32_t *d_new_row = nullptr, *d_counts = nullptr;
    if ((rc = retain_limited_to_scratch(e, in, limit, now_ms, &d_new_row, &d_counts))) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    HIPCHK(e, hipMemcpyAsync(out_row_ptr, d_new_row, sizeof(uint32_t) * (n_filters + 1), hipMemcpyDeviceToHost, e->stream));
    if (out_match_count) HIPCHK(e, hipMemcpyAsync(out_match_count, d_counts, sizeof(uint32_t) * n_filters, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const uint64_t kept = out_row_ptr[n_filters];
    *out_needed = kept;
    if (kept > out_capacity || (kept && !out_topic_ids)) return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
    if (kept) HIPCHK(e, hipMemcpy(out_topic_ids, e->cur->s_lim_ids.p, sizeof(uint32_t) * kept, hipMemcpyDeviceToHost));
    return BMQ_OK;
}

// ---- id -> retainMessageKey on the device (key_len_one / key_write_one: bmq_retain_core.h; the store of the bulk-loaded strings: RetainDyn) ----
int bmq_retain_keys_prepare(bmq_engine* e, uint64_t* out_store_bytes) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (out_store_bytes) *out_store_bytes = 0;
    if (!e->rbuilt) return set_err(e, BMQ_E_STATE, "no retained-topic index");
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    uint64_t bytes = 0;
    const bool ok = retain_try(e, [&](auto& rt) { return rt.keys_prepare(e->rhost, &bytes); });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    if (out_store_bytes) *out_store_bytes = bytes;
    return BMQ_OK;
}

int bmq_retain_keys_by_id(const bmq_engine* ce, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    if (!e || !out_off || (n && !topic_ids)) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    memset(out_off, 0, sizeof(uint64_t) * ((size_t)n + 1));
    if (!e->rbuilt || n == 0) return BMQ_OK;
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    bool nospace = false;
    const bool ok = retain_try(e, [&](auto& rt) { return rt.keys_by_id(e->rhost, topic_ids, n, out, cap, (unsigned long long*)out_off, nospace); });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    if (nospace) return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
    return BMQ_OK;
}

int bmq_retain_keys_match(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* filter_tenant,
                          const uint8_t* filters, const uint32_t* filter_off, uint32_t n_filters, const uint32_t* limit, uint64_t now_ms,
                          uint32_t* out_row_ptr, uint32_t* out_topic_ids, uint64_t out_capacity, uint64_t* out_needed, uint32_t* out_match_count,
                          uint64_t* out_key_off, uint8_t* out_keys, uint64_t keys_cap, uint64_t* out_needed_key_bytes) {
    std::unique_lock<std::recursive_mutex> api_lock;
    if (e) api_lock = std::unique_lock<std::recursive_mutex>(e->api);
    const BatchInput in{tenants, tenant_off, n_tenants, filter_tenant, filters, filter_off, n_filters};
    int rc;
    if (!e) return BMQ_E_INVAL;
    if (out_key_off && out_needed_key_bytes && retain_empty_batch(e, n_filters, out_row_ptr, out_needed, &rc)) {
        out_key_off[0] = 0;
        *out_needed_key_bytes = 0;
        return rc;
    }
    if ((rc = retain_host_args_ok(e, in, out_row_ptr, out_needed))) return rc;
    if (!limit) return set_err(e, BMQ_E_INVAL, "null limit array");
    if (!out_key_off || !out_needed_key_bytes) return set_err(e, BMQ_E_INVAL, "null output pointer");
    if (n_filters == 0) return set_err(e, BMQ_E_INVAL, "null pointer or empty batch");
    uint32_t *d_row = nullptr, *d_counts = nullptr;
    if ((rc = retain_limited_to_scratch(e, in, limit, now_ms, &d_row, &d_counts))) return rc;
    std::lock_guard<std::mutex> g(e->mu);
    HIPCHK(e, hipMemcpyAsync(out_row_ptr, d_row, sizeof(uint32_t) * (n_filters + 1), hipMemcpyDeviceToHost, e->stream));
    if (out_match_count) HIPCHK(e, hipMemcpyAsync(out_match_count, d_counts, sizeof(uint32_t) * n_filters, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const uint64_t kept = out_row_ptr[n_filters];
    *out_needed = kept;
    *out_needed_key_bytes = 0;
    out_key_off[0] = 0;
    if (kept == 0) return BMQ_OK; // nothing kept: no key kernel, no scan over nothing
    // the keys of the kept ids, composed where the select left them (s_lim_ids); the lengths are known before anything is copied out
    const unsigned long long* d_koff = nullptr;
    const uint8_t* d_keys = nullptr;
    uint64_t key_bytes = 0;
    if (!e->drt->keys_compose(e->rhost, e->cur->s_lim_ids.as<uint32_t>(), (uint32_t)kept, d_koff, d_keys, key_bytes))
        return set_err(e, retain_rc(e->drt->error), e->drt->error);
    *out_needed_key_bytes = key_bytes;
    if (kept > out_capacity || !out_topic_ids) { // (out_key_off has out_capacity + 1 entries: nothing of the rows fits)
        HIPCHK(e, hipStreamSynchronize(e->stream));
        return set_err(e, BMQ_E_NOSPACE, "output buffer too small");
    }
    HIPCHK(e, hipMemcpyAsync(out_topic_ids, e->cur->s_lim_ids.p, sizeof(uint32_t) * kept, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(out_key_off, d_koff, sizeof(uint64_t) * (kept + 1), hipMemcpyDeviceToHost, e->stream));
    const bool fits = key_bytes <= keys_cap && (key_bytes == 0 || out_keys);
    if (fits && key_bytes) HIPCHK(e, hipMemcpyAsync(out_keys, d_keys, key_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!fits) return set_err(e, BMQ_E_NOSPACE, "key buffer too small");
    return BMQ_OK;
}

} // extern "C"
