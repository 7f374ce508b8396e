// bmq_prefix_engine.inc -- bmq_routes_prefix_census / bmq_routes_prefix_census_info_get: the live routes under each of a batch of key
// prefixes in one pass over the key store (DistIndex::prefix_census, bmq_prefix_core.h), what the dist worker's split hinter asks its KV
// range per prefix (DW/hinter/FanoutSplitHinter.java:174-178).  Included at the end of bmq_engine.hip.
static_assert(BMQ_PREFIX_MAX == PREFIX_MAX, "BMQ_PREFIX_MAX of include/bmq.h and PREFIX_MAX of bmq_prefix_core.h");

extern "C" int bmq_routes_prefix_census(const bmq_engine* ce, const uint8_t* prefixes, const uint32_t* prefix_off, uint32_t n, uint64_t* out_stats) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (n > BMQ_PREFIX_MAX) return set_err(e, BMQ_E_INVAL, "more than BMQ_PREFIX_MAX prefixes");
    if (n && (!prefix_off || !out_stats)) return set_err(e, BMQ_E_INVAL, "prefix_off and out_stats are needed");
    for (uint32_t i = 0; i < n; i++) {
        if (prefix_off[i + 1] < prefix_off[i]) return set_err(e, BMQ_E_INVAL, "prefix_off descends");
        if (prefix_off[i + 1] - prefix_off[i] >= (1u << 24)) return set_err(e, BMQ_E_INVAL, "prefix of 16 MiB or more");
    }
    if (n && prefix_off[n] > prefix_off[0] && !prefixes) return set_err(e, BMQ_E_INVAL, "prefix bytes are needed");
    if (int rc_open = complete_apply(e)) return rc_open; // (a batch handed over with bmq_routes_apply_async first)
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = with_index(e, [&](auto& ix) { // (the serving generation, also while a compaction builds the next one)
        // the scratch grows rarely; a free waits for every stream of the device, so the persistent matcher leaves first then
        const bool r = ix.prefix_census(prefixes, prefix_off, n, out_stats, e->prefix_stats, [&] {
            if (e->device >= 0) poller_stop_locked(e);
        });
        if (!r) e->err = ix.error;
        return r;
    });
    if (!ok) return index_error(e, e->err, false);
    e->prefix_last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return BMQ_OK;
}

extern "C" int bmq_routes_prefix_census_info_get(const bmq_engine* ce, bmq_prefix_census_info* out) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e || !out) return BMQ_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    memset(out, 0, sizeof(*out));
    out->struct_size = (uint32_t)sizeof(*out);
    out->prefix_max = BMQ_PREFIX_MAX;
    const PrefixStats& s = e->prefix_stats;
    out->n_calls = s.n_calls, out->n_prefixes = s.n_prefixes, out->n_distinct = s.n_distinct, out->n_nested = s.n_nested;
    out->n_keys_scanned = s.n_keys_scanned, out->max_chain = s.max_chain;
    out->last_ms = e->prefix_last_ms;
    return BMQ_OK;
}
