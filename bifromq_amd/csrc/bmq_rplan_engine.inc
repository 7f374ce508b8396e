// bmq_rplan_engine.inc -- bmq_retain_plan / bmq_retain_plan_commit: the two native halves of RetainStoreCoProc.batchRetain around the KV
// commit (RS/RetainStoreCoProc.java:193-255).  The plan (bmq_rplan_core.h; the control is RetainDyn::plan) reads the serving generation of
// the retained-topic index on the engine stream; the commit selects the winners' ops and hands them to the apply path of
// bmq_retain_engine.inc as they are.  Included at the end of bmq_engine.hip.
static_assert(BMQ_PLAN_NONE == RP_NONE && BMQ_PLAN_ADD == RP_ADD && BMQ_PLAN_UPDATE == RP_UPDATE && BMQ_PLAN_REMOVE == RP_REMOVE && BMQ_PLAN_SUPERSEDED == RP_SUPERSEDED,
              "BMQ_PLAN_* of include/bmq.h and RP_* of bmq_rplan_core.h");

static int rplan_args_ok(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant, const uint8_t* topics,
                         const uint32_t* topic_off, uint32_t n) {
    if (!tenant_off || !topic_off || n_tenants == 0) return set_err(e, BMQ_E_INVAL, "tenant table and topic offsets are needed");
    if (n > (1u << 28)) return set_err(e, BMQ_E_INVAL, "more than 2^28 ops in one plan");
    if ((tenant_off[n_tenants] > tenant_off[0] && !tenants) || (topic_off[n] > topic_off[0] && !topics)) return set_err(e, BMQ_E_INVAL, "null input pointer");
    for (uint32_t t = 0; t < n_tenants; t++)
        if (tenant_off[t + 1] < tenant_off[t]) return set_err(e, BMQ_E_INVAL, "tenant_off descends");
    for (uint32_t i = 0; i < n; i++) {
        if (topic_off[i + 1] < topic_off[i]) return set_err(e, BMQ_E_INVAL, "topic_off descends");
        if (op_tenant && op_tenant[i] >= n_tenants) return set_err(e, BMQ_E_INVAL, "op_tenant index out of range");
    }
    return BMQ_OK;
}

extern "C" int bmq_retain_plan(const bmq_engine* ce, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                               const uint8_t* topics, const uint32_t* topic_off, const uint8_t* clear, uint32_t n, uint8_t* out_code, uint8_t* out_action,
                               uint32_t* out_winner, uint32_t* out_topic_id, int32_t* out_delta, uint64_t* out_key_off, uint8_t* out_keys, uint64_t keys_cap,
                               bmq_retain_plan_info* out_info) {
    bmq_engine* e = const_cast<bmq_engine*>(ce);
    if (!e) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api);
    std::lock_guard<std::mutex> g(e->mu);
    if (out_info) {
        memset(out_info, 0, sizeof(*out_info));
        out_info->generation = e->rgeneration;
        out_info->epoch = e->repoch;
    }
    if (n == 0) { // nothing is launched
        if (out_key_off) out_key_off[0] = 0;
        if (out_delta && tenant_off) memset(out_delta, 0, sizeof(int32_t) * n_tenants);
        return BMQ_OK;
    }
    if (!out_key_off || !clear) return set_err(e, BMQ_E_INVAL, "clear flags and out_key_off are needed");
    if (int rc = rplan_args_ok(e, tenants, tenant_off, n_tenants, op_tenant, topics, topic_off, n)) return rc; // (nothing was written)
    if (e->device >= 0) HIPCHK(e, hipSetDevice(e->device));
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t by_action[4] = {0, 0, 0, 0}, key_bytes = 0;
    bool nospace = false;
    static const uint8_t none[1] = {0};
    const bool ok = retain_try(e, [&](auto& rt) { // (the serving generation, also while a compaction builds the next one)
        typename std::remove_reference_t<decltype(rt)>::PlanOut o{};
        o.code = out_code, o.action = out_action, o.winner = out_winner, o.topic_id = out_topic_id, o.delta = out_delta;
        o.key_off = (unsigned long long*)out_key_off, o.keys = out_keys, o.keys_cap = keys_cap;
        const bool r = rt.plan(tenants ? tenants : none, tenant_off, n_tenants, op_tenant, topics ? topics : none, topic_off, clear, n, 0u, o);
        for (int a = 0; a < 4; a++) by_action[a] = o.by_action[a];
        key_bytes = o.key_bytes, nospace = o.nospace;
        return r;
    });
    if (!ok) return set_err(e, retain_rc(e->err), e->err);
    if (out_info) {
        out_info->n_none = by_action[RP_NONE], out_info->n_add = by_action[RP_ADD], out_info->n_update = by_action[RP_UPDATE], out_info->n_remove = by_action[RP_REMOVE];
        out_info->n_groups = by_action[0] + by_action[1] + by_action[2] + by_action[3];
        out_info->key_bytes = key_bytes;
        out_info->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (nospace) return set_err(e, BMQ_E_NOSPACE, "key buffer too small");
    return BMQ_OK;
}

extern "C" int bmq_retain_plan_commit(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                                      const uint8_t* topics, const uint32_t* topic_off, uint32_t n, const uint8_t* action, const uint64_t* timestamp_hlc,
                                      const uint32_t* expiry_seconds, uint64_t generation, uint64_t epoch, uint32_t* out_topic_ids) {
    if (!e) return BMQ_E_INVAL;
    std::unique_lock<std::recursive_mutex> api_lock(e->api); // (held across the check and the apply: nothing gets in between)
    if ((timestamp_hlc == nullptr) != (expiry_seconds == nullptr)) return set_err(e, BMQ_E_INVAL, "timestamps and expiry intervals come together");
    std::vector<uint32_t> sel, sel_tenant, sel_off{0}, sel_expiry, sel_ids;
    std::vector<uint8_t> sel_topics, sel_op;
    std::vector<uint64_t> sel_ts;
    {
        std::lock_guard<std::mutex> g(e->mu);
        if (n && !action) return set_err(e, BMQ_E_INVAL, "the plan's actions are needed");
        if (n == 0) return (generation == e->rgeneration && epoch == e->repoch) ? (int)BMQ_OK : set_err(e, BMQ_E_STATE, "the retained-topic index has changed since the plan");
        if (int rc = rplan_args_ok(e, tenants, tenant_off, n_tenants, op_tenant, topics, topic_off, n)) return rc;
        for (uint32_t i = 0; i < n; i++)
            if (action[i] > BMQ_PLAN_SUPERSEDED) return set_err(e, BMQ_E_INVAL, "action must be one of BMQ_PLAN_*");
        if (generation != e->rgeneration || epoch != e->repoch) return set_err(e, BMQ_E_STATE, "the retained-topic index has changed since the plan");
    }
    for (uint32_t i = 0; i < n; i++) {
        if (out_topic_ids) out_topic_ids[i] = NONE;
        if (action[i] != BMQ_PLAN_ADD && action[i] != BMQ_PLAN_UPDATE && action[i] != BMQ_PLAN_REMOVE) continue;
        sel.push_back(i);
        sel_tenant.push_back(op_tenant ? op_tenant[i] : 0u);
        sel_topics.insert(sel_topics.end(), topics + topic_off[i], topics + topic_off[i + 1]);
        sel_off.push_back((uint32_t)sel_topics.size());
        sel_op.push_back(action[i] == BMQ_PLAN_REMOVE ? 1 : 0); // an add of a retained topic replaces its stamps (rcommit_one)
        if (timestamp_hlc) sel_ts.push_back(timestamp_hlc[i]), sel_expiry.push_back(expiry_seconds[i]);
    }
    if (sel.empty()) return BMQ_OK; // (nothing of the batch changes the index: the epoch stays)
    sel_topics.resize(sel_topics.size() + 16, 0);
    sel_ids.assign(sel.size(), NONE);
    static const uint8_t none[1] = {0};
    const int rc = bmq_retain_apply_batch(e, tenants ? tenants : none, tenant_off, n_tenants, sel_tenant.data(), sel_topics.data(), sel_off.data(), sel_op.data(),
                                          timestamp_hlc ? sel_ts.data() : nullptr, timestamp_hlc ? sel_expiry.data() : nullptr, (uint32_t)sel.size(), sel_ids.data());
    if (rc) return rc;
    if (out_topic_ids)
        for (size_t k = 0; k < sel.size(); k++) out_topic_ids[sel[k]] = sel_ids[k];
    return BMQ_OK;
}
