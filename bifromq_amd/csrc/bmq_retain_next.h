// bmq_retain_next.h -- the generation change of the retained-topic index without the engine around it: the ONE packer / unpacker of
// (tenant, topic, stamps[, op]) items, what a compaction holds per executor type (RetainNext) and the step that turns a snapshot into the
// next image, catalogue and mutable part (retain_build_next: bmq_retain_compact_build under bmq_config.retain_builder = 3).  Knows no
// bmq_engine and no HIP: bmq_retain_engine.inc and tools/retain_snapshot_check.cpp (sanitizer builds over HostExec) call the same code.
#pragma once
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/bmq.h" // (the status codes)
#include "bmq_retain.h"
#include "bmq_retain_build.h"
#include "bmq_retain_dyn.h"

namespace bmq {

// what an executor's / builder's message means to the caller of the C ABI (the first rule that matches)
inline int retain_rc(const std::string& msg) {
    if (msg.find("malformed") != std::string::npos || msg.find("too many") != std::string::npos) return BMQ_E_INVAL;
    if (msg.find("exceed") != std::string::npos) return BMQ_E_RANGE;
    return msg.find("out of memory") != std::string::npos ? BMQ_E_NOMEM : BMQ_E_HIP;
}

// Items as the executors take them: a table of distinct tenant ids, per item an index into it, topic bytes + offsets, stamps, op codes.
struct PackedTopics {
    using Item = RetainIndexHost::Item;
    std::vector<uint8_t> tenants, topics, op;
    std::vector<uint32_t> tenant_off{0}, topic_off{0}, item_tenant, expiry;
    std::vector<uint64_t> ts;
    bool any_ts = false; // an item came with stamps

    uint32_t n() const { return (uint32_t)topic_off.size() - 1; }
    uint32_t n_tenants() const { return (uint32_t)tenant_off.size() - 1; }
    // false (nothing added): the topic bytes would reach what a 32-bit offset cannot address
    bool add(const std::string& tenant, const std::string& topic, bool has_ts, uint64_t t, uint32_t ex, uint8_t o = 0) {
        if (topics.size() + topic.size() >= 0xFFFFFFF0ull) return false;
        auto f = tix.find(tenant);
        if (f == tix.end()) {
            f = tix.emplace(tenant, (uint32_t)tix.size()).first;
            tenants.insert(tenants.end(), tenant.begin(), tenant.end());
            tenant_off.push_back((uint32_t)tenants.size());
        }
        item_tenant.push_back(f->second);
        topics.insert(topics.end(), topic.begin(), topic.end());
        topic_off.push_back((uint32_t)topics.size());
        ts.push_back(has_ts ? t : 0ull);
        expiry.push_back(has_ts ? ex : 0xFFFFFFFFu);
        op.push_back(o);
        any_ts = any_ts || has_ts;
        return true;
    }
    void pad() { tenants.resize(tenants.size() + 16, 0), topics.resize(topics.size() + 16, 0); } // (the kernels read 16 bytes at a time)
    RbInput rb_input() const { return RbInput{tenants.data(), tenant_off.data(), n_tenants(), item_tenant.data(), topics.data(), topic_off.data(), n(), ts.data(), expiry.data()}; }

    // ---- the inverse, over any packed arrays: cut(i) gives item i's (tenant, topic); its stamps are (ts, expiry)[stamp_of ? stamp_of[i] : i] ----
    // "no stamps" is stored as (0, 0xFFFFFFFF: never expires), so an item stamped exactly so comes back as one without
    static bool has_stamps(uint64_t t, uint32_t ex) { return !(t == 0 && ex == 0xFFFFFFFFu); }
    template <class Cut> static std::vector<Item> items(size_t n, Cut&& cut, const uint64_t* ts, const uint32_t* expiry, const uint32_t* stamp_of = nullptr) {
        std::vector<Item> out(n);
        for (size_t i = 0; i < n; i++) {
            const std::pair<std::string_view, std::string_view> s = cut(i);
            out[i].tenant.assign(s.first), out[i].topic.assign(s.second);
            if (!ts) continue;
            const size_t k = stamp_of ? stamp_of[i] : i;
            out[i].ts = ts[k], out[i].expiry = expiry[k];
            out[i].has_ts = has_stamps(ts[k], expiry[k]);
        }
        return out;
    }
    // RbInput's layout: a tenant table and an index per item
    static auto by_table(const uint8_t* tenants, const uint32_t* tenant_off, const uint32_t* item_tenant, const uint8_t* topics, const uint32_t* topic_off) {
        return [=](size_t i) {
            const uint32_t t = item_tenant[i];
            return std::make_pair(std::string_view((const char*)tenants + tenant_off[t], tenant_off[t + 1] - tenant_off[t]),
                                  std::string_view((const char*)topics + topic_off[i], topic_off[i + 1] - topic_off[i]));
        };
    }
    // tenant id and topic back to back per item, the first tlen[i] bytes the tenant's
    static auto by_prefix(const uint8_t* bytes, const uint64_t* off, const uint32_t* tlen) {
        return [=](size_t i) {
            return std::make_pair(std::string_view((const char*)bytes + off[i], tlen[i]), std::string_view((const char*)bytes + off[i] + tlen[i], (size_t)(off[i + 1] - off[i]) - tlen[i]));
        };
    }
    std::vector<Item> items() const { return items(n(), by_table(tenants.data(), tenant_off.data(), item_tenant.data(), topics.data(), topic_off.data()), ts.data(), expiry.data()); }

private:
    std::unordered_map<std::string, uint32_t> tix;
};

// What a compaction under bmq_config.retain_builder = 3 holds in exec memory, per executor type: the snapshot of the live topics (begin), then
// the next generation's image and mutable part, built from it on an executor of its own (build) and ready for the swap to take over.
template <class Exec> struct RetainNext {
    std::unique_ptr<RetainSnapshot<Exec>> snap;
    std::unique_ptr<RetainBuild<Exec>> rb;
    std::unique_ptr<RetainDyn<Exec>> rt;
    bool exec_built = false; // build left the next generation in exec memory (false after a fallback: the catalogue holds a host-built one)
    uint32_t fallback = 0;
    uint64_t n_items = 0;    // what bmq_retain_build_info tells of the generation once it serves
};

// The next image from nx.snap, the next catalogue (`next`) from ONE copy of the snapshot to the host, the next mutable part ready in exec
// memory.  Runs on bx; the caller holds no lock the serving generation needs.  A load the executor builder declines (a topic of more than
// RB_MAX_DEPTH levels) goes to the host builder: `next` is then a complete host-built index.  *msg: why it failed (the result is not BMQ_OK).
template <class Exec> int retain_build_next(RetainNext<Exec>& nx, Exec& bx, RetainIndexHost& next, bool tiny, std::string& msg) {
    const RetainSnapshot<Exec>& snap = *nx.snap;
    const RsSnap& S = snap.s;
    PackedTopics P; // the snapshot on the host
    // the tenant table is small: the builder de-duplicates and byte-sorts it on the host
    P.tenant_off.assign((size_t)S.n_tenants + 1, 0);
    if (!bx.copy_out(P.tenant_off.data(), S.tenant_off, 4 * P.tenant_off.size())) return msg = bx.err, BMQ_E_HIP;
    P.tenants.resize((size_t)P.tenant_off[S.n_tenants] + 16, 0);
    if (!bx.copy_out(P.tenants.data(), S.tenants, P.tenant_off[S.n_tenants])) return msg = bx.err, BMQ_E_HIP;
    RbInput in{P.tenants.data(), P.tenant_off.data(), S.n_tenants, S.item_tenant, S.topics, S.topic_off, S.n, nullptr, nullptr};
    in.in_exec = true;
    in.topic_bytes = snap.topic_bytes;
    nx.rb = std::make_unique<RetainBuild<Exec>>(bx);
    nx.rb->keep_perm = true;
    const bool built = nx.rb->build(in);
    if (!built && !nx.rb->too_deep) return msg = nx.rb->error, retain_rc(msg);
    // the packed snapshot on the host, once: what the catalogue's strings and stamps are cut from (or what the host builder loads)
    P.topics.resize((size_t)snap.topic_bytes + 16, 0);
    P.topic_off.assign((size_t)S.n + 1, 0), P.item_tenant.resize(S.n), P.expiry.resize(S.n), P.ts.resize(S.n);
    if (!bx.copy_out(P.topics.data(), S.topics, snap.topic_bytes) || !bx.copy_out(P.topic_off.data(), S.topic_off, 4 * P.topic_off.size()) ||
        !bx.copy_out(P.ts.data(), S.ts, 8 * (size_t)S.n) || !bx.copy_out(P.expiry.data(), S.expiry, 4 * (size_t)S.n) ||
        (!built && !bx.copy_out(P.item_tenant.data(), S.item_tenant, 4 * (size_t)S.n)))
        return msg = bx.err, BMQ_E_HIP;
    nx.n_items = S.n;
    if (!built) { // declined.  The host builder over the same items; the swap is then an upload
        nx.rb.reset();
        if (!next.rebuild(P.items())) return msg = next.error, BMQ_E_INVAL;
        nx.fallback = 1;
        nx.exec_built = false;
        return BMQ_OK;
    }
    in = P.rb_input();
    in.item_tenant = nullptr; // (retain_catalogue reads topics, offsets and stamps)
    retain_catalogue(next, in, *nx.rb);
    nx.rt = std::make_unique<RetainDyn<Exec>>(bx);
    nx.rt->tiny = tiny;
    if (!nx.rt->reset_exec(S, nx.rb->d_perm, (uint32_t)nx.rb->info.n_topics, nx.rb->names, nx.rb->t_begin)) return msg = nx.rt->error, retain_rc(msg);
    nx.rb->drop_perm();
    nx.exec_built = true;
    return BMQ_OK;
}

} // namespace bmq
