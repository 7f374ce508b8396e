// retain_fuzz.cpp -- test tool, not product: the retain index without a GPU, under AddressSanitizer/UBSan and ThreadSanitizer.
//   * the bulk load (bmq_retain.cpp: RetainIndexHost::rebuild): ids must enumerate (tenant, topic) in (tenant bytes, level-list bytes)
//     order; a CPU walk over the HBM image (directory, breadth-first node array, edge hash, '$' runs) done the way k_retain_walk
//     does it -- frontier of node ranges, '+' = children range, '#' = subtree id ranges -- must return exactly the topics the rule
//     of SURVEY.md 8a-0 selects by brute force;
//   * the MUTATION path (bmq_retain_core.h through RetainDyn<HostExec>, bmq_retain_dyn.h): the very functions the gfx950 kernels
//     k_r_locate / k_r_commit / k_r_rank run, here on several host threads with minimal capacities (every growth path runs all the
//     time).  After every batch: ids are stable (an untouched topic keeps its id, a re-added one gets its id back, a new one a fresh
//     id), stamps are those of the last add, the image walk (dead ids dropped) + a walk over the overlay trie done the way the kernel
//     does it equal the brute force, the GC scan and the live-id listing equal the model, overlay ids resolve to their strings;
//   * removal by id (remove_id_one: live ids, dead ones, repeats, the 64 ids of one word in one batch) interleaved with the batches and
//     the compactions, and after every step the retained topics per tenant (census_bulk_one, census_topic_one) against the model;
//   * id -> retainMessageKey (key_len_one / key_write_one over the string store of the bulk-loaded ids: what k_r_key_len / k_r_key_write
//     run): after every step the keys of every id in [0, id_bound + 8) against retain_message_key of the model's strings (bmq_codec.cpp),
//     empty for every id that is dead, was never handed out or lies behind the bound.
//   * the KV boundary of the range (retain_key_cmp / retain_key_in_boundary through RetainDyn::boundary_select: what k_r_boundary runs): after
//     every step count_in / ids_in of boundaries cut out of the model's keys (whole keys, prefixes that end in every segment, neighbours of
//     keys) against `start <= key < end` over retain_message_key; every fourth step the steps of a split -- the topics inside a boundary
//     loaded into an index of their own (an import into an empty range), ops inside and outside the boundary of which only the inside ones are
//     replayed there (the bounded generation change), the other half added on top through the apply path (an import into a non-empty range) --
//     each against the key-set model.
// Build + run: make -C bifromq_amd/csrc fuzz   (tests/test_host.py runs a short round of both builds)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../bifromq_amd/csrc/bmq_codec.h"
#include "../bifromq_amd/csrc/bmq_exec_host.h"
#include "../bifromq_amd/csrc/bmq_retain.h"
#include "../bifromq_amd/csrc/bmq_retain_dyn.h"

using namespace bmq;

static std::vector<std::string> split(std::string_view s, char sep) {
    std::vector<std::string> out;
    size_t b = 0;
    for (size_t i = 0; i <= s.size(); i++)
        if (i == s.size() || s[i] == sep) {
            out.emplace_back(s.substr(b, i - b));
            b = i + 1;
        }
    return out;
}
static bool filter_matches(const std::vector<std::string>& f, const std::vector<std::string>& t) {
    for (size_t i = 0; i < f.size(); i++) {
        const bool wild0 = i == 0 && !t.empty() && !t[0].empty() && t[0][0] == '$';
        if (f[i] == "#" && i + 1 == f.size()) return !wild0;
        if (i >= t.size()) return false;
        if (f[i] == "+") {
            if (wild0) return false;
            continue;
        }
        if (f[i] != t[i]) return false;
    }
    return f.size() == t.size();
}

static std::vector<uint32_t> image_match(const RetainIndexHost& h, std::string_view tenant, std::string_view filter) {
    std::vector<uint32_t> ids;
    const uint32_t ttok = dict_find(h.dict, h.pool, tenant);
    if (ttok == TOK_UNKNOWN) return ids;
    const uint32_t mask = (uint32_t)h.tenants.size() - 1;
    uint32_t d = tenant_hash(ttok) & mask;
    while (h.tenants[d].token != ttok) {
        if (h.tenants[d].token == 0) return ids;
        d = (d + 1) & mask;
    }
    const RTenantSlot ten = h.tenants[d];
    auto node = [&](uint32_t local) -> const RNode& { return h.nodes[ten.node_base + local]; };
    const auto levels = split(filter, '/');
    std::vector<std::pair<uint32_t, uint32_t>> cur{{0, 1}}, nxt; // node ranges (begin, count), tenant-local
    auto emit = [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; i++) ids.push_back(ten.id_base + i);
    };
    for (size_t li = 0; li < levels.size(); li++) {
        const std::string& lv = levels[li];
        if (lv == "#" && li + 1 == levels.size()) {
            for (auto& r : cur)
                for (uint32_t n = r.first; n < r.first + r.second; n++) {
                    const RNode& q = node(n);
                    if (li == 0) { // '#' at position 0: everything but the '$' topics
                        emit(q.sub_begin, std::min(q.sub_end, ten.sys_id_lo > q.sub_begin ? ten.sys_id_lo : q.sub_begin));
                        emit(std::max(q.sub_begin, ten.sys_id_hi), q.sub_end);
                    } else emit(q.sub_begin, q.sub_end);
                }
            std::sort(ids.begin(), ids.end());
            return ids;
        }
        nxt.clear();
        if (lv == "+") {
            for (auto& r : cur) {
                const uint32_t cb = node(r.first).child_begin;
                const RNode& last = node(r.first + r.second - 1);
                const uint32_t ce = last.child_begin + (last.child_count & ~RN_TERM);
                if (ce <= cb) continue;
                if (li == 0) { // skip the run of '$' children
                    if (ten.sys_node_lo > cb) nxt.push_back({cb, std::min(ce, ten.sys_node_lo) - cb});
                    if (ce > ten.sys_node_hi && ten.sys_node_hi >= cb) nxt.push_back({std::max(cb, ten.sys_node_hi), ce - std::max(cb, ten.sys_node_hi)});
                    if (ten.sys_node_lo == ten.sys_node_hi && ten.sys_node_lo <= cb) { nxt.clear(); nxt.push_back({cb, ce - cb}); }
                } else nxt.push_back({cb, ce - cb});
            }
        } else {
            const uint32_t tok = dict_find(h.dict, h.pool, lv);
            if (tok != TOK_UNKNOWN)
                for (auto& r : cur)
                    for (uint32_t n = r.first; n < r.first + r.second; n++) {
                        uint32_t bk = redge_bucket(n, tok, ten.edge_bucket_mask);
                        for (uint32_t probes = 0; probes <= ten.edge_bucket_mask; probes++) {
                            const REdge* e = &h.edges[ten.edge_base + 4 * (size_t)bk];
                            bool hit = false, hole = false;
                            for (int j = 0; j < 4; j++) {
                                if (e[j].parent == n && e[j].token == tok) {
                                    nxt.push_back({e[j].child & ~RE_OVERFLOW, 1});
                                    hit = true;
                                }
                                hole |= e[j].parent == NONE;
                            }
                            if (hit || hole) break;
                            bk = (bk + 1) & ten.edge_bucket_mask;
                        }
                    }
        }
        cur.swap(nxt);
        if (cur.empty()) break;
    }
    for (auto& r : cur)
        for (uint32_t n = r.first; n < r.first + r.second; n++)
            if (node(n).child_count & RN_TERM) ids.push_back(ten.id_base + node(n).sub_begin);
    std::sort(ids.begin(), ids.end());
    return ids;
}

// the overlay trie walked the way k_retain_walk does it: frontier of single nodes, '+' / '#' over child lists, literal levels by hash
static std::vector<uint32_t> overlay_match(const RetainDynView& dv, std::string_view tenant, std::string_view filter) {
    std::vector<uint32_t> ids;
    if (!dv.ov_live) return ids;
    auto find = [&](uint32_t parent, std::string_view label) {
        const LevelHash h = hash_level(label);
        std::string padded(label);
        padded.append(16, '\0');
        return ov_find(dv.onodes, dv.oedges, dv.oedge_mask, dv.opool, parent, h.h1, h.h2, (uint32_t)label.size(), (const uint8_t*)padded.data(), 0);
    };
    auto live = [&](uint32_t node) {
        const uint32_t id = dv.onodes[node].topic_id;
        if (id != NONE && !id_dead(dv.dead_bits, id)) ids.push_back(id);
    };
    const uint32_t tnode = find(0, tenant);
    if (tnode == NONE) return ids;
    const auto levels = split(filter, '/');
    std::vector<uint32_t> cur{tnode}, nxt;
    for (size_t li = 0; li < levels.size() && !cur.empty(); li++) {
        const std::string& lv = levels[li];
        if (lv == "#" && li + 1 == levels.size()) {
            bool first = true;
            while (!cur.empty()) {
                nxt.clear();
                for (uint32_t n : cur) {
                    if (!(first && li == 0)) live(n);
                    for (uint32_t c = dv.onodes[n].first_child; c != NONE; c = dv.onodes[c].next_sibling)
                        if (!(first && li == 0 && (dv.onodes[c].str_len & ON_SYS))) nxt.push_back(c);
                }
                cur.swap(nxt);
                first = false;
            }
            std::sort(ids.begin(), ids.end());
            return ids;
        }
        nxt.clear();
        for (uint32_t n : cur) {
            if (lv == "+") {
                for (uint32_t c = dv.onodes[n].first_child; c != NONE; c = dv.onodes[c].next_sibling)
                    if (!(li == 0 && (dv.onodes[c].str_len & ON_SYS))) nxt.push_back(c);
            } else {
                const uint32_t c = find(n, lv);
                if (c != NONE) nxt.push_back(c);
            }
        }
        cur.swap(nxt);
    }
    for (uint32_t n : cur) live(n);
    std::sort(ids.begin(), ids.end());
    return ids;
}

#define FAIL(...)                     \
    do {                              \
        fprintf(stderr, __VA_ARGS__); \
        return 1;                     \
    } while (0)

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 30;
    const unsigned threads = argc > 3 ? (unsigned)atoi(argv[3]) : 4;
    std::mt19937_64 rng(seed);
    const std::vector<std::string> tenants = {"t", "tenantB", "x", "a-much-longer-tenant-identifier"};
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "$x", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "0"};
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    auto rand_topic = [&]() {
        std::string t;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) t += (i ? "/" : "") + alpha[rnd(alpha.size())];
        return t;
    };
    auto rand_filter = [&]() {
        std::string f;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) {
            if (i) f += '/';
            if (i + 1 == depth && rnd(3) == 0) f += "#";
            else if (rnd(3) == 0) f += "+";
            else f += alpha[rnd(alpha.size())];
        }
        return f;
    };
    using Key = std::pair<std::string, std::string>; // (tenant, topic)
    std::map<Key, uint32_t> live;                    // retained now -> id
    std::map<Key, uint32_t> ever;                    // every topic that got an id in this generation -> id (ids are never reused)
    std::map<Key, std::pair<uint64_t, uint32_t>> stamp; // (HLC timestamp, expirySeconds) of the LAST add
    RetainIndexHost h;
    HostExec hx;
    hx.threads = threads;
    RetainDyn<HostExec> rt(hx);
    rt.tiny = true;
    RetainIndexView bview{};
    uint64_t checks = 0, n_ops = 0, n_batches = 0, n_id_removals = 0, n_keys = 0;
    auto view_of = [](const RetainIndexHost& h) {
        RetainIndexView v{};
        v.nodes = h.nodes.data();
        v.edges = h.edges.data();
        v.posts = h.posts.data();
        v.gps = h.gps.data();
        v.tenants = h.tenants.data();
        v.tenant_mask = (uint32_t)h.tenants.size() - 1;
        v.dict = h.dict.data();
        v.dict_group_mask = (uint32_t)h.dict.size() / DICT_GROUP - 1;
        v.pool = h.pool.data();
        return v;
    };
    auto base_view = [&]() { return view_of(h); };
    uint64_t n_bounds = 0;
    using Stamp = std::pair<uint64_t, uint32_t>;
    // BoundaryUtil.inRange over the model's key
    auto inside = [](const std::string& k, uint32_t flags, const std::string& s, const std::string& e) {
        return (!(flags & 1u) || k.compare(s) >= 0) && (!(flags & 2u) || k.compare(e) < 0);
    };
    // (tenant, topic) -> stamps of what an index retains now, through its own listing calls
    auto state_of = [&](RetainDyn<HostExec>& r, const RetainIndexHost& hh, std::map<Key, Stamp>& out, const std::vector<uint32_t>* only) -> bool {
        std::vector<uint32_t> ids;
        GcQuery q{};
        q.live_only = 1;
        q.override_expiry = -1;
        if (only) ids = *only;
        else if (!r.select(q, nullptr, 0, ids)) return false;
        std::vector<unsigned long long> ts;
        std::vector<uint32_t> ex, ov, lens;
        std::vector<uint8_t> bytes;
        if (!r.payload(ts, ex)) return false;
        for (uint32_t id : ids)
            if (id >= hh.n_topics) ov.push_back(id);
        if (!r.overlay_topics(ov.data(), (uint32_t)ov.size(), lens, bytes)) return false;
        size_t off = 0, k = 0;
        out.clear();
        for (uint32_t id : ids) {
            Key key;
            if (id < hh.n_topics) {
                std::string_view tn, tp;
                if (!hh.topic(id, tn, tp)) return false;
                key = {std::string(tn), std::string(tp)};
            } else {
                key = {std::string((const char*)bytes.data() + off, lens[2 * k]), std::string((const char*)bytes.data() + off + lens[2 * k], lens[2 * k + 1] - lens[2 * k])};
                off += lens[2 * k + 1];
                k++;
            }
            out[key] = {ts[id], ex[id]};
        }
        return true;
    };
    auto items_of = [](const std::map<Key, Stamp>& m) {
        std::vector<RetainIndexHost::Item> items;
        for (auto& kv : m) {
            RetainIndexHost::Item it;
            it.tenant = kv.first.first, it.topic = kv.first.second;
            it.ts = kv.second.first, it.expiry = kv.second.second;
            it.has_ts = !(it.ts == 0 && it.expiry == 0xFFFFFFFFu);
            items.push_back(std::move(it));
        }
        return items;
    };
    // ops (add with its stamps / remove) through the apply path of an index, one op per tenant table entry
    struct MOp {
        Key k;
        uint8_t op;
        Stamp st;
    };
    auto apply_ops = [&](RetainDyn<HostExec>& r, const std::vector<MOp>& ops) -> bool {
        if (ops.empty()) return true;
        std::string tb, pb;
        std::vector<uint32_t> toff{0}, poff{0}, ot, ex;
        std::vector<uint8_t> op;
        std::vector<unsigned long long> ts;
        for (size_t i = 0; i < ops.size(); i++) {
            tb += ops[i].k.first, toff.push_back((uint32_t)tb.size());
            pb += ops[i].k.second, poff.push_back((uint32_t)pb.size());
            ot.push_back((uint32_t)i), op.push_back(ops[i].op), ts.push_back(ops[i].st.first), ex.push_back(ops[i].st.second);
        }
        tb.append(16, '\0'), pb.append(16, '\0');
        return r.apply((const uint8_t*)tb.data(), toff.data(), (uint32_t)ops.size(), ot.data(), (const uint8_t*)pb.data(), poff.data(), op.data(), ts.data(), ex.data(),
                       (uint32_t)ops.size(), nullptr);
    };
    for (int round = 0; round < rounds; round++) {
        const bool full = round == 0 || rnd(8) == 0;
        if (full) { // a bulk load: either fresh random content, or a COMPACTION of what is live (what bmq_retain_compact does)
            const bool compact = round != 0 && rnd(2);
            std::vector<RetainIndexHost::Item> items;
            if (compact) {
                for (auto& kv : live) {
                    RetainIndexHost::Item it;
                    it.tenant = kv.first.first;
                    it.topic = kv.first.second;
                    it.ts = stamp[kv.first].first;
                    it.expiry = stamp[kv.first].second;
                    it.has_ts = !(it.ts == 0 && it.expiry == 0xFFFFFFFFu);
                    items.push_back(std::move(it));
                }
            } else {
                live.clear();
                stamp.clear();
                const size_t n = rnd(3) == 0 ? 0 : 1 + rnd(2500);
                for (size_t i = 0; i < n; i++) {
                    RetainIndexHost::Item it;
                    it.tenant = tenants[rnd(tenants.size())];
                    it.topic = rand_topic();
                    it.has_ts = rnd(4) != 0;
                    it.ts = (uint64_t)(1000 + rnd(100000)) << 16 | rnd(65536);
                    it.expiry = (uint32_t)rnd(500);
                    stamp[{it.tenant, it.topic}] = it.has_ts ? std::make_pair(it.ts, it.expiry) : std::make_pair<uint64_t, uint32_t>(0, 0xFFFFFFFFu);
                    live[{it.tenant, it.topic}] = 0;
                    items.push_back(std::move(it));
                }
            }
            if (!h.rebuild(std::move(items))) FAIL("round %d: rebuild failed: %s\n", round, h.error.c_str());
            bview = base_view();
            if (!rt.reset(bview, h)) FAIL("round %d: reset failed: %s\n", round, rt.error.c_str());
            // ids enumerate (tenant, level list) in order
            if (h.n_topics != live.size()) FAIL("round %d: n_topics %llu != %zu\n", round, (unsigned long long)h.n_topics, live.size());
            ever.clear();
            std::pair<std::string, std::vector<std::string>> prev;
            for (uint32_t id = 0; id < h.n_topics; id++) {
                std::string_view tn, tp;
                if (!h.topic(id, tn, tp) || !live.count({std::string(tn), std::string(tp)})) FAIL("round %d: topic(%u) is not in the model\n", round, id);
                std::pair<std::string, std::vector<std::string>> key{std::string(tn), split(tp, '/')};
                if (id && !(prev < key)) FAIL("round %d: ids are not in (tenant, level list) order at %u\n", round, id);
                prev = std::move(key);
                live[{std::string(tn), std::string(tp)}] = id;
                ever[{std::string(tn), std::string(tp)}] = id;
            }
        } else if (!ever.empty() && rnd(4) == 0) { // removal BY ID (bmq_retain_remove_ids: remove_id_one): live ids, dead ones, repeats
            std::map<uint32_t, Key> by_id;
            for (auto& kv : ever) by_id[kv.second] = kv.first;
            std::vector<uint32_t> ids;
            const size_t n = 1 + rnd(rnd(3) == 0 ? 700 : 70);
            const uint32_t start = (uint32_t)rnd(rt.info.id_bound);
            for (size_t i = 0; i < n; i++) {
                const size_t how = rnd(8);
                if (how < 4) ids.push_back((uint32_t)((start + i) % rt.info.id_bound)); // neighbours: the ids of one 64-id word in one batch
                else if (how < 7 || ids.empty()) ids.push_back((uint32_t)rnd(rt.info.id_bound));
                else ids.push_back(ids[rnd(ids.size())]);
            }
            uint64_t want = 0, removed = 0;
            for (uint32_t id : ids) {
                auto f = by_id.find(id);
                if (f != by_id.end()) want += live.erase(f->second);
            }
            if (!rt.remove_ids(ids.data(), (uint32_t)ids.size(), removed)) FAIL("round %d: remove_ids failed: %s\n", round, rt.error.c_str());
            if (removed != want) FAIL("round %d: remove_ids reports %llu topics removed, the model %llu\n", round, (unsigned long long)removed, (unsigned long long)want);
            n_id_removals += want;
        } else { // one batch of adds / removes over several tenants, duplicates inside the batch included
            std::vector<std::string> tn_list;
            std::string tbytes, pbytes;
            std::vector<uint32_t> toff{0}, poff{0}, op_tenant;
            std::vector<uint8_t> op;
            std::vector<unsigned long long> ts;
            std::vector<uint32_t> ex;
            const size_t n_ten = 1 + rnd(tenants.size());
            for (size_t t = 0; t < n_ten; t++) {
                tbytes += tenants[(t + round) % tenants.size()];
                toff.push_back((uint32_t)tbytes.size());
                tn_list.push_back(tenants[(t + round) % tenants.size()]);
            }
            const size_t n = 1 + rnd(rnd(4) == 0 ? 1500 : 40);
            const bool with_ts = rnd(5) != 0, single = n_ten == 1 && rnd(2);
            std::vector<Key> keys;
            for (size_t i = 0; i < n; i++) {
                const uint32_t ti = (uint32_t)rnd(n_ten);
                std::string tp;
                uint8_t o;
                if (!live.empty() && rnd(2)) { // mostly removals of live topics (sometimes of another tenant's name or a random topic)
                    auto it = live.begin();
                    std::advance(it, rnd(std::min<size_t>(live.size(), 300)));
                    tp = rnd(20) ? it->first.second : rand_topic();
                    o = 1;
                } else if (!ever.empty() && rnd(4) == 0) { // re-add something that had an id before
                    auto it = ever.begin();
                    std::advance(it, rnd(std::min<size_t>(ever.size(), 300)));
                    tp = it->first.second;
                    o = 0;
                } else {
                    tp = rand_topic();
                    o = 0;
                }
                pbytes += tp;
                poff.push_back((uint32_t)pbytes.size());
                op_tenant.push_back(ti);
                op.push_back(o);
                ts.push_back((uint64_t)(1000 + rnd(100000)) << 16 | rnd(65536));
                ex.push_back((uint32_t)rnd(500));
                keys.push_back({tn_list[ti], tp});
            }
            pbytes.append(16, '\0');
            tbytes.append(16, '\0');
            std::vector<uint32_t> out(n);
            if (!rt.apply((const uint8_t*)tbytes.data(), toff.data(), (uint32_t)n_ten, single ? nullptr : op_tenant.data(), (const uint8_t*)pbytes.data(), poff.data(), op.data(),
                          with_ts ? ts.data() : nullptr, with_ts ? ex.data() : nullptr, (uint32_t)n, out.data()))
                FAIL("round %d: apply failed: %s\n", round, rt.error.c_str());
            n_ops += n;
            n_batches++;
            // the model: ops in order; the LAST op on a topic decides and is the one that reports the id
            std::map<Key, size_t> last;
            for (size_t i = 0; i < n; i++) {
                if (single) keys[i].first = tn_list[0];
                last[keys[i]] = i;
            }
            for (size_t i = 0; i < n; i++) {
                const Key& k = keys[i];
                if (last[k] != i) {
                    if (out[i] != NONE) FAIL("round %d: op %zu (%d '%s' '%s') was superseded by op %zu (%d) but reports id %u; n=%zu single=%d\n", round, i, op[i], k.first.c_str(), k.second.c_str(), last[k], op[last[k]], out[i], n, (int)single);
                    continue;
                }
                if (op[i] == 0) {
                    if (out[i] == NONE) FAIL("round %d: add %zu reports no id\n", round, i);
                    auto ev = ever.find(k);
                    if (ev != ever.end() && ev->second != out[i]) FAIL("round %d: re-added topic changed its id %u -> %u\n", round, ev->second, out[i]);
                    if (ev == ever.end()) {
                        for (auto& kv : ever)
                            if (kv.second == out[i]) FAIL("round %d: id %u handed out twice\n", round, out[i]);
                        if (out[i] < h.n_topics) FAIL("round %d: a new topic got a bulk-loaded id %u\n", round, out[i]);
                    }
                    ever[k] = out[i];
                    live[k] = out[i];
                    stamp[k] = with_ts ? std::make_pair((uint64_t)ts[i], ex[i]) : std::make_pair<uint64_t, uint32_t>(0, 0xFFFFFFFFu);
                } else {
                    auto ev = ever.find(k);
                    if (ev == ever.end()) {
                        if (out[i] != NONE) FAIL("round %d: removal of a topic that never existed reports id %u\n", round, out[i]);
                    } else if (out[i] != ev->second) FAIL("round %d: removal reports id %u, the topic's id is %u\n", round, out[i], ev->second);
                    live.erase(k);
                }
            }
        }
        // ---- after the step: counters, listing, stamps, strings -----------------------------------------------------------------------
        if (rt.info.n_live != live.size()) FAIL("round %d: n_live %llu != %zu\n", round, (unsigned long long)rt.info.n_live, live.size());
        uint64_t base_dead = 0;
        for (auto& kv : ever) base_dead += kv.second < h.n_topics && !live.count(kv.first);
        if (rt.info.base_dead != base_dead) FAIL("round %d: base_dead %llu != %llu\n", round, (unsigned long long)rt.info.base_dead, (unsigned long long)base_dead);
        { // retained topics per tenant (bmq_retain_tenant_counts: census_bulk_one over the rank ranges + census_topic_one over the overlay ids)
            std::vector<uint32_t> ranges, bulk_live;
            for (const RTenantState* t : h.order) ranges.push_back(t->id_base), ranges.push_back(t->id_base + (uint32_t)t->topics.size());
            std::vector<std::pair<std::string, uint64_t>> ov;
            if (!rt.tenant_counts(ranges, bulk_live, ov)) FAIL("round %d: tenant_counts failed: %s\n", round, rt.error.c_str());
            std::map<std::string, uint64_t> got, want;
            for (size_t i = 0; i < h.order.size(); i++)
                if (bulk_live[i]) got[h.order[i]->name] += bulk_live[i];
            for (auto& o : ov) got[o.first] += o.second;
            for (auto& kv : live) want[kv.first.first]++;
            if (got != want) FAIL("round %d: tenant counts differ from the model (%zu tenants against %zu)\n", round, got.size(), want.size());
        }
        std::vector<uint32_t> ids, want_ids;
        GcQuery q{};
        q.live_only = 1;
        q.override_expiry = -1;
        if (!rt.select(q, nullptr, 0, ids)) FAIL("round %d: select failed\n", round);
        for (auto& kv : live) want_ids.push_back(kv.second);
        std::sort(want_ids.begin(), want_ids.end());
        if (ids != want_ids) FAIL("round %d: live ids differ (%zu vs %zu)\n", round, ids.size(), want_ids.size());
        {
            std::vector<uint32_t> ov;
            for (auto& kv : ever)
                if (kv.second >= h.n_topics) ov.push_back(kv.second);
            std::vector<uint32_t> lens;
            std::vector<uint8_t> bytes;
            if (!rt.overlay_topics(ov.data(), (uint32_t)ov.size(), lens, bytes)) FAIL("round %d: overlay_topics failed\n", round);
            size_t off = 0, k = 0;
            for (auto& kv : ever) {
                if (kv.second < h.n_topics) continue;
                const std::string got((const char*)bytes.data() + off, lens[2 * k + 1]);
                if (lens[2 * k] != kv.first.first.size() || got != kv.first.first + kv.first.second)
                    FAIL("round %d: overlay id %u resolves to '%s', want '%s%s'\n", round, kv.second, got.c_str(), kv.first.first.c_str(), kv.first.second.c_str());
                off += lens[2 * k + 1];
                k++;
            }
        }
        { // the key of every id: the per-item key functions through the host executor against the codec over the model's strings
            std::map<uint32_t, Key> live_by_id;
            for (auto& kv : live) live_by_id[kv.second] = kv.first;
            std::vector<uint32_t> all((size_t)rt.info.id_bound + 8);
            for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)i;
            if (round % 3 == 0) std::reverse(all.begin(), all.end());
            if (round % 5 == 0) all.push_back(0xFFFFFFFFu), all.push_back(all[0]);
            std::vector<unsigned long long> off(all.size() + 1, 77);
            std::string want;
            std::vector<unsigned long long> want_off{0};
            for (uint32_t id : all) {
                auto f = live_by_id.find(id);
                if (f != live_by_id.end()) want += retain_message_key(f->second.first, f->second.second);
                want_off.push_back(want.size());
            }
            std::vector<uint8_t> out(want.size() + 1, 0xEE);
            bool nospace = false;
            if (!want.empty()) { // one byte short: the offsets come, the bytes do not
                if (!rt.keys_by_id(h, all.data(), (uint32_t)all.size(), out.data(), want.size() - 1, off.data(), nospace)) FAIL("round %d: keys_by_id failed: %s\n", round, rt.error.c_str());
                if (!nospace || off != want_off || out[0] != 0xEE) FAIL("round %d: keys_by_id with a short buffer: nospace %d\n", round, (int)nospace);
            }
            if (!rt.keys_by_id(h, all.data(), (uint32_t)all.size(), out.data(), want.size(), off.data(), nospace)) FAIL("round %d: keys_by_id failed: %s\n", round, rt.error.c_str());
            if (nospace || off != want_off) FAIL("round %d: key offsets differ from the model (%llu bytes against %zu)\n", round, off.back(), want.size());
            if (want.compare(0, want.size(), (const char*)out.data(), want.size()) != 0 || out[want.size()] != 0xEE) FAIL("round %d: key bytes differ from retain_message_key\n", round);
            n_keys += live_by_id.size();
        }
        { // the KV boundary: count_in / ids_in against `start <= key < end` over the model's keys
            std::vector<std::pair<std::string, uint32_t>> keyed;
            for (auto& kv : live) keyed.push_back({retain_message_key(kv.first.first, kv.first.second), kv.second});
            auto cut = [&]() -> std::string {
                if (keyed.empty() || rnd(12) == 0) return rnd(2) ? std::string() : std::string(1 + rnd(4), (char)(rnd(2) ? 0xFF : 0x00));
                std::string k = keyed[rnd(keyed.size())].first;
                switch (rnd(6)) {
                case 0: return k;
                case 1: return k.substr(0, rnd(k.size()));                 // ends in any segment: a proper prefix sorts first
                case 2: return k + std::string(1 + rnd(300), '\0');
                case 3: k.back() = (char)((uint8_t)k.back() + 1); return k;
                case 4: k[rnd(k.size())] ^= (char)(1 + rnd(255)); return k; // one byte off, anywhere
                default: return k.substr(0, 3 + ((uint8_t)k[2] | ((uint8_t)k[1] << 8)));   // the head exactly
                }
            };
            for (int b = 0; b < 24; b++) {
                std::string s = cut(), e = cut();
                const uint32_t flags = b == 0 ? 0u : (uint32_t)(1 + rnd(3));
                if (flags == 3u && s.compare(e) >= 0) std::swap(s, e);
                if (flags == 3u && s == e) e += '\0';
                uint64_t topics = 0, kbytes = 0, want_bytes = 0;
                std::vector<uint32_t> got, want;
                if (!rt.boundary_select(h, flags, (const uint8_t*)s.data(), (uint32_t)s.size(), (const uint8_t*)e.data(), (uint32_t)e.size(), topics, b % 2 ? &kbytes : nullptr,
                                        b % 3 ? &got : nullptr))
                    FAIL("round %d: boundary_select failed: %s\n", round, rt.error.c_str());
                for (auto& kv : keyed)
                    if (inside(kv.first, flags, s, e)) want.push_back(kv.second), want_bytes += kv.first.size();
                std::sort(want.begin(), want.end());
                if (topics != want.size() || (b % 2 && kbytes != want_bytes) || (b % 3 && got != want))
                    FAIL("round %d: boundary (flags %u): %llu topics / %llu bytes / %zu ids, the model %zu / %llu\n", round, flags, (unsigned long long)topics,
                         (unsigned long long)kbytes, got.size(), want.size(), (unsigned long long)want_bytes);
                n_bounds++;
            }
            if (round % 4 == 0 && !keyed.empty()) { // the steps of a split at a key of the model
                const std::string c = cut();
                std::map<Key, Stamp> all, lower, upper, got;
                for (auto& kv : live) (inside(retain_message_key(kv.first.first, kv.first.second), 2u, "", c) ? lower : upper)[kv.first] = stamp[kv.first];
                // an import into an EMPTY range: the ids inside [c, +inf), their strings and stamps, bulk-loaded
                uint64_t topics = 0;
                std::vector<uint32_t> ids;
                if (!rt.boundary_select(h, 1u, (const uint8_t*)c.data(), (uint32_t)c.size(), nullptr, 0, topics, nullptr, &ids) || !state_of(rt, h, got, &ids))
                    FAIL("round %d: split: snapshot failed: %s\n", round, rt.error.c_str());
                if (got != upper) FAIL("round %d: split: the upper half has %zu topics, the model %zu\n", round, got.size(), upper.size());
                RetainIndexHost h2;
                RetainDyn<HostExec> rt2(hx);
                rt2.tiny = true;
                if (!h2.rebuild(items_of(got))) FAIL("round %d: split: rebuild failed\n", round);
                const RetainIndexView v2 = view_of(h2);
                if (!rt2.reset(v2, h2) || !state_of(rt2, h2, got, nullptr)) FAIL("round %d: split: load failed\n", round);
                if (got != upper || rt2.info.base_n != upper.size()) FAIL("round %d: split: the loaded sibling differs from the model\n", round);
                // the bounded generation change of the sibling's own range: ops inside and outside, only the inside ones are replayed
                std::vector<MOp> ops, kept;
                for (int i = 0; i < 40; i++) {
                    MOp o;
                    if (!live.empty() && rnd(2)) {
                        auto it = live.begin();
                        std::advance(it, rnd(live.size()));
                        o.k = it->first;
                    } else o.k = {tenants[rnd(tenants.size())], rand_topic()};
                    o.op = (uint8_t)rnd(2);
                    o.st = {(uint64_t)(1000 + rnd(100000)) << 16, (uint32_t)rnd(500)};
                    ops.push_back(o);
                    if (!inside(retain_message_key(o.k.first, o.k.second), 1u, c, "")) continue;
                    kept.push_back(o);
                    if (o.op == 0) upper[o.k] = o.st;
                    else upper.erase(o.k);
                }
                if (!apply_ops(rt2, kept) || !state_of(rt2, h2, got, nullptr)) FAIL("round %d: split: replay failed: %s\n", round, rt2.error.c_str());
                if (got != upper) FAIL("round %d: split: after the replay the sibling has %zu topics, the model %zu\n", round, got.size(), upper.size());
                uint64_t in2 = 0;
                if (!rt2.boundary_select(h2, 2u, nullptr, 0, (const uint8_t*)c.data(), (uint32_t)c.size(), in2, nullptr, nullptr) || in2 != 0)
                    FAIL("round %d: split: %llu topics of the sibling lie below the cut\n", round, (unsigned long long)in2);
                // an import into a NON-EMPTY range (the merge back): the lower half as add ops on top
                std::vector<MOp> adds;
                for (auto& kv : lower) adds.push_back({kv.first, 0, kv.second});
                const uint64_t before = rt2.info.n_live;
                if (!apply_ops(rt2, adds) || !state_of(rt2, h2, got, nullptr)) FAIL("round %d: merge: apply failed: %s\n", round, rt2.error.c_str());
                all = upper;
                for (auto& kv : lower) all[kv.first] = kv.second;
                if (got != all || rt2.info.n_live - before != lower.size()) FAIL("round %d: merge: %zu topics, the model %zu\n", round, got.size(), all.size());
            }
        }
        for (int s = 0; s < 40 && !live.empty(); s++) { // stamps of the last add
            auto it = live.begin();
            std::advance(it, rnd(live.size()));
            unsigned long long ts = 0, at = 0;
            uint32_t ex = 0;
            bool lv = false;
            if (!rt.topic_info(it->second, ts, ex, at, lv) || !lv) FAIL("round %d: topic_info(%u) fails for a live topic\n", round, it->second);
            const auto st = stamp[it->first];
            if (st.first != ts || st.second != ex || at != ((ts == 0 && ex == 0xFFFFFFFFu) ? RETAIN_NEVER : (ts >> 16) + (uint64_t)ex * 1000))
                FAIL("round %d: stamp of id %u differs\n", round, it->second);
        }
        // the GC scan: one tenant (its '$' topics are out of reach of match(tenant, "#")) and all tenants, with and without an override
        for (int s = 0; s < 4; s++) {
            const uint64_t now = 1000 + rnd(160000);
            const long long over = s % 2 ? (long long)rnd(300) : -1;
            const bool all = s >= 2;
            const std::string tn = tenants[rnd(tenants.size())];
            GcQuery g{};
            g.now = now;
            g.override_expiry = over;
            g.skip_sys = 1;
            if (!all) {
                g.has_tenant = 1;
                auto f = h.by_name.find(tn);
                if (f != h.by_name.end()) {
                    g.t_lo = f->second->id_base, g.t_hi = f->second->id_base + (uint32_t)f->second->topics.size();
                    g.sys_lo = f->second->id_base + f->second->sys_id_lo, g.sys_hi = f->second->id_base + f->second->sys_id_hi;
                }
                g.t_node = NONE;
            }
            std::vector<uint32_t> got, want;
            if (!rt.select(g, all ? nullptr : (const uint8_t*)tn.data(), (uint32_t)tn.size(), got)) FAIL("round %d: gc select failed\n", round);
            for (auto& kv : live) {
                if (!all && (kv.first.first != tn || (!kv.first.second.empty() && kv.first.second[0] == '$'))) continue;
                const auto st = stamp[kv.first];
                uint64_t at = (st.first == 0 && st.second == 0xFFFFFFFFu) ? RETAIN_NEVER : (st.first >> 16) + (uint64_t)st.second * 1000;
                if (over >= 0) at = (st.first >> 16) + (uint64_t)over * 1000;
                if (at <= now) want.push_back(kv.second);
            }
            std::sort(want.begin(), want.end());
            if (got != want) FAIL("round %d: GC scan (%s, override %lld) gives %zu ids, the model %zu\n", round, all ? "all" : tn.c_str(), over, got.size(), want.size());
        }
        // ---- match: image walk (dead ids dropped) + overlay walk == brute force ----------------------------------------------------------
        RetainDynView dv = rt.view();
        for (int qn = 0; qn < 120; qn++) {
            const std::string tn = qn % 25 == 24 ? std::string("nobody") : tenants[rnd(tenants.size())];
            const std::string filter = rand_filter();
            const auto fl = split(filter, '/');
            std::vector<uint32_t> want, got;
            for (auto& kv : live)
                if (kv.first.first == tn && filter_matches(fl, split(kv.first.second, '/'))) want.push_back(kv.second);
            std::sort(want.begin(), want.end());
            for (uint32_t id : image_match(h, tn, filter))
                if (!id_dead(dv.dead_bits, id)) got.push_back(id);
            const auto ov = overlay_match(dv, tn, filter);
            if (!ov.empty() && !got.empty() && ov.front() <= got.back()) FAIL("round %d: overlay ids are not above the bulk-loaded ones\n", round);
            got.insert(got.end(), ov.begin(), ov.end());
            checks++;
            if (got != want) FAIL("round %d: tenant '%s' filter '%s': index gives %zu topics, the rule %zu\n", round, tn.c_str(), filter.c_str(), got.size(), want.size());
            // the live count of every matched range comes from the rank directory
            if (dv.use_dead) {
                const auto all_ids = image_match(h, tn, filter);
                for (size_t a = 0; a < all_ids.size();) {
                    size_t b = a;
                    while (b + 1 < all_ids.size() && all_ids[b + 1] == all_ids[b] + 1) b++;
                    const uint32_t lo = all_ids[a], hi = all_ids[b] + 1;
                    uint32_t dead = 0;
                    for (uint32_t id = lo; id < hi; id++) dead += id_dead(dv.dead_bits, id);
                    if (dead_before(dv.dead_bits, dv.dead_rank, hi) - dead_before(dv.dead_bits, dv.dead_rank, lo) != dead) FAIL("round %d: rank directory is off in [%u, %u)\n", round, lo, hi);
                    a = b + 1;
                }
            }
        }
    }
    printf("retain_fuzz ok: seed %llu, %d rounds, %u threads, %llu ops in %llu batches, %llu topics removed by id, %llu filter checks, %llu keys, %llu boundaries\n", (unsigned long long)seed, rounds,
           threads, (unsigned long long)n_ops, (unsigned long long)n_batches, (unsigned long long)n_id_removals, (unsigned long long)checks, (unsigned long long)n_keys,
           (unsigned long long)n_bounds);
    return 0;
}
