// host_fuzz.cpp -- test tool, not product: runs the index BUILDER (bmq_build_core.h -- the code the gfx950 builder kernels
// execute, bmq_dist_index.h -- its host-side control) on host threads through HostExec, under AddressSanitizer/UBSan or
// ThreadSanitizer, without a GPU.
//   * model: std::map route key -> id (byte order = KV order); after a rebuild ids must be the ranks, a put gets the next id,
//     a key keeps its id until it is deleted;
//   * after every rebuild/apply the image (TenantSlot directory, TrieSlot regions, DictSlot table, route_pos, key store) is
//     walked on the CPU exactly as k_walk does it (bucket probes, Bloom mask, root payload from the directory) for random
//     topics and compared with a brute-force application of the matching rule of SURVEY.md 8a-0 to every key of the model;
//   * tiny initial capacities (BMQ_FUZZ_SMALL, default on) force region growth, dictionary growth, id-list pool growth,
//     directory growth and key-store growth all the time.
//   * every third round a random KV boundary: count_in and the per-tenant census (tenant_stats) against the model, a bounded generation change (reserve_like with the boundary,
//     the boundary predicate on every chunk) and an import into a second index (import_refs: unknown tenants, duplicates) against the
//     model's key set restricted to the boundary.
//   * after every step bmq_routes_find's per-key lookup (DistIndex::find_keys over find_key_one) against the model's key -> id, absent, deleted and
//     malformed keys included; member tables of shared subscriptions carried through a bmq_compact and through the generation change
//     beside the index (Share::carry_prepare / carry_finish) against the model: carried iff the route was not deleted since, at its key's new id.
//   * after every step the delivery plan (Delivery::plan, bmq_delivery.h) of a random CSR -- live, deleted and never handed out ids, fresh member
//     tables whose members live under the deliverer keys of normal routes and under keys of their own -- against a plain merge, by key bytes, of
//     Fanout::group and Share::resolve over the same CSR: the same rows per DelivererKey in (topic, route, sender) order, special groups last.
//   * after every step reads in key order (DistIndex::window, ::gc_sweep: bmq_routes_window / bmq_routes_gc_sweep) against the model's map order:
//     windows from every kind of cursor, sweeps of random step and quota against the reference's loop walked over the map.
//   * after every step the two filters of that CSR (Caps::run, Gate::run: bmq_caps.h, bmq_gate.h) under random tables against the model: classes from the decoded
//     keys, the first k of a class by key survive in the input's order (k: the cap; gate_row_rule's kept count); once per run a row with a class of more than
//     CAPS_RANK_MAX members, which both rank on the host.
// Build + run: make -C bifromq_amd/csrc fuzz   (tests/test_host.py runs short rounds)
#include <cstdio>
#include <algorithm>
#include <array>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../bifromq_amd/csrc/bmq_caps.h"
#include "../bifromq_amd/csrc/bmq_codec.h"
#include "../bifromq_amd/csrc/bmq_delivery.h"
#include "../bifromq_amd/csrc/bmq_dist_index.h"
#include "../bifromq_amd/csrc/bmq_exec_host.h"
#include "../bifromq_amd/csrc/bmq_fanout.h"
#include "../bifromq_amd/csrc/bmq_gate.h"
#include "../bifromq_amd/csrc/bmq_share.h"

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

// the rule itself, on level lists
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

static uint32_t dict_find_host(const DistIndex<HostExec>& h, std::string_view level) {
    LevelHash lh = level_hash_init();
    uint32_t inl[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < level.size(); i += 4) {
        uint32_t w = 0;
        for (size_t k = 0; k < 4 && i + k < level.size(); k++) w |= (uint32_t)(uint8_t)level[i + k] << (8 * k);
        level_hash_word(lh, w);
        if (i < 16) inl[i >> 2] = w;
    }
    const uint32_t gmask = h.dict_slots / DICT_GROUP - 1, tag = level_hash_tag(lh);
    uint32_t g = level_hash_slot(lh, (uint32_t)level.size()) & gmask;
    for (uint32_t probes = 0; probes <= gmask; probes++) {
        bool group_full = true;
        for (uint32_t j = 0; j < DICT_GROUP; j++) {
            const DictSlot& d = h.dict[DICT_GROUP * g + j];
            if (!d.tag) {
                group_full = false;
                continue;
            }
            if (d.tag == tag && d.len == level.size() && d.inl[0] == inl[0] && d.inl[1] == inl[1] && d.inl[2] == inl[2] && d.inl[3] == inl[3] &&
                (level.size() <= 16 || memcmp(h.dpool + d.pool_off, level.data(), level.size()) == 0))
                return d.token;
        }
        if (!group_full) return TOK_UNKNOWN;
        g = (g + 1) & gmask;
    }
    return TOK_UNKNOWN;
}

// the walk of k_walk, on the host image
static std::vector<uint32_t> image_match(const DistIndex<HostExec>& h, std::string_view tenant, std::string_view topic, uint64_t* visits, uint64_t* beside = nullptr /* [2]: '+' children found beside their parent, '+' children found below a non-root node */) {
    std::vector<uint32_t> ids;
    const DistIndexMut ix = h.mut();
    const uint32_t d = tenant_find(ix.tenants, ix.tenant_mask, ix.tenant_names, (const uint8_t*)tenant.data(), 0, tenant.size());
    if (d == NONE) return ids;
    const TenantSlot rg = h.dir[d];
    const auto levels = split(topic, '/');
    std::vector<uint32_t> toks;
    for (auto& l : levels) toks.push_back(dict_find_host(h, l));
    const bool sys = !levels[0].empty() && levels[0][0] == '$';
    auto emit = [&](uint32_t b, uint32_t cf) {
        const uint32_t c = cf & ~RANGE_INDIRECT;
        for (uint32_t i = 0; i < c; i++) ids.push_back((cf & RANGE_INDIRECT) ? h.route_pos[b + i] : b + i);
    };
    // Layout v3 (bmq_layout.h): the '+' child of a node lies in the OTHER slot of the node's line if that slot was free when the child came
    // into being, else at its hashed home; the root's '+' child P0 lies at its hashed home and the directory entry names the slot.  This walker reads the image by that rule and nothing else.
    constexpr uint64_t AT_ROOT = ~0ull;
    struct Item {
        uint32_t node, tok, level;
        uint64_t pslot; // where `node`'s own slot is (relative to the region), or AT_ROOT
    };
    std::vector<Item> st;
    auto visit = [&](uint32_t node, uint64_t slot, uint32_t dl, uint32_t own_b, uint32_t own_c, uint32_t hash_b, uint32_t hash_c, uint32_t bloom) {
        const bool root_sys = dl == 0 && sys;
        if (dl == toks.size() && own_c) emit(own_b, own_c);
        if (hash_c && !root_sys) emit(hash_b, hash_c);
        if (dl < toks.size()) {
            const uint32_t t = toks[dl];
            if (t != TOK_UNKNOWN && ((bloom >> bloom_bit(t)) & 1u)) st.push_back({node, t, dl, slot});
            if ((bloom & BLOOM_PLUS) && !root_sys) st.push_back({node, TOK_PLUS, dl, slot});
        }
    };
    visit(0, AT_ROOT, 0, 0, 0, rg.root_hash_begin, rg.root_hash_count, rg.root_lit_bloom); // round 0: payload from the directory
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        auto arrive = [&](const TrieSlot* hit, uint64_t slot) {
            if (visits) (*visits)++;
            visit(hit->node, slot, it.level + 1, hit->own_begin, hit->own_count, hit->hash_begin, hit->hash_count, hit->lit_bloom);
        };
        if (it.tok == TOK_PLUS) {
            if (it.pslot == AT_ROOT) {
                if (rg.root_plus != NONE) {
                    const TrieSlot& p0 = h.trie[rg.base + rg.root_plus];
                    if (p0.parent != 0 || p0.token != TOK_PLUS) {
                        fprintf(stderr, "root_plus of a tenant does not name the root's '+' child\n");
                        abort();
                    }
                    arrive(&p0, rg.root_plus);
                    continue;
                }
            } else {
                const uint64_t ns = it.pslot ^ 1ull;
                const TrieSlot& o = h.trie[rg.base + ns];
                if (o.parent == it.node && o.token == TOK_PLUS) {
                    if (beside) beside[0]++, beside[1]++;
                    arrive(&o, ns);
                    continue;
                }
                // (a free or otherwise taken neighbour says nothing: a region growth leaves a '+' child that was not beside its parent at its hashed home)
            }
        }
        uint32_t bk = edge_bucket(it.node, it.tok, rg.buckets);
        for (uint32_t probes = 0; probes < rg.buckets; probes++) { // bucket probes, first-free order
            const TrieSlot& a = h.trie[rg.base + 2 * bk];
            const TrieSlot& b = h.trie[rg.base + 2 * bk + 1];
            if (a.parent == it.node && a.token == it.tok) {
                if (beside && it.tok == TOK_PLUS && it.pslot != AT_ROOT) beside[1]++;
                arrive(&a, 2ull * bk);
                break;
            }
            if (b.parent == it.node && b.token == it.tok) {
                if (beside && it.tok == TOK_PLUS && it.pslot != AT_ROOT) beside[1]++;
                arrive(&b, 2ull * bk + 1);
                break;
            }
            if (a.parent == NONE || b.parent == NONE) break;
            bk = bk + 1 == rg.buckets ? 0 : bk + 1;
        }
    }
    std::sort(ids.begin(), ids.end());
    return ids;
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 30;
    const size_t max_keys = argc > 3 ? (size_t)atoll(argv[3]) : 3000; // keys of a rebuild round
    const unsigned threads = argc > 4 ? (unsigned)atoi(argv[4]) : 4;
    std::mt19937_64 rng(seed);
    std::vector<std::string> tenants = {"t", "tenantB", "x", "a-much-longer-tenant-identifier", ""};
    const std::vector<std::string> alpha = {"a", "b", "c", "", "$sys", "+", "a-level-longer-than-sixteen-bytes", "\xE4\xBD\xA0\xE5\xA5\xBD", "0",
                                            "exactly-16-bytes", "seventeen-bytes-x", "#"};
    auto rnd = [&](size_t n) { return (size_t)(rng() % n); };
    auto rand_filter = [&]() {
        std::string f;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) {
            if (i) f += '/';
            if (i + 1 == depth && rnd(5) == 0) f += "#";
            else {
                std::string l = alpha[rnd(alpha.size())];
                if (l == "#") l = "#x"; // '#' is a wildcard only as the last level; as a literal level it never appears in a valid filter
                f += l;
            }
        }
        return f;
    };
    auto rand_topic = [&]() {
        std::string t;
        const size_t depth = 1 + rnd(5);
        for (size_t i = 0; i < depth; i++) {
            if (i) t += '/';
            std::string l = alpha[rnd(alpha.size())];
            if (l == "+" || l == "#") l = "zz"; // topics carry no wildcards; "zz" is never a filter level
            t += l;
        }
        return t;
    };
    uint64_t extra_tenants = 0;
    auto rand_key = [&]() {
        if (rnd(400) == 0) tenants.push_back("late-tenant-" + std::to_string(extra_tenants++)); // tenants appear over time
        const std::string& tn = tenants[rnd(tenants.size())];
        const uint8_t flag = rnd(10) == 0 ? (uint8_t)(2 + rnd(2)) : 1; // ($share and $oshare routes: the delivery plan below resolves both)
        // receiverUrl = subBrokerId NUL receiverId NUL delivererKey: a few brokers x a few deliverer keys (the fan-out grouping below)
        return encode_route_key(tn, rand_filter(), flag,
                                flag == 1 ? std::to_string(rnd(3)) + std::string("\0", 1) + "inbox" + std::to_string(rnd(40)) + std::string("\0d", 2) +
                                                std::to_string(rnd(12))
                                          : "g" + std::to_string(rnd(3)));
    };
    std::map<std::string, uint32_t> model; // key -> id
    uint32_t next_id = 0;
    HostExec hx;
    hx.threads = threads;
    DistIndex<HostExec> h(hx);
    h.tiny = getenv("BMQ_FUZZ_BIG") == nullptr;
    uint64_t checks = 0, n_apply = 0, n_rebuild = 0, fo_pairs = 0, n_generations = 0, n_census = 0, n_bounded = 0, n_imports = 0, plus_stat[2] = {0, 0};
    Fanout<HostExec> fo(hx, h); // fan-out grouping (bmq_fanout.h) over the same index, kept across rebuilds and applies
    fo.initial_table = 4;       // 36 deliverer keys: the group table grows twice
    // ---- reads in key order (bmq_routes_window / bmq_routes_gc_sweep: DistIndex::window and ::gc_sweep) against the model, whose std::map IS the
    // key order: windows from cursors absent, equal to a key, a proper prefix of one, a key plus a byte, below and above all keys, inclusive and
    // exclusive, of 1 key, a few, all and more than all; sweeps of random step and quota from such cursors against the loop of
    // DW/DistWorkerCoProc.java:554-701 walked over the map with an iterator -- and nothing may change by looking
    uint64_t n_windows = 0, n_sweeps = 0, n_sweeps_wrapped = 0, n_windows_over_a_bucket = 0;
    OrderStats order_stats;
    auto check_order = [&](int round, const char* what) -> bool {
        std::vector<std::pair<std::string, uint32_t>> mk(model.begin(), model.end()); // sorted by key
        auto rand_cursor = [&](bool& has) {
            has = true;
            const std::string some = mk.empty() ? rand_key() : mk[rnd(mk.size())].first;
            switch (rnd(7)) {
            case 0: has = false; return std::string();
            case 1: return some;
            case 2: return some.substr(0, some.size() - 1 - rnd(std::min<size_t>(some.size() - 1, 4)));
            case 3: return some + std::string(1, (char)rnd(256));
            case 4: return std::string();
            case 5: return std::string(3, '\xff');
            default: return rand_key();
            }
        };
        auto lower = [&](const std::string& lo, bool has, bool exclusive) {
            if (!has) return (size_t)0;
            auto cmp = [](const std::pair<std::string, uint32_t>& e, const std::string& k) { return e.first < k; };
            size_t at = (size_t)(std::lower_bound(mk.begin(), mk.end(), lo, cmp) - mk.begin());
            if (exclusive && at < mk.size() && mk[at].first == lo) at++;
            return at;
        };
        DistIndexStats before, after;
        h.stats(before);
        for (int w = 0; w < 6; w++) {
            bool has;
            const std::string lo = rand_cursor(has);
            const bool exclusive = has && rnd(2);
            const uint32_t sizes[5] = {1, 7, (uint32_t)mk.size(), (uint32_t)mk.size() + 3, (uint32_t)(1 + rnd(mk.size() + 1))};
            const uint32_t m = std::min<uint32_t>(sizes[rnd(5)], ORDER_WINDOW_MAX);
            std::vector<uint32_t> got(m ? m : 1, 12345u);
            uint32_t n = 0, more = 0;
            std::vector<uint8_t> lob(lo.begin(), lo.end()); // (the exact bytes: no padding)
            if (!h.window(has ? lob.data() : nullptr, (uint32_t)lob.size(), has, exclusive, false, 0, m, got.data(), n, more, order_stats)) {
                fprintf(stderr, "round %d (%s): window failed: %s\n", round, what, h.error.c_str());
                return false;
            }
            const size_t at = lower(lo, has, exclusive), want = std::min<size_t>(m, mk.size() - at);
            if (n != want || (more != 0) != (mk.size() - at > m)) {
                fprintf(stderr, "round %d (%s): window gives %u routes, more %u; the model %zu of %zu behind the cursor\n", round, what, n, more, want, mk.size() - at);
                return false;
            }
            for (size_t i = 0; i < want; i++)
                if (got[i] != mk[at + i].second) {
                    fprintf(stderr, "round %d (%s): window position %zu holds id %u, the model %u\n", round, what, i, got[i], mk[at + i].second);
                    return false;
                }
            n_windows++, n_windows_over_a_bucket += mk.size() - at > ORDER_BUCKET_MAX;
        }
        for (int w = 0; w < 4; w++) {
            bool has;
            const std::string lo = rand_cursor(has);
            const uint32_t step_hint = (uint32_t)rnd(12), scan_quota = rnd(3) == 0 ? 0u : (uint32_t)(1 + rnd(mk.size() + 2));
            // the reference's loop over the model
            const uint64_t step = std::max<uint32_t>(step_hint, 1u), quota = scan_quota ? scan_quota : 256 * step;
            std::vector<uint32_t> x_ids;
            bool x_wrapped = false;
            size_t itr = lower(lo, has, false);
            long long x_start = -1;
            if (itr >= mk.size()) x_wrapped = true, itr = mk.size();
            else
                for (;;) {
                    if (itr >= mk.size()) {
                        if (x_wrapped) break;
                        itr = 0, x_wrapped = true;
                    }
                    if (x_wrapped && (long long)itr == x_start) break;
                    if (x_start < 0) x_start = (long long)itr;
                    x_ids.push_back(mk[itr].second);
                    if (x_ids.size() >= quota) {
                        itr++;
                        break;
                    }
                    itr += step; // (the skip loop and the next() behind it: invalid as soon as one of them leaves the tail)
                }
            const bool x_has_next = itr < mk.size();
            const uint32_t cap = rnd(4) == 0 ? (uint32_t)(x_ids.size() / 2) : (uint32_t)x_ids.size() + 2;
            std::vector<uint32_t> got(cap ? cap : 1, 12345u);
            std::vector<uint8_t> lob(lo.begin(), lo.end());
            DistIndex<HostExec>::SweepResult r;
            if (!h.gc_sweep(has ? lob.data() : nullptr, (uint32_t)lob.size(), has, step_hint, scan_quota, got.data(), cap, r, order_stats)) {
                fprintf(stderr, "round %d (%s): gc_sweep failed: %s\n", round, what, h.error.c_str());
                return false;
            }
            if (r.inspected != x_ids.size() || r.wrapped != x_wrapped || r.has_next != x_has_next || (x_has_next && r.next_id != mk[itr].second) ||
                !std::equal(x_ids.begin(), x_ids.begin() + std::min<size_t>(cap, x_ids.size()), got.begin())) {
                fprintf(stderr, "round %d (%s): gc_sweep(step %u, quota %u) inspected %llu wrapped %d next %d; the model %zu %d %d\n", round, what, step_hint, scan_quota,
                        (unsigned long long)r.inspected, (int)r.wrapped, (int)r.has_next, x_ids.size(), (int)x_wrapped, (int)x_has_next);
                return false;
            }
            n_sweeps++, n_sweeps_wrapped += x_wrapped;
        }
        h.stats(after);
        if (before.n_nodes != after.n_nodes || before.n_tokens != after.n_tokens || before.n_routes != after.n_routes || before.next_id != after.next_id) {
            fprintf(stderr, "round %d (%s): a read in key order changed the index\n", round, what);
            return false;
        }
        return true;
    };
    // ---- key -> id (bmq_routes_find: DistIndex::find_keys over find_key_one) against the model, after every step: a sample of the live keys, keys
    // deleted at some point (live again or not: the model decides), random keys, repeats -- and nothing may come into being by looking
    std::vector<std::string> once_deleted;
    uint64_t n_find = 0, n_carries = 0, n_tables_carried = 0, n_tables_dropped = 0;
    auto check_find = [&](int round, const char* what) -> bool {
        std::vector<std::string> q;
        size_t pos = 0;
        for (auto& e : model)
            if (pos++ % (1 + model.size() / 400) == 0) q.push_back(e.first);
        for (size_t i = 0; i < 40; i++) q.push_back(rand_key());
        for (size_t i = 0; i < 40 && !once_deleted.empty(); i++) q.push_back(once_deleted[rnd(once_deleted.size())]);
        for (size_t i = 0; i < 20; i++) q.push_back(q[rnd(q.size())]);
        std::shuffle(q.begin(), q.end(), rng);
        if (once_deleted.size() > 4000) once_deleted.erase(once_deleted.begin(), once_deleted.begin() + 2000);
        std::vector<uint8_t> qb;
        std::vector<uint32_t> qo{0};
        for (auto& k : q) {
            qb.insert(qb.end(), k.begin(), k.end());
            qo.push_back((uint32_t)qb.size());
        }
        DistIndexStats before, after;
        h.stats(before);
        std::vector<uint32_t> got(q.size(), 12345u);
        uint32_t n_bad = 0;
        if (!h.find_keys(qb.data(), qo.data(), (uint32_t)q.size(), got.data(), n_bad) || n_bad) { // (the exact bytes: no padding behind the last key)
            fprintf(stderr, "round %d (%s): find_keys failed (%u malformed): %s\n", round, what, n_bad, h.error.c_str());
            return false;
        }
        for (size_t i = 0; i < q.size(); i++) {
            auto it = model.find(q[i]);
            const uint32_t want = it == model.end() ? NONE : it->second;
            if (got[i] != want) {
                fprintf(stderr, "round %d (%s): find_keys gives id %u for query %zu, the model %u\n", round, what, got[i], i, want);
                return false;
            }
        }
        h.stats(after);
        if (before.n_nodes != after.n_nodes || before.n_tokens != after.n_tokens || before.n_routes != after.n_routes || before.next_id != after.next_id) {
            fprintf(stderr, "round %d (%s): find_keys changed the index\n", round, what);
            return false;
        }
        std::vector<uint8_t> one(q[0].begin(), q[0].end() - 1); // a malformed key is counted, whatever stands beside it
        const uint32_t oo[2] = {0, (uint32_t)one.size()};
        uint32_t id1 = 0;
        if (!h.find_keys(one.data(), oo, 1, &id1, n_bad) || n_bad != 1) {
            fprintf(stderr, "round %d (%s): a truncated key was not refused\n", round, what);
            return false;
        }
        n_find += q.size();
        return check_order(round, what);
    };
    // ---- member tables of shared subscriptions through a generation change (bmq_config.share_carry: Share::carry_prepare / carry_finish) ----
    Share<HostExec> sh(hx);
    Share<HostExec> sh_plan(hx); // the tables of the delivery-plan check: given afresh for every CSR (sh above belongs to the carry checks)
    Delivery<HostExec> dl(hx);
    uint64_t dl_rows = 0, dl_merged = 0;
    // ---- the two filters of a match CSR (Caps::run, bmq_caps.h; Gate::run, bmq_gate.h) against the model: the classes come from the decoded keys, of
    // every class of a row the first k members by key survive, in the input's order -- k the cap for the caps, the kept count of gate_row_rule for
    // the gate.  `big`: the one row of the run with a class of more than CAPS_RANK_MAX members (the rank on the host), under limits that bind.
    Caps<HostExec> cp(hx);
    Gate<HostExec> gt(hx);
    uint64_t flt_in = 0, flt_caps_kept = 0, flt_gate_kept = 0, flt_events = 0, flt_host_rows = 0;
    auto check_filters = [&](int round, DistIndex<HostExec>& ix, const std::map<uint32_t, const std::string*>& by_id, const std::vector<uint32_t>& row, std::vector<uint32_t> ids,
                             bool big) -> bool {
        const uint32_t n_rows = (uint32_t)row.size() - 1, total = row[n_rows];
        ids.resize(total + 4);
        std::vector<uint8_t> cls(total);
        for (uint32_t i = 0; i < total; i++) {
            auto it = by_id.find(ids[i]);
            cls[i] = CAPS_DEAD;
            if (it == by_id.end()) continue;
            RouteKeyParts kp;
            decode_route_key(*it->second, kp);
            size_t p = 0;
            unsigned long long broker = 0;
            while (p < kp.receiver.size() && kp.receiver[p] >= '0' && kp.receiver[p] <= '9') broker = broker * 10 + (unsigned long long)(kp.receiver[p++] - '0');
            cls[i] = kp.flag != 1 ? CAPS_GROUP : (broker == 1 && p > 0 ? CAPS_PERSISTENT : CAPS_TRANSIENT);
        }
        // of the members of class cl in row r the first k by key stay; `over`: the ids of the others, in key order
        auto keep_first = [&](uint32_t r, uint32_t cl, uint64_t k, std::vector<uint8_t>& keep, std::vector<uint32_t>* over) {
            std::vector<std::pair<std::string_view, uint32_t>> m;
            for (uint32_t i = row[r]; i < row[r + 1]; i++)
                if (cls[i] == cl) m.push_back({std::string_view(*by_id.at(ids[i])), i});
            std::sort(m.begin(), m.end());
            for (size_t j = 0; j < m.size(); j++) {
                keep[m[j].second] = j < k;
                if (j >= k && over) over->push_back(ids[m[j].second]);
            }
        };
        auto survivors = [&](const std::vector<uint8_t>& keep, std::vector<uint32_t>& o_row, std::vector<uint32_t>& o_ids) {
            o_row.assign(1, 0u), o_ids.clear();
            for (uint32_t r = 0; r < n_rows; r++) {
                for (uint32_t i = row[r]; i < row[r + 1]; i++)
                    if (keep[i]) o_ids.push_back(ids[i]);
                o_row.push_back((uint32_t)o_ids.size());
            }
        };
        const int32_t limits[] = {0, 1, 2, 5, 0x7FFFFFFF};
        const long long byte_limits[] = {0, 50, 0x7FFFFFFFFFFFFFFFll};
        const uint32_t n_tab = big ? 1 : 1 + (uint32_t)rnd(3), thr = (uint32_t)rnd(6);
        std::vector<int32_t> pf(n_tab), gf(n_tab);
        std::vector<int64_t> pb(n_tab);
        std::vector<uint8_t> bw(n_tab + 16);
        for (uint32_t t = 0; t < n_tab; t++)
            pf[t] = big ? 7 : limits[rnd(5)], gf[t] = big ? 3 : limits[rnd(5)], pb[t] = big ? byte_limits[2] : byte_limits[rnd(3)], bw[t] = big ? 3 : (uint8_t)rnd(4);
        std::vector<uint32_t> row_tab(n_rows + 4), pack(n_rows + 4);
        for (uint32_t r = 0; r < n_rows; r++) row_tab[r] = (uint32_t)rnd(n_tab), pack[r] = (uint32_t)rnd(40);
        std::vector<uint32_t> want_row, want_ids, got_row(n_rows + 4), got_ids(total + 4);
        std::vector<uint8_t> keep(total);
        // -- the caps: a row no longer than both caps is copied through as it is; elsewhere dead ids leave, and a class over its cap keeps `cap` members
        std::vector<int32_t> want_ev, got_ev(4 * (size_t)total + 4);
        for (uint32_t r = 0; r < n_rows; r++) {
            const uint32_t t = row_tab[r], n = row[r + 1] - row[r];
            const bool through = n <= (uint32_t)std::min(pf[t], gf[t]);
            for (uint32_t i = row[r]; i < row[r + 1]; i++) keep[i] = through || cls[i] != CAPS_DEAD;
            for (uint32_t k = 0; k < 2 && !through; k++) {
                const uint32_t cap = (uint32_t)(k == 0 ? pf[t] : gf[t]);
                if ((uint32_t)std::count(cls.begin() + row[r], cls.begin() + row[r + 1], (uint8_t)(CAPS_PERSISTENT + k)) <= cap) continue;
                std::vector<uint32_t> over;
                keep_first(r, CAPS_PERSISTENT + k, cap, keep, &over);
                for (uint32_t id : over) want_ev.insert(want_ev.end(), {(int32_t)k, (int32_t)r, (int32_t)id, (int32_t)cap});
            }
        }
        survivors(keep, want_row, want_ids);
        CapsResult cr;
        if (!cp.run(ix, row.data(), ids.data(), n_rows, total, row_tab.data(), pf.data(), gf.data(), n_tab, pf.data(), gf.data(), got_row.data(), got_ids.data(), total, nullptr,
                    got_ev.data(), total, cr)) {
            fprintf(stderr, "round %d: caps failed: %s\n", round, cp.error.c_str());
            return false;
        }
        got_ev.resize(4 * (size_t)std::min<uint32_t>(cr.n_events, total));
        if (cr.overflow || cr.n_in != total || cr.n_kept != want_ids.size() || !std::equal(want_row.begin(), want_row.end(), got_row.begin()) ||
            !std::equal(want_ids.begin(), want_ids.end(), got_ids.begin()) || got_ev != want_ev || (big && cr.n_rows_fallback == 0)) {
            fprintf(stderr, "round %d: the capped CSR differs from the model (%llu vs %zu ids, %u vs %zu events, %u rows ranked on the host)\n", round, (unsigned long long)cr.n_kept,
                    want_ids.size(), cr.n_events, want_ev.size() / 4, cr.n_rows_fallback);
            return false;
        }
        flt_in += total, flt_caps_kept += cr.n_kept, flt_events += cr.n_events, flt_host_rows += cr.n_rows_fallback;
        // -- the gate: dead ids leave every row; what stays of a class is the rule's count
        std::vector<uint32_t> want_fl(n_rows), got_fl(n_rows + 4), want_mr(n_tab, 0u), got_mr(n_tab + 4);
        std::vector<uint64_t> want_mb(n_tab, 0ull), got_mb(n_tab + 4);
        for (uint32_t r = 0; r < n_rows; r++) {
            const uint32_t t = row_tab[r];
            uint32_t cnt[3] = {0, 0, 0};
            for (uint32_t i = row[r]; i < row[r + 1]; i++)
                if (cls[i] != CAPS_DEAD) cnt[gate_slot_of(cls[i])]++;
            const GateRow o = gate_row_rule(cnt[0], cnt[1], cnt[2], pack[r], (uint32_t)pf[t], (uint32_t)gf[t], (unsigned long long)pb[t], bw[t], thr);
            for (uint32_t i = row[r]; i < row[r + 1]; i++) keep[i] = cls[i] != CAPS_DEAD && o.keep[gate_slot_of(cls[i])] > 0;
            for (const uint32_t cl : {(uint32_t)CAPS_PERSISTENT, (uint32_t)CAPS_GROUP}) keep_first(r, cl, o.keep[gate_slot_of(cl)], keep, nullptr);
            want_fl[r] = o.flags, want_mb[t] += o.meter, want_mr[t] += o.record;
        }
        survivors(keep, want_row, want_ids);
        GateTable T;
        T.max_pf = pf.data(), T.max_gf = gf.data(), T.max_pb = pb.data(), T.bw = bw.data(), T.n_gate = n_tab;
        GateResult gr;
        if (!gt.run(ix, row.data(), ids.data(), n_rows, total, pack.data(), row_tab.data(), T, thr, got_row.data(), got_ids.data(), total, got_fl.data(), nullptr, got_mb.data(),
                    got_mr.data(), gr)) {
            fprintf(stderr, "round %d: gate failed: %s\n", round, gt.error.c_str());
            return false;
        }
        if (gr.overflow || gr.n_in != total || gr.n_kept != want_ids.size() || !std::equal(want_row.begin(), want_row.end(), got_row.begin()) ||
            !std::equal(want_ids.begin(), want_ids.end(), got_ids.begin()) || !std::equal(want_fl.begin(), want_fl.end(), got_fl.begin()) ||
            !std::equal(want_mb.begin(), want_mb.end(), got_mb.begin()) || !std::equal(want_mr.begin(), want_mr.end(), got_mr.begin()) || (big && gr.n_rows_fallback == 0)) {
            fprintf(stderr, "round %d: the gated CSR differs from the model (%llu vs %zu ids, %u rows ranked on the host)\n", round, (unsigned long long)gr.n_kept, want_ids.size(),
                    gr.n_rows_fallback);
            return false;
        }
        flt_gate_kept += gr.n_kept, flt_host_rows += gr.n_rows_fallback;
        return true;
    };
    std::map<uint32_t, std::pair<std::string, std::vector<std::string>>> sh_model; // route id -> (its key when the table was given, URLs)
    auto give_tables = [&](int round) -> bool { // fresh tables for up to 40 group routes of the model
        sh.drop();
        sh_model.clear();
        std::vector<uint32_t> ids, moff{0}, uoff{0};
        std::vector<uint8_t> urls;
        for (auto& e : model) {
            RouteKeyParts kp;
            if (ids.size() >= 40 || !decode_route_key(e.first, kp) || kp.flag == 1 || rnd(3) == 0) continue;
            auto& t = sh_model[e.second];
            t.first = e.first;
            const size_t n = 1 + rnd(rnd(5) == 0 ? 70 : 4);
            for (size_t m = 0; m < n; m++) {
                t.second.push_back(std::to_string(rnd(3)) + std::string("\0", 1) + "r" + std::to_string(m) + std::string("\0", 1) + "dk" + std::to_string(rnd(5)));
                urls.insert(urls.end(), t.second.back().begin(), t.second.back().end());
                uoff.push_back((uint32_t)urls.size());
            }
            ids.push_back(e.second);
            moff.push_back((uint32_t)(uoff.size() - 1));
        }
        if (!ids.empty() && !sh.apply(h, ids.data(), (uint32_t)ids.size(), moff.data(), urls.data(), uoff.data())) {
            fprintf(stderr, "round %d: share apply failed: %s\n", round, sh.error.c_str());
            return false;
        }
        return true;
    };
    // after carry_finish(next): the tables of the routes that were not deleted since (same id, same key in the model) sit at the ids `next` gives their keys
    auto check_carry = [&](int round, DistIndex<HostExec>& next, const std::map<std::string, uint32_t>& old_ids, const std::map<std::string, uint32_t>& new_ids, uint64_t from) -> bool {
        size_t want_carried = 0, want_members = 0;
        for (auto& e : sh_model) {
            auto was = old_ids.find(e.second.first);
            auto now = new_ids.find(e.second.first);
            if (was == old_ids.end() || was->second != e.first || now == new_ids.end()) continue;
            want_carried++;
            want_members += e.second.second.size();
            for (size_t m = 0; m <= e.second.second.size(); m++) {
                std::string url;
                const bool ok = sh.member(next, now->second, (uint32_t)m, url);
                if (ok != (m < e.second.second.size()) || (ok && url != e.second.second[m])) {
                    fprintf(stderr, "round %d: carried table of id %u -> %u: member %zu differs\n", round, e.first, now->second, m);
                    return false;
                }
            }
        }
        ShareInfo si;
        const auto& ci = sh.carry_info;
        if (!sh.info(next, si) || si.n_tables != want_carried || si.n_members != want_members || si.generation != next.generation || ci.status != 1 ||
            ci.n_carried != want_carried || ci.n_dropped != sh_model.size() - want_carried || ci.n_members_carried != want_members || ci.from_generation != from ||
            ci.to_generation != next.generation) {
            fprintf(stderr, "round %d: carry: %llu tables / %llu members (want %zu / %zu), %llu carried %llu dropped of %zu, status %u: %s\n", round,
                    (unsigned long long)si.n_tables, (unsigned long long)si.n_members, want_carried, want_members, (unsigned long long)ci.n_carried,
                    (unsigned long long)ci.n_dropped, sh_model.size(), ci.status, sh.error.c_str());
            return false;
        }
        n_carries++;
        n_tables_carried += want_carried;
        n_tables_dropped += sh_model.size() - want_carried;
        return true;
    };
    for (int round = 0; round < rounds; round++) {
        std::vector<std::string> keys;
        std::vector<uint8_t> ops;
        const bool full = round == 0 || rnd(8) == 0;
        if (full) {
            model.clear();
            const size_t n = rnd(3) == 0 ? 0 : 1 + rnd(max_keys);
            std::set<std::string> ks;
            for (size_t i = 0; i < n; i++) ks.insert(rand_key());
            keys.assign(ks.begin(), ks.end());
            uint32_t r = 0;
            for (auto& k : ks) model[k] = r++;
            next_id = r;
            if (rnd(3) == 0) { // not a KV scan: shuffled and with a duplicate
                std::shuffle(keys.begin(), keys.end(), rng);
                if (!keys.empty()) keys.push_back(keys[0]);
            }
            n_rebuild++;
        } else {
            const size_t n = 1 + rnd(rnd(4) == 0 ? 2000 : 60);
            for (size_t i = 0; i < n; i++) {
                if (!model.empty() && rnd(2)) { // delete an existing key (or, rarely, a key that is not there)
                    auto it = model.begin();
                    std::advance(it, rnd(std::min<size_t>(model.size(), 500)));
                    keys.push_back(rnd(20) ? it->first : rand_key());
                    ops.push_back(1);
                } else {
                    keys.push_back(rnd(6) == 0 && !keys.empty() ? keys[rnd(keys.size())] : rand_key()); // sometimes a key of this very batch again
                    ops.push_back(0);
                }
            }
            uint32_t put_no = 0;
            for (size_t i = 0; i < keys.size(); i++) { // in order; a put's id = next_id + number of puts before it
                if (ops[i]) model.erase(keys[i]), once_deleted.push_back(keys[i]);
                else {
                    if (!model.count(keys[i])) model[keys[i]] = next_id + put_no;
                    put_no++;
                }
            }
            next_id += put_no;
            n_apply++;
        }
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> off{0};
        for (auto& k : keys) {
            bytes.insert(bytes.end(), k.begin(), k.end());
            off.push_back((uint32_t)bytes.size());
        }
        bytes.resize(bytes.size() + 16, 0);
        const bool ok = full ? h.rebuild(bytes.data(), off.data(), (uint32_t)keys.size()) : h.apply(bytes.data(), off.data(), ops.data(), (uint32_t)keys.size());
        if (!ok) {
            fprintf(stderr, "round %d: %s failed: %s\n", round, full ? "rebuild" : "apply", h.error.c_str());
            return 1;
        }
        DistIndexStats st;
        h.stats(st);
        if (st.n_routes != model.size() || st.next_id != next_id) {
            fprintf(stderr, "round %d (%s): n_routes %llu (model %zu) next_id %u (model %u)\n", round, full ? "rebuild" : "apply",
                    (unsigned long long)st.n_routes, model.size(), st.next_id, next_id);
            return 1;
        }
        { // tenants with routes
            std::set<std::string> live;
            for (auto& e : model) {
                RouteKeyParts kp;
                decode_route_key(e.first, kp);
                live.insert(std::string(kp.tenant));
            }
            if (st.n_tenants != live.size()) {
                fprintf(stderr, "round %d: n_tenants %llu != %zu\n", round, (unsigned long long)st.n_tenants, live.size());
                return 1;
            }
        }
        // id -> key, single and batched
        std::vector<uint32_t> all_ids;
        for (auto& e : model) all_ids.push_back(e.second);
        size_t q = 0;
        for (auto& e : model) {
            if (q++ % (1 + model.size() / 300)) continue;
            std::string k;
            if (!h.route_key(e.second, k) || k != e.first) {
                fprintf(stderr, "round %d: route_key(%u) differs\n", round, e.second);
                return 1;
            }
        }
        {
            std::vector<uint8_t> kb;
            std::vector<uint64_t> ko;
            if (!h.route_keys(all_ids.data(), (uint32_t)all_ids.size(), kb, ko)) return 3;
            size_t i = 0;
            for (auto& e : model) {
                if (std::string_view((const char*)kb.data() + ko[i], ko[i + 1] - ko[i]) != e.first) {
                    fprintf(stderr, "round %d: route_keys entry %zu differs\n", round, i);
                    return 1;
                }
                i++;
            }
        }
        if (!check_find(round, full ? "rebuild" : "apply")) return 1;
        // ---- bmq_compact with share_carry: the rebuild happens inside the same object, so the tables' key bytes are copied first; ids become ranks ----
        if (h.built && rnd(5) == 0) {
            if (!give_tables(round)) return 1;
            const std::map<std::string, uint32_t> old_ids = model;
            const uint64_t from = h.generation;
            if (!sh.carry_prepare(h, true) || !h.compact() || !sh.carry_finish(h)) {
                fprintf(stderr, "round %d: compact with a carry failed: %s | %s\n", round, h.error.c_str(), sh.error.c_str());
                return 1;
            }
            uint32_t r = 0;
            for (auto& e : model) e.second = r++;
            next_id = r;
            if (!check_carry(round, h, old_ids, model, from) || !check_find(round, "compact")) return 1;
        }
        // ---- a generation change beside this index (bmq_compact_begin / _poll / _swap: DistIndex::reserve_like, import_snapshot, import_apply,
        // the log, its replay): chunks of random size, `h` mutated between a chunk's snapshot and its apply and between the chunks; afterwards
        // the new generation holds exactly the model's keys, with dense ids + at most the replayed ops' garbage.  `h` stays the index of the
        // following rounds (the engine would swap the two).
        if (h.built && rnd(4) == 0) {
            DistIndex<HostExec> g(hx);
            g.tiny = h.tiny;
            if (!g.reserve_like(h)) {
                fprintf(stderr, "round %d: reserve_like failed: %s\n", round, g.error.c_str());
                return 1;
            }
            h.defer_release = true;
            if (!give_tables(round)) return 1;
            std::vector<std::string> log_keys;
            std::vector<uint8_t> log_ops;
            auto mutate = [&]() -> bool { // a small batch into h, the model and the log
                std::vector<std::string> mk;
                std::vector<uint8_t> mo;
                const size_t n = 1 + rnd(40);
                for (size_t i = 0; i < n; i++) {
                    if (!model.empty() && rnd(2)) {
                        auto it = model.begin();
                        std::advance(it, rnd(std::min<size_t>(model.size(), 500)));
                        mk.push_back(it->first);
                        mo.push_back(1);
                    } else {
                        mk.push_back(rnd(5) == 0 && !mk.empty() ? mk[rnd(mk.size())] : rand_key());
                        mo.push_back(0);
                    }
                }
                uint32_t put_no = 0;
                for (size_t i = 0; i < mk.size(); i++) {
                    if (mo[i]) model.erase(mk[i]), once_deleted.push_back(mk[i]);
                    else {
                        if (!model.count(mk[i])) model[mk[i]] = next_id + put_no;
                        put_no++;
                    }
                }
                next_id += put_no;
                std::vector<uint8_t> mb;
                std::vector<uint32_t> mf{0};
                for (auto& k : mk) {
                    mb.insert(mb.end(), k.begin(), k.end());
                    mf.push_back((uint32_t)mb.size());
                }
                mb.resize(mb.size() + 16, 0);
                log_keys.insert(log_keys.end(), mk.begin(), mk.end());
                log_ops.insert(log_ops.end(), mo.begin(), mo.end());
                n_apply++;
                return h.apply(mb.data(), mf.data(), mo.data(), (uint32_t)mk.size()) && check_find(round, "apply during a generation change");
            };
            const uint32_t n_ids = h.id_bound();
            uint64_t carried = 0;
            for (uint32_t cursor = 0; cursor < n_ids;) {
                const uint32_t hi = (uint32_t)std::min<uint64_t>(n_ids, (uint64_t)cursor + 1 + rnd(rnd(3) == 0 ? 2000 : 150));
                uint32_t n_live = 0;
                if (!g.import_snapshot(h, cursor, hi) || (rnd(3) == 0 && !mutate()) || !g.import_apply(n_live)) {
                    fprintf(stderr, "round %d: generation change failed at id %u: %s | %s\n", round, cursor, g.error.c_str(), h.error.c_str());
                    return 1;
                }
                carried += n_live;
                cursor = hi;
                if (rnd(4) == 0 && !mutate()) {
                    fprintf(stderr, "round %d: apply during a generation change failed: %s\n", round, h.error.c_str());
                    return 1;
                }
            }
            if (!log_keys.empty()) { // the replay: ONE merged batch, in order
                std::vector<uint8_t> mb;
                std::vector<uint32_t> mf{0};
                for (auto& k : log_keys) {
                    mb.insert(mb.end(), k.begin(), k.end());
                    mf.push_back((uint32_t)mb.size());
                }
                mb.resize(mb.size() + 16, 0);
                if (!g.apply(mb.data(), mf.data(), log_ops.data(), (uint32_t)log_keys.size())) {
                    fprintf(stderr, "round %d: replay failed: %s\n", round, g.error.c_str());
                    return 1;
                }
            }
            { // the swap's carry, while both generations are alive: the lookup reads the key bytes from h's pool
                g.generation = h.generation + 1;
                DistIndexStats cs;
                g.stats(cs);
                std::vector<uint32_t> gi(cs.next_id);
                for (uint32_t i = 0; i < cs.next_id; i++) gi[i] = i;
                std::vector<uint8_t> gb;
                std::vector<uint64_t> go;
                if (!g.route_keys(gi.data(), cs.next_id, gb, go)) return 3;
                std::map<std::string, uint32_t> new_ids;
                for (uint32_t i = 0; i < cs.next_id; i++)
                    if (go[i + 1] > go[i]) new_ids[std::string((const char*)gb.data() + go[i], go[i + 1] - go[i])] = i;
                if (!sh.carry_prepare(h, false) || !sh.carry_finish(g)) {
                    fprintf(stderr, "round %d: the carry of a generation change failed: %s\n", round, sh.error.c_str());
                    return 1;
                }
                if (!check_carry(round, g, model, new_ids, h.generation)) return 1;
            }
            h.defer_release = false;
            h.release_deferred();
            DistIndexStats gs;
            g.stats(gs);
            if (gs.n_routes != model.size() || gs.next_id - gs.n_routes > log_keys.size()) {
                fprintf(stderr, "round %d: new generation: %llu routes (model %zu), %u ids, %zu ops replayed, %llu carried\n", round,
                        (unsigned long long)gs.n_routes, model.size(), gs.next_id, log_keys.size(), (unsigned long long)carried);
                return 1;
            }
            std::vector<uint32_t> ids(gs.next_id);
            for (uint32_t i = 0; i < gs.next_id; i++) ids[i] = i;
            std::vector<uint8_t> kb;
            std::vector<uint64_t> ko;
            if (!g.route_keys(ids.data(), gs.next_id, kb, ko)) return 3;
            std::set<std::string> got;
            for (uint32_t i = 0; i < gs.next_id; i++)
                if (ko[i + 1] > ko[i]) got.insert(std::string((const char*)kb.data() + ko[i], ko[i + 1] - ko[i]));
            if (got.size() != model.size() || !std::equal(got.begin(), got.end(), model.begin(), [](const std::string& a, const auto& b) { return a == b.first; })) {
                fprintf(stderr, "round %d: the new generation's key set differs from the model (%zu keys against %zu)\n", round, got.size(), model.size());
                return 1;
            }
            n_generations++;
        }
        // ---- split and merge by KV boundary (bmq_routes_count_in, bmq_compact_begin_in, bmq_routes_import: Boundary, DistIndex::count_in,
        // reserve_like(old, boundary), set_import_boundary, import_refs and the boundary predicate of bmq_build_core.h that k_b_boundary
        // runs on the device).  The boundary's keys are keys of the model, prefixes of them, a tenant prefix, or absent.
        if (h.built && rnd(3) == 0) {
            auto rand_bound = [&]() {
                if (model.empty() || rnd(6) == 0) return std::string(rnd(2) ? "" : "\xff\xff");
                auto it = model.begin();
                std::advance(it, rnd(model.size()));
                const std::string& k = it->first;
                switch (rnd(4)) {
                case 0: return k;
                case 1: return k.substr(0, rnd(k.size() + 1));
                case 2: return k.substr(0, 3 + (((size_t)(uint8_t)k[1] << 8) | (uint8_t)k[2])); // 00 | u16be(len) | tenant
                default: return k + std::string(1, (char)rnd(256));
                }
            };
            Boundary bd;
            bd.flags = (uint8_t)rnd(4);
            bd.start = (bd.flags & 1) ? rand_bound() : std::string();
            bd.end = (bd.flags & 2) ? rand_bound() : std::string();
            if (!bd.valid()) std::swap(bd.start, bd.end);
            if (!bd.valid()) bd.flags = 1; // (start == end)
            std::set<std::string> inside;
            uint64_t inside_bytes = 0;
            for (auto& e : model)
                if ((!(bd.flags & 1) || e.first >= bd.start) && (!(bd.flags & 2) || e.first < bd.end)) inside.insert(e.first), inside_bytes += e.first.size();
            uint64_t cr = 0, cb = 0;
            if (!h.count_in(bd, cr, cb) || cr != inside.size() || cb != inside_bytes) {
                fprintf(stderr, "round %d: count_in gives %llu keys / %llu bytes, the model %zu / %llu (%s)\n", round, (unsigned long long)cr,
                        (unsigned long long)cb, inside.size(), (unsigned long long)inside_bytes, h.error.c_str());
                return 1;
            }
            // the per-tenant census over the same boundary (bmq_routes_tenant_stats: DistIndex::tenant_stats, census_key_one -- what
            // k_b_census runs per lane on the device) against the model's keys taken apart here: tenant from the front, flag from the back
            {
                std::map<std::string, std::array<uint64_t, 4>> want;
                for (const std::string& k : inside) {
                    const size_t tl = ((size_t)(uint8_t)k[1] << 8) | (uint8_t)k[2], rl = ((size_t)(uint8_t)k[k.size() - 2] << 8) | (uint8_t)k[k.size() - 1];
                    auto& w = want[k.substr(3, tl)];
                    w[(uint8_t)k[k.size() - 3 - rl] - 1]++;
                    w[3] += k.size();
                }
                std::vector<DistIndex<HostExec>::TenantStat> got;
                bool same = h.tenant_stats(bd, got) && got.size() == want.size();
                auto it = want.begin();
                for (size_t i = 0; same && i < got.size(); i++, ++it)
                    same = got[i].tenant == it->first && got[i].n_normal == it->second[0] && got[i].n_unordered_share == it->second[1] &&
                           got[i].n_ordered_share == it->second[2] && got[i].key_bytes == it->second[3];
                if (!same) {
                    fprintf(stderr, "round %d: the tenant census differs from the model (%zu tenants against %zu) (%s)\n", round, got.size(), want.size(), h.error.c_str());
                    return 1;
                }
                n_census++;
            }
            // the per-prefix census (bmq_routes_prefix_census: DistIndex::prefix_census, prefix_key_one -- what k_b_prefix_census runs per
            // lane on the device) over random byte prefixes, nested ones and a repeat included, against the model's keys as std::string
            // compares them
            {
                std::vector<std::string> ps;
                for (uint32_t i = 0, e = 1 + rnd(40); i < e; i++) ps.push_back(rand_bound());
                ps.push_back(ps[rnd(ps.size())]);
                ps.push_back(std::string());
                std::vector<uint8_t> pb;
                std::vector<uint32_t> po(1, 0u);
                for (const std::string& p : ps) pb.insert(pb.end(), p.begin(), p.end()), po.push_back((uint32_t)pb.size());
                pb.resize(pb.size() + 16, 0);
                std::vector<uint64_t> got(4 * ps.size(), 77), want(4 * ps.size(), 0);
                for (auto& e : model) {
                    const std::string& k = e.first;
                    const size_t rl = ((size_t)(uint8_t)k[k.size() - 2] << 8) | (uint8_t)k[k.size() - 1];
                    for (size_t i = 0; i < ps.size(); i++)
                        if (k.size() >= ps[i].size() && k.compare(0, ps[i].size(), ps[i]) == 0) want[4 * i + (uint8_t)k[k.size() - 3 - rl] - 1]++, want[4 * i + 3] += k.size();
                }
                PrefixStats pst;
                if (!h.prefix_census(pb.data(), po.data(), (uint32_t)ps.size(), got.data(), pst, [] {}) || got != want) {
                    fprintf(stderr, "round %d: the prefix census differs from the model (%zu prefixes) (%s)\n", round, ps.size(), h.error.c_str());
                    return 1;
                }
            }
            auto key_set = [&](DistIndex<HostExec>& ix, std::set<std::string>& got) {
                DistIndexStats is;
                ix.stats(is);
                std::vector<uint32_t> ids(is.next_id);
                for (uint32_t i = 0; i < is.next_id; i++) ids[i] = i;
                std::vector<uint8_t> kb;
                std::vector<uint64_t> ko;
                if (!ix.route_keys(ids.data(), is.next_id, kb, ko)) return false;
                size_t live = 0;
                for (uint32_t i = 0; i < is.next_id; i++)
                    if (ko[i + 1] > ko[i]) got.insert(std::string((const char*)kb.data() + ko[i], ko[i + 1] - ko[i])), live++;
                return live == got.size() && is.n_routes == live; // (no key stored twice)
            };
            { // the range that shrinks: a bounded generation change, chunks of random size
                DistIndex<HostExec> g(hx);
                g.tiny = h.tiny;
                if (!g.reserve_like(h, &bd) || !g.set_import_boundary(bd)) {
                    fprintf(stderr, "round %d: bounded reserve_like failed: %s\n", round, g.error.c_str());
                    return 1;
                }
                h.defer_release = true;
                const uint32_t n_ids = h.id_bound();
                uint64_t carried = 0;
                for (uint32_t cursor = 0; cursor < n_ids;) {
                    const uint32_t hi = (uint32_t)std::min<uint64_t>(n_ids, (uint64_t)cursor + 1 + rnd(rnd(3) == 0 ? 2000 : 150));
                    uint32_t n_live = 0;
                    if (!g.import_snapshot(h, cursor, hi) || !g.import_apply(n_live)) {
                        fprintf(stderr, "round %d: bounded generation change failed at id %u: %s\n", round, cursor, g.error.c_str());
                        return 1;
                    }
                    carried += n_live;
                    cursor = hi;
                }
                h.defer_release = false;
                h.release_deferred();
                std::set<std::string> got;
                if (!key_set(g, got) || got != inside || carried != inside.size()) {
                    fprintf(stderr, "round %d: the bounded generation holds %zu keys (%llu carried), the model has %zu inside\n", round, got.size(),
                            (unsigned long long)carried, inside.size());
                    return 1;
                }
                n_bounded++;
            }
            { // the sibling of a split / a merge: into an index that already holds some of the keys and some others
                DistIndex<HostExec> d(hx);
                d.tiny = h.tiny;
                std::set<std::string> want = inside;
                uint64_t want_dups = 0;
                if (rnd(2)) {
                    std::vector<std::string> pre;
                    for (auto& e : model)
                        if (rnd(5) == 0) pre.push_back(e.first);
                    for (int i = 0; i < 5; i++) pre.push_back(rand_key());
                    std::sort(pre.begin(), pre.end());
                    pre.erase(std::unique(pre.begin(), pre.end()), pre.end());
                    std::vector<uint8_t> pb;
                    std::vector<uint32_t> po{0};
                    for (auto& k : pre) {
                        pb.insert(pb.end(), k.begin(), k.end());
                        po.push_back((uint32_t)pb.size());
                        want_dups += inside.count(k);
                        want.insert(k);
                    }
                    pb.resize(pb.size() + 16, 0);
                    if (!d.rebuild(pb.data(), po.data(), (uint32_t)pre.size())) return 3;
                }
                const uint32_t n_ids = h.id_bound();
                std::vector<unsigned long long> snap(h.kref, h.kref + n_ids); // (the engine: a copy in exec memory, src held meanwhile)
                h.defer_release = true;
                ApplyResult res;
                bool ok = d.set_import_boundary(bd);
                for (uint32_t lo = 0; ok && lo < n_ids;) {
                    const uint32_t n = (uint32_t)std::min<uint64_t>(n_ids - lo, 1 + rnd(rnd(3) == 0 ? 3000 : 200));
                    ok = d.import_refs(snap.data() + lo, n, h.kpool, res);
                    lo += n;
                }
                h.defer_release = false;
                h.release_deferred();
                std::set<std::string> got;
                if (!ok || !key_set(d, got) || got != want || res.added != inside.size() - want_dups || res.dups != want_dups) {
                    fprintf(stderr, "round %d: import: %s; %zu keys (want %zu), %u added %u dups (want %llu dups)\n", round, d.error.c_str(), got.size(),
                            want.size(), res.added, res.dups, (unsigned long long)want_dups);
                    return 1;
                }
                n_imports++;
            }
        }
        // decoded form of the model, for the brute force
        struct Dec {
            std::string tenant;
            std::vector<std::string> levels;
            uint32_t id;
        };
        std::vector<Dec> dec;
        std::map<std::pair<std::string, std::string>, std::vector<uint32_t>> by_filter;
        for (auto& e : model) {
            RouteKeyParts kp;
            if (!decode_route_key(e.first, kp)) return 2;
            dec.push_back({std::string(kp.tenant), split(kp.esc_filter, '\0'), e.second});
            std::string mq(kp.esc_filter);
            for (auto& c : mq)
                if (c == '\0') c = '/';
            by_filter[{std::string(kp.tenant), mq}].push_back(e.second);
        }
        { // exact filter lookup
            size_t i = 0;
            for (auto& e : by_filter) {
                if (i++ % (1 + by_filter.size() / 60)) continue;
                std::vector<uint32_t> got, want = e.second;
                std::sort(want.begin(), want.end());
                if (!h.find(e.first.first, e.first.second, got)) return 3;
                std::sort(got.begin(), got.end());
                if (got != want) {
                    fprintf(stderr, "round %d: find('%s','%s') gives %zu ids, model %zu\n", round, e.first.first.c_str(), e.first.second.c_str(), got.size(),
                            want.size());
                    return 1;
                }
            }
        }
        if (h.built) { // fan-out grouping of a random CSR (ids live, deleted and never handed out) against the model
            std::map<uint32_t, const std::string*> by_id;
            for (auto& e : model) by_id[e.second] = &e.first;
            const uint32_t n_rows = 1 + (uint32_t)rnd(rnd(4) == 0 ? 800 : 40); // now and then enough pairs for several host threads
            std::vector<uint32_t> row{0}, ids;
            for (uint32_t r = 0; r < n_rows; r++) {
                std::set<uint32_t> s;
                for (size_t k = rnd(4) ? rnd(30) : 0; k > 0; k--) s.insert((uint32_t)rnd(next_id + 3));
                ids.insert(ids.end(), s.begin(), s.end());
                row.push_back((uint32_t)ids.size());
            }
            const uint32_t total = (uint32_t)ids.size(), gcap = 64;
            std::vector<uint32_t> ot(total + 1), orr(total + 1), goff(gcap + 1), grep(gcap);
            ids.resize(total + 4);
            FanoutResult fr;
            if (!fo.group(row.data(), ids.data(), n_rows, total, ot.data(), orr.data(), goff.data(), grep.data(), gcap, fr) || fr.group_overflow) {
                fprintf(stderr, "round %d: fan-out grouping failed: %s\n", round, fo.error.c_str());
                return 1;
            }
            // model: DelivererKey (subBrokerId, delivererKey) / "shared" / "dead" -> pairs in (row, id) order
            std::map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> want, got;
            for (uint32_t r = 0; r < n_rows; r++)
                for (uint32_t k = row[r]; k < row[r + 1]; k++) {
                    auto it = by_id.find(ids[k]);
                    std::string name = "dead";
                    if (it != by_id.end()) {
                        RouteKeyParts kp;
                        decode_route_key(*it->second, kp);
                        if (kp.flag != 1) name = "shared";
                        else {
                            const auto parts = split(kp.receiver, '\0');
                            name = "k:" + parts[0] + "|" + parts[2];
                        }
                    }
                    want[name].push_back({r, ids[k]});
                }
            bool bad = goff[0] != 0 || goff[fr.n_groups] != total;
            for (uint32_t g = 0; g < fr.n_groups && !bad; g++) {
                std::string name = grep[g] == 0xFFFFFFFFu ? "dead" : grep[g] == 0xFFFFFFFEu ? "shared" : "";
                if (name.empty()) {
                    auto it = by_id.find(grep[g]);
                    if (it == by_id.end()) {
                        bad = true;
                        break;
                    }
                    RouteKeyParts kp;
                    decode_route_key(*it->second, kp);
                    const auto parts = split(kp.receiver, '\0');
                    name = "k:" + parts[0] + "|" + parts[2];
                }
                if (got.count(name)) bad = true;
                for (uint32_t k = goff[g]; k < goff[g + 1]; k++) got[name].push_back({ot[k], orr[k]});
            }
            const uint32_t sp = (want.count("shared") ? 1u : 0u) | (want.count("dead") ? 2u : 0u);
            if (bad || got != want || fr.special != sp) {
                fprintf(stderr, "round %d: fan-out groups differ from the model (%zu vs %zu groups, special %u vs %u)\n", round, got.size(), want.size(),
                        fr.special, sp);
                return 1;
            }
            fo_pairs += total;
            // ---- the delivery plan of the same CSR (bmq_delivery.h) against a plain merge, by key BYTES, of the groups above and a resolve of
            // their shared slice.  Members live under the deliverer keys of normal routes (so that groups merge) and under keys of their own.
            std::map<uint32_t, std::vector<std::string>> tabs;
            {
                std::vector<std::string> normal_dk;
                for (auto& e : by_id) {
                    RouteKeyParts kp;
                    decode_route_key(*e.second, kp);
                    const auto parts = split(kp.receiver, '\0');
                    if (kp.flag == 1 && parts.size() == 3) normal_dk.push_back(parts[0] + std::string("\0", 1) + "m" + std::to_string(rnd(3)) + std::string("\0", 1) + parts[2]);
                }
                std::vector<uint32_t> t_ids, moff{0}, uoff{0};
                std::vector<uint8_t> urls;
                for (auto& e : by_id) {
                    RouteKeyParts kp;
                    decode_route_key(*e.second, kp);
                    if (kp.flag == 1 || rnd(4) == 0) continue;
                    auto& t = tabs[e.first];
                    for (size_t m = 1 + rnd(4); m > 0; m--) {
                        if (!normal_dk.empty() && rnd(2)) t.push_back(normal_dk[rnd(normal_dk.size())]);
                        else t.push_back(std::to_string(rnd(3)) + std::string("\0", 1) + "r" + std::to_string(m) + std::string("\0", 1) + "own" + std::to_string(rnd(4)));
                        urls.insert(urls.end(), t.back().begin(), t.back().end());
                        uoff.push_back((uint32_t)urls.size());
                    }
                    t_ids.push_back(e.first);
                    moff.push_back((uint32_t)(uoff.size() - 1));
                }
                sh_plan.drop();
                if (!t_ids.empty() && !sh_plan.apply(h, t_ids.data(), (uint32_t)t_ids.size(), moff.data(), urls.data(), uoff.data())) {
                    fprintf(stderr, "round %d: delivery plan: share apply failed: %s\n", round, sh_plan.error.c_str());
                    return 1;
                }
            }
            std::vector<uint32_t> s_off{0}, s_hash;
            for (uint32_t r = 0; r < n_rows; r++) {
                for (size_t k = rnd(4); k > 0; k--) s_hash.push_back((uint32_t)rnd(1ull << 32));
                s_off.push_back((uint32_t)s_hash.size());
            }
            s_hash.resize(s_hash.size() + 4);
            const unsigned long long nonce = rnd(1ull << 62);
            using Row = std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>; // topic, route, sender, member
            auto key_name = [&](uint32_t route, uint32_t member) -> std::string {
                if (member != SH_NONE) {
                    const auto parts = split(tabs[route][member], '\0');
                    return "k:" + parts[0] + "|" + parts[2];
                }
                RouteKeyParts kp;
                decode_route_key(*by_id.at(route), kp);
                const auto parts = split(kp.receiver, '\0');
                return "k:" + parts[0] + "|" + parts[2];
            };
            std::map<std::string, std::vector<Row>> want_plan, got_plan;
            uint32_t s_lo = total, s_hi = total;
            for (uint32_t g = 0; g < fr.n_groups; g++) {
                if (grep[g] == 0xFFFFFFFEu) {
                    s_lo = goff[g], s_hi = goff[g + 1];
                    continue;
                }
                const std::string name = grep[g] == 0xFFFFFFFFu ? "dead" : key_name(grep[g], SH_NONE);
                for (uint32_t k = goff[g]; k < goff[g + 1]; k++) want_plan[name].push_back(Row{ot[k], orr[k], SH_NONE, SH_NONE});
            }
            const uint32_t rcap = (s_hi - s_lo) * 4 + 4;
            std::vector<uint32_t> rp(rcap), rs(rcap), rm(rcap), rgo(rcap + 1);
            ShareResult sres;
            if (!sh_plan.resolve(h, ot.data() + s_lo, orr.data() + s_lo, s_hi - s_lo, s_off.data(), s_hash.data(), n_rows, s_off.back(), nonce, rp.data(), rs.data(),
                                 rm.data(), rcap, rgo.data(), rcap, sres) || sres.overflow) {
                fprintf(stderr, "round %d: delivery plan: resolve failed: %s\n", round, sh_plan.error.c_str());
                return 1;
            }
            for (uint32_t k = 0; k < sres.n_rows; k++) {
                const uint32_t t = ot[s_lo + rp[k]], route = orr[s_lo + rp[k]];
                want_plan[rm[k] == SH_NONE ? std::string("unresolved") : key_name(route, rm[k])].push_back(Row{t, route, rs[k], rm[k]});
            }
            for (auto& e : want_plan) std::sort(e.second.begin(), e.second.end());
            const uint32_t n_want_rows = total - (s_hi - s_lo) + sres.n_rows;
            std::vector<uint32_t> pt(n_want_rows + 1), pr(n_want_rows + 1), pa(n_want_rows + 1), ps(sres.n_rows + 1), pm(sres.n_rows + 1), pgo(want_plan.size() + 2);
            DeliveryResult dr;
            if (!dl.plan(fo, sh_plan, h, row.data(), ids.data(), n_rows, total, s_off.data(), s_hash.data(), s_off.back(), nonce, pt.data(), pr.data(), pa.data(), n_want_rows,
                         ps.data(), pm.data(), sres.n_rows, pgo.data(), (uint32_t)want_plan.size(), dr) || dr.overflow) {
                fprintf(stderr, "round %d: delivery plan failed (%u rows, %u share rows, %u groups; the merge has %u, %u, %zu): %s\n", round, dr.n_rows, dr.n_share_rows,
                        dr.n_groups, n_want_rows, sres.n_rows, want_plan.size(), dl.error.c_str());
                return 1;
            }
            bool bad_plan = dr.n_rows != n_want_rows || dr.n_share_rows != sres.n_rows || dr.n_groups != want_plan.size() || pgo[0] != 0 || pgo[dr.n_groups] != dr.n_rows;
            uint32_t n_merged = 0;
            for (uint32_t g = 0; g < dr.n_groups && !bad_plan; g++) {
                std::vector<Row> rows_g;
                std::string name;
                bool both[2] = {false, false};
                for (uint32_t k = pgo[g]; k < pgo[g + 1] && !bad_plan; k++) {
                    const uint32_t a = pa[k];
                    if (a != SH_NONE && a >= dr.n_share_rows) {
                        bad_plan = true;
                        break;
                    }
                    const Row rw{pt[k], pr[k], a == SH_NONE ? SH_NONE : ps[a], a == SH_NONE ? SH_NONE : pm[a]};
                    std::string nm;
                    if (a != SH_NONE) nm = pm[a] == SH_NONE ? std::string("unresolved") : key_name(pr[k], pm[a]);
                    else nm = by_id.count(pr[k]) ? std::string() : std::string("dead");
                    if (nm.empty()) {
                        RouteKeyParts kp;
                        decode_route_key(*by_id.at(pr[k]), kp);
                        nm = kp.flag == 1 ? key_name(pr[k], SH_NONE) : std::string("dead?");
                    }
                    both[a != SH_NONE] = true;
                    if (k == pgo[g]) name = nm;
                    bad_plan |= nm != name; // every row of a group names the group's DelivererKey
                    rows_g.push_back(rw);
                }
                bad_plan |= rows_g.empty() || got_plan.count(name) || !std::is_sorted(rows_g.begin(), rows_g.end());
                n_merged += both[0] && both[1];
                got_plan[name] = std::move(rows_g);
            }
            if (!bad_plan && dr.n_groups) { // the special groups come last: unresolved, then dead
                const uint32_t n_sp = (dr.special & 1u) + ((dr.special >> 1) & 1u);
                bad_plan |= ((dr.special & 1u) != 0) != (want_plan.count("unresolved") != 0) || ((dr.special & 2u) != 0) != (want_plan.count("dead") != 0);
                if (!bad_plan && (dr.special & 2u)) bad_plan |= pa[pgo[dr.n_groups - 1]] != SH_NONE || by_id.count(pr[pgo[dr.n_groups - 1]]);
                if (!bad_plan && (dr.special & 1u)) bad_plan |= pa[pgo[dr.n_groups - n_sp]] == SH_NONE || pm[pa[pgo[dr.n_groups - n_sp]]] != SH_NONE;
            }
            if (bad_plan || got_plan != want_plan || n_merged != dr.n_merged_groups) {
                fprintf(stderr, "round %d: the delivery plan differs from the merge of its parts (%zu vs %zu groups, %u vs %u rows, special %u, merged %u vs %u)\n", round,
                        got_plan.size(), want_plan.size(), dr.n_rows, n_want_rows, dr.special, dr.n_merged_groups, n_merged);
                return 1;
            }
            dl_rows += dr.n_rows;
            dl_merged += dr.n_merged_groups;
            if (!check_filters(round, h, by_id, row, ids, false)) return 1;
        }
        for (int tq = 0; tq < 150; tq++) {
            const std::string& tn = tq % 25 == 24 ? std::string("nobody") : tenants[rnd(tenants.size())];
            const std::string topic = rand_topic();
            const auto tl = split(topic, '/');
            std::vector<uint32_t> want;
            for (auto& d : dec)
                if (d.tenant == tn && filter_matches(d.levels, tl)) want.push_back(d.id);
            std::sort(want.begin(), want.end());
            const auto got = image_match(h, tn, topic, nullptr, plus_stat);
            checks++;
            if (got != want) {
                fprintf(stderr, "round %d (%s): tenant '%s' topic '%s': image gives %zu ids, the rule %zu\n", round, full ? "rebuild" : "apply", tn.c_str(),
                        topic.c_str(), got.size(), want.size());
                for (uint32_t id : want)
                    if (!std::binary_search(got.begin(), got.end(), id)) fprintf(stderr, "  missing id %u\n", id);
                for (uint32_t id : got)
                    if (!std::binary_search(want.begin(), want.end(), id)) fprintf(stderr, "  extra id %u\n", id);
                return 1;
            }
        }
    }
    { // once per run: a row whose persistent class has more than CAPS_RANK_MAX members, in an index of its own, beside a short row and an empty one
        std::set<std::string> ks;
        for (uint32_t i = 0; i < CAPS_RANK_MAX + 40; i++)
            ks.insert(encode_route_key("t", "big/" + std::to_string(rnd(1000000)) + "/" + std::to_string(i), 1, "1" + std::string("\0", 1) + "inbox" + std::string("\0d", 2) + "0"));
        for (uint32_t i = 0; i < 12; i++) ks.insert(encode_route_key("t", "big/g/" + std::to_string(i), (uint8_t)(2 + i % 2), "g" + std::to_string(i)));
        for (uint32_t i = 0; i < 12; i++) ks.insert(encode_route_key("t", "big/t/" + std::to_string(i), 1, "0" + std::string("\0", 1) + "inbox" + std::string("\0d", 2) + "0"));
        std::vector<std::string> keys(ks.begin(), ks.end());
        std::vector<uint8_t> bytes;
        std::vector<uint32_t> off{0};
        for (auto& k : keys) {
            bytes.insert(bytes.end(), k.begin(), k.end());
            off.push_back((uint32_t)bytes.size());
        }
        bytes.resize(bytes.size() + 16, 0);
        DistIndex<HostExec> big(hx);
        if (!big.rebuild(bytes.data(), off.data(), (uint32_t)keys.size())) {
            fprintf(stderr, "the index of the long row: rebuild failed: %s\n", big.error.c_str());
            return 1;
        }
        std::map<uint32_t, const std::string*> by_id; // (ids are the ranks)
        std::vector<uint32_t> row{0}, ids;
        for (uint32_t i = 0; i < keys.size(); i++) by_id[i] = &keys[i], ids.push_back(i);
        std::shuffle(ids.begin(), ids.end(), rng); // the input's order is not the keys'
        ids.push_back((uint32_t)keys.size() + 5); // (an id never handed out)
        row.push_back((uint32_t)ids.size());
        row.push_back((uint32_t)ids.size());
        for (uint32_t i = 0; i < 9; i++) ids.push_back(i * 7);
        row.push_back((uint32_t)ids.size());
        if (!check_filters(rounds, big, by_id, row, ids, true)) return 1;
    }
    printf("caps and gate: %llu ids in, %llu / %llu kept, %llu events, %llu rows ranked on the host\n", (unsigned long long)flt_in, (unsigned long long)flt_caps_kept,
           (unsigned long long)flt_gate_kept, (unsigned long long)flt_events, (unsigned long long)flt_host_rows);
    DistIndexStats st;
    h.stats(st);
    printf("layout v3: %llu of the %llu nodes the checks discovered through a '+' edge below a non-root node lay beside their parent\n", (unsigned long long)plus_stat[0], (unsigned long long)plus_stat[1]);
    printf("reads in key order: %llu windows, %llu sweeps (%llu wrapped); %llu bucketing rounds, %llu buckets ranked\n", (unsigned long long)n_windows, (unsigned long long)n_sweeps,
           (unsigned long long)n_sweeps_wrapped, (unsigned long long)order_stats.n_rounds, (unsigned long long)order_stats.n_bucket_sorts);
    if (n_windows == 0 || n_sweeps == 0 || n_sweeps_wrapped == 0 || (n_windows_over_a_bucket != 0 && order_stats.n_rounds == 0)) {
        fprintf(stderr, "the reads in key order were not exercised\n");
        return 1;
    }
    printf("find and carry: %llu keys looked up, %llu carries (%llu tables carried, %llu dropped)\n", (unsigned long long)n_find, (unsigned long long)n_carries,
           (unsigned long long)n_tables_carried, (unsigned long long)n_tables_dropped);
    printf("delivery plan: %llu rows planned, %llu groups held normal and member rows\n", (unsigned long long)dl_rows, (unsigned long long)dl_merged);
    printf("host_fuzz ok: seed %llu, %d rounds (%llu rebuilds, %llu applies, %llu generation changes, %llu bounded ones, %llu imports, %llu tenant censuses), %llu topic checks, final %zu routes, %llu nodes, %llu tokens, "
           "%llu trie slots (%llu garbage), %llu id-list words (%llu garbage), %llu fan-out pairs grouped\n",
           (unsigned long long)seed, rounds, (unsigned long long)n_rebuild, (unsigned long long)n_apply, (unsigned long long)n_generations, (unsigned long long)n_bounded, (unsigned long long)n_imports, (unsigned long long)n_census, (unsigned long long)checks, model.size(),
           (unsigned long long)st.n_nodes, (unsigned long long)st.n_tokens, (unsigned long long)st.trie_slots, (unsigned long long)st.trie_garbage_slots,
           (unsigned long long)st.id_list_words, (unsigned long long)st.id_list_garbage, (unsigned long long)fo_pairs);
    return 0;
}
