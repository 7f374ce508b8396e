/*
 * bmq.h -- C ABI of the MI355X-native MQTT topic-match engine (libbmq.so).
 *
 * This is the drop-in boundary.  The reference (apache/bifromq, 100 % Java) has no FFI of its own;
 * each entry point below names the Java seam it sits behind (paths relative to the reference root,
 * DW = bifromq-dist/bifromq-dist-worker/src/main/java/org/apache/bifromq/dist/worker,
 * RS = bifromq-retain/bifromq-retain-store/src/main/java/org/apache/bifromq/retain/store,
 * SCHEMA = bifromq-dist/bifromq-dist-worker-schema/src/main/java/org/apache/bifromq/dist/worker/schema,
 * KVAPI = base-kv/base-kv-store-coproc-api/src/main/java/org/apache/bifromq/basekv/store/api).
 * INTEGRATION.md shows the JNI stub a maintainer would add on the Java side.
 *
 * Conventions
 *   - every function returns BMQ_OK (0) or a negative bmq_status; nothing throws across the ABI;
 *   - strings are packed: `bytes` + `off[n+1]` (uint32 byte offsets, off[0] == 0), UTF-8, not NUL-terminated;
 *   - a route id is a STABLE handle of one route key.  bmq_rebuild numbers the routes by the RANK of their KV key in
 *     unsigned-byte order (== KV iteration order, the order MatchedRoutes applies fan-out caps in,
 *     DW/cache/MatchedRoutes.java:87-141); a route added later by bmq_routes_apply gets the next unused id.  An id never
 *     changes and is never given to another key until the next bmq_rebuild (bmq_index_info.generation counts rebuilds);
 *     the id of a deleted route resolves to "no such route".  bmq_route_key() / bmq_route_keys() map ids back to keys;
 *     bmq_match_all() applies the fan-out caps in KEY order whatever the ids are;
 *   - match results are CSR: row_ptr[n+1] + ids, ids ascending inside each row;
 *   - buffers are caller-owned; *_dev variants take DEVICE pointers (HBM-resident inputs/outputs) and
 *     run asynchronously on the engine's HIP stream until bmq_match_finish().  Device string buffers (tenants,
 *     topics, filters) must be 16-byte aligned and readable 16 bytes past their last byte (the kernels read them in
 *     aligned words); the host-buffer variants stage and pad internally, so host callers have no such duty;
 *   - thread-safety: every call on one engine is serialised internally (matcher threads of the reference's
 *     ForkJoinPool, DW/DistWorkerCoProcFactory.java:74-88, may all call into it); ONE device batch may be in flight
 *     per engine through the *_dev protocol: bmq_match_batch_dev / bmq_retain_match_batch_dev take the engine for their caller
 *     until the SAME thread calls bmq_match_finish (other threads' calls wait; another thread's *_dev launch gets BMQ_E_STATE).
 *     bmq_match_submit / bmq_match_wait keep up to BMQ_MAX_TICKETS host batches in flight.  Use one engine per KV range replica.
 *   - the engine REQUIRES a gfx950 device for every match call.  There is no CPU fallback: without a
 *     device bmq_engine_create(device >= 0) fails with BMQ_E_NODEVICE.
 */
#ifndef BMQ_H
#define BMQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum bmq_status {
    BMQ_OK = 0,
    BMQ_E_INVAL = -1,     /* bad argument / malformed route key                                   */
    BMQ_E_NODEVICE = -2,  /* no HIP device (or engine created host-only) -- match is impossible    */
    BMQ_E_NOSPACE = -3,   /* caller's output buffer too small; *out_needed tells the size          */
    BMQ_E_NOMEM = -4,     /* host or device allocation failed                                      */
    BMQ_E_HIP = -5,       /* a HIP runtime call failed; see bmq_last_error()                       */
    BMQ_E_RANGE = -6,     /* a 32-bit size limit of the ABI exceeded (>= 2^32 ids in one batch...) */
    BMQ_E_STATE = -7      /* call not valid in this state (e.g. match before rebuild)              */
} bmq_status;

typedef struct bmq_engine bmq_engine;

/* Tunables.  Zero-initialise, set struct_size = sizeof(bmq_config), override what you need.
 * The *_cap fields exist so tests can force the LDS overflow (global spill) paths; 0 = default. */
typedef struct bmq_config {
    uint32_t struct_size;
    int32_t device;            /* HIP device ordinal; -1 = host-only engine (build/inspect, no match)      */
    uint32_t wave_queue_cap;   /* per-wave LDS work stack of the walk kernel.  Its LDS geometry is compiled in, so the two caps are a  */
                               /* SELECTOR, not sizes: 0 = default (176 stack items / 152 range entries); 128 in either = the smallest */
                               /* lists (128 / 128: tests force the overflow paths with them).  Any other value is refused           */
                               /* (BMQ_E_INVAL): it would silently run the default.  Overflow is parked in global memory, never an error */
    uint32_t wave_pair_cap;    /* per-wave LDS matched-range buffer: 0 or 128, as above                                          */
    uint32_t slow_scratch_mb;  /* global scratch for the per-lane DFS slow path (default 64)               */
    uint32_t kernel_timing;    /* 1: HIP events around k_walk / k_expand of every batch -> bmq_stats.ms_walk /  */
                               /* ms_expand (two extra events per batch, ~4 us each on the stream); 0: ms_total  */
    uint32_t dedup_min_topics; /* a batch of at least this many topics is de-duplicated on the device first: identical      */
                               /* (tenant, topic) rows are walked once, every row keeps its own row in the result (matchAll   */
                               /* takes a Set<String>, TenantRouteMatcher.java:67-78).  0 = default = UINT32_MAX = never: on  */
                               /* the survey's Zipf batches it takes 16 % off the walk kernel and costs more than that in the */
                               /* two kernels around it                                                 */
    uint32_t dedup_sorted;     /* 1: the caller's batches are ORDERED by (tenant index, topic bytes) -- BatchDistRequest is "sorted by   */
                               /* tenantId and topic" (DistWorkerCoProc.proto:75-83) --, so the de-duplication above compares a row with */
                               /* the row before it instead of hashing, and the walk runs on a dense copy of the distinct rows.  Only    */
                               /* speed depends on the order: a row that equals no neighbour is matched on its own.  0 = hash.          */
                               /* Measured on the survey's 1 M-publish batch (profiles/r05b/): 56 us of de-duplication (hash: 125 us)  */
                               /* for 31 us less walking -- a loss there; a caller that sends every topic ONCE gains 17 %              */
    uint32_t region_slack;     /* a tenant's region of the filter trie holds nodes x (1 + region_slack / 4) buckets of two 32-byte slots:    */
                               /* 0 = default = 6 (load factor 0.2, 160 bytes of region per trie node); 1 = load factor 0.4 (64 + 16 bytes  */
                               /* per node: the layout of rounds 2-5; k_walk is 8 % slower on the survey's workload -- more second probes), */
                               /* up to 64.  A memory / speed trade, nothing else depends on it                                            */
    uint32_t tail_records;     /* 0 = default = on: after a bulk load and before a compacted generation serves, a node whose subtree is a   */
                               /* unary chain of <= 4 levels with the routes at its end gets a 32-byte TAIL RECORD in the free slot of its   */
                               /* line (the chain's tokens + its leaf's payload): the walk resolves the chain from the line it already has. */
                               /* A put / delete whose path runs through the node invalidates the record (a tombstone); a region growth     */
                               /* drops it; the next rebuild / compaction forms records again.  1 = off (no records).  Results are the same */
                               /* either way                                                                           */
    uint32_t child_filters;    /* 0 = default = on: the walk kernel also asks a node's CHILD FILTER WORDS -- the begin word of each of its    */
                               /* empty route ranges, 32 more filter bits over its literal children that the index builder maintains --      */
                               /* before it probes for a literal child: fewer probes for children that do not exist.  1 = the walk ignores    */
                               /* the words (the builder keeps them all the same).  Results are the same either way    */
    uint32_t retain_builder;   /* who BULK-LOADS the retained-topic index (bmq_retain_rebuild*, bmq_retain_compact, bmq_retain_import into an empty   */
                               /* engine): 0 = default = the host builder (host threads, parallel over tenants; the image is uploaded); 1 = the      */
                               /* executor builder (bmq_retain_build_core.h): sorts, scans and CAS inserts as gfx950 kernels on a device engine, the  */
                               /* same functions on host threads on a device = -1 engine; the arrays are built where the walk reads them.  Topic ids, */
                               /* results and every other call are the same either way; bmq_retain_build_info_get says which one built the serving    */
                               /* generation.  3 = 1, and the executor builder also serves the generation change that does not stop the world,       */
                               /* bmq_retain_compact_begin[_in] / _build / _swap (see there); under 0 and 1 those three stay the host builder's.      */
                               /* Any other value (2 included: the generation change needs the bulk loader): BMQ_E_INVAL                              */
    uint32_t share_carry;      /* what a generation change of the route index does with the member tables of shared subscriptions                      */
                               /* (bmq_share_members_apply): 0 = default = they are dropped; 1 = bmq_compact and bmq_compact_swap carry every table to  */
                               /* the id its route KEY has in the new generation, on the device (see bmq_share_members_apply, bmq_share_carry_info_get). */
                               /* Any other value: BMQ_E_INVAL                                                                                          */
} bmq_config;

/* Counters of the last completed match batch (for roofline accounting). */
typedef struct bmq_stats {
    uint64_t n_topics;
    uint64_t n_visit;        /* filter-trie nodes discovered (root excluded), all topics                    */
    uint64_t n_match;        /* route ids emitted                                                           */
    uint64_t n_ranges;       /* matched (filter node) ranges                                                */
    uint64_t n_slow_topics;  /* topics resolved by the slow path (more than 16 levels)                     */
    uint64_t n_sorted_rows;  /* rows that needed the element-level fix-up sort                              */
    uint64_t topic_bytes;    /* sum of topic lengths                                                        */
    float ms_total;          /* HIP-event time of the whole batch on the engine stream (0 for batches of fewer */
                             /* than 4096 topics unless bmq_config.kernel_timing: the two events cost ~8 us)  */
    float ms_walk;           /* ... of the tokenise+walk kernel alone (0 unless bmq_config.kernel_timing)   */
    float ms_expand;         /* ... of the expand kernel alone (0 unless bmq_config.kernel_timing)          */
    uint32_t n_walked;       /* rows the walk kernel walked: n_topics, fewer with bmq_config.dedup_sorted (the distinct  */
                             /* rows), 0 = not counted (the hashing de-duplication)                                       */
    uint32_t n_split_blocks; /* 64-row blocks of the batch the expand kernel gave to four waves each (blocks of more than  */
                             /* ~2 x the ranges / ids of the mean block: batches of 65536 rows and more)                   */
    uint32_t reserved0;
} bmq_stats;

typedef struct bmq_index_info {
    uint64_t n_routes, n_tenants, n_nodes, n_tokens;
    uint64_t trie_slots, dict_slots;      /* table sizes in 32-byte slots (trie: sum of the tenant regions)  */
    uint64_t device_bytes;                /* HBM held by the index                                          */
    uint64_t epoch;                       /* +1 per bmq_rebuild / bmq_routes_apply                          */
    uint64_t generation;                  /* +1 per bmq_rebuild: ids of different generations are unrelated */
    uint64_t next_route_id;               /* ids handed out so far (live + deleted)                         */
    uint64_t garbage_bytes;               /* HBM held by abandoned regions / id lists until the next rebuild */
} bmq_index_info;

/* ---- lifecycle -------------------------------------------------------------------------------------- */
/* One engine per KV range replica, like DistWorkerCoProc's SubscriptionCache
 * (DW/DistWorkerCoProcFactory.java:91-93). */
int bmq_engine_create(const bmq_config* cfg, bmq_engine** out);
void bmq_engine_destroy(bmq_engine* e);
const char* bmq_last_error(const bmq_engine* e);
const char* bmq_version(void);

/* ---- dist direction: index maintenance -------------------------------------------------------------- */
/* Full (re)load from a KV scan -- replaces IKVRangeCoProc.reset(Boundary) (KVAPI/IKVRangeCoProc.java:64,
 * DW/DistWorkerCoProc.java:283-291).  keys = route keys in the layout of SCHEMA/KVSchemaUtil.java:91-130 (the packed bytes
 * must be readable 16 bytes past the last key).  The keys are uploaded and parsed, and the index is built, ON THE DEVICE
 * (builder kernels, bmq_build_core.h).  A KV iterator yields the keys strictly ascending: that is the fast path and route
 * id = position = rank; any other order is sorted + de-duplicated on the host first.  On failure the previous index is gone. */
int bmq_rebuild(bmq_engine* e, const uint8_t* keys, const uint32_t* key_off, uint32_t n_keys);

/* Post-commit route mutations -- replaces ISubscriptionCache.refresh(AddRoutesTask/RemoveRoutesTask)
 * (DW/DistWorkerCoProc.java:188-209, DW/cache/SubscriptionCache.java:127-134).  op[i]: 0 = put, 1 = delete.
 * Applied in order by builder kernels on the engine stream (between match batches, which therefore never see half a batch);
 * the call returns when the device has applied it.  A put of a key that is already there keeps its id, a delete of an absent
 * key is a no-op; the j-th put of the batch that adds a route gets id next_route_id + j.  A malformed key or op code fails
 * the whole batch with BMQ_E_INVAL before anything is changed. */
int bmq_routes_apply(bmq_engine* e, const uint8_t* keys, const uint32_t* key_off, const uint8_t* op, uint32_t n);
/* The same without the wait (DistWorkerCoProc applies a batch of mutations and goes on serving, DW/DistWorkerCoProc.java:188-209): the ops
 * are uploaded on the engine's copy stream -- beside a batch handed over with bmq_match_submit* that still runs --, the builder kernels are
 * queued behind that batch, the call returns after the enqueue.  The buffers (page-locked memory from bmq_host_alloc, or the upload is
 * not asynchronous) must stay untouched until the batch's outcome has been fetched: bmq_routes_apply_wait returns what bmq_routes_apply
 * would have returned (nothing is changed by a batch that holds a malformed key).  Every later call that reads or changes the route index
 * fetches the outcome first -- a match launched behind a failed batch returns that batch's error.  At most one batch is open: a second
 * bmq_routes_apply[_async] completes the first. */
int bmq_routes_apply_async(bmq_engine* e, const uint8_t* keys, const uint32_t* key_off, const uint8_t* op, uint32_t n);
int bmq_routes_apply_wait(bmq_engine* e);

/* Route keys -> route ids, batched, where the index lives: out_ids[i] = id of the live route whose key equals keys[key_off[i] .. key_off[i + 1]),
 * 0xFFFFFFFF if there is none.  Keys are in the layout bmq_rebuild / bmq_routes_apply take, any flag (1 / 2 / 3), in any order, repeats
 * included (the packed bytes need no padding).  This is how a caller learns the ids of the keys it put: bmq_routes_apply says only that the
 * j-th put THAT ADDS A ROUTE gets next_route_id + j.  A malformed key fails the call with BMQ_E_INVAL, as it fails bmq_routes_apply; n = 0
 * returns BMQ_OK.  The call is read-only: one lane per key walks the index on the device (k_b_find_keys: the read-only half of what a
 * delete does) and creates no dictionary token, no trie node and no filter bit, invalidates no tail record and leaves the epoch alone.
 * Locks and state are those of bmq_route_keys / bmq_routes_count_in: an open bmq_routes_apply_async batch is completed first; while a
 * compaction runs the SERVING generation answers (keys mutated since bmq_compact_begin included); the persistent matcher keeps running (it leaves only
 * when the call's own upload buffers have to grow -- the first call and every larger batch: a free waits for every stream of the device).  A key
 * of 16 MiB or more is malformed.
 * A host-only engine runs the same per-key function on host threads. */
int bmq_routes_find(const bmq_engine* e, const uint8_t* keys, const uint32_t* key_off, uint32_t n, uint32_t* out_ids);

/* ---- reads in KEY order: a window of the route keys, and the dist worker's GC sweep over it ------------------------------------
 * The index holds every route key in device memory, under ids that follow the key order only right after bmq_rebuild.  A WINDOW is
 * what a KV iterator gives after seek(lo): the ids of the first min(max_routes, C) of the C live routes whose key is >= lo (> lo with
 * lo_exclusive != 0; lo NULL: from the first key; a present lo may be empty), ascending in KV order -- unsigned bytes, a proper prefix
 * first, as BoundaryUtil orders keys.  *out_more = 1 if a further live key follows the window.  lo is compared as bytes: it need not
 * be a well-formed route key.  max_routes <= BMQ_WINDOW_MAX (more: BMQ_E_INVAL); out_route_ids holds max_routes ids.
 * Read-only, on the device: one pass flags and compacts the candidates, rounds of <= 255 pivot keys narrow them to max_routes and
 * split them into buckets, each bucket is ranked by counting, a wave per key (bifromq_amd/csrc/bmq_order_kernels.h).  The key bytes stay where they
 * are; only the cursor goes up and counters and ids come down.  Locks and state are those of bmq_routes_find / bmq_routes_count_in:
 * an open bmq_routes_apply_async batch is completed first, the SERVING generation answers while a compaction runs, the epoch stays;
 * the persistent matcher leaves only when the call's scratch has to grow (the first call, and after the id space grew).  A host-only
 * engine runs the same passes on the host.  FanoutSplitHinter.doEstimate (bifromq-dist-worker/.../hinter/FanoutSplitHinter.java:
 * 187-198) is one window: seek(prefix), split_at_scale steps, the key there. */
#define BMQ_WINDOW_MAX 65536u
int bmq_routes_window(const bmq_engine* e, const uint8_t* lo, uint32_t lo_len /* lo NULL: from the first key */, uint32_t lo_exclusive,
                      uint32_t max_routes, uint32_t* out_route_ids, uint32_t* out_n, uint32_t* out_more);
/* DistWorkerCoProc.gc (bifromq-dist-worker/.../DistWorkerCoProc.java:554-701; DistWorkerCleaner.java:57-66,216-217 drives it) over
 * positions of the key order K[0 .. N): step = max(step_hint, 1), quota = scan_quota > 0 ? scan_quota : 256 * step, p0 = the position
 * of the first key >= start_key (0: start_key NULL).  N == 0 or p0 == N: inspected 0, wrapped 1, no next key (:584-591; also when keys
 * lie in front of the cursor).  Else positions p0, p0 + step, ... are inspected; running off the tail the first time sets wrapped and
 * goes on at position 0 (the stride's phase is not kept), where the sweep stops in front of a position that holds K[p0] -- tested at
 * inspected positions only, so a stride that jumps over p0 goes on and inspects routes again (:613-617) -- and running off the tail a
 * second time ends it without a next key.  After the quota-th inspection the cursor moves ONE position on and the sweep ends
 * (:654-657).  has_next / next_route_id name the key under the cursor when the sweep ends, if there is one (nextStartKey, :669-671;
 * bmq_route_key gives its bytes).  out_route_ids[0 .. inspected) are the inspected routes in inspection order; cap < inspected:
 * BMQ_E_NOSPACE with out->inspected = the count needed.  The keys come from successive windows of <= BMQ_WINDOW_MAX, each behind the
 * last key of the one before; a sweep that could span more than 16 of them per phase ((quota - 1) * step + 2 keys) is refused with
 * BMQ_E_INVAL -- the reference's largest is 51 200 keys.  The boundary clamp of :563-574 is the caller's (the engine holds exactly its
 * range's keys), and so are the routeCache.isCached filter, the members of group routes and the CheckRequests. */
typedef struct bmq_gc_sweep_reply { uint32_t struct_size, inspected, wrapped, has_next, next_route_id; uint64_t epoch; } bmq_gc_sweep_reply;
int bmq_routes_gc_sweep(const bmq_engine* e, const uint8_t* start_key, uint32_t start_len /* start_key NULL: absent */, uint32_t step_hint,
                        uint32_t scan_quota, uint32_t* out_route_ids, uint32_t cap /* < inspected: BMQ_E_NOSPACE, reply.inspected = needed */,
                        bmq_gc_sweep_reply* out);
/* Cumulative counters of the windows of this engine (those of sweeps included): calls, candidates behind the cursors, bucketing rounds,
 * buckets ranked, the largest of them, rounds that split a bucket of an earlier round again; last_ms: host time of the last window or sweep. */
typedef struct bmq_window_info { uint32_t struct_size, window_max, bucket_max; uint64_t n_calls, n_candidates, n_rounds, n_bucket_sorts, max_bucket, n_rebucketed; double last_ms; } bmq_window_info;
int bmq_routes_window_info_get(const bmq_engine* e, bmq_window_info* out);

/* ---- per-prefix census: how many live routes lie under each of a batch of key prefixes ---------------------------------------------
 * What FanoutSplitHinter.doEstimate asks its KV range per matchRecordKeyPrefix of a mutation batch (bifromq-dist-worker/.../hinter/
 * FanoutSplitHinter.java:174-178: reader.size([prefix, upperBound(prefix)))), for ALL prefixes of the batch in one pass over the key
 * store.  Prefix i is prefixes[prefix_off[i] .. prefix_off[i + 1]); out_stats[4 i ..] = live keys under it with flag 1 (normal),
 * 2 (unordered share), 3 (ordered share), and the sum of their key lengths -- the columns of bmq_routes_tenant_stats.  A live key k
 * counts for prefix p iff len(k) >= len(p) and k[0, len(p)) == p: a key equal to the prefix counts, the empty prefix counts every
 * key.  A prefix is compared as bytes: it need not be a well-formed route key nor end at a level or field border, so the granularity
 * (a tenant, a filter, one route) is the caller's.  Prefixes come in any order; repeats get the same answer; they may nest to any
 * depth, and a key counts for EVERY prefix that is a prefix of it.  n = 0 returns BMQ_OK; n > BMQ_PREFIX_MAX or a prefix of 16 MiB or
 * more is BMQ_E_INVAL with nothing written.
 * Read-only.  The host sorts and de-duplicates the prefixes and links each to its parent (the longest other prefix that is a proper
 * prefix of it); on the device one lane per key reference finds the last prefix <= its key by binary search, walks up the parent links
 * to the first one that is a prefix of the key, and the wave adds to that deepest prefix only, reduced per wave as the tenant census is
 * (bifromq_amd/csrc/bmq_prefix_kernels.h); the sums are then carried from every prefix to its parent.  Only the prefix table goes up and
 * four counters per distinct prefix come down.  Locks and state are those of bmq_routes_count_in: an open bmq_routes_apply_async batch is
 * completed first, the SERVING generation answers while a compaction runs (keys mutated since bmq_compact_begin included), the epoch
 * stays; the persistent matcher leaves only when the call's own device buffers have to grow.  A host-only engine runs the same per-key
 * function on host threads. */
#define BMQ_PREFIX_MAX 65536u
int bmq_routes_prefix_census(const bmq_engine* e, const uint8_t* prefixes, const uint32_t* prefix_off /* n + 1 */, uint32_t n,
                             uint64_t* out_stats /* 4 * n */);
/* Cumulative counters of the prefix censuses of this engine: calls, prefixes passed, distinct prefixes, distinct prefixes that have a
 * parent, key references scanned, the longest chain of parent links seen; last_ms: host time of the last call. */
typedef struct bmq_prefix_census_info { uint32_t struct_size, prefix_max; uint64_t n_calls, n_prefixes, n_distinct, n_nested, n_keys_scanned, max_chain; double last_ms; } bmq_prefix_census_info;
int bmq_routes_prefix_census_info_get(const bmq_engine* e, bmq_prefix_census_info* out);

/* Maintenance: re-build the index from its own live routes (the keys are gathered from the HBM key store).  Frees what churn leaves
 * behind until then -- abandoned tenant regions and id lists, trie nodes and dictionary tokens of filters nobody subscribes to any
 * more (bmq_index_info.garbage_bytes) -- and re-numbers the route ids to ranks: a new generation, like bmq_rebuild. */
int bmq_compact(bmq_engine* e);
/* The same without the stall (TopicLevelTrie contracts as it goes, UTIL/index/TopicLevelTrie.java:257-384; GenerationalRangeIndex.java /
 * bifromq_amd/generations.py did this with two handles on the caller's side, shipping every key through the host).  The next generation of
 * the route index is built BESIDE the serving one, inside the engine: on its own executor and a lowest-priority stream, from the serving
 * generation's live keys -- gathered HBM to HBM: the key bytes never leave the device, nothing is sorted on the host --, in chunks the caller
 * paces from a maintenance thread while its matcher threads go on:
 *   bmq_compact_begin   starts one: sizes the next generation's regions, pools and tables from the serving one's (BMQ_E_STATE while one is
 *                       running; bmq_rebuild / bmq_compact are refused until it is swapped or aborted).
 *   bmq_compact_poll    carries the live keys among the next max_ids route ids over.  The engine lock is held only while the build stream is
 *                       put behind what the serving generation was told so far and a copy of the chunk's key references is ENQUEUED; the
 *                       gather, the builder kernels and the waits touch the new generation alone.  *out_done_permille = 1000: ready to swap.
 *                       Matching and bmq_routes_apply[_async] go on meanwhile; what is mutated is logged.  Measured (bench.py, compaction
 *                       leg: 10 M routes, 1 M-publish batches back to back on another thread): batch p99 0.35 -> 0.60 ms while it runs.
 *   bmq_compact_swap    replays the log, swaps the generations (no batch may be in flight: BMQ_E_STATE) and frees the old one.  Route ids are
 *                       re-numbered: bmq_index_info.generation + 1, ids of the old generation mean nothing any more (as after bmq_compact).
 *   bmq_compact_abort   drops the half-built generation.
 * One compaction call at a time (they serialise among themselves; call them from a maintenance thread, not from the matcher threads); a
 * host-only engine runs the same procedure over the host executor.  The log of mutations lives in host memory and grows until
 * bmq_compact_swap / _abort: a caller that begins a compaction finishes it.  Only the route index is covered (retained topics:
 * bmq_retain_compact). */
int bmq_compact_begin(bmq_engine* e);
int bmq_compact_poll(bmq_engine* e, uint32_t max_ids, uint32_t* out_done_permille);
int bmq_compact_swap(bmq_engine* e, uint64_t* out_carried /* may be NULL */, uint64_t* out_replayed /* may be NULL */);
int bmq_compact_abort(bmq_engine* e);

/* ---- split and merge by KV boundary, without a KV scan ---------------------------------------------------------------------------------
 * IKVRangeCoProc.reset(Boundary) fires when a dist-worker range is split or merged (DW/DistWorkerCoProc.java:283-291); the reference's
 * matcher then scans tenantBoundary ^ rangeBoundary only (DW/cache/TenantRouteMatcher.java:81-86).  bmq_rebuild answers it with a full KV
 * scan; the three calls below answer it from the keys the engine already holds in device memory.
 *
 * Boundary arguments, as bmq_router_lookup_boundary takes them: flags bit 0 = a start key is present, bit 1 = an end key is present; a
 * present key may be empty.  A key is inside iff (no start or key >= start) and (no end or key < end), unsigned lexicographic, a proper
 * prefix first: BoundaryUtil.inRange (base-kv/.../utils/BoundaryUtil.java:241-252).  Both present with start >= end: BMQ_E_INVAL.  No
 * start with an empty end (NULL_BOUNDARY) is valid and holds nothing.  BoundaryUtil.split (:509-533) cuts [start, end) at a key s into
 * [start, s) and [s, end): the two halves of the recipes below.
 *
 *   bmq_routes_count_in    live routes inside the boundary and the sum of their key lengths: the native reader.size(boundary)
 *                          (DW/hinter/FanoutSplitHinter.java:175-178).  One pass of the boundary kernel over a scratch copy of the key
 *                          references; the index is not changed.  An open bmq_routes_apply_async batch is completed first.
 *   bmq_compact_begin_in   bmq_compact_begin for a range that SHRINKS: the next generation takes the keys inside the boundary only
 *                          (bmq_compact_begin is this call with flags = 0).  bmq_compact_poll / _swap / _abort are used as before; tenants
 *                          that lie wholly outside get no region in the next generation, logged mutations of keys outside are not replayed.
 *                          *out_carried of the swap counts the keys inside that were carried over, *out_replayed the ops replayed.  The
 *                          serving generation matches and mutates over ALL its keys until the swap.  After the swap the engine does NOT
 *                          police later mutations against the boundary: base-kv routes a mutation to the range that owns its key.
 *   bmq_routes_import      puts every live key of src inside the boundary into dst, device memory to device memory, through dst's ordinary
 *                          apply path (unknown tenants are created, regions grow).  Blocking; chunks of at most 65536 route ids.  Empty
 *                          dst + [s, end) is the new sibling of a split; non-empty dst + the full boundary (flags = 0) is a merge.  It is a
 *                          mutation of dst: ids dst handed out stay valid, its generation is unchanged, its epoch advances.  Keys dst
 *                          already holds are counted in *out_dups and stored once; *out_imported counts the keys added.  src is locked
 *                          only while its key references are copied; it matches and mutates meanwhile (a key mutated during the call is
 *                          imported as the snapshot saw it).  BMQ_E_INVAL: dst == src, a host-only engine paired with a device engine, two
 *                          devices.  BMQ_E_STATE: a compaction runs on either engine, src already lends its keys to another import, dst
 *                          has a batch in flight.  Until the call returns bmq_rebuild / bmq_compact / bmq_compact_begin[_in] on src are
 *                          refused with BMQ_E_STATE, and src must not be destroyed.
 * A split of range A at key s:  bmq_routes_import(B, A, start = s)  then  bmq_compact_begin_in(A, end = s) ... bmq_compact_swap(A).
 * A merge of B into A:          bmq_routes_import(A, B, flags = 0).
 * Route ids cached outside the engine (bmq_route_cache) belong to a generation: bmq_route_cache_reset after a bounded swap or an import. */
int bmq_routes_count_in(const bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                        uint64_t* out_routes /* may be NULL */, uint64_t* out_key_bytes /* may be NULL */);
int bmq_compact_begin_in(bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len);
int bmq_routes_import(bmq_engine* dst, bmq_engine* src, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end,
                      uint32_t end_len, uint64_t* out_imported /* may be NULL */, uint64_t* out_dups /* may be NULL */);

/* ---- per-tenant statistics of the route index, without a KV scan ---------------------------------------------------------------------
 * TenantsStats.doReset walks every key of the range on every reset and counts, per tenant, normal routes and shared routes from the key's
 * flag (bifromq-dist/bifromq-dist-worker/.../TenantsStats.java:229-246); the tenant's space gauge asks reader.size(tenantSection)
 * (:140-162).  bmq_routes_tenant_stats answers both from the keys the engine holds: ONE read-only pass of the census kernel over the key
 * references (no scratch copy; a wave reduces its lanes per tenant before it adds), whatever the number of tenants.
 *
 * Boundary arguments as for bmq_routes_count_in (flags = 0: everything).  For every tenant with at least one live route inside the
 * boundary, in unsigned byte order of the tenant ids (a proper prefix first): its id bytes, packed into out_tenants with out_tenant_off
 * [n + 1], and four numbers in out_stats[4 i ..]: live keys with flag 1 (normal), 2 (unordered share), 3 (ordered share), and key_bytes,
 * the sum of their key lengths.  A tenant with nothing inside is left out (TenantsStats destroys an entry at isNoRoutes).  A shared-
 * subscription key counts ONCE (doReset: doAddSharedRoutes(tenantId, 1) per key); member counts live in the KV value, which the engine
 * does not hold.  key_bytes against reader.size: KEYS ONLY -- the caller adds the 8-byte value of every normal route.
 * Over the full boundary a tenant's three counts sum to its live routes and all tenants to bmq_index_info.n_routes; over any boundary the
 * sums equal bmq_routes_count_in's routes and bytes.
 *
 * Buffers: `cap` = tenants out_tenant_off (cap + 1 entries) and out_stats (4 * cap entries) have room for, tenants_cap = bytes of
 * out_tenants.  *out_n_tenants and *out_tenant_bytes (either may be NULL) always receive the needed sizes; BMQ_E_NOSPACE when a cap is too
 * small (offsets and numbers are still written when `cap` suffices).
 * Locks and state as bmq_routes_count_in: an open bmq_routes_apply_async batch is completed first; while a compaction runs the SERVING
 * generation is read, after the swap the new one; nothing is changed and the persistent matcher keeps running. */
int bmq_routes_tenant_stats(const bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                            uint8_t* out_tenants, uint64_t tenants_cap, uint64_t* out_tenant_off, uint64_t* out_stats, uint32_t cap,
                            uint32_t* out_n_tenants /* may be NULL */, uint64_t* out_tenant_bytes /* may be NULL */);

int bmq_index_info_get(const bmq_engine* e, bmq_index_info* out);
/* id -> key (so the Java adapter can materialise Matching objects, SCHEMA/KVSchemaUtil.java:73-89).  BMQ_E_INVAL: no such
 * route (the id was never handed out, or its route has been deleted). */
int bmq_route_key(const bmq_engine* e, uint32_t route_id, uint8_t* out, uint32_t cap, uint32_t* out_len);
/* Many ids at once (one device gather): out_off[n + 1] byte offsets into out; a dead id gives an empty key.
 * BMQ_E_NOSPACE if cap < out_off[n] (offsets are still written). */
int bmq_route_keys(const bmq_engine* e, const uint32_t* route_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off);
/* exact lookup (no wildcard semantics): ids of the routes stored under (tenant, topicFilter); for tests
 * and for RouteDetailCache-style inspection.  Writes up to cap ids, *out_n = total. */
int bmq_index_find(const bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filter,
                   uint32_t filter_len, uint32_t* out_ids, uint32_t cap, uint32_t* out_n);

/* ---- dist direction: match --------------------------------------------------------------------------- */
/* Batch form of ITenantRouteMatcher.matchAll (DW/cache/ITenantRouteMatcher.java:37; implementation
 * DW/cache/TenantRouteMatcher.java:67-161) across tenants, as DistWorkerCoProc.batchDist iterates
 * DistPack(tenant) x TopicMessagePack(topic) (DW/DistWorkerCoProc.java:515-552).
 *   tenants/tenant_off : the distinct tenant ids of the batch (n_tenants packed strings)
 *   topic_tenant[i]    : index into that table for topic i
 *   topics/topic_off   : n_topics packed topic strings
 * Output: out_row_ptr[n_topics+1], out_route_ids[*out_needed] (ascending per row).  If out_capacity is too
 * small nothing is written to out_route_ids, *out_needed is set and BMQ_E_NOSPACE returned. */
int bmq_match_batch(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                    const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off,
                    uint32_t n_topics, uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_capacity,
                    uint64_t* out_needed);

/* Same, all seven data pointers are DEVICE pointers (inputs already resident in HBM; results stay in HBM).
 * Asynchronous on the engine stream; d_out_total (device uint64) receives the id count.  Call bmq_sync()
 * (or bmq_match_finish()) before reading results.  d_topics must be 16-byte aligned and readable up to
 * topic_off[n_topics] rounded up to the next multiple of 16 bytes. */
int bmq_match_batch_dev(bmq_engine* e, const uint8_t* d_tenants, const uint32_t* d_tenant_off, uint32_t n_tenants,
                        const uint32_t* d_topic_tenant, const uint8_t* d_topics, const uint32_t* d_topic_off,
                        uint32_t n_topics, uint32_t* d_out_row_ptr, uint32_t* d_out_route_ids,
                        uint64_t out_capacity, uint64_t* d_out_total);
/* Waits for the stream, resolves deferred conditions of the last *_dev batch (internal scratch growth ->
 * transparent re-run; BMQ_E_NOSPACE if out_capacity was too small) and fills stats. */
int bmq_match_finish(bmq_engine* e, uint64_t* out_total);
int bmq_sync(bmq_engine* e);
int bmq_stats_get(const bmq_engine* e, bmq_stats* out);
/* switches bmq_config.kernel_timing at run time (profilers / bench.py); takes effect with the next batch */
int bmq_set_kernel_timing(bmq_engine* e, int on);
/* The hipStream_t the engine launches on (as void*), so a harness can bracket it with HIP events. */
void* bmq_stream(const bmq_engine* e);

/* ---- asynchronous host-buffer match (the host-visible fast path) ------------------------------------------------------ */
/* Page-locked host memory.  Buffers from here move over PCIe by DMA at full speed and truly asynchronously; a JNI binding wraps
 * them with NewDirectByteBuffer.  (Any host pointer is accepted everywhere; pageable memory is staged by the HIP runtime.) */
void* bmq_host_alloc(size_t bytes);
void bmq_host_free(void* p);
/* bmq_match_batch split in two so that several batches can be in flight: the upload of batch i+1 (copy-in stream) and the download
 * of batch i-1 (copy-out stream, inside bmq_match_wait) overlap the kernels of batch i (engine stream).  Steady state: one batch
 * costs max(upload, kernels, download) instead of their sum.  Input buffers must stay valid and unchanged until the matching
 * bmq_match_wait returns.  *out_ticket is 0 .. BMQ_MAX_TICKETS - 1; BMQ_E_STATE when all are taken (three, so that a single caller thread
 * that blocks in the download of batch i still has batch i + 1 on the GPU and batch i + 2 on its way up).  bmq_match_wait blocks until the batch is
 * done, copies row_ptr[n_topics + 1] and the ids out (same NOSPACE protocol as bmq_match_batch) and frees the ticket.
 * Tickets may be waited for from any thread; bmq_routes_apply between a submit and its wait is applied BEHIND the submitted batch
 * (stream order). */
#define BMQ_MAX_TICKETS 3
int bmq_match_submit(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                     const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics,
                     int* out_ticket);
int bmq_match_wait(bmq_engine* e, int ticket, uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_capacity,
                   uint64_t* out_needed);

/* Tickets over DEVICE-ACCESSIBLE buffers: every pointer is HBM or page-locked host memory from bmq_host_alloc, which the GPU reads and
 * writes in place over PCIe (same alignment / padding duties as bmq_match_batch_dev).  Nothing is staged, nothing copied: for small
 * launches -- the batching front's: tens to thousands of topics -- the five uploads, three downloads and their synchronisation cost
 * more than the kernels.  The results (d_out_row_ptr[n + 1], d_out_route_ids, *d_out_total) are complete when bmq_match_wait_dev
 * returns; BMQ_E_NOSPACE + *out_total if out_capacity was short (row pointers are written).  Unlike bmq_match_batch_dev the engine is
 * not taken for the caller: BMQ_MAX_TICKETS such launches may be in flight, from any threads. */
int bmq_match_submit_dev(bmq_engine* e, const uint8_t* d_tenants, const uint32_t* d_tenant_off, uint32_t n_tenants,
                         const uint32_t* d_topic_tenant, const uint8_t* d_topics, const uint32_t* d_topic_off, uint32_t n_topics,
                         uint32_t* d_out_row_ptr, uint32_t* d_out_route_ids, uint64_t out_capacity, uint64_t* d_out_total,
                         int* out_ticket);
int bmq_match_wait_dev(bmq_engine* e, int ticket, uint64_t* out_total /* may be NULL */);

/* ---- host-visible result formats (host enqueue -> results visible on host) ------------------------------------------------------------------------------ */
/* The id CSR of a million-topic batch is ~77 MB over PCIe -- more than twice the topics that went in.  What the callers of the
 * reference's match path do next needs less, so a ticket can be submitted for one of these formats instead (bmq_match_submit_fmt takes the
 * arguments of bmq_match_submit + the format; every format has its own wait; waiting with another format's call is BMQ_E_STATE and
 * leaves the ticket in flight):
 *   BMQ_FMT_IDS      bmq_match_wait: row_ptr + ids.
 *   BMQ_FMT_COUNTS   bmq_match_wait_counts: out_row_ptr[n + 1] only -- the fan-out of topic i is row_ptr[i + 1] - row_ptr[i].  This is
 *                    all DistWorkerCoProc.batchDist replies with (DW/DistWorkerCoProc.java:535-538: BatchDistReply carries the fan-out per
 *                    topic).  4 bytes per topic come back; no id is ever written (the expansion kernel lays down the row pointers and leaves).
 *   BMQ_FMT_RANGES   bmq_match_wait_ranges: the MATCHED RANGES.  Every matched filter owns a run of route ids begin .. begin + count - 1
 *                    (its routes are neighbours in KV key order, SCHEMA/KVSchemaUtil.java:91-117), so a row is a handful of (begin, count)
 *                    pairs -- ~6 per topic where the id row has 18 entries.  out_range_ptr[n + 1] delimits the rows in out_ranges.  A range
 *                    whose count has BMQ_RANGE_SIDE set (filters touched by bmq_routes_apply since the last rebuild) lists its ids
 *                    explicitly: out_side_ids[begin .. begin + (count & ~BMQ_RANGE_SIDE)).  The result is self-contained: expanding
 *                    needs nothing of the index.  The ranges of a row come in ascending order of their first id (rows of more than 32
 *                    ranges: as matched); expanding them in that order yields the row's ids in ascending order -- exactly the row of
 *                    BMQ_FMT_IDS -- unless ranges overlap (interleaved id sets: only after churn), which the consumer sees while expanding
 *                    (first id <= last id of the range before it) and repairs by ordering that row's ids;
 *                    out_info->n_overlapping_rows says how many such rows the batch has.  After a rebuild no row of up to 32 ranges
 *                    is among them; rows of more than 32 ranges may be at any time: "as matched" is the order the walk found the
 *                    filters in, which is not the order of their ids, so such a row is counted wherever a range begins at or below the
 *                    end of the one before it.  A consumer may skip the ordering only for a batch with n_overlapping_rows == 0.
 *                    out_row_ptr (may be NULL) receives the id row pointers as well, so that the consumer knows where every expanded
 *                    row goes.
 *                    BMQ_E_NOSPACE when range_cap / side_cap are too small: out_info holds the sizes, row pointers are written, the ticket
 *                    is released (as with bmq_match_wait).
 *   BMQ_FMT_GROUPED  bmq_match_wait_grouped: the (topic, route) pairs of the batch regrouped by DelivererKey -- the output of
 *                    bmq_fanout_group (see there for the meaning of every array) without the CSR ever leaving the GPU.
 *   BMQ_FMT_DELIVERY (4, defined with bmq_delivery_plan below) bmq_delivery_wait: the delivery plan of the batch -- those groups with
 *                    the receivers of shared subscriptions resolved and merged in. */
#define BMQ_FMT_IDS 0
#define BMQ_FMT_COUNTS 1
#define BMQ_FMT_RANGES 2
#define BMQ_FMT_GROUPED 3
#define BMQ_RANGE_SIDE 0x80000000u
typedef struct bmq_id_range {
    uint32_t begin, count;
} bmq_id_range;
typedef struct bmq_ranges_info {
    uint64_t n_ranges, n_side_ids;
    uint64_t n_ids;              /* what the id CSR of the batch would hold */
    uint64_t n_overlapping_rows; /* rows whose expanded ids the consumer has to order */
} bmq_ranges_info;
int bmq_match_submit_fmt(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                         const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics,
                         int format, int* out_ticket);
int bmq_match_wait_counts(bmq_engine* e, int ticket, uint32_t* out_row_ptr, uint64_t* out_total /* may be NULL */);
int bmq_match_wait_ranges(bmq_engine* e, int ticket, uint32_t* out_row_ptr /* may be NULL */, uint32_t* out_range_ptr, bmq_id_range* out_ranges,
                          uint64_t range_cap, uint32_t* out_side_ids, uint64_t side_cap, bmq_ranges_info* out_info);
int bmq_match_wait_grouped(bmq_engine* e, int ticket, uint32_t* out_topic, uint32_t* out_route, uint64_t pair_cap, uint32_t* out_group_off,
                           uint32_t* out_group_rep, uint32_t group_cap, uint32_t* out_n_groups, uint32_t* out_special, uint64_t* out_total);

/* ---- multi-GPU exchange -------------------------------------------------------------------------------------- */
/* One process per GPU, tenants sharded by hash(tenantId) mod N; after the per-rank match ONE exchange step over RCCL / xGMI.
 * RCCL is loaded at run time (librccl.so.1); a process that already carries it (PyTorch) keeps using that copy.
 *   bmq_comm_unique_id : rank 0 creates the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any means
 *   bmq_comm_init      : every rank, with its engine (ncclCommInitRank on the engine's device)
 *   bmq_exchange_fanout: per-topic fan-out counts of every rank to every rank -- all the reference sends upstream
 *                        (DW/DistWorkerCoProc.java:535-538).  d_row_ptr[n + 1] -> d_counts_all[world * n], all device pointers
 *   bmq_exchange_csr   : the complete CSR of every rank on every rank: totals (-> out_totals[world], host), row pointers
 *                        (d_rows_all[world * (n + 1)]), then a true all-gatherv of the ids into d_ids_all (rank r's ids start at
 *                        sum(out_totals[0 .. r))): one ncclBroadcast per rank with its exact size in one group.  n must be the
 *                        same on every rank; BMQ_E_NOSPACE if ids_cap < sum(out_totals) (totals are still reported)
 * Both run asynchronously on the engine's exchange stream, ordered behind everything queued on the engine stream when they are
 * called (the batch whose results they send), so they overlap the NEXT batch's match; bmq_exchange_wait blocks until done. */
int bmq_comm_unique_id(uint8_t out[128]);
int bmq_comm_init(bmq_engine* e, int world, int rank, const uint8_t id[128]);
void bmq_comm_destroy(bmq_engine* e);
int bmq_exchange_fanout(bmq_engine* e, const uint32_t* d_row_ptr, uint32_t n, uint32_t* d_counts_all);
int bmq_exchange_csr(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_ids, uint32_t n, uint64_t total,
                     uint32_t* d_rows_all, uint32_t* d_ids_all, uint64_t ids_cap, uint64_t* out_totals);
int bmq_exchange_wait(bmq_engine* e);
/* The ids bmq_exchange_csr gathers are rank-local handles: rank r's rows are d_rows_all[r * (n + 1) ...], its ids the stretch of
 * d_ids_all behind sum(out_totals[0 .. r)) -- the position frames them as (rank, id); a consumer resolves an id on the rank that owns it.
 *
 * The node-wide batch: ONE publish batch for all tenants arrives on every GPU; a rank matches the topics whose tenant
 * it owns (d_owner[tenant index] == rank) and those of tenants split by filter over all ranks (d_owner < 0: the reference's analogue is
 * a hot range split by DW/hinter/FanoutSplitHinter.java:49, dist-server sums the per-range fan-outs, BatchDistServerCall.java:186-205).
 * All pointers are device pointers; the part is picked by kernels on the engine stream (mask, two prefix sums, scatter):
 *   d_out_sel[m]        global topic index of the part's k-th topic
 *   d_out_topics/_off   the part's topics packed (the buffer must hold the batch's bytes + 32 and be 16-byte aligned: it is handed to
 *                       bmq_match_batch_dev as is), d_out_off[m + 1]
 *   d_out_tenant[m]     tenant index of every topic (the batch's tenant table stays as it is)
 * *out_n = m, *out_bytes = bytes of the part: the one host read of the step. */
int bmq_partition_batch_dev(bmq_engine* e, const int32_t* d_owner, uint32_t n_tenants, int32_t rank, const uint32_t* d_topic_tenant,
                            const uint8_t* d_topics, const uint32_t* d_topic_off, uint32_t n_topics, uint32_t* d_out_sel, uint8_t* d_out_topics,
                            uint32_t* d_out_off, uint32_t* d_out_tenant, uint32_t* out_n, uint64_t* out_bytes);

/* ---- batching front ------------------------------------------------------------------- */
/* Production asks for one topic per call: TenantRouteCache issues matchAll(singleton(topic)) per cache miss from
 * the matchExecutor pool (DW/cache/TenantRouteCache.java:180-193, DW/DistWorkerCoProcFactory.java:74-88).  A batcher
 * collects the calls of all threads that are waiting right now into ONE bmq_match_batch (leader/follower: no timer,
 * no extra thread; the batch is whatever piled up while the previous one was on the GPU) and hands every caller
 * its rows (identical (tenant, topic) pairs of one launch are matched once).  Any number of threads may call bmq_batcher_match_all concurrently; the call blocks until the batch
 * that contains the request has been matched.  bmq_rebuild / bmq_routes_apply may run concurrently (they serialise
 * with the batches on the engine lock); *out_epoch tells which epoch the returned route ids are ranks of. */
typedef struct bmq_batcher bmq_batcher;
typedef struct bmq_batcher_config {
    uint32_t struct_size;
    uint32_t max_batch_topics; /* upper bound of one launch (default 2^20); a single larger request still runs alone */
    uint32_t reserved[6];
} bmq_batcher_config;
typedef struct bmq_batcher_stats {
    uint64_t n_requests, n_topics, n_batches, max_batch_topics;
    uint64_t n_deduped; /* requested topics that shared a row with an identical (tenant, topic) of the same launch */
} bmq_batcher_stats;
int bmq_batcher_create(bmq_engine* e, const bmq_batcher_config* cfg /* may be NULL */, bmq_batcher** out);
/* Waits for the calls in flight; calls arriving afterwards fail with BMQ_E_STATE.  Destroy before the engine. */
void bmq_batcher_destroy(bmq_batcher* b);
/* ITenantRouteMatcher.matchAll(topics) for ONE tenant, caps not applied (INT_MAX), through the collector.
 * out_row_ptr[n_topics + 1] is relative to this request; BMQ_E_NOSPACE + *out_needed if out_capacity is too small
 * (row pointers are still written). */
int bmq_batcher_match_all(bmq_batcher* b, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics,
                          const uint32_t* topic_off, uint32_t n_topics, uint32_t* out_row_ptr,
                          uint32_t* out_route_ids, uint64_t out_capacity, uint64_t* out_needed, uint64_t* out_epoch);
/* A whole multi-tenant batch (the arguments of bmq_match_batch) as ONE launch of its own, taking its turn with the collected launches;
 * *out_epoch = the epoch of the index the batch saw (bmq_match_batch alone cannot tell).  For callers that already hold many topics:
 * bmq_route_cache_get_batch matches the cache misses of one BatchDistRequest this way. */
int bmq_batcher_match_batch(bmq_batcher* b, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* topic_tenant,
                            const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics, uint32_t* out_row_ptr, uint32_t* out_route_ids,
                            uint64_t out_capacity, uint64_t* out_needed, uint64_t* out_epoch);
/* Asynchronous form for loaders that return a future (Caffeine's AsyncCache in TenantRouteCache.java:116-139): the topic is
 * copied and packed into the batch being collected and the call returns at once; a dispatcher thread owned by the batcher
 * (started by the first submit) matches whatever has been collected whenever the engine is free and then calls
 * cb(user, status, ids, n_ids, epoch) once per request, on the dispatcher thread, in submission order.  `ids` is only
 * valid during the callback.  A submitter blocks only while max_batch_topics requests are already waiting.
 * bmq_batcher_destroy matches and calls back everything submitted before it. */
typedef void (*bmq_batcher_cb)(void* user, int status, const uint32_t* route_ids, uint32_t n_ids, uint64_t epoch);
int bmq_batcher_submit(bmq_batcher* b, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topic, uint32_t topic_len,
                       bmq_batcher_cb cb, void* user);
int bmq_batcher_stats_get(bmq_batcher* b, bmq_batcher_stats* out);

/* ---- the persistent matcher behind the batching front (round 6; bmq_poll_kernel.h) ------------------------------------------------------
 * A generation of the batching front of at most 64 topics is not LAUNCHED any more: a few resident one-wave workgroups (k_poll) poll a ring
 * of request descriptors in page-locked host memory, run the walk + expansion of k_walk / k_expand on the generation whose doorbell rang and
 * write the CSR in place; the leader spins on the slot's completion word.  The reference's call shape -- one matchAll(singleton(topic)) per
 * cache miss from the matchExecutor pool (DW/cache/TenantRouteCache.java:180-193, DW/DistWorkerCoProcFactory.java:74-88) -- pays a
 * PCIe round trip per generation instead of a kernel launch and an event.  It needs no call of its own: bmq_batcher_match_all /
 * bmq_route_cache_get use it whenever it is enabled (the default on a device engine).
 *   - the index never changes under it: bmq_rebuild, bmq_routes_apply[_async], bmq_routes_import, bmq_compact, bmq_compact_swap and bmq_engine_destroy stop it
 *     first (it finishes the generation in hand, a few microseconds); the next generation starts it again.  The FIRST generation after a
 *     start pays the launch (~15 us); a generation whose doorbell it never saw is launched the old way by its leader;
 *   - it leaves the GPU by itself after 20 ms without a doorbell and after 2 s whatever happens;
 *   - a generation not answered within 250 ms marks it wedged: it is told to leave, never started again on this engine
 *     (bmq_poller_stats.n_timeouts), and the generation -- like every later one -- is launched the old way: callers see results, not errors. */
typedef struct bmq_poller_stats {
    uint32_t enabled;     /* generations of <= 64 topics go to it */
    uint32_t running;     /* a k_poll launch is resident right now */
    uint64_t n_starts;    /* k_poll launches so far */
    uint64_t n_served;    /* generations answered by it */
    uint64_t n_fallback;  /* generations handed back or never seen: launched the old way */
    uint64_t n_unserved;  /* ... of which: rang while it was leaving */
    uint64_t n_timeouts;  /* generations that waited 250 ms in vain (the poller is off for good after the first) */
    uint64_t n_bad_input; /* generations a wave refused to touch: offsets or tenant indices out of range (handed back, launched the old way) */
} bmq_poller_stats;
enum { BMQ_POLLER_DISABLE = 0, BMQ_POLLER_ENABLE = 1, BMQ_POLLER_STOP = 2 /* leave now; the next generation starts it again */,
       BMQ_POLLER_TEST_IGNORE_DOORBELLS = 3 /* test hook: doorbells are seen and not answered -- the leaders' time-out path */ };
int bmq_poller_stats_get(bmq_engine* e, bmq_poller_stats* out);
int bmq_poller_control(bmq_engine* e, int what);

/* ---- route cache ---------------------------------------------------------------------------------- */
/* ISubscriptionCache (DW/cache/ISubscriptionCache.java:30-40) on the engine's side of the boundary: SubscriptionCache ->
 * TenantRouteCache (DW/cache/TenantRouteCache.java:116-296: topic -> matched routes, loaded by matchAll(singleton(topic)), bounded by
 * DistMaxCachedRoutesPerTenant with weight max(1, #routes after the caps), expireAfterAccess DistTopicMatchExpirySeconds) with its TopicIndex
 * (DW/TopicIndex.java:39-156: the cached topics, queried with the topic filter of a route mutation).  A hit is answered on the host;
 * a miss goes through the batching front, i.e. into ONE GPU launch with every other miss of the moment.
 *   get       ISubscriptionCache.get(tenantId, topic) = IMatchedRoutes.routes() (DW/cache/TenantRouteCache.java:299-301): the matched
 *             route ids (ascending) AFTER MatchedRoutes' fan-out caps (DW/cache/MatchedRoutes.java:87-141: persistent and group routes
 *             admitted first-come in KV key order), *out_epoch = the engine epoch they were matched at.  The caps are the tenant's
 *             (bmq_route_cache_set_caps; defaults of Setting.java:60-61: MaxPersistentFanout = INT_MAX, MaxGroupFanout = 100); every route
 *             a load throws away is reported to the event sink (bmq_route_cache_set_event_sink) before the load returns; a hit reports
 *             nothing (the reference reports when it loads, too).  An entry met under caps other than the ones it was loaded with follows
 *             MatchedRoutes.adjust (:150-200): it is re-matched when a raised cap could admit more routes or a lowered one is exceeded,
 *             else it adopts the new caps.  The cache weighs an entry by its capped size (TenantRouteCache.java:108).
 *             now_ms is the caller's clock (Caffeine's Ticker).  BMQ_E_NOSPACE + *out_n if cap is short.
 *   is_cached ISubscriptionCache.isCached(tenantId, filterLevels) = !index.match(filterLevels).isEmpty(): 1 / 0
 *   apply     ISubscriptionCache.refresh(AddRoutesTask / RemoveRoutesTask): bmq_routes_apply on the engine, then every cached topic
 *             one of the mutated filters matches is dropped and reloads on its next get (the reference patches those entries in
 *             place -- TenantRouteCache.java:224-277 -- which yields the same route set a reload computes).  A load that was matched
 *             before a mutation but finishes after it is recognised by its epoch and not cached.
 *   rebuild   IKVRangeCoProc.reset: bmq_rebuild + drop everything (route ids of different generations are unrelated); nothing is
 *             served from the cache while the engine swaps the index.   reset: drop everything (ISubscriptionCache.reset(boundary)).
 * Any number of threads may call get / is_cached; apply / rebuild / reset come from one thread at a time (the range's apply thread)
 * and may run concurrently with the getters.  Destroy before the batcher. */
typedef struct bmq_route_cache bmq_route_cache;
typedef struct bmq_route_cache_config {
    uint32_t struct_size;
    uint32_t mutation_log_entries;   /* per tenant; default 4096 */
    uint64_t max_routes_per_tenant;  /* DistMaxCachedRoutesPerTenant, default 200000 */
    uint64_t expiry_ms;              /* DistTopicMatchExpirySeconds, default 60000 */
    uint64_t shards_per_tenant;      /* power of two, default 16: a tenant's topics are spread over that many independently locked */
                                     /* slices, so one hot tenant does not serialise its callers; the route budget is the tenant's */
    uint64_t direct_batch_topics;    /* bmq_route_cache_get_batch: a request of at least this many topics (default 8192) is matched in one */
                                     /* launch without consulting or filling the cache -- at that size the GPU is faster than the probes */
    int32_t default_max_persistent_fanout; /* MaxPersistentFanout of tenants without bmq_route_cache_set_caps; 0 = INT_MAX (Setting.java:61) */
    int32_t default_max_group_fanout;      /* MaxGroupFanout ...; 0 = 100 (Setting.java:60) */
    uint64_t tenant_idle_ms;         /* a tenant nobody called get for since that long loses its whole cache at the next bmq_route_cache_expire */
                                     /* (DW/cache/SubscriptionCache.java:79-107); 0 = 2 x expiry_ms, as there */
} bmq_route_cache_config;
typedef struct bmq_route_cache_stats {
    uint64_t hits, misses, evictions, invalidations, expired;
    uint64_t stale_loads;            /* loads overtaken by a mutation of a matching filter: returned to their caller, not cached */
    uint64_t entries, cached_routes; /* now */
    uint64_t tenants;                /* tenant caches alive now */
    uint64_t tenants_expired;        /* tenant caches destroyed after tenant_idle_ms without a get (their counters stay in the sums above) */
} bmq_route_cache_stats;
/* What TenantRouteCache registers per tenant (DW/cache/TenantRouteCache.java:141-147: MqttRouteCacheHitCount / MissCount / EvictCount
 * counters, MqttRouteCacheSize gauge); like there, the meters go when the tenant's cache is destroyed. */
typedef struct bmq_route_cache_tenant_stats {
    uint64_t hits, misses, evictions;
    uint64_t entries, cached_routes; /* estimatedSize, current weight */
    uint64_t last_get_ms;
    int32_t max_persistent_fanout, max_group_fanout; /* the caps in force */
} bmq_route_cache_tenant_stats;
int bmq_route_cache_create(bmq_engine* e, bmq_batcher* b, const bmq_route_cache_config* cfg /* may be NULL */, bmq_route_cache** out);
void bmq_route_cache_destroy(bmq_route_cache* c);
int bmq_route_cache_get(bmq_route_cache* c, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topic, uint32_t topic_len, uint64_t now_ms,
                        uint32_t* out_route_ids, uint32_t cap, uint32_t* out_n, uint64_t* out_epoch);
/* The same as a future (ISubscriptionCache.get returns a CompletableFuture; Caffeine's AsyncLoadingCache, TenantRouteCache.java:116-139):
 * a hit calls cb(user, BMQ_OK, ids, n, epoch) on the calling thread before the call returns; a miss is handed to bmq_batcher_submit and
 * cb runs on the batcher's dispatcher thread once the launch that carries it has finished (the row is cached first, under the same
 * epoch rule).  `route_ids` is only valid during the callback.  Nobody blocks on the GPU: a few threads keep millions of gets per
 * second in flight. */
typedef void (*bmq_route_cache_cb)(void* user, int status, const uint32_t* route_ids, uint32_t n_ids, uint64_t epoch);
int bmq_route_cache_get_async(bmq_route_cache* c, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topic, uint32_t topic_len,
                              uint64_t now_ms, bmq_route_cache_cb cb, void* user);
/* DistWorkerCoProc.batchDist (DW/DistWorkerCoProc.java:515-552) asks the cache once per (tenant, topic) of a BatchDistRequest; this is the
 * whole request in one call (arguments and CSR output as bmq_match_batch): the rows of cached topics are copied from the cache, all the
 * others -- identical (tenant, topic) pairs once -- are matched in ONE launch (bmq_batcher_match_batch) and cached under the epoch rule.
 * out_hit[i] (may be NULL) = 1 if row i came from the cache.  BMQ_E_NOSPACE + *out_needed if out_capacity is short (row pointers are
 * written; what was loaded is cached, so the second call hits).  Requests of bmq_route_cache_config.direct_batch_topics topics and more
 * skip the cache altogether: topics must then be readable 16 bytes past their end, as for bmq_match_batch. */
int bmq_route_cache_get_batch(bmq_route_cache* c, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* topic_tenant,
                              const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics, uint64_t now_ms, uint32_t* out_row_ptr,
                              uint32_t* out_route_ids, uint64_t out_capacity, uint64_t* out_needed, uint8_t* out_hit);
int bmq_route_cache_is_cached(bmq_route_cache* c, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filter, uint32_t filter_len);
int bmq_route_cache_apply(bmq_route_cache* c, const uint8_t* keys, const uint32_t* key_off, const uint8_t* op, uint32_t n);
int bmq_route_cache_rebuild(bmq_route_cache* c, const uint8_t* keys, const uint32_t* key_off, uint32_t n_keys);
int bmq_route_cache_reset(bmq_route_cache* c);
/* Caffeine expires idle entries from a scheduler thread (TenantRouteCache.java:104-114: expireAfterAccess + Scheduler.systemScheduler());
 * here get() drops an expired entry when it meets one and this sweep -- to be called now and then by the owner -- drops the rest: every entry
 * not accessed for expiry_ms at now_ms -- and every TENANT nobody called get for since tenant_idle_ms, whole (SubscriptionCache.java:79-107:
 * the tenant cache expires 2 x the match expiry after its last get; isCached / refresh do not count).  *out_dropped (may be NULL) =
 * entries dropped. */
int bmq_route_cache_expire(bmq_route_cache* c, uint64_t now_ms, uint64_t* out_dropped);
int bmq_route_cache_stats_get(bmq_route_cache* c, bmq_route_cache_stats* out);
/* BMQ_E_STATE: the tenant has no cache (nothing loaded for it yet, or destroyed after tenant_idle_ms) */
int bmq_route_cache_tenant_stats_get(bmq_route_cache* c, const uint8_t* tenant, uint32_t tenant_len, bmq_route_cache_tenant_stats* out);
/* The tenant's MaxPersistentFanout / MaxGroupFanout (ISettingProvider.provide(..., tenantId), asked per task loop in
 * DW/cache/TenantRouteCache.java:174-175 and again on every fan-out check, :124-138).  Takes effect with the next get: cached rows the
 * change can affect are re-matched, the others adopt the new caps (MatchedRoutes.adjust).  Survives the tenant cache's expiry. */
int bmq_route_cache_set_caps(bmq_route_cache* c, const uint8_t* tenant, uint32_t tenant_len, int32_t max_persistent_fanout,
                             int32_t max_group_fanout);
/* IEventCollector.report(PersistentFanoutThrottled / GroupFanoutThrottled) (DW/cache/MatchedRoutes.java:95-101,124-130): called once
 * per route a load rejects -- type 0 = PersistentFanoutThrottled, 1 = GroupFanoutThrottled; route_id's key gives mqttTopicFilter
 * (bmq_route_key) -- on the thread that completes the load (the caller of get / get_batch, the batcher's dispatcher thread for
 * get_async), before the rows are handed out.  NULL switches reporting off.  Callback and user pointer are replaced together (one atomic
 * pointer to the pair).  May be called while getters run: a load that picked the previous sink up just before the call may still report to
 * it once more afterwards, so a `user` object that was ever installed has to stay valid until bmq_route_cache_destroy has returned. */
typedef void (*bmq_route_cache_event_cb)(void* user, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topic, uint32_t topic_len,
                                         int32_t type, uint32_t route_id, int32_t max_count);
int bmq_route_cache_set_event_sink(bmq_route_cache* c, bmq_route_cache_event_cb cb, void* user);

/* ---- host-side mirror of MatchedRoutes (fan-out caps in KV order) -------------------------------------- */
/* One ITenantRouteMatcher.matchAll(topics, maxPersistentFanout, maxGroupFanout) call for one tenant,
 * including DW/cache/MatchedRoutes.java:87-141: persistent (subBrokerId == 1) and group fan-out caps applied
 * first-come in key order, throttle events reported.  events: 4 int32 each {type 0=PersistentFanoutThrottled
 * 1=GroupFanoutThrottled, topic index, rejected route id, max count}. */
int bmq_match_all(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics,
                  const uint32_t* topic_off, uint32_t n_topics, int32_t max_persistent_fanout,
                  int32_t max_group_fanout, uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_capacity,
                  uint64_t* out_needed, int32_t* out_events, uint32_t events_cap, uint32_t* out_n_events);

/* MatchedRoutes (DW/cache/MatchedRoutes.java:87-141) over rows somebody else matched (the route cache caps what the batching front
 * loaded): row r = route_ids[row_ptr[r] .. row_ptr[r + 1]).  out_row_ptr[n_rows + 1] / out_route_ids (at least row_ptr[n_rows] ids) = the
 * rows after the caps, ascending ids; out_class_counts (may be NULL) [2 r] / [2 r + 1] = persistent / group routes kept in row r, or
 * 0xFFFFFFFF when the row was not longer than either cap and therefore never classified; events as in bmq_match_all with the row
 * index in place of the topic index.  Ids of routes deleted since the match are dropped from classified rows. */
int bmq_routes_cap(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_rows, int32_t max_persistent_fanout,
                   int32_t max_group_fanout, uint32_t* out_row_ptr, uint32_t* out_route_ids, uint32_t* out_class_counts,
                   int32_t* out_events, uint32_t events_cap, uint32_t* out_n_events);

/* ---- fan-out grouping: the step behind the match --------------------------------------------------------------- */
/* DistWorkerCoProc.batchDist hands every topic's matched routes to DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-241);
 * each NormalMatching becomes a DeliveryCall (DW/DeliverExecutor.java:85-90) that the deliverer batches by
 * DelivererKey(subBrokerId, delivererKey) (bifromq-deliverer/.../DelivererKey.java:22, BatchDeliveryCall.java:71-76: per key, tenant ->
 * message pack -> set of MatchInfo).  This is that regrouping for a whole match batch, as a segmented sort of its CSR on the device:
 *   in : row_ptr[n_topics + 1], route_ids[row_ptr[n_topics]]                  (what bmq_match_batch* returned)
 *   out: out_topic[k], out_route[k], k < row_ptr[n_topics]: the (topic index, route id) pairs ordered by (group, topic, route id);
 *        out_group_off[*out_n_groups + 1]: group g owns the pairs out_group_off[g] .. out_group_off[g + 1];
 *        out_group_rep[g]: a route id of the group (bmq_route_key of it gives the group's subBrokerId and delivererKey: the first
 *        and the third NUL-separated part of its receiverUrl, SCHEMA/KVSchemaUtil.java:56-58), 0xFFFFFFFE for the group of
 *        shared-subscription routes (flag 2 / 3: DeliverExecutorGroup.java:243-279 picks the receiver per message; bmq_share_resolve
 *        below does that for the group's pairs on the device), 0xFFFFFFFF for
 *        the group of ids whose route has been deleted since the match.
 * A group = one DelivererKey, exactly (key bytes are compared, not only hashes).  The normal groups come first, in no particular
 * order (the reference's batcher map is a HashMap), then the shared-subscription group (*out_special bit 0), then the dead group
 * (bit 1).  The fan-out caps of submit() are not applied here: the count caps were applied by MatchedRoutes in key order
 * (bmq_match_all), the byte / bandwidth throttles depend on the message.
 * BMQ_E_NOSPACE: pair_cap < row_ptr[n_topics], or group_cap < *out_n_groups (the pairs are written, the group table is not).
 * Works on a host-only engine too (it is not a match: the same per-pair functions run on host threads).
 * _dev: all six array arguments are device pointers (the CSR may be the one bmq_match_batch_dev left in HBM, after
 * bmq_match_finish); runs on the engine stream and returns when the groups are complete. */
int bmq_fanout_group(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_topics, uint32_t* out_topic,
                     uint32_t* out_route, uint64_t pair_cap, uint32_t* out_group_off, uint32_t* out_group_rep, uint32_t group_cap,
                     uint32_t* out_n_groups, uint32_t* out_special);
int bmq_fanout_group_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_topics, uint64_t total,
                         uint32_t* d_out_topic, uint32_t* d_out_route, uint32_t* d_out_group_off, uint32_t* d_out_group_rep,
                         uint32_t group_cap, uint32_t* out_n_groups, uint32_t* out_special);
/* Which way the grouping answered.  On the device a call takes a counting sort written for up to 1024 deliverer keys (the fast path,
 * bifromq_amd/csrc/bmq_fanout_kernels.h) and, with more keys than that, generic radix-sort passes; a host-only engine has only the
 * generic passes and reports n_fast_calls == 0.  Both give the same groups.  The counts are kept by the host-side control (no kernel
 * takes part) and belong to the grouping state, which is tied to ONE generation of the route index: they restart at 0 when that state is
 * dropped or built anew -- the first grouping after bmq_rebuild / bmq_compact, and bmq_compact_swap.  All fields are 0 before the first
 * grouping of a batch that is not empty. */
typedef struct bmq_fanout_info {
    uint64_t n_fast_calls;    /* calls answered by the fast path */
    uint64_t n_generic_calls; /* calls answered by the generic passes */
    uint64_t n_refill_calls;  /* calls of the fast path that met route ids without a group (the first batch of a generation, routes added
                                 since), mapped them and ran again -- whichever path answered in the end */
    uint64_t n_table_grows;   /* times the group table was emptied to continue four times as large (kept at most half full) */
    uint64_t n_table_reseeds; /* times it was emptied because two deliverer keys shared a 64-bit hash */
    uint64_t n_keys;          /* distinct deliverer keys mapped so far (used slots of the table) */
    uint64_t table_slots;     /* capacity of the group table */
    uint64_t generation;      /* generation of the route index the state belongs to (bmq_index_info.generation) */
} bmq_fanout_info;
int bmq_fanout_info_get(const bmq_engine* e, bmq_fanout_info* out);

/* ---- receivers of shared subscriptions: the step behind the fan-out grouping ------------------------------------------------------ */
/* DeliverExecutorGroup.send(GroupMatching, ...) (bifromq-dist/bifromq-dist-worker/src/main/java/org/apache/bifromq/dist/worker/
 * DeliverExecutorGroup.java:242-278) turns every route of a shared subscription into deliveries to MEMBERS of the group; the members
 * are the `members: receiverUrl -> incarnation` of the group route's value, receiverList = that map in entry order (bifromq-dist/
 * bifromq-dist-worker-schema/src/main/java/org/apache/bifromq/dist/worker/schema/cache/GroupMatching.java:41-50):
 *   unordered share ($share, route-key flag 2): the topic's whole message pack goes to ONE member, picked uniformly at random;
 *   ordered share ($oshare, flag 3): per publisher of the pack, the member with the highest score wins (base-util/src/main/java/org/
 *     apache/bifromq/base/util/RendezvousHash.java:45-61), score = murmur3_128(seed 0) over [int32 little-endian sender hash][UTF-8
 *     receiverUrl], asLong() = h1 of MurmurHash3_x64_128 compared as a SIGNED 64-bit value, strict '>' in list order (the first of equal
 *     scores wins).  The sender hash is ClientInfo.hashCode(): only the JVM can compute it, it is an input here.  (The reference caches
 *     the winner per (filter, sender) and drops the cache when the group mutates: recomputing per batch gives the same answer.)
 * The chosen member is a NormalMatching of its own receiverUrl "<subBrokerId> NUL <receiverId> NUL <delivererKey>": it is sent like any
 * normal route, under ITS DelivererKey(subBrokerId, delivererKey).
 *
 * bmq_share_members_apply: replaces the member list of each of the n named group routes by the URLs member_off[i] .. member_off[i + 1]
 *   of (urls, url_off[member_off[n] + 1]), in that order (= receiverList order); an empty list removes the route's table.  Before anything
 *   changes it is checked (BMQ_E_INVAL) that every id is a live route of flag 2 or 3, that every URL has exactly the three NUL-separated
 *   parts, and that no list has more than 65 535 members.  Ordered or not comes from the route key's flag.  The tables live in device
 *   memory (bmq_share_info.device_bytes), pre-mixed for the hash (bifromq_amd/csrc/bmq_share_core.h).  They are keyed by route id, so they
 *   belong to ONE generation of the route index, and bmq_share_info.generation says which.  bmq_rebuild drops them all: the caller reloads
 *   the KV range then and has the group values in hand.  bmq_compact and bmq_compact_swap (after bmq_compact_begin and after
 *   bmq_compact_begin_in) change the generation WITHOUT a KV scan, and by default (bmq_config.share_carry = 0) they drop every table too:
 *   all $share / $oshare rows come back unresolved until the caller has pushed every group value through this call again.  With
 *   bmq_config.share_carry = 1 they carry the tables instead: each one moves to the id its route KEY has in the new generation (old id ->
 *   key -> new id, looked up on the device: the keys never leave HBM); a table whose route is dead, lies outside the boundary of a bounded
 *   swap or is otherwise not found there is dropped (its members leave bmq_share_info.n_members; the pools keep the garbage until they are
 *   next re-laid, as replaced tables do).  Member order, the ordered / unordered flag, the URLs and the share-deliverer numbers stay as
 *   they are (n_deliverers does not change), bmq_share_info.generation becomes the new generation, and bmq_share_carry_info_get reports
 *   what the last carry did.  If the executor fails half-way every table is dropped (the generation change itself succeeds).
 *   bmq_routes_import moves no tables between engines.  A route deleted by bmq_routes_apply leaves its table unreachable (its id is
 *   dead; a put of the same key later is another route: the table does not come back).  Every distinct (subBrokerId, delivererKey) among the members of a generation gets a
 *   dense share-deliverer number (exact byte comparison); members that differ only in receiverId share one.
 *
 * bmq_share_resolve: in : n_pairs (topic index, route id) pairs -- typically the slice out_group_off[g] .. out_group_off[g + 1] of the
 *        0xFFFFFFFE group of bmq_fanout_group / bmq_match_wait_grouped, but any pair list is accepted --; the publishers of each topic's
 *        message pack as sender_off[n_topics + 1], sender_hash[sender_off[n_topics]]; a nonce, fresh per batch.
 *   out: delivery rows (out_pair[r], out_sender[r], out_member[r]), r < *out_n_rows:
 *        unordered route: one row, out_sender = 0xFFFFFFFF (the whole pack), out_member = the picked index into the route's list:
 *            x = fmix64((nonce ^ ((uint64_t)route_id << 32 | topic_index)) + 0x9E3779B97F4A7C15), 64-bit wrap-around, where fmix64 is
 *            MurmurHash3's finalizer (k ^= k >> 33; k *= 0xff51afd7ed558ccd; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33);
 *            member = (uint32_t)(((x >> 32) * n_members) >> 32);
 *        ordered route: one row per sender of the pair's topic (none if it has none), out_sender = index into sender_hash, out_member =
 *            the rendezvous winner;
 *        a pair whose route has no table, is dead, or is no shared route: one row with out_member = 0xFFFFFFFF.
 *        out_pair is the index into the pair list.  Rows are ordered by (share-deliverer number, pair, sender); group g owns the rows
 *        out_group_off[g] .. out_group_off[g + 1] and its DelivererKey is that of its first row's member (bmq_share_member gives the URL);
 *        the unresolved rows form the last group (*out_special bit 0).
 *   BMQ_E_NOSPACE: row_cap < *out_n_rows or group_cap < *out_n_groups; both counts are reported, nothing else is valid.
 *   Fewer than 2^31 pairs and rows per call.  Works on a host-only engine too (the same per-item functions on host threads).
 * _dev: every array is a device pointer (the pairs may be those bmq_fanout_group_dev left in HBM), n_senders = the length of
 *   d_sender_hash; runs on the engine stream and returns when the rows are complete. */
typedef struct bmq_share_info {
    uint64_t n_tables;     /* group routes with a member table */
    uint64_t n_members;    /* members in all of them */
    uint64_t n_deliverers; /* share-deliverer numbers handed out in this generation */
    uint64_t device_bytes; /* tables and resolve scratch in device memory (0: host-only engine) */
    uint64_t generation;   /* generation of the route index the tables belong to (bmq_index_info.generation) */
    /* HIP-event times of the last resolve on the device while bmq_set_kernel_timing is on (else 0): rows per pair + scan, the rows'
     * pairs and senders, the resolve kernel, the sort by share-deliverer number, group heads + scan + offsets */
    float ms_count, ms_rows, ms_resolve, ms_sort, ms_group;
    uint32_t reserved0;
} bmq_share_info;
int bmq_share_members_apply(bmq_engine* e, const uint32_t* route_ids, uint32_t n, const uint32_t* member_off, const uint8_t* urls,
                            const uint32_t* url_off);
int bmq_share_resolve(bmq_engine* e, const uint32_t* pair_topic, const uint32_t* pair_route, uint32_t n_pairs, const uint32_t* sender_off,
                      const int32_t* sender_hash, uint32_t n_topics, uint64_t nonce, uint32_t* out_pair, uint32_t* out_sender,
                      uint32_t* out_member, uint32_t row_cap, uint32_t* out_group_off, uint32_t group_cap, uint32_t* out_n_rows,
                      uint32_t* out_n_groups, uint32_t* out_special);
int bmq_share_resolve_dev(bmq_engine* e, const uint32_t* d_pair_topic, const uint32_t* d_pair_route, uint32_t n_pairs,
                          const uint32_t* d_sender_off, const int32_t* d_sender_hash, uint32_t n_topics, uint32_t n_senders, uint64_t nonce,
                          uint32_t* d_out_pair, uint32_t* d_out_sender, uint32_t* d_out_member, uint32_t row_cap, uint32_t* d_out_group_off,
                          uint32_t group_cap, uint32_t* out_n_rows, uint32_t* out_n_groups, uint32_t* out_special);
/* receiverUrl of member `index` of the route's table -> out_url[*out_len]; BMQ_E_INVAL: no such table / member; BMQ_E_NOSPACE: cap < *out_len */
int bmq_share_member(const bmq_engine* e, uint32_t route_id, uint32_t index, uint8_t* out_url, uint32_t cap, uint32_t* out_len);
int bmq_share_info_get(const bmq_engine* e, bmq_share_info* out);
/* What the last generation change that ran with bmq_config.share_carry = 1 did with the member tables. */
typedef struct bmq_share_carry_info {
    uint64_t from_generation, to_generation;  /* of the last generation change that ran with share_carry = 1 (0, 0: none yet) */
    uint64_t n_carried, n_dropped, n_members_carried;
    float ms_gather, ms_find, ms_rekey;       /* HIP-event times while bmq_set_kernel_timing is on, else 0 */
    uint32_t status;                          /* 0 none, 1 carried, 2 failed: every table was dropped */
    uint32_t reserved0;
} bmq_share_carry_info;
int bmq_share_carry_info_get(const bmq_engine* e, bmq_share_carry_info* out);

/* ---- the delivery plan of a match batch: the step behind the two above -------------------------------------------------------------- */
/* What DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-278) produces is ONE set of delivery calls per
 * DelivererKey(subBrokerId, delivererKey): inside a key per tenant -> message pack (topic) -> MatchInfo (BatchDeliveryCall.java:71-76), and the
 * member picked for a $share / $oshare route is filed by DeliverExecutor.send (DW/DeliverExecutor.java:85-90) under ITS OWN DelivererKey,
 * beside the normal routes of that key.  bmq_fanout_group names its groups by a route, bmq_share_resolve names its groups by a member; whether
 * two of them are one DelivererKey is decided here, on the executor, by the key bytes -- a 64-bit hash that agrees never merges two keys.
 *
 * bmq_delivery_plan: in : a match CSR as for bmq_fanout_group (row_ptr[n_topics + 1], route_ids[row_ptr[n_topics]]); the publishers of every
 *        topic's message pack and a nonce as for bmq_share_resolve (sender_off[n_topics + 1], sender_hash[sender_off[n_topics]]).
 *   out: delivery rows (out_topic[r], out_route[r], out_aux[r]), r < out_info->n_rows.
 *        out_aux[r] == 0xFFFFFFFF: the route itself is the receiver (a normal route -- or, in the trailing group of dead ids, what is left of it).
 *        otherwise s = out_aux[r] < out_info->n_share_rows indexes (out_share_sender[s], out_share_member[s]): the sender index (0xFFFFFFFF for
 *        an unordered share: the whole pack) and the chosen member of the route's table, 0xFFFFFFFF when there is none -- exactly the values
 *        bmq_share_resolve documents for out_sender / out_member (the pick formula, the signed rendezvous comparison and the first-of-equals
 *        rule are those: the same code runs).  One row per (pair, sender) of an ordered share, none for a topic without senders.
 *        out_group_off[n_groups + 1]: group g owns the rows out_group_off[g] .. out_group_off[g + 1].  A group is exactly one DelivererKey;
 *        inside it the rows are ordered by (topic, route id, sender index), so all deliveries of one message pack to one deliverer are
 *        adjacent, whether they come from normal routes or from chosen members.  There is no representative array: the DelivererKey of
 *        group g is that of its first row -- out_aux == 0xFFFFFFFF: the route's receiverUrl (bmq_route_key), else the member's URL
 *        (bmq_share_member(route, out_share_member[aux])) --, subBrokerId and delivererKey being parts 0 and 2 of "<subBrokerId> NUL
 *        <receiverId> NUL <delivererKey>".
 *        Group order: the resolved groups first, in no particular order; then the group of shared rows that could not be resolved (no
 *        table, not a shared route: out_info->special bit 0; its side entries carry member 0xFFFFFFFF); then the group of route ids deleted
 *        since the match or never handed out (bit 1; a shared route deleted since is found here too).  Either is absent when empty.
 *   out_info: n_rows, n_share_rows, n_groups as written; n_merged_groups: groups that hold rows of both kinds; n_share_only_groups: a
 *        DelivererKey reached through members only -- none of its normal routes, if the index has any, matched in this batch --; generation:
 *        of the route index the ids belong to; ms_*: HIP-event times of the four steps while bmq_set_kernel_timing is on, else 0 (the
 *        grouping, the resolve, the map of share groups to normal groups, the merge).
 *   BMQ_E_NOSPACE: row_cap < n_rows, share_cap < n_share_rows or group_cap < n_groups; out_info holds all three counts, nothing else is valid.
 *   Fewer than 2^31 pairs and rows per call.  Works on a host-only engine too (the same per-item functions on host threads).
 * _dev: every array is a device pointer (the CSR may be what bmq_match_submit_dev left in HBM), total = d_row_ptr[n_topics], n_senders = the
 *   length of d_sender_hash; runs on the engine stream and returns when the rows are complete.  Needs a device.
 * bmq_delivery_wait: the wait of a BMQ_FMT_DELIVERY ticket (bmq_match_submit_fmt): the plan of the batch without its CSR ever leaving
 *   the GPU.  The senders are handed over here -- a few bytes per publisher, staged on the engine stream in front of the plan's kernels.
 *   *out_total = the ids the CSR holds.  BMQ_E_NOSPACE as above, and the ticket is released, as with the other waits; waiting on a ticket
 *   of another format, or on this one with another format's call, is BMQ_E_STATE and leaves the ticket in flight.  Needs a device. */
#define BMQ_FMT_DELIVERY 4
typedef struct bmq_delivery_info {
    uint32_t n_rows, n_share_rows, n_groups;
    uint32_t n_merged_groups, n_share_only_groups;
    uint32_t special; /* bit 0: the group of unresolved shared rows is present, bit 1: the group of dead route ids */
    uint64_t generation;
    float ms_group, ms_resolve, ms_map, ms_merge;
} bmq_delivery_info;
int bmq_delivery_plan(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_topics, const uint32_t* sender_off,
                      const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap,
                      uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap,
                      bmq_delivery_info* out_info);
int bmq_delivery_plan_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_topics, uint64_t total,
                          const uint32_t* d_sender_off, const int32_t* d_sender_hash, uint32_t n_senders, uint64_t nonce, uint32_t* d_out_topic,
                          uint32_t* d_out_route, uint32_t* d_out_aux, uint32_t row_cap, uint32_t* d_out_share_sender, uint32_t* d_out_share_member,
                          uint32_t share_cap, uint32_t* d_out_group_off, uint32_t group_cap, bmq_delivery_info* out_info);
int bmq_delivery_wait(bmq_engine* e, int ticket, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic,
                            uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                            uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total);

/* ---- the fan-out caps of MatchedRoutes over a whole match batch ------------------------------------------------------------- */
/* bmq_routes_cap for a CSR whose rows carry caps of their own, answered where the CSR lies.  DistWorkerCoProc.batchDist never sees an
 * uncapped match: every topic's routes come out of a MatchedRoutes (DW/cache/MatchedRoutes.java:87-141) under its tenant's
 * MaxPersistentFanout / MaxGroupFanout.
 *   in : row_ptr[n_rows + 1], route_ids[row_ptr[n_rows]]: what bmq_match_batch* returned (rows ascending by id, no repeats);
 *        the caps table max_persistent_fanout[n_caps] / max_group_fanout[n_caps] (one entry per tenant, say) and row_caps[n_rows], the
 *        table entry of every row (NULL: every row takes entry 0).  A negative cap or an index >= n_caps: BMQ_E_INVAL, nothing is written.
 *   out: for row r with caps (pf, gf) exactly what bmq_routes_cap(e, row r, pf, gf) gives: a row no longer than min(pf, gf) is copied
 *        through (dead ids and all; out_class_counts[2 r], [2 r + 1] == 0xFFFFFFFF); in every other row dead ids are dropped and a class
 *        with more members than its cap keeps the members with the smallest KEYS (unsigned bytes, a proper prefix first), in the input's
 *        order; out_class_counts (may be NULL) = the persistent / group routes kept.
 *   events (out_events may be NULL): 4 int32 each {type 0 = PersistentFanoutThrottled 1 = GroupFanoutThrottled, row, rejected route id,
 *        max count}.  Rows ascend; inside a row the persistent events come first, in key order, then the group events, in key order (the
 *        two classes are not interleaved as bmq_routes_cap interleaves them).  *out_n_events counts all of them, also those behind events_cap.
 *   out_info: n_in / n_kept: ids in / out; n_rows_classified: rows longer than a cap; n_rows_ranked: rows with a class over its cap,
 *        ordered by key on the device; n_rows_fallback: such rows with a class of more than 4096 members, whose keys were sorted on the
 *        host instead; n_events; generation: of the route index the ids belong to; ms_*: HIP-event times of the three passes while
 *        bmq_set_kernel_timing is on, else 0.
 *   BMQ_E_NOSPACE: out_cap < out_info->n_kept; the events and out_info are valid, the rows are not.
 * Read-only: nothing is written to the index, nothing is cached per route.  Works on a host-only engine too (the same per-item functions
 * on host threads).
 * _dev: every array is a device pointer (the CSR may be what bmq_match_submit_dev left in HBM), total = d_row_ptr[n_rows]; runs on the
 *   engine stream and returns when the rows are complete.  Needs a device.
 * bmq_delivery_wait_capped: bmq_delivery_wait with the caps applied in between -- the CSR the batch left in the slot is capped with row_caps =
 *   the batch's topic_tenant and the plan is made of the capped CSR, neither leaving the GPU.  n_caps must be the batch's tenant count
 *   (else BMQ_E_INVAL, and the ticket stays in flight); the caps are host arrays.  *out_total = the ids of the UNCAPPED CSR.  BMQ_E_NOSPACE
 *   as bmq_delivery_wait reports it; the events and out_caps_info are valid then too. */
typedef struct bmq_caps_info {
    uint64_t n_in, n_kept;
    uint32_t n_rows_classified, n_rows_ranked, n_rows_fallback, n_events;
    uint64_t generation;
    float ms_classify, ms_rank, ms_write;
} bmq_caps_info;
int bmq_routes_cap_batch(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_rows, const uint32_t* row_caps,
                         const int32_t* max_persistent_fanout, const int32_t* max_group_fanout, uint32_t n_caps, uint32_t* out_row_ptr,
                         uint32_t* out_route_ids, uint64_t out_cap, uint32_t* out_class_counts, int32_t* out_events, uint32_t events_cap,
                         uint32_t* out_n_events, bmq_caps_info* out_info);
int bmq_routes_cap_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_rows, uint64_t total,
                       const uint32_t* d_row_caps, const int32_t* d_max_persistent_fanout, const int32_t* d_max_group_fanout, uint32_t n_caps,
                       uint32_t* d_out_row_ptr, uint32_t* d_out_route_ids, uint64_t out_cap, uint32_t* d_out_class_counts, int32_t* d_out_events,
                       uint32_t events_cap, uint32_t* out_n_events, bmq_caps_info* out_info);
int bmq_delivery_wait_capped(bmq_engine* e, int ticket, const int32_t* max_persistent_fanout, const int32_t* max_group_fanout, uint32_t n_caps,
                             const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic, uint32_t* out_route,
                             uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member, uint32_t share_cap,
                             uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total, int32_t* out_events,
                             uint32_t events_cap, uint32_t* out_n_events, bmq_caps_info* out_caps_info);

/* ---- the submit-time fan-out gate of DeliverExecutorGroup.submit over a whole match batch ----------------------------------------- */
/* What DeliverExecutorGroup.submit (DW/DeliverExecutorGroup.java:112-231) does to every message pack before it calls send, for a whole
 * CSR, answered where the CSR lies.  submit re-reads MaxPersistentFanout / MaxGroupFanout and reads MaxPersistentFanoutBytes
 * (Setting.java:62) (:131-133), asks the resource throttler for transient and persistent fan-out bandwidth (:135-139), admits persistent
 * routes while count < maxCount && bytes < maxBytes, every admitted route adding the pack's estimated size (:152-156), drops every
 * transient route of a tenant without bandwidth (:190-202), admits groups up to MaxGroupFanout (:206-208), reports ONE event per kind and
 * pack (:158-186, :193-201, :210-218), meters MqttPersistentFanOutBytes (:122, :229), decides `inline` from routes.size() <
 * inlineFanOutThreshold (:134) and bypasses all of it for a pack of exactly one route (:115-129).  `routes` is a concurrent hash set
 * (DW/cache/MatchedRoutes.java:42), so WHICH routes fill the admitted places is unspecified there; the counts, the flags and the metered
 * bytes depend only on how many routes of each class the row has.  This engine keeps the members with the smallest KEYS (unsigned bytes,
 * a proper prefix first), in the input's order, as the caps do.  The break at :225 loses nothing: a class throttled once stays throttled.
 *   in : row_ptr[n_rows + 1], route_ids[row_ptr[n_rows]] (rows ascending by id, no repeats); pack_bytes[n_rows] = SizeUtil.estSizeOf(msgPack);
 *        the gate table of n_gate entries (one per tenant, say): max_persistent_fanout, max_group_fanout (int32),
 *        max_persistent_fanout_bytes (int64), bandwidth (uint8: bit 0 = the tenant has transient fan-out bandwidth, bit 1 = persistent);
 *        row_gate[n_rows], the table entry of every row (NULL: every row takes entry 0); inline_threshold, one per call.  A negative limit,
 *        a bandwidth above 3 or an index >= n_gate: BMQ_E_INVAL, nothing is written.
 *   per row, with n live routes of which nP persistent, nT transient, nG groups (dead ids always leave the row), s = pack_bytes[r]:
 *        n == 0: nothing is kept, flags 0, no meter record.  n == 1: the route is kept whatever the table says, flags = BMQ_GATE_INLINE; a
 *        persistent route meters s bytes and one record.  n > 1: BMQ_GATE_INLINE iff n < inline_threshold; with A = min(pf, ceil(pb / s))
 *        (pb == 0: 0; s == 0: pf) and persistent bandwidth min(nP, A) persistent routes are kept and, if nP > A, BMQ_GATE_P_COUNT iff A >= pf,
 *        BMQ_GATE_P_BYTES iff A * s >= pb (64 bits; both can be set); without persistent bandwidth none is kept and, if nP > 0,
 *        BMQ_GATE_NO_P_BANDWIDTH when pf > 0 && pb > 0, else P_COUNT iff pf == 0 and P_BYTES iff pb == 0; the transient routes are all kept
 *        with transient bandwidth, else none and BMQ_GATE_NO_T_BANDWIDTH iff nT > 0; min(nG, gf) groups are kept, BMQ_GATE_GROUP iff nG > gf;
 *        the meter of the row's entry takes kept persistent routes * s bytes and one record (also when the bytes are 0).
 *   out: the gated CSR out_row_ptr[n_rows + 1] / out_route_ids; out_row_flags[n_rows]: BMQ_GATE_* bits, one event kind each (P_COUNT =
 *        PersistentFanoutThrottled, P_BYTES = PersistentFanoutBytesThrottled, NO_P_BANDWIDTH / NO_T_BANDWIDTH = OutOfTenantResource with
 *        reason TotalPersistentFanOutBytesPerSeconds / TotalTransientFanOutBytesPerSeconds -- the adapter reports it once per publisher of
 *        the pack --, GROUP = GroupFanoutThrottled); out_class_counts[3 n_rows] (may be NULL): persistent, transient, group routes kept;
 *        out_meter_bytes[n_gate] (uint64) / out_meter_records[n_gate]: MqttPersistentFanOutBytes per table entry, zeroed by the call.
 *   out_info: n_in / n_kept: ids in / out; n_rows_single: rows of one live route; n_rows_gated: rows of more; n_rows_flagged: rows with any
 *        bit but INLINE; n_rows_ranked: rows with a class of which some but not all members stay, ordered by key on the device;
 *        n_rows_fallback: such rows with a class of more than 4096 members, whose keys were sorted on the host instead; generation: of the
 *        route index the ids belong to; ms_*: HIP-event times of the three passes while bmq_set_kernel_timing is on, else 0.
 *   BMQ_E_NOSPACE: out_cap < out_info->n_kept; flags, class counts, meters and out_info are valid, the rows are not.
 * Read-only: nothing is written to the index.  Locks and state are those of bmq_routes_cap_batch.  Works on a host-only engine too.
 * _dev: every array is a device pointer, total = d_row_ptr[n_rows]; runs on the engine stream and returns when the rows are complete.
 * bmq_delivery_wait_gated: bmq_delivery_wait_capped with the gate applied between the caps and the plan -- caps, gate and plan run on the
 *   slot's CSR without it leaving the GPU.  The same max_persistent_fanout / max_group_fanout serve the caps (per-route events, as
 *   bmq_delivery_wait_capped reports them) and the gate; row_gate is the batch's topic_tenant, n_gate must be its tenant count (else
 *   BMQ_E_INVAL, and the ticket stays in flight); pack_bytes[n_topics].  out_row_flags[n_topics], out_meter_bytes / out_meter_records
 *   [n_gate].  BMQ_E_STATE, BMQ_E_INVAL and BMQ_E_NOSPACE exactly as bmq_delivery_wait_capped; flags, meters and out_gate_info are valid
 *   with BMQ_E_NOSPACE too. */
#define BMQ_GATE_INLINE 1u
#define BMQ_GATE_P_COUNT 2u
#define BMQ_GATE_P_BYTES 4u
#define BMQ_GATE_NO_P_BANDWIDTH 8u
#define BMQ_GATE_NO_T_BANDWIDTH 16u
#define BMQ_GATE_GROUP 32u
typedef struct bmq_gate_info {
    uint64_t n_in, n_kept;
    uint32_t n_rows_single, n_rows_gated, n_rows_flagged, n_rows_ranked, n_rows_fallback;
    uint64_t generation;
    float ms_classify, ms_rank, ms_write;
} bmq_gate_info;
int bmq_routes_gate_batch(bmq_engine* e, const uint32_t* row_ptr, const uint32_t* route_ids, uint32_t n_rows, const uint32_t* pack_bytes,
                          const uint32_t* row_gate, const int32_t* max_persistent_fanout, const int32_t* max_group_fanout,
                          const int64_t* max_persistent_fanout_bytes, const uint8_t* bandwidth, uint32_t n_gate, uint32_t inline_threshold,
                          uint32_t* out_row_ptr, uint32_t* out_route_ids, uint64_t out_cap, uint32_t* out_row_flags, uint32_t* out_class_counts,
                          uint64_t* out_meter_bytes, uint32_t* out_meter_records, bmq_gate_info* out_info);
int bmq_routes_gate_dev(bmq_engine* e, const uint32_t* d_row_ptr, const uint32_t* d_route_ids, uint32_t n_rows, uint64_t total,
                        const uint32_t* d_pack_bytes, const uint32_t* d_row_gate, const int32_t* d_max_persistent_fanout,
                        const int32_t* d_max_group_fanout, const int64_t* d_max_persistent_fanout_bytes, const uint8_t* d_bandwidth, uint32_t n_gate,
                        uint32_t inline_threshold, uint32_t* d_out_row_ptr, uint32_t* d_out_route_ids, uint64_t out_cap, uint32_t* d_out_row_flags,
                        uint32_t* d_out_class_counts, uint64_t* d_out_meter_bytes, uint32_t* d_out_meter_records, bmq_gate_info* out_info);
int bmq_delivery_wait_gated(bmq_engine* e, int ticket, const int32_t* max_persistent_fanout, const int32_t* max_group_fanout,
                            const int64_t* max_persistent_fanout_bytes, const uint8_t* bandwidth, uint32_t n_gate, const uint32_t* pack_bytes,
                            uint32_t inline_threshold, const uint32_t* sender_off, const int32_t* sender_hash, uint64_t nonce, uint32_t* out_topic,
                            uint32_t* out_route, uint32_t* out_aux, uint32_t row_cap, uint32_t* out_share_sender, uint32_t* out_share_member,
                            uint32_t share_cap, uint32_t* out_group_off, uint32_t group_cap, bmq_delivery_info* out_info, uint64_t* out_total,
                            int32_t* out_events, uint32_t events_cap, uint32_t* out_n_events, bmq_caps_info* out_caps_info, uint32_t* out_row_flags,
                            uint64_t* out_meter_bytes, uint32_t* out_meter_records, bmq_gate_info* out_gate_info);

/* ---- dist-server side range pruning ---------------------------------------------------------------------- */
/* TenantRangeLookupCache.lookup (bifromq-dist/bifromq-dist-server/src/main/java/org/apache/bifromq/dist/server/scheduler/
 * TenantRangeLookupCache.java:62-109) for a batch of topics of ONE tenant against the tenant's candidate KV ranges in boundary
 * order: which ranges can hold a route whose filter matches the topic, judged -- exactly as the reference does -- from each
 * range's Fact{firstGlobalFilterLevels, lastGlobalFilterLevels} (Fact.proto:27-34) alone.
 *   cand_kind[c]: 0 = the range has no Fact (always kept), 1 = Fact without first/last (empty range: dropped), 2 = first/last given
 *   first / last : packed strings, entry c = the global filter levels (tenant id first) joined by NUL
 *   out_keep[t * n_cand + c] = 1 if candidate c is kept for topic t, else 0 (a candidate behind the point where the reference's
 *   loop stops -- no expansion filter at or after its first filter -- is dropped, as there). */
int bmq_range_lookup(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics, const uint32_t* topic_off,
                     uint32_t n_topics, const uint8_t* cand_kind, const uint8_t* first, const uint32_t* first_off, const uint8_t* last,
                     const uint32_t* last_off, uint32_t n_cand, uint8_t* out_keep);

/* ---- route-key codec (SCHEMA/KVSchemaUtil.java:91-130, SCHEMA/cache/RouteDetailCache.java:53-117) ------- */
/* flag: 1 normal (receiver = receiverUrl), 2 unordered share, 3 ordered share (receiver = group name).
 * filter = MQTT topic filter WITHOUT a $share/$oshare prefix.  Returns key length (writes if <= cap). */
uint32_t bmq_route_key_encode(const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filter,
                              uint32_t filter_len, uint8_t flag, const uint8_t* receiver, uint32_t receiver_len,
                              uint8_t* out, uint32_t cap);
/* Decode: spans (offset,len) into `key` for tenant, escaped filter (levels joined by NUL), receiver.
 * Returns flag (1..3) or BMQ_E_INVAL. */
int bmq_route_key_decode(const uint8_t* key, uint32_t key_len, uint32_t spans[6]);
int32_t bmq_java_string_hash(const uint8_t* utf8, uint32_t len);

/* ---- retain store key schema (bifromq-retain/bifromq-retain-store-schema/.../schema/KVSchemaUtil.java:44-73,
 * LevelHash.java:30-50) ---------------------------------------------------------------------------------------------------------- */
/* retainMessageKey(tenantId, topic) = 0x00 | u16be(len tenant) | tenant | u16be(#levels) | LevelHash(levels) | escape(topic);
 * LevelHash = one byte per level (FNV-1a 32 over the level's UTF-16 code units, lowest byte).  Returns the key length. */
uint32_t bmq_retain_message_key(const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topic, uint32_t topic_len, uint8_t* out,
                                uint32_t cap);
/* What MatchCallRangeRouter.rangeLookup derives from ONE topic filter before it consults the range router
 * (bifromq-retain-server/.../scheduler/MatchCallRangeRouter.java:60-134): for a filter without wildcards the exact
 * retainMessageKey; otherwise retainKeyPrefix(tenant, levels, filterPrefix) with levels = level count (a trailing '#' not counted)
 * and filterPrefix = the levels in front of the first wildcard, plus LevelHash(filterPrefix) (the pruning key of findCandidates).
 * Returns a bit mask: 1 = the filter has a wildcard, 2 = it ends with '#' (matches keys of MORE levels too); negative on error. */
int bmq_retain_filter_route(const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filter, uint32_t filter_len,
                            uint8_t* out_key_prefix, uint32_t cap, uint32_t* out_key_len, uint8_t* out_level_hash, uint32_t hash_cap,
                            uint32_t* out_hash_len, uint32_t* out_levels);

/* ---- KV range router: the step between a match request and the range replicas that serve it ----------- */
/* The reference's client-side router is a TreeMap<Boundary, KVRangeSetting> in BoundaryUtil.compare order
 * (base-kv/base-kv-type-proto/.../utils/BoundaryUtil.java:142-195); here it is an array of n_ranges boundaries in that order:
 *   range_flags[r]        : bit 0 = the boundary has a start key, bit 1 = it has an end key (an absent side is open; a present key may
 *                           be empty: NULL_BOUNDARY = no start, end "")
 *   start/start_off, end/end_off : packed keys, entry r empty where the side is absent
 * BMQ_E_INVAL if the array is not strictly ascending in that order.
 * KVRangeRouterUtil.findByKey (base-kv/base-kv-store-client/.../client/KVRangeRouterUtil.java:41-52): *out_index = the range that holds
 * `key`, or -1.  KVRangeRouterUtil.findByBoundary (:54-103): the ranges it returns are contiguous: [*out_first, *out_first + *out_count);
 * query_flags as range_flags.  (Where TreeMap.subMap would throw "fromKey > toKey" -- a router that does not cover the query's start --
 * the result is empty.) */
int bmq_router_find_by_key(const uint8_t* range_flags, const uint8_t* start, const uint32_t* start_off, const uint8_t* end,
                           const uint32_t* end_off, uint32_t n_ranges, const uint8_t* key, uint32_t key_len, int32_t* out_index);
int bmq_router_find_by_boundary(const uint8_t* range_flags, const uint8_t* start, const uint32_t* start_off, const uint8_t* end,
                                const uint32_t* end_off, uint32_t n_ranges, uint8_t query_flags, const uint8_t* q_start, uint32_t q_start_len,
                                const uint8_t* q_end, uint32_t q_end_len, uint32_t* out_first, uint32_t* out_count);
/* MatchCallRangeRouter.rangeLookup(tenantId, topicFilters, effectiveRouter) (bifromq-retain/bifromq-retain-server/.../scheduler/
 * MatchCallRangeRouter.java:56-134) for a batch of topic filters of ONE tenant: out_keep[f * n_ranges + r] = 1 if filter f has to be
 * sent to range r -- a plain topic to the range holding its retainMessageKey, a filter of a fixed level count to the ranges
 * overlapping [retainKeyPrefix, upperBound), a filter ending in '#' to the ranges overlapping [retainKeyPrefix, end of the tenant)
 * minus those findCandidates prunes by LevelHash (:96-133).  BMQ_E_INVAL: a plain topic no range holds (the reference asserts), or a
 * boundary key findCandidates cannot parse (the reference throws).  One deviation: a filter prefix whose LevelHash is all 0xFF bytes
 * makes the reference fail with a NullPointerException (upperBound(levelHash) == null); here its upper bound is open and nothing is
 * pruned by the first rule.
 * mode BMQ_ROUTER_REFERENCE reproduces findCandidates rule for rule.  Those rules look at the LevelHash of a range's start / end key
 * only, as if a range never spanned two level counts: a range [key of 4 levels, key of 6 levels) is pruned for `a/#` when its start
 * key's hash sorts behind hash(a), although every 5-level topic under `a` lives in it (tests/test_router.py shows the case) -- retained
 * messages are then missing from the reply.  mode BMQ_ROUTER_EXACT keeps a range iff it meets one of the key intervals
 * [tenant | L | hash(prefix), tenant | L | upperBound(hash(prefix))), L >= levels, the filter can match in: never a range too few,
 * never one too many. */
#define BMQ_ROUTER_REFERENCE 0u
#define BMQ_ROUTER_EXACT 1u
int bmq_retain_range_lookup(const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filters, const uint32_t* filter_off, uint32_t n_filters,
                            const uint8_t* range_flags, const uint8_t* start, const uint32_t* start_off, const uint8_t* end,
                            const uint32_t* end_off, uint32_t n_ranges, uint32_t mode, uint8_t* out_keep);

/* The same three lookups over a router OBJECT: the boundaries are copied, checked and indexed once and asked many times (the reference
 * keeps its TreeMap between calls as well and rebuilds it only when the range landscape changes).  n_ranges of bmq_router_retain_lookup's
 * out_keep rows = the n_ranges the router was created with.  A router is immutable: any number of threads may ask it. */
typedef struct bmq_router bmq_router;
int bmq_router_create(const uint8_t* range_flags, const uint8_t* start, const uint32_t* start_off, const uint8_t* end,
                      const uint32_t* end_off, uint32_t n_ranges, bmq_router** out);
void bmq_router_destroy(bmq_router* r);
int bmq_router_lookup_key(const bmq_router* r, const uint8_t* key, uint32_t key_len, int32_t* out_index);
int bmq_router_lookup_boundary(const bmq_router* r, uint8_t query_flags, const uint8_t* q_start, uint32_t q_start_len, const uint8_t* q_end,
                               uint32_t q_end_len, uint32_t* out_first, uint32_t* out_count);
int bmq_router_retain_lookup(const bmq_router* r, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* filters,
                             const uint32_t* filter_off, uint32_t n_filters, uint32_t mode, uint8_t* out_keep);

/* ---- retain direction (RS/index/IRetainTopicIndex.java:27-35) -------------------------------------------- */
/* A retained-topic id is a STABLE handle, like a route id: a bulk load (bmq_retain_rebuild*, bmq_retain_compact) numbers the topics by
 * the rank of (tenant, level list) in byte order -- tenants in byte order of their ids, a tenant's topics level list by level list, so
 * that every subtree is one id range --; a topic added later by bmq_retain_apply* gets the next unused id; the id of a removed topic
 * goes dead and comes back to life when the topic is retained again.  No id changes or is reused until the next bulk load
 * (bmq_retain_info.generation counts them).
 * Load the retained-topic index: (tenant, topic) pairs.  Replaces the full-scan rebuild in RS/RetainStoreCoProc.java:134-137,279-296.
 * _ex: with what IRetainTopicIndex.add(tenantId, topic, timestamp, expirySeconds) carries (RS/index/IRetainTopicIndex.java:28):
 * timestamp_hlc[i] = Message.timestamp (an HLC: milliseconds << 16 | counter, base-hlc HLC.java:145-151), expiry_seconds[i] =
 * Message.expiryInterval; the message expires at (timestamp_hlc >> 16) + 1000 * expiry_seconds ms (RS/RetainStoreCoProc.java:298-304).
 * Both arrays NULL (or the plain entry points): the topics never expire. */
int bmq_retain_rebuild(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                       const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off,
                       uint32_t n_topics);
int bmq_retain_rebuild_ex(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                          const uint32_t* topic_tenant, const uint8_t* topics, const uint32_t* topic_off, uint32_t n_topics,
                          const uint64_t* timestamp_hlc, const uint32_t* expiry_seconds);
/* IRetainTopicIndex.add / remove (RS/index/RetainTopicIndex.java:126-134; UTIL/index/TopicLevelTrie.java:49-182) as the post-commit
 * closures of RetainStoreCoProc.batchRetain / gc issue them (RS/RetainStoreCoProc.java:240-255,270-275); op[i]: 0 = add (an add of a
 * topic that is there replaces its timestamp / expiry: :246-249), 1 = remove (of an absent topic: a no-op).  The index is mutated
 * WHERE IT LIVES, by three kernels on the engine stream (bmq_retain_core.h): the batch lands behind every match batch launched before
 * it and in front of every later one; matching is never refused while a batch is applied, and the call returns when the device has
 * applied it.  Ops on the same topic inside one batch take effect in order (the last one decides).  A malformed op (op code, tenant
 * index) fails the batch with BMQ_E_INVAL before anything is changed.
 * _batch: ops of several tenants in one call -- op_tenant[i] indexes the tenant table (NULL: every op belongs to tenant 0);
 * out_topic_ids (may be NULL) [i] = the id of op i's topic, 0xFFFFFFFF for the removal of an absent topic or an op that a later op on
 * the same topic superseded. */
int bmq_retain_apply(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics,
                     const uint32_t* topic_off, const uint8_t* op, uint32_t n);
int bmq_retain_apply_ex(bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, const uint8_t* topics, const uint32_t* topic_off,
                        const uint8_t* op, const uint64_t* timestamp_hlc, const uint32_t* expiry_seconds, uint32_t n);
int bmq_retain_apply_batch(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                           const uint8_t* topics, const uint32_t* topic_off, const uint8_t* op, const uint64_t* timestamp_hlc,
                           const uint32_t* expiry_seconds, uint32_t n, uint32_t* out_topic_ids);
/* Maintenance: fold what bmq_retain_apply* changed into a fresh bulk load (removed topics and their ids go, added topics become ranks
 * again: every subtree one id range, the fast path of '+' and '#').  A new generation of ids. */
int bmq_retain_compact(bmq_engine* e);
/* The same generation change without the stall (round 6): TopicLevelTrie contracts tombed branches as it goes
 * (UTIL/index/TopicLevelTrie.java:257-384); bmq_retain_compact holds the engine for the whole load (2 s for 1 M topics).
 *   bmq_retain_compact_begin   snapshot of the live topics with their stamps (the engine lock for tens of milliseconds);
 *   bmq_retain_compact_build   loads them into an index of their own: the long part, NO engine lock held -- matching and bmq_retain_apply* go
 *                              on meanwhile, what they add / remove is logged;
 *   bmq_retain_compact_swap    uploads the new generation, replays the log in order and makes it the serving one (no batch may be in flight:
 *                              BMQ_E_STATE).  Topic ids are re-numbered: bmq_retain_info.generation + 1, as after bmq_retain_compact.
 *                              *out_carried = topics of the new bulk load, *out_replayed = logged ops replayed.  BMQ_E_NOSPACE: the log outgrew
 *                              1 GiB (abort and begin again; no mutation is ever refused).
 *   bmq_retain_compact_abort   drops the half-built generation.
 * One compaction call at a time; bmq_retain_rebuild* / bmq_retain_compact are refused (BMQ_E_STATE) between begin and swap / abort.
 * Which builder serves them is bmq_config.retain_builder's choice:
 *   0 (default)  the HOST builder.  _begin copies the live topics to host strings under the lock, _build loads them into a host index, _swap
 *                uploads its image and re-creates the per-id arrays from host loops under the lock.
 *   1            as 0: the value moves the bulk loads to the executor, not these three calls (bmq_retain_build_info.builder = 0 after _swap).
 *   3            the EXECUTOR builder, and the snapshot never leaves the executor.  _begin selects the live ids where the index lives and
 *                gathers their strings and stamps into a private snapshot in executor memory, on the engine's stream (what crosses to the host
 *                under the lock is a handful of words); the strings of bulk-loaded ids come from the generation's key store, which _begin
 *                builds from the host's copy of the load, under the lock, if the generation has none -- a caller that minds calls
 *                bmq_retain_keys_prepare ahead; a generation made by _swap brings its store along, so only the first round after a
 *                bmq_retain_rebuild* pays.  _build runs the builder on an executor and stream of its own, reads the snapshot only, copies it
 *                to the host once for the next catalogue (outside the lock) and lays out the next key store, per-id stamps, dead bitmap and
 *                empty overlay in executor memory.  _swap exchanges pointers -- no upload, no host loop over the topics, no copy whose size
 *                grows with the number of topics -- and replays the log.  A live topic of more than 128 levels makes the builder decline:
 *                _build then runs the host builder over the host copy of the snapshot and _swap is the upload of retain_builder = 0
 *                (bmq_retain_build_info.builder = 0, fallback = 1); results are the same.
 * bmq_retain_compact_info_get tells of the running compaction, or of the last one that ended in a swap. */
int bmq_retain_compact_begin(bmq_engine* e);
int bmq_retain_compact_build(bmq_engine* e);
int bmq_retain_compact_swap(bmq_engine* e, uint64_t* out_carried /* may be NULL */, uint64_t* out_replayed /* may be NULL */);
int bmq_retain_compact_abort(bmq_engine* e);
typedef struct bmq_retain_compact_info {
    uint32_t state;             /* 0 = none yet, 1 = begun, 2 = built, 3 = swapped (an abort leaves the last swapped one, or none)              */
    uint32_t builder;           /* who builds / built the next generation: 0 = host builder, 1 = executor builder (known after _build; until    */
                                /* then what bmq_config.retain_builder asks for)                                                              */
    uint32_t fallback;          /* 1 = the executor builder declined (a topic of more than 128 levels) and the host builder ran                  */
    uint32_t reserved0;
    uint64_t n_items;           /* topics in the snapshot                                                                                      */
    uint64_t snapshot_bytes;    /* what the snapshot holds: executor memory (builder 1), or the bytes of its host strings (builder 0)            */
    uint64_t replayed;          /* logged ops replayed by the swap                                                                             */
    uint64_t locked_copy_bytes; /* bytes of all host <-> executor copies issued while the engine lock was held in _begin and in _swap before     */
                                /* the replay (device engines: host <-> device; host-only engines: the same call sites, a memcpy each)          */
    float begin_ms;             /* host clock around _begin's own work ...                                                                     */
    float build_ms;             /* ... _build's ...                                                                                            */
    float swap_ms;              /* ... and _swap's, up to the start of the replay                                                              */
    uint32_t reserved1;
} bmq_retain_compact_info;
int bmq_retain_compact_info_get(const bmq_engine* e, bmq_retain_compact_info* out);
/* Split and merge of the retain store's base-kv range WITHOUT a KV scan: IKVRangeCoProc.reset(Boundary) fires on every split and merge, and
 * RetainStoreCoProc answers it with load(), a scan of the whole range (RS/RetainStoreCoProc.java:133-137,279-296).  The retained-topic index
 * holds no KV keys, and no id range is a key range (tenants are ranked in byte order, keys sort by tenant length first), so "is
 * retainMessageKey(id) inside [start, end)" is a predicate over the ids, evaluated where the index lives: one kernel pass that walks the
 * key's segments against the boundary keys and stops at the first difference, without composing the key (bmq_retain_core.h: retain_key_cmp;
 * host-only engines run the same function on host threads).  Boundary arguments as for bmq_routes_count_in: flags bit 0 / 1 = start / end
 * present, a present key may be empty, both present with start >= end is BMQ_E_INVAL; order = unsigned bytes, a proper prefix first
 * (BoundaryUtil.inRange).  The key store of bmq_retain_keys_prepare is built on the first call of a generation.
 *   bmq_retain_count_in          retained topics whose key lies inside the boundary and (out_key_bytes != NULL) the sum of their key lengths
 *                                -- keys only, no values.  Read-only, one pass; locks and state as bmq_retain_expired.  No index loaded: 0.
 *   bmq_retain_ids_in            their ids, ascending; buffer protocol of bmq_retain_live_ids.
 *   bmq_retain_compact_begin_in  bmq_retain_compact_begin for a range that SHRINKS (flags = 0 is bmq_retain_compact_begin): the snapshot takes
 *                                only the topics inside; _build / _swap / _abort as before.  The serving generation matches and mutates over
 *                                ALL its topics until the swap; at the swap, logged ops (adds, removes, bmq_retain_remove_ids) whose key lies
 *                                outside are not replayed: *out_carried = topics inside, *out_replayed = ops replayed.  Afterwards the engine
 *                                does not police mutations against the boundary.
 *   bmq_retain_import            every retained topic of src whose key lies inside the boundary goes into dst with its timestamp_hlc /
 *                                expiry_seconds.  src is locked only while ids, stamps and strings are snapshotted, then goes on serving; a
 *                                topic mutated during the call is imported as it was at the snapshot.  An EMPTY dst (no index, or no retained
 *                                topic and no compaction running: the new sibling of a split) is bulk-loaded -- ranks, the fast path of '+'
 *                                and '#', a new generation; *out_imported = topics.  Otherwise chunks of at most 65 536 add ops go through the
 *                                ordinary apply path (a compaction running on dst logs them): a topic dst holds already has its stamps
 *                                replaced and counts in *out_replaced, the others in *out_imported.  dst == src: BMQ_E_INVAL.  Host-only and
 *                                device engines may be paired, and two devices (the strings cross the host; dst bulk-loads with the builder its
 *                                bmq_config.retain_builder names).
 * A split of range A at key s:  bmq_retain_import(B, A, start = s)  then  bmq_retain_compact_begin_in(A, end = s), _build, _swap.
 * A merge of B into A:          bmq_retain_import(A, B, flags = 0). */
int bmq_retain_count_in(const bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                        uint64_t* out_topics /* may be NULL */, uint64_t* out_key_bytes /* may be NULL */);
int bmq_retain_ids_in(const bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len,
                      uint32_t* out_ids, uint32_t cap, uint32_t* out_n);
int bmq_retain_compact_begin_in(bmq_engine* e, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end, uint32_t end_len);
int bmq_retain_import(bmq_engine* dst, bmq_engine* src, uint8_t flags, const uint8_t* start, uint32_t start_len, const uint8_t* end,
                      uint32_t end_len, uint64_t* out_imported /* may be NULL */, uint64_t* out_replaced /* may be NULL */);
typedef struct bmq_retain_info {
    uint64_t n_topics;        /* retained topics now */
    uint64_t n_tenants;       /* tenants of the last bulk load */
    uint64_t id_bound;        /* every id handed out in this generation is below */
    uint64_t loaded_topics;   /* ids below are ranks of the last bulk load ... */
    uint64_t loaded_removed;  /* ... of which that many have been removed since */
    uint64_t added_ids;       /* ids handed out to topics added since the bulk load */
    uint64_t overlay_nodes;   /* nodes of the overlay trie that holds them */
    uint64_t epoch;           /* +1 per rebuild / apply / compact */
    uint64_t generation;      /* +1 per bulk load (rebuild / compact): ids of different generations are unrelated */
} bmq_retain_info;
int bmq_retain_info_get(const bmq_engine* e, bmq_retain_info* out);
/* The BULK LOAD behind the serving generation (bmq_retain_rebuild*, bmq_retain_compact, bmq_retain_compact_swap, bmq_retain_import into an
 * empty engine, the empty load the first bmq_retain_apply* of a fresh engine starts from).  BMQ_E_STATE: nothing is loaded. */
typedef struct bmq_retain_build_info {
    uint32_t builder;          /* 0 = the host builder, 1 = the executor builder (bmq_config.retain_builder) built this generation           */
    uint32_t fallback;         /* 0, or why a retain_builder = 1 / 3 engine ran the host builder: 1 = a topic of more than 128 levels        */
    uint64_t n_items;          /* items handed in ...                                                                                       */
    uint64_t n_topics;         /* ... distinct (tenant, topic) pairs among them = topic ids of the load                                      */
    uint64_t n_tenants;
    uint64_t n_nodes;          /* trie nodes, the tenants' roots included                                                                    */
    uint64_t n_edges;          /* entries in use of the edge regions (= nodes - tenants)                                                     */
    uint64_t n_edge_overflows; /* edges that lie behind their home bucket (counted by the executor builder; the host builder reports 0)       */
    uint64_t n_posts;          /* grandchild postings                                                                                        */
    uint64_t n_gp_runs;        /* (grandparent, token) runs of them = entries in use of the RGp tables                                       */
    uint64_t n_tokens;         /* distinct level strings and tenant ids in the dictionary                                                    */
    uint32_t max_depth;        /* levels of the deepest topic                                                                                */
    float ms_total;            /* host clock around the build, the last synchronise included (without the snapshot of bmq_retain_compact)    */
    float ms_sort;             /* ... of which the ordering of the items (executor builder; 0 for the host builder)                          */
    uint32_t n_gp_overflows;   /* RGp runs that lie behind their home bucket (executor builder; 0 for the host builder)                       */
} bmq_retain_build_info;
int bmq_retain_build_info_get(const bmq_engine* e, bmq_retain_build_info* out);
/* id -> the topic the id denotes in this generation (whether or not it is retained right now: bmq_retain_topic_info tells): out
 * receives the tenant id followed by the topic (no separator), *out_tenant_len bytes of tenant, *out_len bytes in total.
 * bmq_retain_topics: many ids at once (bulk-loaded ids from the host's copy of the load, added ones with ONE device gather):
 * out_off[n + 1] byte offsets into out, out_tenant_len[n]; an unknown id gives an empty string. */
int bmq_retain_topic(const bmq_engine* e, uint32_t topic_id, uint8_t* out, uint32_t cap, uint32_t* out_len,
                     uint32_t* out_tenant_len);
int bmq_retain_topics(const bmq_engine* e, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off,
                      uint32_t* out_tenant_len);
/* id -> the rest of RetainedMsgInfo (RS/index/RetainedMsgInfo.java:29-36) + the expiry instant in ms (~0: never); any out may be NULL.
 * BMQ_E_INVAL: the id was never handed out, or its topic is not retained any more. */
int bmq_retain_topic_info(const bmq_engine* e, uint32_t topic_id, uint64_t* out_timestamp_hlc, uint32_t* out_expiry_seconds,
                          uint64_t* out_expire_at_ms);
/* IRetainTopicIndex.findAll() (RS/index/RetainTopicIndex.java:140-143): *out_n_topics = retained topics now, *out_epoch (may be
 * NULL) counts the retain mutations so far; bmq_retain_live_ids lists their ids, ascending -- of one tenant (every topic of it, '$'
 * ones too) or, tenant == NULL, of all.  Writes up to cap ids, *out_n = total; BMQ_E_NOSPACE if cap was too small. */
int bmq_retain_find_all(const bmq_engine* e, uint64_t* out_n_topics, uint64_t* out_epoch);
int bmq_retain_live_ids(const bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, uint32_t* out_ids, uint32_t cap, uint32_t* out_n);
/* Retained topics per tenant, without a KV scan: RetainStoreCoProc.load() counts them while it scans (RS/RetainStoreCoProc.java:279-296,
 * tenantsStats.increaseTopicCount per key -- '$' topics included).  Every tenant with at least one retained topic NOW, in unsigned byte
 * order of the ids, with its count in out_counts[i]; the counts sum to bmq_retain_info.n_topics.  Bulk-loaded tenants: size of the
 * tenant's rank range minus the dead ids inside (the rank directory: no pass over the ids); ids handed out since the load: one pass of
 * the census kernel; a tenant with both parts comes out once, with the sum.  Buffer protocol of bmq_routes_tenant_stats (one number per
 * tenant). */
int bmq_retain_tenant_counts(const bmq_engine* e, uint8_t* out_tenants, uint64_t tenants_cap, uint64_t* out_tenant_off, uint64_t* out_counts,
                             uint32_t cap, uint32_t* out_n_tenants /* may be NULL */, uint64_t* out_tenant_bytes /* may be NULL */);
/* The two native halves of RetainStoreCoProc.gc around the KV commit (RS/RetainStoreCoProc.java:258-277), for ids the engine handed out
 * (bmq_retain_expired, bmq_retain_live_ids, a match):
 *   bmq_retain_message_keys  out_off[n + 1] / out: retainMessageKey(tenant, topic) of every id (the keys gc deletes and match gets with
 *                            reader.get), equal to bmq_retain_message_key of bmq_retain_topics id for id; EMPTY for an id that is unknown
 *                            or not retained now.  Host code under one engine lock (bmq_retain_keys_by_id composes the same bytes on
 *                            the device).  BMQ_E_NOSPACE if cap < out_off[n] (offsets are still written).
 *   bmq_retain_remove_ids    the post-commit index removal (:270-275) BY ID: every live id goes dead exactly as a remove op of
 *                            bmq_retain_apply_batch leaves it (dead bit, expire_at = 0, the counts behind bmq_retain_info), then the
 *                            rank directory is rebuilt -- one kernel over the ids, nothing is looked up level by level -- on the engine
 *                            stream behind batches in flight.  Ids that are dead already and repeats inside the call are no-ops;
 *                            *out_removed (may be NULL) = topics removed.  `generation` = bmq_retain_info.generation the ids belong to:
 *                            BMQ_E_STATE if it has changed; BMQ_E_INVAL if any id is >= id_bound (checked before anything changes).
 *                            The epoch advances as after bmq_retain_apply_batch; a later add of the same topic gets the same id back.
 *                            Between bmq_retain_compact_begin and _swap the removals enter the compaction log as remove ops of the
 *                            topics' strings, so the swap replays them (the log cap applies). */
int bmq_retain_message_keys(const bmq_engine* e, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off);
int bmq_retain_remove_ids(bmq_engine* e, const uint32_t* topic_ids, uint32_t n, uint64_t generation, uint64_t* out_removed /* may be NULL */);
/* The scan of RetainStoreCoProc's GC (RS/RetainStoreCoProc.java:257-277): ids (ascending) of the retained topics whose message has
 * expired at now_ms (expireTime <= now) -- of every tenant (tenant == NULL: the reference's findAll() branch), or of `tenant`: there the
 * reference scans index.match(tenantId, "#"), which does not reach topics whose first level starts with '$'
 * (RS/index/RetainTopicIndex.java:60,86,99), and neither does this.  override_expiry_seconds >= 0 replaces the stored expiry interval
 * as GCRequest.expirySeconds does.  One kernel over the ids + a device select.  Writes up to cap ids, *out_n = total; BMQ_E_NOSPACE
 * if cap was too small. */
int bmq_retain_expired(const bmq_engine* e, const uint8_t* tenant, uint32_t tenant_len, uint64_t now_ms,
                       int64_t override_expiry_seconds, uint32_t* out_ids, uint32_t cap, uint32_t* out_n);
/* Batch of IRetainTopicIndex.match(tenant, topicFilter) (RS/index/RetainTopicIndex.java:136-138; selector
 * :36-124; walk UTIL/index/TopicLevelTrie.java:190-249).  Output CSR of topic ids (ascending per row). */
int bmq_retain_match_batch(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                           const uint32_t* filter_tenant, const uint8_t* filters, const uint32_t* filter_off,
                           uint32_t n_filters, uint32_t* out_row_ptr, uint32_t* out_topic_ids,
                           uint64_t out_capacity, uint64_t* out_needed);
/* RetainStoreCoProc.match(tenant, filter, limit, now) (RS/RetainStoreCoProc.java:167-190; limit from RetainStoreCoProc.proto:63,
 * tenant default RetainMessageMatchLimit = 10, Setting.java:77): the reference walks the FULL match set and returns the first
 * `limit` messages that have not expired (expireAt > now).  The order it walks in is a HashSet's (UTIL/index/StrategySet.java:31),
 * i.e. unspecified; here it is ascending topic id: row i = the limit[i] SMALLEST ids among the matching topics that are still
 * live at now_ms (fewer if fewer are live; limit 0 -> empty row).  out_match_count[i] (may be NULL) = number of topics filter i
 * matches, expired ones included.  With every limit <= 64 nothing is expanded: the ids are picked from the matched id ranges.
 * Same buffer protocol as bmq_retain_match_batch. */
int bmq_retain_match_limited(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                             const uint32_t* filter_tenant, const uint8_t* filters, const uint32_t* filter_off,
                             uint32_t n_filters, const uint32_t* limit, uint64_t now_ms, uint32_t* out_row_ptr,
                             uint32_t* out_topic_ids, uint64_t out_capacity, uint64_t* out_needed, uint32_t* out_match_count);
/* The second half of RetainStoreCoProc.match(tenant, filter, limit, now) (RS/RetainStoreCoProc.java:167-190): for every hit the reference
 * calls reader.get(retainMessageKey(tenant, topic)) (:181), and gc deletes the same keys (:258-277).  The calls below compose
 * retainMessageKey (KVSchemaUtil.java:44-73, LevelHash.java:30-50; the format of bmq_retain_message_key) where the index lives, by two
 * kernels on the engine stream -- key lengths + a 64-bit scan, then the bytes -- behind whatever is in flight; host-only engines run the
 * same functions on host threads.  The strings of the bulk-loaded ids (ranks: the index holds no labels for them) come from a store in
 * device memory that is built from the host's copy of the load on the first of these calls in a generation and dropped at every
 * generation change (bmq_retain_rebuild*, bmq_retain_compact, bmq_retain_compact_swap): a load nobody asks keys of pays nothing.
 *   bmq_retain_keys_prepare  builds the store now if this generation has none (idempotent); *out_store_bytes (may be NULL) = the bytes it
 *                            holds.  BMQ_E_STATE: no retained-topic index is loaded.
 *   bmq_retain_keys_by_id    the contract of bmq_retain_message_keys word for word, and the same bytes: out_off[n + 1] / out =
 *                            retainMessageKey(tenant, topic) of every id, EMPTY for an id that is unknown or not retained now -- decided on
 *                            the device from the dead bitmap, no host copy of it is made.  BMQ_E_NOSPACE if cap < out_off[n] (offsets
 *                            are still written).  bmq_retain_message_keys stays the host-side cross-check.
 *   bmq_retain_keys_match    bmq_retain_match_limited (same rows, ids and match counts for the same input) plus the key of every kept id in
 *                            row order: out_key_off[kept + 1] (room for out_capacity + 1 entries) / out_keys.  The kept ids do not leave
 *                            the device between the select and the key kernels.  A kept id is live at now_ms, so no key is empty; when
 *                            nothing is kept no key kernel runs.  *out_needed = kept ids and *out_needed_key_bytes = key bytes are always
 *                            reported; BMQ_E_NOSPACE if either buffer is too small (ids too few: nothing but the row pointers, the counts
 *                            and the two sizes is written; key bytes too few: ids and key offsets are).  Host-only engines:
 *                            BMQ_E_NODEVICE, as for every match. */
int bmq_retain_keys_prepare(bmq_engine* e, uint64_t* out_store_bytes /* may be NULL */);
int bmq_retain_keys_by_id(const bmq_engine* e, const uint32_t* topic_ids, uint32_t n, uint8_t* out, uint64_t cap, uint64_t* out_off);
int bmq_retain_keys_match(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                          const uint32_t* filter_tenant, const uint8_t* filters, const uint32_t* filter_off,
                          uint32_t n_filters, const uint32_t* limit, uint64_t now_ms, uint32_t* out_row_ptr,
                          uint32_t* out_topic_ids, uint64_t out_capacity, uint64_t* out_needed, uint32_t* out_match_count,
                          uint64_t* out_key_off, uint8_t* out_keys, uint64_t keys_cap, uint64_t* out_needed_key_bytes);
int bmq_retain_match_batch_dev(bmq_engine* e, const uint8_t* d_tenants, const uint32_t* d_tenant_off,
                               uint32_t n_tenants, const uint32_t* d_filter_tenant, const uint8_t* d_filters,
                               const uint32_t* d_filter_off, uint32_t n_filters, uint32_t* d_out_row_ptr,
                               uint32_t* d_out_topic_ids, uint64_t out_capacity, uint64_t* d_out_total);

/* The two native halves of RetainStoreCoProc.batchRetain around the KV commit (RS/RetainStoreCoProc.java:193-255), for a whole batch of
 * (tenant, topic, message) ops.  Topics are bytes, taken literally ('+' and '#' are levels like any other, as for bmq_retain_apply*);
 * clear[i] != 0 says that the message's payload is empty.  There is no `now`: an expired topic that has not been collected is still
 * retained, as index.match returns it (:213).
 *   bmq_retain_plan         the pre-commit half, read-only, on the engine stream behind whatever is in flight (locks and state of
 *                           bmq_retain_keys_by_id: the serving generation answers while a retain compaction runs, the epoch stays).  Ops
 *                           with equal tenant BYTES and equal topic BYTES form a group whose LAST op is the winner, as
 *                           BatchRetainCallHelper.makeBatch keeps the last request per topic (two tenant-table entries with the same bytes
 *                           are one tenant).  Per op i, with w = the winner of its group and `present` = the topic has a live id now:
 *                             out_code[i]     clear[w] ? 1 (CLEARED) : 0 (RETAINED)   -- RetainResult.Code, RetainStoreCoProc.proto:50-53
 *                             out_winner[i]   w
 *                             out_action[i]   i != w: BMQ_PLAN_SUPERSEDED; else clear[w] ? (present ? REMOVE : NONE) : (present ? UPDATE : ADD)
 *                             out_topic_id[i] the live id if present (every op of the group), else 0xFFFFFFFF
 *                             key i           retainMessageKey(tenant, topic) if i == w and the action is not NONE (the KV put of an ADD /
 *                                             UPDATE, the KV delete of a REMOVE), else empty: out_key_off[n + 1] / out_keys
 *                             out_delta[t]    += 1 per ADD, -= 1 per REMOVE, filed under the winner's op_tenant (the topic-count change)
 *                           BMQ_E_INVAL (a tenant index out of range among them): no output is written.  BMQ_E_NOSPACE: keys_cap <
 *                           out_key_off[n]; everything except the key bytes is written.  n == 0: BMQ_OK, nothing is launched.  Host-only
 *                           engines run the same functions on host threads.
 *   bmq_retain_plan_commit  the post-commit closure (:240-255), with the op arrays of the plan and its out_action: BMQ_E_STATE and no
 *                           change if (generation, epoch) are not bmq_retain_info's any more; otherwise the winners with ADD / UPDATE go
 *                           through bmq_retain_apply_batch as adds (with their stamps), those with REMOVE as removes.  out_topic_ids[i]
 *                           (may be NULL) = the topic's id for the winners that changed the index, else 0xFFFFFFFF. */
enum { BMQ_PLAN_NONE = 0, BMQ_PLAN_ADD = 1, BMQ_PLAN_UPDATE = 2, BMQ_PLAN_REMOVE = 3, BMQ_PLAN_SUPERSEDED = 4 };
typedef struct bmq_retain_plan_info {
    uint64_t generation, epoch; /* of the index the plan was made on: what bmq_retain_plan_commit takes */
    uint64_t n_groups;          /* distinct (tenant, topic) pairs = winners */
    uint64_t n_add, n_update, n_remove, n_none;
    uint64_t key_bytes;
    double ms;                  /* host clock around the call */
} bmq_retain_plan_info;
int bmq_retain_plan(const bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants,
                    const uint32_t* op_tenant /* NULL: tenant 0 */, const uint8_t* topics, const uint32_t* topic_off, const uint8_t* clear,
                    uint32_t n, uint8_t* out_code, uint8_t* out_action, uint32_t* out_winner, uint32_t* out_topic_id /* each [n], may be NULL */,
                    int32_t* out_delta /* [n_tenants], may be NULL */, uint64_t* out_key_off /* [n + 1] */, uint8_t* out_keys, uint64_t keys_cap,
                    bmq_retain_plan_info* out_info /* may be NULL */);
int bmq_retain_plan_commit(bmq_engine* e, const uint8_t* tenants, const uint32_t* tenant_off, uint32_t n_tenants, const uint32_t* op_tenant,
                           const uint8_t* topics, const uint32_t* topic_off, uint32_t n, const uint8_t* action, const uint64_t* timestamp_hlc,
                           const uint32_t* expiry_seconds, uint64_t generation, uint64_t epoch, uint32_t* out_topic_ids /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* BMQ_H */
