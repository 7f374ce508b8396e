"""Python face of the C-ABI engine (include/bmq.h).  Thin: packs strings, calls libbmq.so, unpacks CSR.

All matching happens in the HIP kernels behind the ABI (bifromq_amd/csrc).  Nothing here matches topics.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

INT_MAX = 2**31 - 1
BMQ_WINDOW_MAX = 65536  # include/bmq.h
BMQ_PREFIX_MAX = 65536  # include/bmq.h
STATUS = {0: "OK", -1: "INVAL", -2: "NODEVICE", -3: "NOSPACE", -4: "NOMEM", -5: "HIP", -6: "RANGE", -7: "STATE"}


class BmqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmq error {STATUS.get(code, code)}: {msg}")
        self.code = code


def _b(s) -> bytes:
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def pack(strings: Sequence) -> Tuple[np.ndarray, np.ndarray]:
    """list of str/bytes -> (uint8 bytes padded by >= 16 zero bytes, uint32 offsets[n+1])"""
    bs = [_b(s) for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint32)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64).astype(np.uint32)
    raw = b"".join(bs)
    data = np.zeros(((len(raw) + 15) & ~15) + 16, dtype=np.uint8)
    if raw:
        data[:len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return data, off


def pinned(shape, dtype) -> np.ndarray:
    """numpy array over page-locked host memory from bmq_host_alloc (never freed explicitly here: benchmark / test helper)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = _lib.lib().bmq_host_alloc(max(n, 16))
    if not p:
        raise MemoryError("bmq_host_alloc")
    buf = (C.c_uint8 * max(n, 16)).from_address(p)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- codec (SCHEMA/KVSchemaUtil.java:91-130) -----------------------------------------------------------
def route_key(tenant, topic_filter, flag: int, receiver) -> bytes:
    t, f, r = _b(tenant), _b(topic_filter), _b(receiver)
    out = C.create_string_buffer(len(t) + len(f) + len(r) + 16)
    n = _lib.lib().bmq_route_key_encode(t, len(t), f, len(f), flag, r, len(r), out, len(out))
    return out.raw[:n]


def route_key_from_mqtt(tenant, mqtt_topic_filter: str, receiver_url: str = "") -> bytes:
    """TopicUtil.from + toNormalRouteKey / toGroupRouteKey (UTIL/TopicUtil.java:252-272)."""
    for prefix, flag in (("$share/", 2), ("$oshare/", 3)):
        if mqtt_topic_filter.startswith(prefix):
            rest = mqtt_topic_filter[len(prefix):]
            i = rest.index("/")
            return route_key(tenant, rest[i + 1:], flag, rest[:i])
    return route_key(tenant, mqtt_topic_filter, 1, receiver_url)


def decode_route_key(key: bytes):
    """-> (flag, tenant, mqttTopicFilter incl. $share prefix, receiver) or None (RouteDetailCache.java:53-109)."""
    spans = (C.c_uint32 * 6)()
    flag = _lib.lib().bmq_route_key_decode(key, len(key), spans)
    if flag < 0:
        return None
    tenant = key[spans[0]:spans[0] + spans[1]].decode()
    filt = key[spans[2]:spans[2] + spans[3]].replace(b"\0", b"/").decode()
    recv = key[spans[4]:spans[4] + spans[5]].decode()
    if flag == 2:
        filt = f"$share/{recv}/{filt}"
    elif flag == 3:
        filt = f"$oshare/{recv}/{filt}"
    return flag, tenant, filt, recv


def retain_message_key(tenant, topic) -> bytes:
    """KVSchemaUtil.retainMessageKey of the retain store schema"""
    t, p = _b(tenant), _b(topic)
    out = C.create_string_buffer(len(t) + 2 * len(p) + 16)
    n = _lib.lib().bmq_retain_message_key(t, len(t), p, len(p), out, len(out))
    return out.raw[:n]


def retain_filter_route(tenant, topic_filter):
    """-> (key or key prefix, LevelHash(filterPrefix), levels, has_wildcard, ends_with_hash): MatchCallRangeRouter's per-filter part"""
    t, f = _b(tenant), _b(topic_filter)
    out, hsh = C.create_string_buffer(len(t) + 2 * len(f) + 16), C.create_string_buffer(len(f) + 2)
    kl, hl, lv = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = _lib.lib().bmq_retain_filter_route(t, len(t), f, len(f), out, len(out), C.byref(kl), hsh, len(hsh), C.byref(hl), C.byref(lv))
    if rc < 0:
        raise BmqError(rc, "bmq_retain_filter_route")
    return out.raw[:kl.value], hsh.raw[:hl.value], lv.value, bool(rc & 1), bool(rc & 2)


class RangeRouter:
    """The client-side KV range router: boundaries (start | None, end | None) in BoundaryUtil.compare order
    (KVRangeRouterUtil.java:41-103); lookups return indices into that list."""

    def __init__(self, boundaries):
        self.n = len(boundaries)
        self.flags = np.array([(1 if s is not None else 0) | (2 if e is not None else 0) for s, e in boundaries], dtype=np.uint8)
        self.start, self.start_off = pack([s or b"" for s, _ in boundaries])
        self.end, self.end_off = pack([e or b"" for _, e in boundaries])

    def _args(self):
        return (_ptr(self.flags), _ptr(self.start), _ptr(self.start_off), _ptr(self.end), _ptr(self.end_off), self.n)

    def build(self):
        """bmq_router_create: copy, check and index the boundaries once; the lookups below then go through the object."""
        if getattr(self, "h", None) is None:
            h = C.c_void_p()
            rc = _lib.lib().bmq_router_create(*self._args(), C.byref(h))
            if rc < 0:
                raise BmqError(rc, "bmq_router_create")
            self.h = h
        return self

    def close(self):
        if getattr(self, "h", None) is not None:
            _lib.lib().bmq_router_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def find_by_key(self, key: bytes):
        out = C.c_int32()
        if getattr(self, "h", None) is not None:
            rc = _lib.lib().bmq_router_lookup_key(self.h, key, len(key), C.byref(out))
        else:
            rc = _lib.lib().bmq_router_find_by_key(*self._args(), key, len(key), C.byref(out))
        if rc < 0:
            raise BmqError(rc, "bmq_router_find_by_key")
        return None if out.value < 0 else out.value

    def find_by_boundary(self, start, end):
        first, count = C.c_uint32(), C.c_uint32()
        fl = (1 if start is not None else 0) | (2 if end is not None else 0)
        q = (fl, start or b"", len(start or b""), end or b"", len(end or b""), C.byref(first), C.byref(count))
        if getattr(self, "h", None) is not None:
            rc = _lib.lib().bmq_router_lookup_boundary(self.h, *q)
        else:
            rc = _lib.lib().bmq_router_find_by_boundary(*self._args(), *q)
        if rc < 0:
            raise BmqError(rc, "bmq_router_find_by_boundary")
        return list(range(first.value, first.value + count.value))

    def retain_range_lookup(self, tenant, topic_filters, exact: bool = False):
        """MatchCallRangeRouter.rangeLookup -> per filter the indices of the ranges it is sent to (exact: BMQ_ROUTER_EXACT)"""
        t = _b(tenant)
        fb, fo = pack(topic_filters)
        keep = np.zeros((len(topic_filters), self.n), dtype=np.uint8)
        if getattr(self, "h", None) is not None:
            rc = _lib.lib().bmq_router_retain_lookup(self.h, t, len(t), _ptr(fb), _ptr(fo), len(topic_filters), 1 if exact else 0, _ptr(keep))
        else:
            rc = _lib.lib().bmq_retain_range_lookup(t, len(t), _ptr(fb), _ptr(fo), len(topic_filters), *self._args(), 1 if exact else 0, _ptr(keep))
        if rc < 0:
            raise BmqError(rc, "bmq_retain_range_lookup")
        return [np.nonzero(keep[i])[0].tolist() for i in range(len(topic_filters))]


def java_string_hash(s) -> int:
    b = _b(s)
    return _lib.lib().bmq_java_string_hash(b, len(b))


PLAN_NONE, PLAN_ADD, PLAN_UPDATE, PLAN_REMOVE, PLAN_SUPERSEDED = range(5)  # BMQ_PLAN_* of include/bmq.h


class RetainPlan:
    """what bmq_retain_plan returns for a batch of n ops (Engine.retain_plan)"""

    def __init__(self, code, action, winner, topic_id, delta, key_off, key_bytes: bytes, info):
        self.code, self.action, self.winner, self.topic_id, self.delta = code, action, winner, topic_id, delta
        self.key_off, self.key_bytes, self.info = key_off, key_bytes, info

    @property
    def keys(self) -> List[bytes]:
        off = self.key_off.tolist()
        return [self.key_bytes[off[i]:off[i + 1]] for i in range(len(off) - 1)]


class Engine:
    """One engine per KV range replica (cf. DistWorkerCoProc's SubscriptionCache)."""

    def __init__(self, device: int = 0, wave_queue_cap: int = 0, wave_pair_cap: int = 0, slow_scratch_mb: int = 0, kernel_timing: bool = False,
                 dedup_min_topics: int = 0, dedup_sorted: bool = False, region_slack: int = 0,
                 tail_records: int = 0, child_filters: int = 0, retain_builder: int = 0, share_carry: int = 0):
        L = _lib.lib()
        cfg = _lib.Config()
        cfg.struct_size = C.sizeof(_lib.Config)
        cfg.device = device
        cfg.wave_queue_cap = wave_queue_cap
        cfg.wave_pair_cap = wave_pair_cap
        cfg.slow_scratch_mb = slow_scratch_mb
        cfg.kernel_timing = 1 if kernel_timing else 0
        cfg.dedup_min_topics = dedup_min_topics  # 0: default = never; n: batches of >= n topics are de-duplicated on the device first
        cfg.dedup_sorted = 1 if dedup_sorted else 0  # ... by comparing neighbours: the batches arrive ordered by (tenant index, topic)
        cfg.region_slack = region_slack  # 0: default (6: trie regions at load factor 0.2); 1: 0.4 (less memory, more second probes)
        cfg.tail_records = tail_records  # 0: default (tail records on); 1: off
        cfg.child_filters = child_filters  # 0: default (the walk reads the nodes' child filter words); 1: it ignores them
        cfg.retain_builder = retain_builder  # 0: default (the host builder bulk-loads the retained-topic index); 1: the executor builder; 3: it also serves retain_compact_begin / _build / _swap
        cfg.share_carry = share_carry  # 0: default (a generation change of the route index drops the member tables of shared subscriptions); 1: compact / compact_swap carry them to the ids their route keys get
        h = C.c_void_p()
        rc = L.bmq_engine_create(C.byref(cfg), C.byref(h))
        if rc:
            raise BmqError(rc, "bmq_engine_create failed (a gfx950 device is required for device >= 0)")
        self.h = h
        self.device = device
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().bmq_engine_destroy(self.h)
            self.h = None
            for arena in getattr(self, "_apply_arenas", ()) if self.device >= 0 else ():  # (apply_async's page-locked buffers: nothing reads them any more)
                for a in arena or ():
                    _lib.lib().bmq_host_free(C.c_void_p(a.ctypes.data))
            self._apply_arenas = [None, None]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())

    # ---- index ---------------------------------------------------------------------------------------
    def rebuild(self, keys: Iterable[bytes] = (), packed: Optional[Tuple[np.ndarray, np.ndarray]] = None):
        data, off = pack(list(keys)) if packed is None else packed
        self._check(_lib.lib().bmq_rebuild(self.h, _ptr(data), _ptr(off), len(off) - 1))
        return self

    def rebuild_raw(self, key_bytes_ptr: int, key_off_ptr: int, n: int):
        self._check(_lib.lib().bmq_rebuild(self.h, key_bytes_ptr, key_off_ptr, n))
        return self

    def apply(self, ops: Sequence[Tuple[int, bytes]]):
        """ops: (0 = put | 1 = delete, route key)"""
        data, off = pack([k for _, k in ops])
        op = np.array([o for o, _ in ops], dtype=np.uint8)
        self._check(_lib.lib().bmq_routes_apply(self.h, _ptr(data), _ptr(off), _ptr(op), len(ops)))
        return self

    def apply_async(self, ops: Sequence[Tuple[int, bytes]]):
        """bmq_routes_apply_async: the batch is uploaded and queued behind whatever the engine stream holds, the call returns at once; its
        outcome is apply_wait()'s (or the next index call's).  The op buffers are kept in page-locked memory owned by this object until then."""
        data, off = pack([k for _, k in ops])
        op = np.array([o for o, _ in ops], dtype=np.uint8)
        # Two page-locked arenas taken in turns, grow-only (a fresh set per call was never freed).  The engine reads batch k's
        # buffers until batch k is completed -- by bmq_routes_apply_wait or inside the NEXT bmq_routes_apply_async --, so call k + 1 must not
        # touch arena k: it takes the other one, whose batch k - 1 was completed during call k.
        if not hasattr(self, "_apply_arenas"):
            self._apply_arenas, self._apply_turn = [None, None], 0
        self._apply_turn ^= 1
        need = (len(data), len(off) * 4, max(len(op), 1))
        arena = self._apply_arenas[self._apply_turn]
        if arena is None or any(a.nbytes < n for a, n in zip(arena, need)):
            if arena is not None:
                for a in arena:
                    _lib.lib().bmq_host_free(C.c_void_p(a.ctypes.data))
            # (a host-only engine has no page-locked allocator -- and nothing to upload: ordinary memory, kept alive the same way)
            arena = tuple((pinned if self.device >= 0 else np.empty)(max(2 * n, 4096), np.uint8) for n in need)
            self._apply_arenas[self._apply_turn] = arena
        b_data, b_off, b_op = arena[0][:len(data)], arena[1][:len(off) * 4].view(np.uint32), arena[2][:max(len(op), 1)]
        b_data[:], b_off[:], b_op[:len(op)] = data, off, op
        self._check(_lib.lib().bmq_routes_apply_async(self.h, _ptr(b_data), _ptr(b_off), _ptr(b_op), len(ops)))
        return self

    def apply_wait(self):
        """bmq_routes_apply_wait: the outcome of the batch handed over with apply_async (raises what apply would have raised)"""
        self._check(_lib.lib().bmq_routes_apply_wait(self.h))
        return self

    POLLER_DISABLE, POLLER_ENABLE, POLLER_STOP, POLLER_TEST_IGNORE_DOORBELLS = 0, 1, 2, 3

    def poller_stats(self) -> _lib.PollerStats:
        """bmq_poller_stats_get: the persistent matcher behind the batching front (k_poll)"""
        out = _lib.PollerStats()
        self._check(_lib.lib().bmq_poller_stats_get(self.h, C.byref(out)))
        return out

    def poller_control(self, what: int):
        self._check(_lib.lib().bmq_poller_control(self.h, what))
        return self

    def compact(self):
        """bmq_compact: re-build from the live routes (ids become ranks again, new generation)."""
        self._check(_lib.lib().bmq_compact(self.h))
        return self

    @staticmethod
    def _boundary(start, end):
        """(flags, start, len, end, len) of a KV boundary: None = the side is absent, b"" = present and empty"""
        flags = (1 if start is not None else 0) | (2 if end is not None else 0)
        s, e = (b"" if start is None else bytes(start)), (b"" if end is None else bytes(end))
        return flags, s, len(s), e, len(e)

    def compact_begin(self, start=None, end=None):
        """bmq_compact_begin[_in]: the next generation of the route index starts being built beside the serving one; with a boundary it
        takes the keys with start <= key < end only (the range that shrinks in a split)"""
        if start is None and end is None:
            self._check(_lib.lib().bmq_compact_begin(self.h))
        else:
            self._check(_lib.lib().bmq_compact_begin_in(self.h, *self._boundary(start, end)))
        return self

    def count_in(self, start=None, end=None) -> Tuple[int, int]:
        """bmq_routes_count_in: (live routes inside the boundary, the sum of their key lengths); the index is not changed"""
        routes, key_bytes = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_routes_count_in(self.h, *self._boundary(start, end), C.byref(routes), C.byref(key_bytes)))
        return int(routes.value), int(key_bytes.value)

    def _named_numbers(self, call, width: int, tenants_cap: int = 4096, cap: int = 256):
        """the buffer protocol of bmq_routes_tenant_stats / bmq_retain_tenant_counts: caps in, needed sizes out, -3 when a cap is too small"""
        n, nb = C.c_uint32(), C.c_uint64()
        while True:
            names, off, nums = np.zeros(max(tenants_cap, 1), dtype=np.uint8), np.zeros(cap + 1, dtype=np.uint64), np.zeros(max(width * cap, 1), dtype=np.uint64)
            rc = call(_ptr(names), tenants_cap, _ptr(off), _ptr(nums), cap, C.byref(n), C.byref(nb))
            if rc == -3:
                cap, tenants_cap = max(cap, int(n.value)), max(tenants_cap, int(nb.value))
                continue
            self._check(rc)
            raw = names.tobytes()
            return [(raw[int(off[i]):int(off[i + 1])],) + tuple(int(v) for v in nums[width * i:width * (i + 1)]) for i in range(n.value)]

    def routes_tenant_stats(self, start=None, end=None, tenants_cap: int = 4096, cap: int = 256) -> List[Tuple[bytes, int, int, int, int]]:
        """bmq_routes_tenant_stats: [(tenant id bytes, normal, unordered share, ordered share, key_bytes)] of every tenant with a live route
        inside the boundary, in byte order of the ids; the index is not changed"""
        b = self._boundary(start, end)
        return self._named_numbers(lambda *a: _lib.lib().bmq_routes_tenant_stats(self.h, *b, *a), 4, tenants_cap, cap)

    def import_routes(self, src: "Engine", start=None, end=None) -> Tuple[int, int]:
        """bmq_routes_import: every live key of src inside the boundary is put into this engine, without a KV scan -> (imported, dups)"""
        imported, dups = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_routes_import(self.h, src.h, *self._boundary(start, end), C.byref(imported), C.byref(dups)))
        return int(imported.value), int(dups.value)

    def compact_poll(self, max_ids: int = 8192) -> int:
        """bmq_compact_poll: hands the next max_ids route ids' live keys to the builder -> progress in permille (1000: ready to swap)"""
        done = C.c_uint32()
        self._check(_lib.lib().bmq_compact_poll(self.h, max_ids, C.byref(done)))
        return int(done.value)

    def compact_swap(self) -> Tuple[int, int]:
        """bmq_compact_swap: replays what was mutated meanwhile, swaps the generations -> (keys carried over, ops replayed)"""
        carried, replayed = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_compact_swap(self.h, C.byref(carried), C.byref(replayed)))
        return int(carried.value), int(replayed.value)

    def compact_abort(self):
        self._check(_lib.lib().bmq_compact_abort(self.h))
        return self

    def info(self) -> _lib.IndexInfo:
        out = _lib.IndexInfo()
        self._check(_lib.lib().bmq_index_info_get(self.h, C.byref(out)))
        return out

    def route_key(self, route_id: int) -> bytes:
        n = C.c_uint32()
        buf = C.create_string_buffer(512)
        rc = _lib.lib().bmq_route_key(self.h, route_id, buf, len(buf), C.byref(n))
        while rc == -3:  # BMQ_E_NOSPACE: n holds the length (ids may move under concurrent apply: retry)
            buf = C.create_string_buffer(max(n.value, 2 * len(buf)))
            rc = _lib.lib().bmq_route_key(self.h, route_id, buf, len(buf), C.byref(n))
        self._check(rc)
        return buf.raw[:n.value]

    def route_keys(self, route_ids) -> List[bytes]:
        """bmq_route_keys: one device gather for many ids; a dead id gives b""."""
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        n = len(ids)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = max(4096, 96 * n)
        while True:
            out = np.zeros(cap, dtype=np.uint8)
            rc = _lib.lib().bmq_route_keys(self.h, _ptr(ids), n, _ptr(out), cap, _ptr(off))
            if rc == -3:
                cap = int(off[n])
                continue
            self._check(rc)
            raw = out.tobytes()
            return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    def find_routes(self, keys: Sequence[bytes] = (), packed: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> np.ndarray:
        """bmq_routes_find: the id of the live route with each key (0xFFFFFFFF: there is none), looked up where the index lives; read-only.
        A malformed key raises BmqError(-1)."""
        data, off = pack(list(keys)) if packed is None else packed
        n = len(off) - 1
        out = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        self._check(_lib.lib().bmq_routes_find(self.h, _ptr(data), _ptr(off), n, _ptr(out)))
        return out

    def window(self, start=None, n: int = BMQ_WINDOW_MAX, exclusive: bool = False) -> Tuple[np.ndarray, bool]:
        """bmq_routes_window: (the ids of the first n live routes whose key is >= start -- > start if exclusive, all without a start --
        in KV order, whether a further live key follows); ordered on the device, read-only.  n <= BMQ_WINDOW_MAX."""
        lo = None if start is None else _b(start)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        got, more = C.c_uint32(), C.c_uint32()
        self._check(_lib.lib().bmq_routes_window(self.h, lo, 0 if lo is None else len(lo), 1 if exclusive else 0, n, _ptr(out), C.byref(got), C.byref(more)))
        return out[:got.value], bool(more.value)

    def gc_sweep(self, start_key=None, step_hint: int = 1, scan_quota: int = 0, boundary=None) -> Tuple[np.ndarray, bool, Optional[bytes]]:
        """bmq_routes_gc_sweep, the loop of DistWorkerCoProc.gc (DW/DistWorkerCoProc.java:554-701): (the inspected route ids in inspection
        order, wrapped, nextStartKey or None).  boundary = (start, end), either may be None: the clamp of :563-574 -- a cursor below the
        start or at / beyond the end becomes the start (the engine holds exactly its range's keys and takes no boundary itself)."""
        lo = None if start_key is None else _b(start_key)
        if lo is not None and boundary is not None:
            b0, b1 = (None if x is None else _b(x) for x in boundary)
            if (b0 is not None and lo < b0) or (b1 is not None and lo >= b1):
                lo = b0
        step = max(int(step_hint), 1)
        cap = scan_quota if scan_quota > 0 else 256 * step
        rep = _lib.GcSweepReply()
        while True:
            out = np.zeros(max(cap, 1), dtype=np.uint32)
            rc = _lib.lib().bmq_routes_gc_sweep(self.h, lo, 0 if lo is None else len(lo), step_hint, scan_quota, _ptr(out), cap, C.byref(rep))
            if rc == -3 and rep.inspected > cap:
                cap = int(rep.inspected)
                continue
            self._check(rc)
            return out[:rep.inspected], bool(rep.wrapped), (self.route_key(rep.next_route_id) if rep.has_next else None)

    def window_info(self) -> _lib.WindowInfo:
        """bmq_routes_window_info_get: cumulative counters of this engine's windows (those of sweeps included)"""
        out = _lib.WindowInfo()
        self._check(_lib.lib().bmq_routes_window_info_get(self.h, C.byref(out)))
        return out

    def split_key_after(self, prefix, split_at_scale: int) -> Optional[bytes]:
        """FanoutSplitHinter.doEstimate's seek-and-advance (DW/hinter/FanoutSplitHinter.java:187-198) as one window: the key at index
        split_at_scale among the live keys >= prefix (not bounded by the prefix), None if there are not that many."""
        if split_at_scale < 0 or split_at_scale >= BMQ_WINDOW_MAX:
            raise ValueError("split_at_scale must lie in [0, BMQ_WINDOW_MAX)")
        ids, _ = self.window(prefix, split_at_scale + 1)
        return self.route_key(int(ids[split_at_scale])) if len(ids) > split_at_scale else None

    def prefix_census(self, prefixes: Sequence[bytes] = (), packed: Optional[Tuple[np.ndarray, np.ndarray]] = None) -> np.ndarray:
        """bmq_routes_prefix_census: uint64 array (n, 4) -- per byte prefix the live keys that start with it with flag 1 / 2 / 3 and the sum
        of their key lengths (the columns of routes_tenant_stats), all prefixes in one pass over the key store; read-only.  Any order,
        repeats and nesting allowed; n <= BMQ_PREFIX_MAX."""
        data, off = pack(list(prefixes)) if packed is None else packed
        n = len(off) - 1
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        self._check(_lib.lib().bmq_routes_prefix_census(self.h, _ptr(data), _ptr(off), n, _ptr(out)))
        return out[:n]

    def prefix_census_info(self) -> _lib.PrefixCensusInfo:
        """bmq_routes_prefix_census_info_get: cumulative counters of this engine's prefix censuses"""
        out = _lib.PrefixCensusInfo()
        self._check(_lib.lib().bmq_routes_prefix_census_info_get(self.h, C.byref(out)))
        return out

    def find(self, tenant, topic_filter) -> List[int]:
        t, f = _b(tenant), _b(topic_filter)
        n = C.c_uint32()
        cap = 1024
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            self._check(_lib.lib().bmq_index_find(self.h, t, len(t), f, len(f), _ptr(out), cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value].tolist()
            cap = n.value

    # ---- match (host buffers) ---------------------------------------------------------------------------
    def match_batch(self, tenants: Sequence, topic_tenant, topics: Sequence = (), packed_topics=None):
        """-> (row_ptr[n+1], route_ids) numpy arrays; ids ascending per row."""
        tdata, toff = pack(tenants)
        pdata, poff = pack(topics) if packed_topics is None else packed_topics
        n = len(poff) - 1
        tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        assert tt.shape == (n,)
        row = np.zeros(n + 1, dtype=np.uint32)
        cap = max(1024, 8 * n)
        need = C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_match_batch(self.h, _ptr(tdata), _ptr(toff), len(toff) - 1, _ptr(tt), _ptr(pdata),
                                            _ptr(poff), n, _ptr(row), _ptr(ids), cap, C.byref(need))
            if rc == -3 and need.value > cap:
                cap = need.value
                continue
            self._check(rc)
            return row, ids[:need.value]

    # ---- asynchronous host-buffer match: up to three batches in flight (bmq_match_submit / bmq_match_wait) ------------------------
    def match_submit(self, tdata, toff, n_tenants, tt, pdata, poff, n_topics) -> int:
        """numpy arrays (ideally views of bmq_host_alloc memory, see pinned()); they must stay alive until match_wait."""
        k = C.c_int()
        self._check(_lib.lib().bmq_match_submit(self.h, _ptr(tdata), _ptr(toff), n_tenants, _ptr(tt), _ptr(pdata), _ptr(poff), n_topics,
                                                C.byref(k)))
        return k.value

    def match_wait(self, ticket: int, row: np.ndarray, ids: np.ndarray) -> int:
        """-> number of ids written (BmqError code -3 with .needed set if ids is too small)"""
        need = C.c_uint64()
        rc = _lib.lib().bmq_match_wait(self.h, ticket, _ptr(row), _ptr(ids), len(ids), C.byref(need))
        if rc:
            err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
            err.needed = need.value
            raise err
        return need.value

    # ---- result formats that fit the wire (include/bmq.h: BMQ_FMT_*) ------------------------------------------------------------
    FMT_IDS, FMT_COUNTS, FMT_RANGES, FMT_GROUPED, FMT_DELIVERY = 0, 1, 2, 3, 4
    RANGE_SIDE = 0x80000000

    def match_submit_fmt(self, tdata, toff, n_tenants, tt, pdata, poff, n_topics, fmt: int) -> int:
        k = C.c_int()
        self._check(_lib.lib().bmq_match_submit_fmt(self.h, _ptr(tdata), _ptr(toff), n_tenants, _ptr(tt), _ptr(pdata), _ptr(poff), n_topics, fmt,
                                                    C.byref(k)))
        return k.value

    def match_wait_counts(self, ticket: int, row: np.ndarray) -> int:
        """row[n + 1] <- the id row pointers (fan-out of topic i = row[i + 1] - row[i]); -> total ids"""
        tot = C.c_uint64()
        self._check(_lib.lib().bmq_match_wait_counts(self.h, ticket, _ptr(row), C.byref(tot)))
        return tot.value

    def match_wait_ranges(self, ticket: int, range_ptr: np.ndarray, ranges: np.ndarray, side: np.ndarray, row: Optional[np.ndarray] = None):
        """ranges: uint32 [cap, 2] (begin, count); side: uint32 [cap]; -> RangesInfo (BmqError -3 carries .info with the sizes)"""
        info = _lib.RangesInfo()
        rc = _lib.lib().bmq_match_wait_ranges(self.h, ticket, _ptr(row) if row is not None else None, _ptr(range_ptr), _ptr(ranges), len(ranges),
                                              _ptr(side), len(side), C.byref(info))
        if rc:
            err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
            err.info = info
            raise err
        return info

    def match_wait_grouped(self, ticket: int, out_topic: np.ndarray, out_route: np.ndarray, group_off: np.ndarray, group_rep: np.ndarray):
        """-> (total pairs, n_groups, special)"""
        ng, sp, tot = C.c_uint32(), C.c_uint32(), C.c_uint64()
        rc = _lib.lib().bmq_match_wait_grouped(self.h, ticket, _ptr(out_topic), _ptr(out_route), len(out_topic), _ptr(group_off), _ptr(group_rep),
                                               len(group_rep), C.byref(ng), C.byref(sp), C.byref(tot))
        if rc:
            err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
            err.needed = tot.value
            raise err
        return tot.value, ng.value, sp.value

    @staticmethod
    def expand_ranges(range_ptr: np.ndarray, ranges: np.ndarray, side: np.ndarray, n: int) -> List[np.ndarray]:
        """What a consumer of BMQ_FMT_RANGES does: the id row of every topic (ordered where ranges overlap)."""
        out = []
        for i in range(n):
            parts, last, overlap = [], -1, False
            for b, c in ranges[range_ptr[i]:range_ptr[i + 1]]:
                b, c = int(b), int(c)
                ids = side[b:b + (c & 0x7FFFFFFF)] if c & 0x80000000 else np.arange(b, b + c, dtype=np.uint32)
                if len(ids) == 0:
                    continue
                overlap |= int(ids[0]) <= last
                last = int(ids[-1])
                parts.append(ids)
            row = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
            out.append(np.sort(row) if overlap else row)
        return out

    def batcher(self, max_batch_topics: int = 0) -> "Batcher":
        """The batching front of SURVEY.md 8f-1 over this engine (close it before the engine)."""
        return Batcher(self, max_batch_topics)

    def match_tenant(self, tenant, topics: Sequence) -> List[List[int]]:
        row, ids = self.match_batch([tenant], np.zeros(len(topics), dtype=np.uint32), topics)
        return [ids[row[i]:row[i + 1]].tolist() for i in range(len(topics))]

    def match_all(self, tenant, topics: Sequence, max_persistent_fanout: int = INT_MAX,
                  max_group_fanout: int = INT_MAX):
        """ITenantRouteMatcher.matchAll for one tenant incl. MatchedRoutes fan-out caps.
        -> (per-topic id lists, events [(type, topic idx, route id, max)])"""
        t = _b(tenant)
        pdata, poff = pack(topics)
        n = len(topics)
        row = np.zeros(n + 1, dtype=np.uint32)
        cap = max(1024, 8 * n)
        need = C.c_uint64()
        ev_cap = 4096
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            ev = np.zeros(4 * ev_cap, dtype=np.int32)
            nev = C.c_uint32()
            rc = _lib.lib().bmq_match_all(self.h, t, len(t), _ptr(pdata), _ptr(poff), n, max_persistent_fanout,
                                          max_group_fanout, _ptr(row), _ptr(ids), cap, C.byref(need), _ptr(ev), ev_cap,
                                          C.byref(nev))
            if rc == -3 and need.value > cap:
                cap = need.value
                continue
            self._check(rc)
            if nev.value > ev_cap:
                ev_cap = nev.value
                continue
            events = [tuple(int(x) for x in ev[4 * i:4 * i + 4]) for i in range(nev.value)]
            return [ids[row[i]:row[i + 1]].tolist() for i in range(n)], events

    def routes_cap(self, row_ptr, route_ids, max_persistent_fanout: int, max_group_fanout: int):
        """bmq_routes_cap: MatchedRoutes' caps over rows already matched
        -> (per-row id lists, per-row (persistent, group) counts, events [(type, row, route id, max)])"""
        row = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        n = len(row) - 1
        o_row, o_ids = np.zeros(n + 1, dtype=np.uint32), np.zeros(max(1, len(ids)), dtype=np.uint32)
        cls = np.zeros(2 * max(n, 1), dtype=np.uint32)
        ev = np.zeros(4 * max(1, len(ids)), dtype=np.int32)
        nev = C.c_uint32()
        self._check(_lib.lib().bmq_routes_cap(self.h, _ptr(row), _ptr(ids), n, max_persistent_fanout, max_group_fanout, _ptr(o_row), _ptr(o_ids),
                                              _ptr(cls), _ptr(ev), len(ids), C.byref(nev)))
        return ([o_ids[o_row[i]:o_row[i + 1]].tolist() for i in range(n)], [(int(cls[2 * i]), int(cls[2 * i + 1])) for i in range(n)],
                [tuple(int(x) for x in ev[4 * i:4 * i + 4]) for i in range(nev.value)])

    # ---- match (device-resident; torch tensors are only carriers of device pointers) ----------------------
    def match_batch_device(self, d_tenants, d_tenant_off, n_tenants, d_topic_tenant, d_topics, d_topic_off, n_topics,
                           d_row_ptr, d_ids, capacity, d_total):
        """All d_* are device pointers (ints).  Asynchronous; call finish()."""
        self._check(_lib.lib().bmq_match_batch_dev(self.h, d_tenants, d_tenant_off, n_tenants, d_topic_tenant, d_topics,
                                                   d_topic_off, n_topics, d_row_ptr, d_ids, capacity, d_total))

    # ---- fan-out grouping --------------------------------------------------------------------------------
    def fanout_group(self, row_ptr, route_ids, group_cap: int = 256):
        """Segmented sort of a match CSR by DelivererKey -> (out_topic, out_route, group_off, group_rep, special)."""
        row = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        n, total = len(row) - 1, int(row[-1])
        ot, orr = np.zeros(max(total, 1), dtype=np.uint32), np.zeros(max(total, 1), dtype=np.uint32)
        ng, sp = C.c_uint32(), C.c_uint32()
        while True:
            goff, grep = np.zeros(group_cap + 1, dtype=np.uint32), np.zeros(max(group_cap, 1), dtype=np.uint32)
            rc = _lib.lib().bmq_fanout_group(self.h, _ptr(row), _ptr(ids), n, _ptr(ot), _ptr(orr), total, _ptr(goff), _ptr(grep), group_cap,
                                             C.byref(ng), C.byref(sp))
            if rc == -3 and ng.value > group_cap:
                group_cap = ng.value
                continue
            self._check(rc)
            return ot[:total], orr[:total], goff[:ng.value + 1], grep[:ng.value], sp.value

    def fanout_group_device(self, d_row_ptr, d_ids, n_topics, total, d_out_topic, d_out_route, d_group_off, d_group_rep, group_cap):
        """All d_* are device pointers (ints).  -> (n_groups, special); BmqError -3 (.needed = groups) if group_cap is too small."""
        ng, sp = C.c_uint32(), C.c_uint32()
        rc = _lib.lib().bmq_fanout_group_dev(self.h, d_row_ptr, d_ids, n_topics, total, d_out_topic, d_out_route, d_group_off, d_group_rep,
                                             group_cap, C.byref(ng), C.byref(sp))
        if rc:
            err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
            err.needed = ng.value
            raise err
        return ng.value, sp.value

    def fanout_info(self) -> _lib.FanoutInfo:
        """bmq_fanout_info_get: which path answered the groupings of this generation, and the state of the group table"""
        out = _lib.FanoutInfo()
        self._check(_lib.lib().bmq_fanout_info_get(self.h, C.byref(out)))
        return out

    # ---- receivers of shared subscriptions (DeliverExecutorGroup.send(GroupMatching, ...)) --------------------------------------------
    def share_members_apply(self, tables):
        """bmq_share_members_apply.  tables: {route id: [receiverUrl, ...]} (or a sequence of such pairs); the list order is the
        reference's receiverList order, an empty list removes the route's table."""
        items = list(tables.items()) if hasattr(tables, "items") else list(tables)
        ids = np.array([i for i, _ in items], dtype=np.uint32)
        moff = np.zeros(len(items) + 1, dtype=np.uint32)
        moff[1:] = np.cumsum([len(m) for _, m in items])
        data, off = pack([_b(u) for _, m in items for u in m])
        self._check(_lib.lib().bmq_share_members_apply(self.h, _ptr(ids), len(items), _ptr(moff), _ptr(data), _ptr(off)))
        return self

    def share_resolve(self, pair_topic, pair_route, sender_off, sender_hash, nonce: int, row_cap: Optional[int] = None, group_cap: int = 256):
        """bmq_share_resolve -> (out_pair, out_sender, out_member, group_off, special): delivery rows ordered by (share-deliverer number,
        pair, sender); group g owns rows group_off[g] .. group_off[g + 1]; special bit 0: the last group holds the unresolved rows."""
        pt = np.ascontiguousarray(pair_topic, dtype=np.uint32)
        pr = np.ascontiguousarray(pair_route, dtype=np.uint32)
        so = np.ascontiguousarray(sender_off, dtype=np.uint32)
        sh = np.ascontiguousarray(sender_hash, dtype=np.int32)
        if row_cap is None:
            row_cap = max(len(pt), 1)
        nr, ng, sp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        while True:
            op, os_, om = (np.zeros(max(row_cap, 1), dtype=np.uint32) for _ in range(3))
            goff = np.zeros(group_cap + 1, dtype=np.uint32)
            rc = _lib.lib().bmq_share_resolve(self.h, _ptr(pt), _ptr(pr), len(pt), _ptr(so), _ptr(sh), len(so) - 1, nonce & 0xFFFFFFFFFFFFFFFF,
                                              _ptr(op), _ptr(os_), _ptr(om), row_cap, _ptr(goff), group_cap, C.byref(nr), C.byref(ng), C.byref(sp))
            if rc == -3 and (nr.value > row_cap or ng.value > group_cap):
                row_cap, group_cap = max(row_cap, nr.value), max(group_cap, ng.value)
                continue
            self._check(rc)
            return op[:nr.value], os_[:nr.value], om[:nr.value], goff[:ng.value + 1], sp.value

    def share_resolve_device(self, d_pair_topic, d_pair_route, n_pairs, d_sender_off, d_sender_hash, n_topics, n_senders, nonce: int,
                             d_out_pair, d_out_sender, d_out_member, row_cap, d_group_off, group_cap):
        """All d_* are device pointers (ints).  -> (n_rows, n_groups, special); BmqError -3 (.needed = (rows, groups)) if a capacity is too small."""
        nr, ng, sp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = _lib.lib().bmq_share_resolve_dev(self.h, d_pair_topic, d_pair_route, n_pairs, d_sender_off, d_sender_hash, n_topics, n_senders,
                                              nonce & 0xFFFFFFFFFFFFFFFF, d_out_pair, d_out_sender, d_out_member, row_cap, d_group_off, group_cap,
                                              C.byref(nr), C.byref(ng), C.byref(sp))
        if rc:
            err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
            err.needed = (nr.value, ng.value)
            raise err
        return nr.value, ng.value, sp.value

    def share_member(self, route_id: int, index: int) -> bytes:
        """bmq_share_member: receiverUrl of member `index` of the route's table"""
        n = C.c_uint32()
        buf = C.create_string_buffer(512)
        rc = _lib.lib().bmq_share_member(self.h, int(route_id), int(index), buf, len(buf), C.byref(n))
        if rc == -3:
            buf = C.create_string_buffer(n.value)
            rc = _lib.lib().bmq_share_member(self.h, int(route_id), int(index), buf, len(buf), C.byref(n))
        self._check(rc)
        return buf.raw[:n.value]

    def share_info(self) -> _lib.ShareInfo:
        out = _lib.ShareInfo()
        self._check(_lib.lib().bmq_share_info_get(self.h, C.byref(out)))
        return out

    def share_carry_info(self) -> _lib.ShareCarryInfo:
        """bmq_share_carry_info_get: what the last generation change that ran with share_carry = 1 did with the member tables"""
        out = _lib.ShareCarryInfo()
        self._check(_lib.lib().bmq_share_carry_info_get(self.h, C.byref(out)))
        return out

    # ---- the delivery plan of a match batch (DeliverExecutorGroup.submit: one set of calls per DelivererKey) --------------------------
    def _delivery_error(self, rc: int, info: "_lib.DeliveryInfo") -> BmqError:
        err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
        err.info = info
        err.needed = (info.n_rows, info.n_share_rows, info.n_groups)
        return err

    def delivery_plan(self, row_ptr, route_ids, sender_off, sender_hash, nonce: int, row_cap: Optional[int] = None, share_cap: int = 256,
                      group_cap: int = 256, retry: bool = True):
        """bmq_delivery_plan -> (topic, route, aux, share_sender, share_member, group_off, info): the delivery rows of a match CSR grouped by
        DelivererKey, shared subscriptions resolved and merged in; group g owns rows group_off[g] .. group_off[g + 1], ordered by
        (topic, route, sender); aux == 0xFFFFFFFF: the route itself receives, else it indexes (share_sender, share_member).  A capacity that
        is too small is retried once with the sizes the call reports (retry=False: BmqError -3, .needed = (rows, share rows, groups))."""
        row = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        so = np.ascontiguousarray(sender_off, dtype=np.uint32)
        sh = np.ascontiguousarray(sender_hash, dtype=np.int32)
        if row_cap is None:
            row_cap = max(int(row[-1]), 1)
        info = _lib.DeliveryInfo()
        for attempt in range(2):
            ot, orr, oa = (np.zeros(max(row_cap, 1), dtype=np.uint32) for _ in range(3))
            ss, sm = (np.zeros(max(share_cap, 1), dtype=np.uint32) for _ in range(2))
            goff = np.zeros(group_cap + 1, dtype=np.uint32)
            rc = _lib.lib().bmq_delivery_plan(self.h, _ptr(row), _ptr(ids), len(row) - 1, _ptr(so), _ptr(sh), nonce & 0xFFFFFFFFFFFFFFFF, _ptr(ot), _ptr(orr),
                                              _ptr(oa), row_cap, _ptr(ss), _ptr(sm), share_cap, _ptr(goff), group_cap, C.byref(info))
            if rc == -3 and retry and attempt == 0:
                row_cap, share_cap, group_cap = max(row_cap, info.n_rows), max(share_cap, info.n_share_rows), max(group_cap, info.n_groups)
                continue
            if rc:
                raise self._delivery_error(rc, info)
            return ot[:info.n_rows], orr[:info.n_rows], oa[:info.n_rows], ss[:info.n_share_rows], sm[:info.n_share_rows], goff[:info.n_groups + 1], info

    def delivery_plan_device(self, d_row_ptr, d_ids, n_topics, total, d_sender_off, d_sender_hash, n_senders, nonce: int, d_out_topic, d_out_route,
                             d_out_aux, row_cap, d_out_share_sender, d_out_share_member, share_cap, d_group_off, group_cap) -> "_lib.DeliveryInfo":
        """All d_* are device pointers (ints).  -> DeliveryInfo; BmqError -3 (.needed = (rows, share rows, groups)) if a capacity is too small."""
        info = _lib.DeliveryInfo()
        rc = _lib.lib().bmq_delivery_plan_dev(self.h, d_row_ptr, d_ids, n_topics, total, d_sender_off, d_sender_hash, n_senders, nonce & 0xFFFFFFFFFFFFFFFF,
                                              d_out_topic, d_out_route, d_out_aux, row_cap, d_out_share_sender, d_out_share_member, share_cap, d_group_off,
                                              group_cap, C.byref(info))
        if rc:
            raise self._delivery_error(rc, info)
        return info

    def match_wait_delivery(self, ticket: int, sender_off, sender_hash, nonce: int, out_topic: np.ndarray, out_route: np.ndarray, out_aux: np.ndarray,
                            share_sender: np.ndarray, share_member: np.ndarray, group_off: np.ndarray):
        """The wait of a FMT_DELIVERY ticket -> (total ids of the CSR, DeliveryInfo); the capacities are the lengths of the arrays
        (group_off: groups + 1).  BmqError -3 carries .needed = (rows, share rows, groups) and the ticket is released."""
        so = np.ascontiguousarray(sender_off, dtype=np.uint32)
        sh = np.ascontiguousarray(sender_hash, dtype=np.int32)
        info, tot = _lib.DeliveryInfo(), C.c_uint64()
        rc = _lib.lib().bmq_delivery_wait(self.h, ticket, _ptr(so), _ptr(sh), nonce & 0xFFFFFFFFFFFFFFFF, _ptr(out_topic), _ptr(out_route), _ptr(out_aux),
                                                min(len(out_topic), len(out_route), len(out_aux)), _ptr(share_sender), _ptr(share_member),
                                                min(len(share_sender), len(share_member)), _ptr(group_off), len(group_off) - 1, C.byref(info), C.byref(tot))
        if rc:
            raise self._delivery_error(rc, info)
        return tot.value, info

    # ---- the fan-out caps of MatchedRoutes over a whole match batch (DW/cache/MatchedRoutes.java:87-141) ------------------------------
    @staticmethod
    def _caps_table(caps):
        """(pf, gf) or [(pf, gf), ...] -> (max_pf, max_gf) int32 arrays; what does not fit an int32 is the caller's error"""
        t = np.asarray(caps, dtype=np.int64).reshape(-1, 2)
        if t.size and (t.max() > 0x7FFFFFFF or t.min() < -0x80000000):
            raise ValueError("a fan-out cap outside int32")
        return np.ascontiguousarray(t[:, 0], dtype=np.int32), np.ascontiguousarray(t[:, 1], dtype=np.int32)

    def _caps_error(self, rc: int, info: "_lib.CapsInfo", n_events: int) -> BmqError:
        err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
        err.info = info
        err.n_events = n_events
        return err

    def routes_cap_batch(self, row_ptr, route_ids, caps, row_caps=None, events_cap: Optional[int] = None, out_cap: Optional[int] = None):
        """bmq_routes_cap_batch: MatchedRoutes' caps over a match CSR, every row under the table entry row_caps names (None: entry 0);
        caps = (pf, gf) or a list of such pairs -> (row_ptr, ids, class_counts [n_rows, 2], events [n, 4] int32, info).  events holds at most
        events_cap events (default: every one), info.n_events counts all."""
        row = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        pf, gf = self._caps_table(caps)
        rc_arr = None if row_caps is None else np.ascontiguousarray(row_caps, dtype=np.uint32)
        n = len(row) - 1
        if rc_arr is not None and len(rc_arr) != n:
            raise ValueError("row_caps: one entry per row")
        if events_cap is None:
            events_cap = len(ids)
        if out_cap is None:
            out_cap = len(ids)
        o_row, o_ids = np.zeros(n + 1, dtype=np.uint32), np.zeros(max(1, out_cap), dtype=np.uint32)
        cls, ev = np.zeros((max(n, 1), 2), dtype=np.uint32), np.zeros((max(1, events_cap), 4), dtype=np.int32)
        nev, info = C.c_uint32(), _lib.CapsInfo()
        rc = _lib.lib().bmq_routes_cap_batch(self.h, _ptr(row), _ptr(ids), n, _ptr(rc_arr), _ptr(pf), _ptr(gf), len(pf), _ptr(o_row), _ptr(o_ids), out_cap,
                                             _ptr(cls), _ptr(ev), events_cap, C.byref(nev), C.byref(info))
        if rc:
            raise self._caps_error(rc, info, nev.value)
        return o_row, o_ids[:info.n_kept], cls[:n], ev[:min(nev.value, events_cap)], info

    def routes_cap_device(self, d_row_ptr, d_ids, n_rows, total, d_row_caps, d_max_pf, d_max_gf, n_caps, d_out_row_ptr, d_out_ids, out_cap, d_out_class_counts,
                          d_out_events, events_cap):
        """bmq_routes_cap_dev: all d_* are device pointers (ints; d_row_caps, d_out_class_counts, d_out_events may be None) -> (n_events, CapsInfo);
        BmqError -3 (.info.n_kept ids are needed) if out_cap is too small."""
        nev, info = C.c_uint32(), _lib.CapsInfo()
        rc = _lib.lib().bmq_routes_cap_dev(self.h, d_row_ptr, d_ids, n_rows, total, d_row_caps, d_max_pf, d_max_gf, n_caps, d_out_row_ptr, d_out_ids, out_cap,
                                           d_out_class_counts, d_out_events, events_cap, C.byref(nev), C.byref(info))
        if rc:
            raise self._caps_error(rc, info, nev.value)
        return nev.value, info

    def match_wait_delivery_capped(self, ticket: int, caps, sender_off, sender_hash, nonce: int, out_topic: np.ndarray, out_route: np.ndarray,
                                   out_aux: np.ndarray, share_sender: np.ndarray, share_member: np.ndarray, group_off: np.ndarray, events_cap: int = 4096):
        """The wait of a FMT_DELIVERY ticket with the caps applied between the match and the plan; caps: one (pf, gf) per tenant of the batch
        -> (total ids of the uncapped CSR, DeliveryInfo, events [n, 4] int32, CapsInfo).  BmqError -3 as match_wait_delivery; it carries
        .events and .caps_info too."""
        so = np.ascontiguousarray(sender_off, dtype=np.uint32)
        sh = np.ascontiguousarray(sender_hash, dtype=np.int32)
        pf, gf = self._caps_table(caps)
        info, tot, nev, cinfo = _lib.DeliveryInfo(), C.c_uint64(), C.c_uint32(), _lib.CapsInfo()
        ev = np.zeros((max(1, events_cap), 4), dtype=np.int32)
        rc = _lib.lib().bmq_delivery_wait_capped(self.h, ticket, _ptr(pf), _ptr(gf), len(pf), _ptr(so), _ptr(sh), nonce & 0xFFFFFFFFFFFFFFFF, _ptr(out_topic),
                                                 _ptr(out_route), _ptr(out_aux), min(len(out_topic), len(out_route), len(out_aux)), _ptr(share_sender),
                                                 _ptr(share_member), min(len(share_sender), len(share_member)), _ptr(group_off), len(group_off) - 1,
                                                 C.byref(info), C.byref(tot), _ptr(ev), events_cap, C.byref(nev), C.byref(cinfo))
        events = ev[:min(nev.value, events_cap)]
        if rc:
            err = self._delivery_error(rc, info)
            err.events, err.caps_info = events, cinfo
            raise err
        return tot.value, info, events, cinfo

    # ---- the submit-time fan-out gate of DeliverExecutorGroup.submit over a whole match batch (DW/DeliverExecutorGroup.java:112-231) --
    GATE_INLINE, GATE_P_COUNT, GATE_P_BYTES, GATE_NO_P_BANDWIDTH, GATE_NO_T_BANDWIDTH, GATE_GROUP = 1, 2, 4, 8, 16, 32

    @staticmethod
    def _gate_table(table):
        """(pf, gf, pb, bw) or [(pf, gf, pb, bw), ...] -> (max_pf, max_gf int32, max_pb int64, bandwidth uint8); what does not fit its
        type is the caller's error"""
        rows = [tuple(int(v) for v in table)] if len(table) and not hasattr(table[0], "__len__") else [tuple(int(v) for v in t) for t in table]
        if any(len(t) != 4 for t in rows):
            raise ValueError("a gate table entry is (max_persistent_fanout, max_group_fanout, max_persistent_fanout_bytes, bandwidth)")
        for pf, gf, pb, bw in rows:
            if not (-2**31 <= pf < 2**31 and -2**31 <= gf < 2**31 and -2**63 <= pb < 2**63 and 0 <= bw < 256):
                raise ValueError("a gate table value outside its type")
        col = lambda k, dt: np.array([t[k] for t in rows], dtype=dt)
        return col(0, np.int32), col(1, np.int32), col(2, np.int64), col(3, np.uint8)

    def _gate_error(self, rc: int, info: "_lib.GateInfo") -> BmqError:
        err = BmqError(rc, (_lib.lib().bmq_last_error(self.h) or b"").decode())
        err.info = info
        return err

    def routes_gate_batch(self, row_ptr, route_ids, pack_bytes, table, row_gate=None, inline_threshold: int = 0, out_cap: Optional[int] = None):
        """bmq_routes_gate_batch: the gate of DeliverExecutorGroup.submit over a match CSR, every row under the table entry row_gate names
        (None: entry 0); table = (pf, gf, pb, bw) or a list of such entries -> (row_ptr, ids, flags [n_rows], class_counts [n_rows, 3]
        persistent / transient / group kept, meter_bytes [n_gate] uint64, meter_records [n_gate], info).  A BmqError -3 carries .info,
        .flags, .class_counts, .meter_bytes and .meter_records."""
        row = np.ascontiguousarray(row_ptr, dtype=np.uint32)
        ids = np.ascontiguousarray(route_ids, dtype=np.uint32)
        pk = np.ascontiguousarray(pack_bytes, dtype=np.uint32)
        pf, gf, pb, bw = self._gate_table(table)
        rg = None if row_gate is None else np.ascontiguousarray(row_gate, dtype=np.uint32)
        n = len(row) - 1
        if len(pk) != n or (rg is not None and len(rg) != n):
            raise ValueError("pack_bytes / row_gate: one entry per row")
        if out_cap is None:
            out_cap = len(ids)
        o_row, o_ids = np.zeros(n + 1, dtype=np.uint32), np.zeros(max(1, out_cap), dtype=np.uint32)
        fl, cc = np.zeros(max(n, 1), dtype=np.uint32), np.zeros((max(n, 1), 3), dtype=np.uint32)
        mb, mr = np.zeros(max(len(pf), 1), dtype=np.uint64), np.zeros(max(len(pf), 1), dtype=np.uint32)
        info = _lib.GateInfo()
        rc = _lib.lib().bmq_routes_gate_batch(self.h, _ptr(row), _ptr(ids), n, _ptr(pk), _ptr(rg), _ptr(pf), _ptr(gf), _ptr(pb), _ptr(bw), len(pf), inline_threshold,
                                              _ptr(o_row), _ptr(o_ids), out_cap, _ptr(fl), _ptr(cc), _ptr(mb), _ptr(mr), C.byref(info))
        if rc:
            err = self._gate_error(rc, info)
            err.flags, err.class_counts, err.meter_bytes, err.meter_records = fl[:n], cc[:n], mb[:len(pf)], mr[:len(pf)]
            raise err
        return o_row, o_ids[:info.n_kept], fl[:n], cc[:n], mb[:len(pf)], mr[:len(pf)], info

    def routes_gate_device(self, d_row_ptr, d_ids, n_rows, total, d_pack_bytes, d_row_gate, d_max_pf, d_max_gf, d_max_pb, d_bandwidth, n_gate, inline_threshold,
                           d_out_row_ptr, d_out_ids, out_cap, d_out_flags, d_out_class_counts, d_out_meter_bytes, d_out_meter_records):
        """bmq_routes_gate_dev: all d_* are device pointers (ints; d_row_gate and d_out_class_counts may be None) -> GateInfo; BmqError -3
        (.info.n_kept ids are needed) if out_cap is too small."""
        info = _lib.GateInfo()
        rc = _lib.lib().bmq_routes_gate_dev(self.h, d_row_ptr, d_ids, n_rows, total, d_pack_bytes, d_row_gate, d_max_pf, d_max_gf, d_max_pb, d_bandwidth, n_gate,
                                            inline_threshold, d_out_row_ptr, d_out_ids, out_cap, d_out_flags, d_out_class_counts, d_out_meter_bytes, d_out_meter_records,
                                            C.byref(info))
        if rc:
            raise self._gate_error(rc, info)
        return info

    def match_wait_delivery_gated(self, ticket: int, table, pack_bytes, inline_threshold: int, sender_off, sender_hash, nonce: int, out_topic: np.ndarray,
                                  out_route: np.ndarray, out_aux: np.ndarray, share_sender: np.ndarray, share_member: np.ndarray, group_off: np.ndarray,
                                  events_cap: int = 4096):
        """The wait of a FMT_DELIVERY ticket with the caps and then the gate applied between the match and the plan; table: one
        (pf, gf, pb, bw) per tenant of the batch, pack_bytes: one per topic -> (total ids of the unthrottled CSR, DeliveryInfo, the caps'
        events [n, 4] int32, CapsInfo, flags [n_topics], meter_bytes [n_tenants], meter_records [n_tenants], GateInfo).  BmqError -3 as
        match_wait_delivery; it carries .events, .caps_info, .flags, .meter_bytes, .meter_records and .gate_info too."""
        so = np.ascontiguousarray(sender_off, dtype=np.uint32)
        sh = np.ascontiguousarray(sender_hash, dtype=np.int32)
        pk = np.ascontiguousarray(pack_bytes, dtype=np.uint32)
        if len(pk) != len(so) - 1:
            raise ValueError("pack_bytes: one entry per topic")
        pf, gf, pb, bw = self._gate_table(table)
        info, tot, nev, cinfo, ginfo = _lib.DeliveryInfo(), C.c_uint64(), C.c_uint32(), _lib.CapsInfo(), _lib.GateInfo()
        ev = np.zeros((max(1, events_cap), 4), dtype=np.int32)
        fl = np.zeros(max(len(pk), 1), dtype=np.uint32)
        mb, mr = np.zeros(max(len(pf), 1), dtype=np.uint64), np.zeros(max(len(pf), 1), dtype=np.uint32)
        rc = _lib.lib().bmq_delivery_wait_gated(self.h, ticket, _ptr(pf), _ptr(gf), _ptr(pb), _ptr(bw), len(pf), _ptr(pk), inline_threshold, _ptr(so), _ptr(sh),
                                                nonce & 0xFFFFFFFFFFFFFFFF, _ptr(out_topic), _ptr(out_route), _ptr(out_aux),
                                                min(len(out_topic), len(out_route), len(out_aux)), _ptr(share_sender), _ptr(share_member),
                                                min(len(share_sender), len(share_member)), _ptr(group_off), len(group_off) - 1, C.byref(info), C.byref(tot), _ptr(ev),
                                                events_cap, C.byref(nev), C.byref(cinfo), _ptr(fl), _ptr(mb), _ptr(mr), C.byref(ginfo))
        events = ev[:min(nev.value, events_cap)]
        if rc:
            err = self._delivery_error(rc, info)
            err.events, err.caps_info, err.gate_info = events, cinfo, ginfo
            err.flags, err.meter_bytes, err.meter_records = fl[:len(pk)], mb[:len(pf)], mr[:len(pf)]
            raise err
        return tot.value, info, events, cinfo, fl[:len(pk)], mb[:len(pf)], mr[:len(pf)], ginfo

    def finish(self) -> int:
        total = C.c_uint64()
        self._check(_lib.lib().bmq_match_finish(self.h, C.byref(total)))
        return total.value

    def sync(self):
        self._check(_lib.lib().bmq_sync(self.h))

    def set_kernel_timing(self, on: bool):
        """HIP events around k_walk / k_expand (stats().ms_walk / ms_expand); ~16 us per batch, off by default."""
        self._check(_lib.lib().bmq_set_kernel_timing(self.h, 1 if on else 0))

    def stats(self) -> _lib.Stats:
        out = _lib.Stats()
        self._check(_lib.lib().bmq_stats_get(self.h, C.byref(out)))
        return out

    # ---- retain direction (IRetainTopicIndex, RS/index/IRetainTopicIndex.java:27-35) --------------------------------
    def retain_rebuild(self, tenants: Sequence, topic_tenant, topics: Sequence = (), packed_topics=None, timestamps=None, expiry=None):
        """Load the retained-topic index; topic id = rank of (tenant, level list).  timestamps (HLC) / expiry (seconds): what
        IRetainTopicIndex.add carries; both None = the topics never expire."""
        tdata, toff = pack(tenants)
        pdata, poff = pack(topics) if packed_topics is None else packed_topics
        tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64)
        ex = None if expiry is None else np.ascontiguousarray(expiry, dtype=np.uint32)
        self._check(_lib.lib().bmq_retain_rebuild_ex(self.h, _ptr(tdata), _ptr(toff), len(toff) - 1, _ptr(tt), _ptr(pdata),
                                                     _ptr(poff), len(poff) - 1, _ptr(ts), _ptr(ex)))
        return self

    def retain_compact_begin(self, start=None, end=None):
        """bmq_retain_compact_begin[_in]: snapshot of the live retained topics -- the next generation starts from it; with a boundary it
        takes the topics with start <= retainMessageKey < end only (the range that shrinks in a split)"""
        if start is None and end is None:
            self._check(_lib.lib().bmq_retain_compact_begin(self.h))
        else:
            self._check(_lib.lib().bmq_retain_compact_begin_in(self.h, *self._boundary(start, end)))
        return self

    def retain_count_in(self, start=None, end=None) -> Tuple[int, int]:
        """bmq_retain_count_in: (retained topics whose key lies inside the boundary, the sum of their key lengths); nothing is changed"""
        topics, key_bytes = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_retain_count_in(self.h, *self._boundary(start, end), C.byref(topics), C.byref(key_bytes)))
        return int(topics.value), int(key_bytes.value)

    def retain_ids_in(self, start=None, end=None) -> List[int]:
        """bmq_retain_ids_in: ids of the retained topics whose key lies inside the boundary, ascending"""
        b = self._boundary(start, end)
        cap = 1024
        n = C.c_uint32()
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_retain_ids_in(self.h, *b, _ptr(out), cap, C.byref(n))
            if rc == -3:
                cap = n.value
                continue
            self._check(rc)
            return out[:n.value].tolist()

    def retain_import(self, src: "Engine", start=None, end=None) -> Tuple[int, int]:
        """bmq_retain_import: every retained topic of src whose key lies inside the boundary is put into this engine with its stamps,
        without a KV scan -> (imported, replaced)"""
        imported, replaced = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_retain_import(self.h, src.h, *self._boundary(start, end), C.byref(imported), C.byref(replaced)))
        return int(imported.value), int(replaced.value)

    def retain_compact_info(self) -> "_lib.RetainCompactInfo":
        """bmq_retain_compact_info_get: the running begin / build / swap compaction, or the last one that ended in a swap -- state, who built, sizes,
        the host clock around each call, and the bytes copied between host and executor while the engine lock was held"""
        st = _lib.RetainCompactInfo()
        self._check(_lib.lib().bmq_retain_compact_info_get(self.h, C.byref(st)))
        return st

    def retain_compact_build(self):
        """bmq_retain_compact_build: loads the snapshot into an index of its own; no engine lock held (matching / add / remove go on).  With
        retain_builder = 3 the snapshot lies in executor memory and the executor builder loads it there, on a stream of its own"""
        self._check(_lib.lib().bmq_retain_compact_build(self.h))
        return self

    def retain_compact_swap(self) -> Tuple[int, int]:
        """bmq_retain_compact_swap: upload (retain_builder = 3: an exchange of pointers), replay of what was added / removed meanwhile, swap ->
        (topics carried over, ops replayed)"""
        carried, replayed = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_retain_compact_swap(self.h, C.byref(carried), C.byref(replayed)))
        return int(carried.value), int(replayed.value)

    def retain_compact_abort(self):
        self._check(_lib.lib().bmq_retain_compact_abort(self.h))
        return self

    def retain_apply(self, tenant, ops: Sequence):
        """ops: (0 = add | 1 = remove, topic[, timestamp_hlc, expiry_seconds]) -- IRetainTopicIndex.add / remove"""
        t = _b(tenant)
        data, off = pack([o[1] for o in ops])
        op = np.array([o[0] for o in ops], dtype=np.uint8)
        if any(len(o) > 2 for o in ops):
            ts = np.array([o[2] if len(o) > 2 else 0 for o in ops], dtype=np.uint64)
            ex = np.array([o[3] if len(o) > 3 else 0xFFFFFFFF for o in ops], dtype=np.uint32)
            self._check(_lib.lib().bmq_retain_apply_ex(self.h, t, len(t), _ptr(data), _ptr(off), _ptr(op), _ptr(ts), _ptr(ex), len(ops)))
        else:
            self._check(_lib.lib().bmq_retain_apply(self.h, t, len(t), _ptr(data), _ptr(off), _ptr(op), len(ops)))
        return self

    def retain_apply_batch(self, tenants: Sequence, op_tenant, ops: Sequence, packed_topics=None, op_codes=None, timestamps=None, expiry=None):
        """bmq_retain_apply_batch: ops of several tenants in one call.  ops: (0 = add | 1 = remove, topic[, timestamp_hlc, expiry_seconds])
        -- or packed_topics + op_codes (+ timestamps, expiry) for large batches.  -> the topic id of every op (0xFFFFFFFF: no-op)"""
        tdata, toff = pack(tenants)
        if packed_topics is None:
            data, off = pack([o[1] for o in ops])
            op = np.array([o[0] for o in ops], dtype=np.uint8)
            if any(len(o) > 2 for o in ops):
                timestamps = np.array([o[2] if len(o) > 2 else 0 for o in ops], dtype=np.uint64)
                expiry = np.array([o[3] if len(o) > 3 else 0xFFFFFFFF for o in ops], dtype=np.uint32)
        else:
            data, off = packed_topics
            op = np.ascontiguousarray(op_codes, dtype=np.uint8)
        n = len(off) - 1
        ot = None if op_tenant is None else np.ascontiguousarray(op_tenant, dtype=np.uint32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64)
        ex = None if expiry is None else np.ascontiguousarray(expiry, dtype=np.uint32)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(_lib.lib().bmq_retain_apply_batch(self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(ot), _ptr(data), _ptr(off), _ptr(op),
                                                      _ptr(ts), _ptr(ex), n, _ptr(out)))
        return out[:n]

    def retain_compact(self):
        self._check(_lib.lib().bmq_retain_compact(self.h))
        return self

    def retain_info(self) -> "_lib.RetainInfo":
        st = _lib.RetainInfo()
        self._check(_lib.lib().bmq_retain_info_get(self.h, C.byref(st)))
        return st

    def retain_build_info(self) -> "_lib.RetainBuildInfo":
        """the bulk load behind the serving generation of the retained-topic index: which builder ran, what it built, how long it took"""
        st = _lib.RetainBuildInfo()
        self._check(_lib.lib().bmq_retain_build_info_get(self.h, C.byref(st)))
        return st

    def retain_live_ids(self, tenant=None) -> List[int]:
        """ids of the retained topics, ascending (tenant None: of every tenant) -- IRetainTopicIndex.findAll()"""
        t = None if tenant is None else _b(tenant)
        cap = 1024
        n = C.c_uint32()
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_retain_live_ids(self.h, t, len(t) if t is not None else 0, _ptr(out), cap, C.byref(n))
            if rc == -3:
                cap = n.value
                continue
            self._check(rc)
            return out[:n.value].tolist()

    def retain_topics(self, topic_ids) -> List[Tuple[str, str]]:
        """many ids -> [(tenant, topic)] (("", "") for an unknown id)"""
        ids = np.ascontiguousarray(topic_ids, dtype=np.uint32)
        n = len(ids)
        off, tl = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
        cap = max(4096, 64 * n)
        while True:
            out = np.zeros(cap, dtype=np.uint8)
            rc = _lib.lib().bmq_retain_topics(self.h, _ptr(ids), n, _ptr(out), cap, _ptr(off), _ptr(tl))
            if rc == -3:
                cap = int(off[n]) + 16
                continue
            self._check(rc)
            raw = out.tobytes()
            return [(raw[int(off[i]):int(off[i]) + int(tl[i])].decode(), raw[int(off[i]) + int(tl[i]):int(off[i + 1])].decode()) for i in range(n)]

    def retain_tenant_counts(self, tenants_cap: int = 4096, cap: int = 256) -> List[Tuple[bytes, int]]:
        """bmq_retain_tenant_counts: [(tenant id bytes, retained topics now)] in byte order of the ids ('$' topics included)"""
        return self._named_numbers(lambda *a: _lib.lib().bmq_retain_tenant_counts(self.h, *a), 1, tenants_cap, cap)

    def retain_remove_ids(self, topic_ids, generation: int) -> int:
        """bmq_retain_remove_ids: the post-commit half of the GC, by id -> topics removed (dead ids and repeats are no-ops)"""
        ids = np.ascontiguousarray(topic_ids, dtype=np.uint32)
        removed = C.c_uint64()
        self._check(_lib.lib().bmq_retain_remove_ids(self.h, _ptr(ids) if len(ids) else None, len(ids), generation, C.byref(removed)))
        return int(removed.value)

    def retain_message_keys(self, topic_ids) -> List[bytes]:
        """bmq_retain_message_keys: retainMessageKey(tenant, topic) per id (b"" for an id that is unknown or not retained now)"""
        ids = np.ascontiguousarray(topic_ids, dtype=np.uint32)
        n = len(ids)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = max(4096, 96 * n)
        while True:
            out = np.zeros(cap, dtype=np.uint8)
            rc = _lib.lib().bmq_retain_message_keys(self.h, _ptr(ids) if n else None, n, _ptr(out), cap, _ptr(off))
            if rc == -3:
                cap = int(off[n]) + 16
                continue
            self._check(rc)
            raw = out.tobytes()
            return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    def retain_keys_prepare(self) -> int:
        """bmq_retain_keys_prepare: build this generation's device-resident string store now (idempotent) -> the bytes it holds"""
        n = C.c_uint64()
        self._check(_lib.lib().bmq_retain_keys_prepare(self.h, C.byref(n)))
        return int(n.value)

    def retain_keys_by_id(self, topic_ids) -> List[bytes]:
        """bmq_retain_keys_by_id: retain_message_keys composed where the index lives (b"" for an id that is unknown or not retained now)"""
        ids = np.ascontiguousarray(topic_ids, dtype=np.uint32)
        n = len(ids)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = max(4096, 96 * n)
        while True:
            out = np.zeros(cap, dtype=np.uint8)
            rc = _lib.lib().bmq_retain_keys_by_id(self.h, _ptr(ids) if n else None, n, _ptr(out), cap, _ptr(off))
            if rc == -3:
                cap = int(off[n]) + 16
                continue
            self._check(rc)
            raw = out.tobytes()
            return [raw[int(off[i]):int(off[i + 1])] for i in range(n)]

    def retain_plan(self, tenants: Sequence, op_tenant, ops: Sequence = (), packed_topics=None, clear=None, keys_cap: int = 0) -> "RetainPlan":
        """bmq_retain_plan: the pre-commit half of RetainStoreCoProc.batchRetain for a batch, read-only.  ops: (topic, clear) pairs -- or
        packed_topics + clear for large batches.  -> RetainPlan: code / action / winner / topic_id per op, delta per tenant-table entry, the
        winners' retainMessageKeys (key_off[n + 1] into key_bytes; .keys lists them, b"" for an op without one) and the info."""
        tdata, toff = pack(tenants)
        if packed_topics is None:
            data, off = pack([o[0] for o in ops])
            clear = [1 if o[1] else 0 for o in ops]
        else:
            data, off = packed_topics
        cl = np.ascontiguousarray(clear, dtype=np.uint8)
        n = len(off) - 1
        assert len(cl) == n
        ot = None if op_tenant is None else np.ascontiguousarray(op_tenant, dtype=np.uint32)
        assert ot is None or len(ot) == n
        code, action = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
        winner, ids = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        delta = np.zeros(max(len(tenants), 1), dtype=np.int32)
        koff = np.zeros(n + 1, dtype=np.uint64)
        info = _lib.RetainPlanInfo()
        kcap = keys_cap or max(4096, 64 * n)
        while True:
            keys = np.zeros(kcap, dtype=np.uint8)
            rc = _lib.lib().bmq_retain_plan(self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(ot), _ptr(data), _ptr(off), _ptr(cl), n, _ptr(code), _ptr(action),
                                            _ptr(winner), _ptr(ids), _ptr(delta), _ptr(koff), _ptr(keys), kcap, C.byref(info))
            if rc == -3 and int(koff[n]) > kcap:
                kcap = int(koff[n]) + 16
                continue
            self._check(rc)
            return RetainPlan(code[:n], action[:n], winner[:n], ids[:n], delta[:len(tenants)], koff, keys[:int(koff[n])].tobytes(), info)

    def retain_plan_commit(self, tenants: Sequence, op_tenant, ops: Sequence, plan: "RetainPlan", packed_topics=None, timestamps=None, expiry=None):
        """bmq_retain_plan_commit: the post-commit closure of batchRetain for the ops the plan was made of -> the topic id of every winner
        that changed the index (0xFFFFFFFF otherwise).  BmqError STATE if the index has changed since the plan."""
        tdata, toff = pack(tenants)
        data, off = pack([o[0] for o in ops]) if packed_topics is None else packed_topics
        n = len(off) - 1
        assert len(plan.action) == n
        ot = None if op_tenant is None else np.ascontiguousarray(op_tenant, dtype=np.uint32)
        act = np.ascontiguousarray(plan.action, dtype=np.uint8)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.uint64)
        ex = None if expiry is None else np.ascontiguousarray(expiry, dtype=np.uint32)
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._check(_lib.lib().bmq_retain_plan_commit(self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(ot), _ptr(data), _ptr(off), n, _ptr(act), _ptr(ts), _ptr(ex),
                                                      plan.info.generation, plan.info.epoch, _ptr(out)))
        return out[:n]

    def batch_retain(self, tenants: Sequence, op_tenant, ops: Sequence, kv_commit, timestamps=None, expiry=None):
        """RetainStoreCoProc.batchRetain around a KV commit: plan, kv_commit(puts, deletes) -- puts: [(key, op index)], deletes: [key] --,
        then the index mutation.  -> (plan, topic ids of retain_plan_commit)"""
        plan = self.retain_plan(tenants, op_tenant, ops)
        keys = plan.keys
        puts = [(keys[i], i) for i in range(len(keys)) if plan.action[i] in (PLAN_ADD, PLAN_UPDATE)]
        deletes = [keys[i] for i in range(len(keys)) if plan.action[i] == PLAN_REMOVE]
        kv_commit(puts, deletes)
        return plan, self.retain_plan_commit(tenants, op_tenant, ops, plan, timestamps=timestamps, expiry=expiry)

    def retain_match_keys(self, tenants: Sequence, filter_tenant, filters: Sequence, limits, now_ms: int = 0, packed_filters=None, keys_cap: int = 0):
        """bmq_retain_keys_match: retain_match_limited plus retainMessageKey of every kept id, composed on the device ->
        (row_ptr[n+1], kept topic ids, match count per filter, key_off[kept+1], key bytes); the key of ids[j] is
        key_bytes[key_off[j]:key_off[j+1]]."""
        tdata, toff = pack(tenants)
        pdata, poff = pack(filters) if packed_filters is None else packed_filters
        n = len(poff) - 1
        ft = np.ascontiguousarray(filter_tenant, dtype=np.uint32)
        lim = np.ascontiguousarray(limits, dtype=np.uint32)
        assert len(lim) == n and len(ft) == n
        row = np.zeros(n + 1, dtype=np.uint32)
        counts = np.zeros(max(n, 1), dtype=np.uint32)
        cap = int(min(int(lim.astype(np.uint64).sum()), 1 << 28)) + 1
        kcap = keys_cap or 64 * cap
        need, kneed = C.c_uint64(), C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            koff = np.zeros(cap + 1, dtype=np.uint64)
            keys = np.zeros(max(kcap, 1), dtype=np.uint8)
            rc = _lib.lib().bmq_retain_keys_match(self.h, _ptr(tdata), _ptr(toff), len(toff) - 1, _ptr(ft), _ptr(pdata), _ptr(poff), n, _ptr(lim), now_ms,
                                                  _ptr(row), _ptr(ids), cap, C.byref(need), _ptr(counts), _ptr(koff), _ptr(keys), kcap, C.byref(kneed))
            if rc == -3 and (need.value > cap or kneed.value > kcap):
                cap, kcap = max(cap, need.value), max(kcap, kneed.value)
                continue
            self._check(rc)
            return row, ids[:need.value], counts[:n], koff[:need.value + 1], keys[:kneed.value].tobytes()

    def retain_topic_info(self, topic_id: int) -> Tuple[int, int, int]:
        """-> (timestamp_hlc, expiry_seconds, expire_at_ms)"""
        ts, ex, at = C.c_uint64(), C.c_uint32(), C.c_uint64()
        self._check(_lib.lib().bmq_retain_topic_info(self.h, topic_id, C.byref(ts), C.byref(ex), C.byref(at)))
        return ts.value, ex.value, at.value

    def retain_find_all(self) -> Tuple[int, int]:
        """IRetainTopicIndex.findAll(): (number of retained topics, retain epoch); retain_live_ids lists the ids"""
        n, ep = C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().bmq_retain_find_all(self.h, C.byref(n), C.byref(ep)))
        return n.value, ep.value

    def retain_expired(self, tenant, now_ms: int, override_expiry_seconds: int = -1) -> List[int]:
        """ids whose message has expired at now_ms (tenant None: all tenants) -- the GC scan of RetainStoreCoProc."""
        t = None if tenant is None else _b(tenant)
        cap = 1024
        n = C.c_uint32()
        while True:
            out = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_retain_expired(self.h, t, len(t) if t is not None else 0, now_ms, override_expiry_seconds, _ptr(out), cap,
                                               C.byref(n))
            if rc == -3:
                cap = n.value
                continue
            self._check(rc)
            return out[:n.value].tolist()

    def retain_topic(self, topic_id: int) -> Tuple[str, str]:
        buf = C.create_string_buffer(140000)
        n, tl = C.c_uint32(), C.c_uint32()
        self._check(_lib.lib().bmq_retain_topic(self.h, topic_id, buf, len(buf), C.byref(n), C.byref(tl)))
        raw = buf.raw[:n.value]
        return raw[:tl.value].decode(), raw[tl.value:].decode()

    def retain_match_batch(self, tenants: Sequence, filter_tenant, filters: Sequence = (), packed_filters=None):
        """Batch of IRetainTopicIndex.match(tenant, topicFilter) -> (row_ptr[n+1], topic ids ascending per row)."""
        tdata, toff = pack(tenants)
        pdata, poff = pack(filters) if packed_filters is None else packed_filters
        n = len(poff) - 1
        ft = np.ascontiguousarray(filter_tenant, dtype=np.uint32)
        row = np.zeros(n + 1, dtype=np.uint32)
        cap = max(1024, 16 * n)
        need = C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_retain_match_batch(self.h, _ptr(tdata), _ptr(toff), len(toff) - 1, _ptr(ft), _ptr(pdata),
                                                   _ptr(poff), n, _ptr(row), _ptr(ids), cap, C.byref(need))
            if rc == -3 and need.value > cap:
                cap = need.value
                continue
            self._check(rc)
            return row, ids[:need.value]

    def retain_match_limited(self, tenants: Sequence, filter_tenant, filters: Sequence, limits, now_ms: int = 0, packed_filters=None):
        """RetainStoreCoProc.match(limit, now) for a batch -> (row_ptr[n+1], kept topic ids, match count per filter):
        row i holds the limits[i] smallest matching topic ids that have not expired at now_ms."""
        tdata, toff = pack(tenants)
        pdata, poff = pack(filters) if packed_filters is None else packed_filters
        n = len(poff) - 1
        ft = np.ascontiguousarray(filter_tenant, dtype=np.uint32)
        lim = np.ascontiguousarray(limits, dtype=np.uint32)
        assert len(lim) == n and len(ft) == n
        row = np.zeros(n + 1, dtype=np.uint32)
        counts = np.zeros(n, dtype=np.uint32)
        cap = int(min(int(lim.astype(np.uint64).sum()), 1 << 28)) + 1
        need = C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_retain_match_limited(self.h, _ptr(tdata), _ptr(toff), len(toff) - 1, _ptr(ft), _ptr(pdata), _ptr(poff),
                                                     n, _ptr(lim), now_ms, _ptr(row), _ptr(ids), cap, C.byref(need), _ptr(counts))
            if rc == -3 and need.value > cap:
                cap = need.value
                continue
            self._check(rc)
            return row, ids[:need.value], counts

    def retain_match(self, tenant, topic_filter) -> List[int]:
        row, ids = self.retain_match_batch([tenant], [0], [topic_filter])
        return ids.tolist()

    def retain_match_batch_device(self, d_tenants, d_tenant_off, n_tenants, d_filter_tenant, d_filters, d_filter_off,
                                  n_filters, d_row_ptr, d_ids, capacity, d_total):
        self._check(_lib.lib().bmq_retain_match_batch_dev(self.h, d_tenants, d_tenant_off, n_tenants, d_filter_tenant,
                                                          d_filters, d_filter_off, n_filters, d_row_ptr, d_ids, capacity,
                                                          d_total))

    @property
    def stream(self) -> int:
        return _lib.lib().bmq_stream(self.h) or 0


class Batcher:
    """bmq_batcher_*: collects the single-topic matchAll calls of many threads (TenantRouteCache.java:180-193) into one
    GPU batch.  match_all blocks; call it from as many threads as there are callers (ctypes drops the GIL)."""

    def __init__(self, engine: Engine, max_batch_topics: int = 0):
        cfg = _lib.BatcherConfig()
        cfg.struct_size = C.sizeof(_lib.BatcherConfig)
        cfg.max_batch_topics = max_batch_topics
        h = C.c_void_p()
        rc = _lib.lib().bmq_batcher_create(engine.h, C.byref(cfg), C.byref(h))
        if rc:
            raise BmqError(rc, "bmq_batcher_create failed")
        self.h = h
        self.engine = engine  # keeps the engine alive

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().bmq_batcher_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def match_all(self, tenant, topics: Sequence) -> Tuple[List[List[int]], int]:
        """-> (per-topic ascending route id lists, epoch the ids belong to)"""
        t = _b(tenant)
        pdata, poff = pack(topics)
        n = len(topics)
        row = np.zeros(n + 1, dtype=np.uint32)
        cap = max(256, 16 * n)
        need, epoch = C.c_uint64(), C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_batcher_match_all(self.h, t, len(t), _ptr(pdata), _ptr(poff), n, _ptr(row), _ptr(ids), cap,
                                                  C.byref(need), C.byref(epoch))
            if rc == -3 and need.value > cap:
                cap = int(need.value)
                continue
            if rc:
                raise BmqError(rc, (_lib.lib().bmq_last_error(self.engine.h) or b"").decode())
            return [ids[row[i]:row[i + 1]].tolist() for i in range(n)], int(epoch.value)

    def stats(self) -> "_lib.BatcherStats":
        st = _lib.BatcherStats()
        rc = _lib.lib().bmq_batcher_stats_get(self.h, C.byref(st))
        if rc:
            raise BmqError(rc, "bmq_batcher_stats_get")
        return st

    CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64)

    def submit(self, tenant, topic, on_done):
        """bmq_batcher_submit: returns at once; on_done(status, ids list, epoch) runs on the batcher's dispatcher thread."""
        t, p = _b(tenant), _b(topic)
        if not hasattr(self, "_live"):
            self._live, self._seq = {}, 0
        self._seq += 1
        key = self._seq

        def tramp(_user, status, ids, n, epoch):
            try:
                on_done(status, [ids[i] for i in range(n)], epoch)
            finally:
                self._live.pop(key, None)

        cb = Batcher.CALLBACK(tramp)
        self._live[key] = cb  # keeps the trampoline alive until it has run
        rc = _lib.lib().bmq_batcher_submit(self.h, t, len(t), p, len(p), C.cast(cb, C.c_void_p), None)
        if rc:
            self._live.pop(key, None)
            raise BmqError(rc, "bmq_batcher_submit")

    def drive_singletons(self, tenants: Sequence, topic_tenant: np.ndarray, topics_packed: Tuple[np.ndarray, np.ndarray],
                         n_threads: int, asynchronous: bool = False):
        """n_threads native threads issue one single-topic call per topic (the production call pattern), blocking
        (bmq_batcher_match_all) or asynchronous (bmq_batcher_submit + callback).
        -> (ids per topic, row hash per topic, seconds)"""
        tdata, toff = pack(tenants)
        pdata, poff = topics_packed
        n = len(poff) - 1
        cnt = np.zeros(n, dtype=np.uint32)
        hsh = np.zeros(n, dtype=np.uint64)
        sec = C.c_double()
        fn = C.cast(_lib.lib().bmq_batcher_submit if asynchronous else _lib.lib().bmq_batcher_match_all, C.c_void_p)
        tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        drive = _lib.gen().bmqgen_drive_async if asynchronous else _lib.gen().bmqgen_drive_singletons
        rc = drive(fn, self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(tt), _ptr(pdata), _ptr(poff),
                                                n, n_threads, _ptr(cnt), _ptr(hsh), C.byref(sec))
        if rc:
            raise BmqError(rc, "bmqgen_drive_singletons")
        return cnt, hsh, sec.value


class RouteCache:
    """bmq_route_cache_*: ISubscriptionCache (DW/cache/ISubscriptionCache.java:30-40) on the engine's side of the boundary -- topic ->
    matched routes per tenant, loads through the batching front, TopicIndex-style invalidation by route mutations."""

    def __init__(self, batcher: Batcher, max_routes_per_tenant: int = 0, expiry_ms: int = 0, mutation_log_entries: int = 0, shards_per_tenant: int = 0,
                 max_persistent_fanout: int = 0, max_group_fanout: int = 0, tenant_idle_ms: int = 0, direct_batch_topics: int = 0):
        """max_persistent_fanout / max_group_fanout: the default caps of tenants without set_caps (0 = the reference's defaults,
        Setting.java:60-61: INT_MAX / 100)"""
        cfg = _lib.RouteCacheConfig()
        cfg.struct_size = C.sizeof(_lib.RouteCacheConfig)
        cfg.max_routes_per_tenant = max_routes_per_tenant
        cfg.expiry_ms = expiry_ms
        cfg.mutation_log_entries = mutation_log_entries
        cfg.shards_per_tenant = shards_per_tenant
        cfg.default_max_persistent_fanout = max_persistent_fanout
        cfg.default_max_group_fanout = max_group_fanout
        cfg.tenant_idle_ms = tenant_idle_ms
        cfg.direct_batch_topics = direct_batch_topics
        h = C.c_void_p()
        rc = _lib.lib().bmq_route_cache_create(batcher.engine.h, batcher.h, C.byref(cfg), C.byref(h))
        if rc:
            raise BmqError(rc, "bmq_route_cache_create failed")
        self.h = h
        self.batcher = batcher  # keeps batcher and engine alive

    def close(self):
        if getattr(self, "h", None):
            _lib.lib().bmq_route_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise BmqError(rc, what + ": " + (_lib.lib().bmq_last_error(self.batcher.engine.h) or b"").decode())

    def get(self, tenant, topic, now_ms: int = 0) -> Tuple[List[int], int]:
        """ISubscriptionCache.get -> (ascending route ids, engine epoch they were matched at)"""
        t, p = _b(tenant), _b(topic)
        cap = 64
        n, ep = C.c_uint32(), C.c_uint64()
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_route_cache_get(self.h, t, len(t), p, len(p), now_ms, _ptr(ids), cap, C.byref(n), C.byref(ep))
            if rc == -3:
                cap = n.value + 16
                continue
            self._check(rc, "bmq_route_cache_get")
            return ids[:n.value].tolist(), int(ep.value)

    def get_batch(self, tenants: Sequence, topic_tenant, topics: Sequence, now_ms: int = 0):
        """bmq_route_cache_get_batch: a whole BatchDistRequest -> (row_ptr, route ids, hit flags); misses share ONE launch"""
        tdata, toff = pack(tenants)
        pdata, poff = pack(topics)
        n = len(topics)
        tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        row, hit = np.zeros(n + 1, dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint8)
        cap, need = max(256, 8 * n), C.c_uint64()
        first_hit = None
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            rc = _lib.lib().bmq_route_cache_get_batch(self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(tt), _ptr(pdata), _ptr(poff), n, now_ms,
                                                      _ptr(row), _ptr(ids), cap, C.byref(need), _ptr(hit))
            if first_hit is None:  # a call that ran out of room has loaded (and cached) its misses already: the retry would call them hits
                first_hit = hit[:n].astype(bool)
            if rc == -3 and need.value > cap:
                cap = int(need.value)
                continue
            self._check(rc, "bmq_route_cache_get_batch")
            return row, ids[:need.value], first_hit

    CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64)

    def get_async(self, tenant, topic, on_done, now_ms: int = 0):
        """bmq_route_cache_get_async: on_done(status, ids list, epoch) runs inline on a hit, on the batcher's dispatcher thread after a miss"""
        t, p = _b(tenant), _b(topic)
        if not hasattr(self, "_live"):
            self._live, self._seq = {}, 0
        self._seq += 1
        key = self._seq

        def tramp(_user, status, ids, n, epoch):
            try:
                on_done(status, [ids[i] for i in range(n)], epoch)
            finally:
                self._live.pop(key, None)

        cb = RouteCache.CALLBACK(tramp)
        self._live[key] = cb  # keeps the trampoline alive until it has run
        rc = _lib.lib().bmq_route_cache_get_async(self.h, t, len(t), p, len(p), now_ms, C.cast(cb, C.c_void_p), None)
        if rc:
            self._live.pop(key, None)
            raise BmqError(rc, "bmq_route_cache_get_async")

    def is_cached(self, tenant, topic_filter) -> bool:
        t, f = _b(tenant), _b(topic_filter)
        rc = _lib.lib().bmq_route_cache_is_cached(self.h, t, len(t), f, len(f))
        if rc < 0:
            raise BmqError(rc, "bmq_route_cache_is_cached")
        return rc == 1

    def apply(self, ops: Sequence[Tuple[int, bytes]]):
        """ISubscriptionCache.refresh: [(0 = put | 1 = delete, route key)] -> engine, then invalidation"""
        data, off = pack([k for _, k in ops])
        op = np.array([o for o, _ in ops], dtype=np.uint8)
        self._check(_lib.lib().bmq_route_cache_apply(self.h, _ptr(data), _ptr(off), _ptr(op), len(ops)), "bmq_route_cache_apply")

    def rebuild(self, keys: Iterable[bytes]):
        data, off = pack(sorted(keys))
        self._check(_lib.lib().bmq_route_cache_rebuild(self.h, _ptr(data), _ptr(off), len(off) - 1), "bmq_route_cache_rebuild")

    def reset(self):
        self._check(_lib.lib().bmq_route_cache_reset(self.h), "bmq_route_cache_reset")

    def expire(self, now_ms: int) -> int:
        """drop every entry not accessed for expiry_ms -> number dropped"""
        n = C.c_uint64()
        self._check(_lib.lib().bmq_route_cache_expire(self.h, now_ms, C.byref(n)), "bmq_route_cache_expire")
        return int(n.value)

    def stats(self) -> "_lib.RouteCacheStats":
        st = _lib.RouteCacheStats()
        self._check(_lib.lib().bmq_route_cache_stats_get(self.h, C.byref(st)), "bmq_route_cache_stats_get")
        return st

    def tenant_stats(self, tenant) -> Optional["_lib.RouteCacheTenantStats"]:
        """the tenant's meters (TenantRouteCache.java:141-147), or None when the tenant has no cache"""
        t = _b(tenant)
        st = _lib.RouteCacheTenantStats()
        rc = _lib.lib().bmq_route_cache_tenant_stats_get(self.h, t, len(t), C.byref(st))
        if rc == -7:
            return None
        self._check(rc, "bmq_route_cache_tenant_stats_get")
        return st

    def set_caps(self, tenant, max_persistent_fanout: int, max_group_fanout: int):
        """the tenant's MaxPersistentFanout / MaxGroupFanout settings"""
        t = _b(tenant)
        self._check(_lib.lib().bmq_route_cache_set_caps(self.h, t, len(t), max_persistent_fanout, max_group_fanout), "bmq_route_cache_set_caps")

    EVENT_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.c_int32, C.c_uint32, C.c_int32)

    def collect_events(self) -> list:
        """installs an event sink (IEventCollector) that appends (tenant, topic, type, route id, max count) to the returned list;
        type 0 = PersistentFanoutThrottled, 1 = GroupFanoutThrottled"""
        events: list = []

        def sink(_user, tenant, tl, topic, pl, typ, rid, mx):
            events.append((bytes(tenant[:tl]), bytes(topic[:pl]), int(typ), int(rid), int(mx)))

        self._event_cb = RouteCache.EVENT_CB(sink)  # kept alive with the cache
        self._check(_lib.lib().bmq_route_cache_set_event_sink(self.h, C.cast(self._event_cb, C.c_void_p), None), "bmq_route_cache_set_event_sink")
        return events

    def drive(self, tenants: Sequence, topic_tenant: np.ndarray, topics_packed: Tuple[np.ndarray, np.ndarray], n_threads: int, passes: int = 2,
              asynchronous: bool = False):
        """n_threads native threads call bmq_route_cache_get (or _get_async) once per topic, `passes` times over the batch.
        -> (ids per topic, row hash per topic, seconds per pass)"""
        tdata, toff = pack(tenants)
        pdata, poff = topics_packed
        n = len(poff) - 1
        cnt, hsh = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
        sec = (C.c_double * passes)()
        tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        fn, drv = ((_lib.lib().bmq_route_cache_get_async, _lib.gen().bmqgen_drive_cache_async) if asynchronous else
                   (_lib.lib().bmq_route_cache_get, _lib.gen().bmqgen_drive_cache))
        rc = drv(C.cast(fn, C.c_void_p), self.h, _ptr(tdata), _ptr(toff), len(tenants), _ptr(tt),
                                           _ptr(pdata), _ptr(poff), n, n_threads, passes, _ptr(cnt), _ptr(hsh), sec)
        if rc:
            raise BmqError(rc, "bmqgen_drive_cache")
        return cnt, hsh, list(sec)
