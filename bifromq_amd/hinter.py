"""The dist worker's fan-out split hinter over the device-resident route index, at the reference's granularity.

DW/hinter/FanoutSplitHinter.java asks its KV range two questions for every key prefix a mutation batch touched: how many records lie
under the prefix (reader.size([prefix, upperBound(prefix))), :175-178) and, if that reaches splitAtScale, which key lies splitAtScale
steps behind seek(prefix) (:187-198).  Here the first is ONE Engine.prefix_census call for all prefixes of the batch (one pass over
the key store in HBM), the second a chain of key-ordered windows (Engine.window), so the reference's default scale of 100 000
(FanoutSplitHinterFactory.java:33) is served although one window holds at most BMQ_WINDOW_MAX keys.

The reference keys its map by the FULL route key (toNormalRouteKey, :94-100) while the names (matchRecordKeyPrefix, load
fanout_topicfilters) and doEstimate treat the key as a prefix that covers a filter's receivers; with the v4 key layout a full key's
prefix range holds that one key.  So the granularity is a choice: "filter" (the intent, the default), "key" (the reference's literal
behaviour) or "tenant" (what shard.py::FanoutSplitHinter approximates from counted mutations).

Documented deviation: the reference estimates a prefix's scale as reader.size / avgRecordSize minus the tombstones of the batch, from
an approximate size (:175-179); here the scale is the exact count of live keys under the prefix after the batch.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

from .engine import BMQ_PREFIX_MAX, BMQ_WINDOW_MAX, Engine

TYPE = "fanout_split_hinter"  # FanoutSplitHinter.TYPE, :50
LOAD_TYPE_FANOUT_TOPIC_FILTERS = "fanout_topicfilters"  # :51
LOAD_TYPE_FANOUT_SCALE = "fanout_scale"  # :52
GRANULARITIES = ("filter", "key", "tenant")


def upper_bound(key: bytes) -> Optional[bytes]:
    """BoundaryUtil.upperBound (base-kv/.../utils/BoundaryUtil.java:299-307): the least key above every key that starts with `key` --
    trailing 0xFF bytes dropped, the last other byte incremented; None (an open end) for an empty or all-0xFF key."""
    k = bytes(key).rstrip(b"\xff")
    return k[:-1] + bytes([k[-1] + 1]) if k else None


def tenant_prefix(route_key: bytes) -> bytes:
    """tenantBeginKey (SCHEMA/KVSchemaUtil.java): 00 | u16be(len tenant) | tenant -- what all route keys of the tenant start with."""
    k = bytes(route_key)
    if len(k) < 3 or k[0] != 0 or len(k) < 3 + ((k[1] << 8) | k[2]):
        raise ValueError("not a route key")
    return k[:3 + ((k[1] << 8) | k[2])]


def filter_prefix(route_key: bytes) -> bytes:
    """tenantRouteStartKey (SCHEMA/KVSchemaUtil.java:96-102): the key cut in front of its bucket byte -- tenant prefix, escaped filter
    levels, two NUL bytes -- which all receivers of the filter share.  Parsed from the key's END as parseFlag does (:66-71): the last two
    bytes are the receiver's length, in front of the receiver lie flag and bucket."""
    k = bytes(route_key)
    if len(k) < 9:
        raise ValueError("not a route key")
    cut = len(k) - 2 - ((k[-2] << 8) | k[-1]) - 2
    if cut < len(tenant_prefix(k)) + 2 or k[cut - 2:cut] != b"\x00\x00":
        raise ValueError("not a route key")
    return k[:cut]


def in_range(key: bytes, boundary) -> bool:
    """BoundaryUtil.inRange (BoundaryUtil.java:241-252): (no start or key >= start) and (no end or key < end)"""
    start, end = boundary
    return (start is None or key >= start) and (end is None or key < end)


def is_splittable(boundary, key: bytes) -> bool:
    """BoundaryUtil.isSplittable (BoundaryUtil.java:489-500): not inside a NULL boundary (no start, an empty end), a non-empty key,
    strictly above a present start and strictly below a present end"""
    start, end = boundary
    if start is None and end == b"":
        return False
    if key == b"":
        return False
    return (start is None or start < key) and (end is None or key < end)


class RangeFanoutSplitHinter:
    """FanoutSplitHinter.java over one engine (= one KV range's routes).  The map `splits` is fanoutSplitKeys (:56): prefix ->
    (data_size, record_size, split_key)."""

    def __init__(self, engine: Engine, split_at_scale: int = 100000, granularity: str = "filter", boundary=(None, None)):
        if granularity not in GRANULARITIES:
            raise ValueError("granularity must be one of %r" % (GRANULARITIES,))
        if split_at_scale < 1:
            raise ValueError("split_at_scale must be at least 1")
        self.engine = engine
        self.split_at_scale = int(split_at_scale)
        self.granularity = granularity
        self.boundary = self._boundary(boundary)
        self.splits: Dict[bytes, Tuple[int, int, bytes]] = {}

    @staticmethod
    def _boundary(boundary):
        start, end = boundary
        return (None if start is None else bytes(start), None if end is None else bytes(end))

    def prefix_of(self, route_key: bytes) -> bytes:
        if self.granularity == "filter":
            return filter_prefix(route_key)
        if self.granularity == "tenant":
            return tenant_prefix(route_key)
        return bytes(route_key)

    # ---- recordMutate, :84-127 ---------------------------------------------------------------------------------------------------
    def record_mutate(self, ops: Iterable[Tuple[int, bytes]]) -> None:
        """`ops` is the [(op, key)] batch that was JUST APPLIED to the engine (after commit; op 0 = put, 1 = delete): every distinct
        prefix it touched is re-estimated, all of them in one census."""
        self._estimate({self.prefix_of(k) for _, k in ops})

    # ---- doEstimate, :171-203 ----------------------------------------------------------------------------------------------------
    def _estimate(self, prefixes) -> None:
        todo = sorted(prefixes)
        if not todo:
            return
        candidates: List[Tuple[bytes, int, int]] = []
        for at in range(0, len(todo), BMQ_PREFIX_MAX):  # (one call; a batch of more distinct prefixes than a call takes goes in several)
            part = todo[at:at + BMQ_PREFIX_MAX]
            stats = self.engine.prefix_census(part)
            for p, row in zip(part, stats):
                scale = int(row[0]) + int(row[1]) + int(row[2])
                if scale >= self.split_at_scale:  # :180-181
                    candidates.append((p, int(row[3]), int(row[3]) // scale))
                elif p in self.splits and 2 * scale < self.split_at_scale:  # :182-184
                    del self.splits[p]
        for p, data_size, record_size in candidates:  # :186-200
            if p in self.splits:  # computeIfAbsent: an existing entry keeps its key, :190
                continue
            key = self.split_key_at(p, self.split_at_scale)
            if key is not None:  # (:197: nothing behind the scale-th key -- no entry)
                self.splits[p] = (data_size, record_size, key)

    def split_key_at(self, prefix: bytes, index: int) -> Optional[bytes]:
        """The key at `index` among the live keys >= prefix, NOT bounded by the prefix (itr.seek(routeKey) and `index` steps, :191-196);
        None if there are not that many.  ceil((index + 1) / BMQ_WINDOW_MAX) windows, each behind the last key of the one before (an
        exclusive cursor by key bytes)."""
        if index < 0:
            raise ValueError("index must not be negative")
        left = index + 1
        cursor, exclusive = bytes(prefix), False
        while True:
            want = min(left, BMQ_WINDOW_MAX)
            ids, _ = self.engine.window(cursor, want, exclusive)
            if len(ids) < want:
                return None
            last = self.engine.route_key(int(ids[-1]))
            left -= want
            if left == 0:
                return last
            cursor, exclusive = last, True

    # ---- reset, :129-145 ---------------------------------------------------------------------------------------------------------
    def reset(self, boundary) -> None:
        """The range's boundary changed (after a split or a merge): entries whose split key lies outside it are dropped and their
        prefixes estimated again, in one census."""
        self.boundary = self._boundary(boundary)
        finished = [p for p, (_, _, key) in self.splits.items() if not in_range(key, self.boundary)]
        for p in finished:
            del self.splits[p]
        self._estimate(finished)

    # ---- estimate, :147-163 ------------------------------------------------------------------------------------------------------
    def estimate(self) -> dict:
        """SplitHint: the load counts the map's entries BEFORE this call removes one (:151); the entry looked at is the smallest prefix
        in byte order (the reference takes a hash map's first entry, which is unspecified); an entry whose key cannot split the boundary
        is removed and no key is reported (:154-155)."""
        hint = {"type": TYPE, "split_key": None, "load": {LOAD_TYPE_FANOUT_TOPIC_FILTERS: len(self.splits), LOAD_TYPE_FANOUT_SCALE: 0.0}}
        if self.splits:
            p = min(self.splits)
            data_size, record_size, key = self.splits[p]
            if not is_splittable(self.boundary, key):
                del self.splits[p]
            else:
                hint["split_key"] = key
                hint["load"][LOAD_TYPE_FANOUT_SCALE] = data_size / float(record_size)
        return hint
