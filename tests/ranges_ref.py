"""A strict consumer of BMQ_FMT_RANGES, written from the text of include/bmq.h (bmq_match_wait_ranges) alone, and the builders of the small
directed batches the shape tests use.  Unlike Engine.expand_ranges -- a lenient consumer: it orders whatever row shows an overlap and never
tells -- this one reports WHICH rows it had to order, so that a test can hold the engine to n_overlapping_rows and to the promised order."""
import numpy as np

from bifromq_amd.engine import pack, pinned

SIDE = 0x80000000
SORT_MAX = 32  # "rows of more than 32 ranges: as matched"


def _ids_of(b, c, side):
    b, c = int(b), int(c)
    if c & SIDE:
        return np.asarray(side[b:b + (c & ~SIDE)], dtype=np.uint32)
    return np.arange(b, b + c, dtype=np.int64).astype(np.uint32)


def strict_rows(range_ptr, ranges, side, n):
    """-> (rows, overlap_flags): every row's ranges expanded in the order given; a row is flagged when a non-empty range's first id is <= the
    last id of the non-empty range before it, and only flagged rows are ordered."""
    rows, flags = [], []
    for i in range(n):
        parts, last, overlap = [], None, False
        for b, c in ranges[int(range_ptr[i]):int(range_ptr[i + 1])]:
            ids = _ids_of(b, c, side)
            if len(ids) == 0:
                continue
            if last is not None and int(ids[0]) <= last:
                overlap = True
            last = int(ids[-1])
            parts.append(ids)
        row = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
        rows.append(np.sort(row) if overlap else row)
        flags.append(overlap)
    return rows, flags


def check_ranges_contract(info, range_ptr, ranges, side, n, erow, eids):
    """the contract of bmq_match_wait_ranges against the expected id CSR (erow, eids); -> (rows, overlap_flags)"""
    rp = np.asarray(range_ptr[:n + 1], dtype=np.int64)
    # (d) range_ptr is non-decreasing and ends at n_ranges
    assert rp[0] == 0 and rp[n] == info.n_ranges and (np.diff(rp) >= 0).all(), "range_ptr"
    # (f) n_ids is the CSR total
    assert info.n_ids == len(eids) == int(erow[n]), "n_ids %d, the id CSR holds %d" % (info.n_ids, len(eids))
    # (e) the side slices of the rows: disjoint, in row order, covering exactly [0, n_side_ids)
    cursor = 0
    for i in range(n):
        spans, empties = [], []
        for b, c in ranges[rp[i]:rp[i + 1]]:
            b, c = int(b), int(c)
            if c & SIDE:
                (spans if c & ~SIDE else empties).append((b, c & ~SIDE))
        start = cursor
        for b, ln in sorted(spans):
            assert b == cursor, "row %d: a side list begins at %d, the row's slice goes on at %d" % (i, b, cursor)
            cursor += ln
        for b, _ in empties:
            assert start <= b <= cursor, "row %d: an empty side list at %d outside the row's slice [%d, %d]" % (i, b, start, cursor)
    assert cursor == info.n_side_ids, "the side lists cover %d words, n_side_ids is %d" % (cursor, info.n_side_ids)
    rows, flags = strict_rows(range_ptr, ranges, side, n)
    # (a) every row is the expected row
    for i in range(n):
        assert np.array_equal(rows[i], eids[int(erow[i]):int(erow[i + 1])]), "row %d: %r, expected %r" % (i, rows[i][:40], eids[int(erow[i]):int(erow[i + 1])][:40])
    # (b) the engine's count of rows to order is the consumer's
    assert info.n_overlapping_rows == sum(flags), "n_overlapping_rows %d, the strict consumer ordered %d rows" % (info.n_overlapping_rows, sum(flags))
    # (c) rows of up to 32 ranges: the first ids of the non-empty ranges ascend
    for i in range(n):
        if rp[i + 1] - rp[i] > SORT_MAX:
            continue
        firsts = [int(_ids_of(b, c, side)[0]) for b, c in ranges[rp[i]:rp[i + 1]] if int(c) & ~SIDE]
        assert all(x < y for x, y in zip(firsts, firsts[1:])), "row %d of %d ranges: first ids %r" % (i, rp[i + 1] - rp[i], firsts)
    return rows, flags


# ---- case builders --------------------------------------------------------------------------------------------------------------
class Batch:
    """a match batch in page-locked memory: tenants, topic_tenant, topics"""

    def __init__(self, tenants, topic_tenant, topics):
        self.tenants, self.topics = list(tenants), list(topics)
        self.tt = np.ascontiguousarray(topic_tenant, dtype=np.uint32)
        self.n = len(self.topics)
        assert self.tt.shape == (self.n,)
        tdata, toff = pack(self.tenants)
        pdata, poff = pack(self.topics)
        self.packed = (pdata, poff)
        self.p_t, self.p_to = pinned(len(tdata) + 16, np.uint8), pinned(len(toff), np.uint32)
        self.p_d, self.p_o, self.p_tt = pinned(len(pdata) + 16, np.uint8), pinned(len(poff), np.uint32), pinned(max(self.n, 1), np.uint32)
        self.p_t[:], self.p_d[:] = 0, 0
        self.p_t[:len(tdata)], self.p_to[:] = tdata, toff
        self.p_d[:len(pdata)], self.p_o[:], self.p_tt[:self.n] = pdata, poff, self.tt

    def submit(self, eng, fmt):
        return eng.match_submit_fmt(self.p_t, self.p_to, len(self.tenants), self.p_tt, self.p_d, self.p_o, self.n, fmt)

    def ids(self, eng):
        """the id CSR of the batch through the synchronous entry point"""
        return eng.match_batch(self.tenants, self.tt, packed_topics=self.packed)

    def ids_async(self, eng):
        """the BMQ_FMT_IDS result of the same batch: submit, wait (a second wait with the size where the first is too small)"""
        row, ids = pinned(self.n + 1, np.uint32), pinned(max(1024, 8 * self.n), np.uint32)
        t = self.submit(eng, eng.FMT_IDS)
        try:
            total = eng.match_wait(t, row, ids)
        except Exception as e:  # BmqError -3 carries the size
            if getattr(e, "code", 0) != -3:
                raise
            ids = pinned(e.needed + 8, np.uint32)
            total = eng.match_wait(self.submit(eng, eng.FMT_IDS), row, ids)
        return row.copy(), ids[:total].copy()


def wait_ranges(eng, ticket, n, range_cap, side_cap):
    """-> (info, range_ptr, ranges, side, row): buffers of exactly range_cap / side_cap entries (pinned() does not take 0: one spare entry is cut off)"""
    rptr, row = pinned(n + 1, np.uint32), pinned(n + 1, np.uint32)
    ranges, side = pinned((range_cap + 1, 2), np.uint32)[:range_cap], pinned(side_cap + 1, np.uint32)[:side_cap]
    ranges[:], side[:] = 0xABABABAB, 0xABABABAB
    info = eng.match_wait_ranges(ticket, rptr, ranges, side, row)
    return info, rptr, ranges, side, row


def ranges_of(eng, batch, erow, eids, range_cap=None, side_cap=None):
    """submit `batch` as BMQ_FMT_RANGES, wait ONCE and hold the result to the contract; -> (info, range_ptr, ranges, side, rows, flags)"""
    total = len(eids)
    t = batch.submit(eng, eng.FMT_RANGES)
    info, rptr, ranges, side, row = wait_ranges(eng, t, batch.n, max(total, 16) + 64 * batch.n if range_cap is None else range_cap, max(total, 16) if side_cap is None else side_cap)
    assert np.array_equal(row, erow), "the id row pointers"
    rows, flags = check_ranges_contract(info, rptr, ranges, side, batch.n, erow, eids)
    return info, rptr, ranges, side, rows, flags


def expected_csr(eng, batch, keys_live=None):
    """the id CSR the semantic oracle expects for `batch` on the engine's LIVE key set (read back with route_keys, compared with keys_live
    where the caller knows it); ranks -> engine ids, every row ascending; eng.match_batch must agree with it.  -> (row_ptr, ids)"""
    from oracle import oracle as O
    from tests import util as U
    nid = eng.info().next_route_id
    id_of = {k: i for i, k in enumerate(eng.route_keys(list(range(nid)))) if k}
    if keys_live is not None:
        assert set(id_of) == set(keys_live)
    live = sorted(id_of)
    res, _ = O.KV(live).match_semantic_batch(batch.tenants, batch.tt, batch.packed, threads=U.host_threads())
    rp = res.row_ptr.astype(np.int64)
    ids = U.csr_sorted(rp, np.asarray([id_of[k] for k in live], dtype=np.int64)[res.routes.astype(np.int64)]) if len(res.routes) else np.zeros(0, dtype=np.int64)
    erow, eids = rp.astype(np.uint32), ids.astype(np.uint32)
    grow, gids = batch.ids(eng)
    assert np.array_equal(grow, erow) and np.array_equal(gids, eids), "match_batch and the semantic oracle disagree"
    return erow, eids
