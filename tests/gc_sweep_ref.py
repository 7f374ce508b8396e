"""A strict model of the dist worker's GC sweep, written from the loop of DistWorkerCoProc.gc (bifromq-dist-worker/.../DistWorkerCoProc.java:
554-701) over a sorted list of keys, and a brute-force key-ordered window built on sorted() (not a conftest; nothing here is collected).
Python compares bytes as unsigned bytes with a proper prefix first, which is the KV order.  Nothing here calls into the library."""
import bisect


def window(keys, lo=None, n=65536, exclusive=False):
    """keys: the live keys, any order -> (the first n keys >= lo (> lo if exclusive; all if lo is None) in KV order, whether more follow)"""
    ks = sorted(keys)
    at = 0 if lo is None else (bisect.bisect_right(ks, lo) if exclusive else bisect.bisect_left(ks, lo))
    return ks[at:at + n], len(ks) > at + n


def clamp(start_key, boundary):
    """:563-574: a cursor below the boundary's start or at / beyond its end becomes the start (None: seekToFirst)"""
    if start_key is None or boundary is None:
        return start_key
    b0, b1 = boundary
    if (b0 is not None and start_key < b0) or (b1 is not None and start_key >= b1):
        return b0
    return start_key


class _Iter:
    """IKVIterator over a sorted list"""

    def __init__(self, ks):
        self.ks, self.at = ks, len(ks)

    def seek(self, key):
        self.at = bisect.bisect_left(self.ks, key)

    def seek_to_first(self):
        self.at = 0

    def is_valid(self):
        return self.at < len(self.ks)

    def key(self):
        return self.ks[self.at]

    def next(self):
        self.at += 1


def sweep(keys, start_key=None, step_hint=1, scan_quota=0, boundary=None):
    """-> (inspected keys in inspection order, wrapped, nextStartKey or None): the statements of :555-671 one by one"""
    step_used = max(step_hint, 1)
    quota = scan_quota if scan_quota > 0 else 256 * step_used
    itr = _Iter(sorted(keys))
    start_key = clamp(start_key, boundary)
    if start_key is not None:
        itr.seek(start_key)
    else:
        itr.seek_to_first()
    if not itr.is_valid():
        return [], True, None
    inspected, wrapped, session_start = [], False, None
    while True:
        if not itr.is_valid():
            if not wrapped:
                itr.seek_to_first()
                if not itr.is_valid():
                    break
                wrapped = True
            else:
                break
        current = itr.key()
        if wrapped and current == session_start:
            break
        if session_start is None:
            session_start = current
        inspected.append(current)
        if len(inspected) >= quota:
            itr.next()
            break
        skip, off_tail = step_used - 1, False
        while skip > 0:
            skip -= 1
            itr.next()
            if not itr.is_valid():
                off_tail = True
                break
        if off_tail:
            continue
        itr.next()
    return inspected, wrapped, (itr.key() if itr.is_valid() else None)
