"""bmq_routes_find (Engine.find_routes): route keys -> route ids, batched, read-only -- on a host-only engine, which runs the per-key
function the gfx950 kernel k_b_find_keys wraps (find_key_one, bifromq_amd/csrc/bmq_build_core.h) on host threads.  The table -- tenants,
filters, receiver sets, absent keys, index states, batch sizes, errors -- is tests/routes_find_cases.py; tests/test_routes_find_gpu.py runs
it on the device."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import routes_find_cases as T


def test_lookup_table_on_the_host_executor():
    counts = T.Scenario([B.Engine(device=-1)]).run()
    for cls in T.expected_classes():
        assert counts[cls] > 0, cls


def test_empty_batches_and_an_engine_without_an_index():
    eng = B.Engine(device=-1)
    assert eng.find_routes([]).tolist() == []
    assert eng.find_routes([T.K(b"x", "a")]).tolist() == [T.NONE]  # no index yet: nothing is live
    for bad in T.malformed():  # ... and a malformed key is refused all the same
        with pytest.raises(B.BmqError) as ex:
            eng.find_routes([T.K(b"x", "a"), bad])
        assert ex.value.code == -1
    eng.rebuild([])
    assert eng.find_routes([T.K(b"x", "a"), T.K(b"", "#")]).tolist() == [T.NONE, T.NONE]
    eng.apply([(0, T.K(b"", "#"))])
    assert eng.find_routes([T.K(b"x", "a"), T.K(b"", "#"), T.K(b"", "#")]).tolist() == [T.NONE, 0, 0]
    eng.close()


def test_an_open_async_batch_is_completed_first():
    eng = B.Engine(device=-1).rebuild([T.K(b"x", "a")])
    eng.apply_async([(0, T.K(b"x", "b")), (1, T.K(b"x", "a"))])
    assert eng.find_routes([T.K(b"x", "a"), T.K(b"x", "b")]).tolist() == [T.NONE, 1]
    eng.close()


def test_ids_of_the_puts_of_a_batch():
    """what the call is for: the ids of the keys a batch put, where some were there already (they keep their ids) and one is put twice"""
    base = sorted(T.K(b"t", "f/%d" % i) for i in range(10))
    eng = B.Engine(device=-1).rebuild(base)
    batch = [T.K(b"t", "new/1"), base[4], T.K(b"t", "new/2"), T.K(b"t", "new/1"), base[0]]
    eng.apply([(0, k) for k in batch])
    ids = eng.find_routes(batch)
    assert ids[1] == 4 and ids[4] == 0 and ids[0] == ids[3] and len({int(ids[0]), int(ids[2])}) == 2 and min(ids[0], ids[2]) >= 10
    assert eng.route_keys(ids) == batch
    assert ids.dtype == np.uint32
    eng.close()
