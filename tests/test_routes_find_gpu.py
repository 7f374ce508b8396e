"""bmq_routes_find on the device: the gfx950 kernel k_b_find_keys (bifromq_amd/csrc/bmq_exec_dev.h) over the HBM-resident index, through the
table of tests/routes_find_cases.py -- a device engine and a host-only engine in lockstep through every index state, each answer compared
with the dict key -> id of its own Engine.route_keys and the two executors' answers id for id."""
import numpy as np
import pytest

import bifromq_amd as B
from tests import routes_find_cases as T

pytestmark = pytest.mark.gpu


def test_lookup_table_on_the_device_and_against_the_host_executor():
    dev, host = B.Engine(device=0), B.Engine(device=-1)
    counts = T.Scenario([dev, host]).run()
    for cls in T.expected_classes():
        assert counts[cls] > 0, cls
    dev.close()
    host.close()


def test_a_grid_that_strides():
    """more keys than one round of the bounded grid holds (4096 one-wave workgroups x 64 lanes), every one checked; empty batch; no index"""
    eng = B.Engine(device=0)
    assert eng.find_routes([]).tolist() == []
    assert eng.find_routes([T.K(b"x", "a")]).tolist() == [T.NONE]
    keys = sorted(T.K(b"t%d" % (i % 7), "s/%d/%d" % (i % 251, i), "0\0in%d\0d" % (i % 3)) for i in range(20000))
    eng.rebuild(keys)
    n = 4096 * 64 + 70
    rnd = np.random.RandomState(3)
    pick = rnd.randint(0, len(keys) + 500, size=n)
    absent = T.K(b"t1", "s/never")
    got = eng.find_routes([keys[i] if i < len(keys) else absent for i in pick.tolist()])
    exp = np.where(pick < len(keys), pick, T.NONE).astype(np.uint32)
    assert (got == exp).all()
    eng.close()
