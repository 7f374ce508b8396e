"""bmq_config.share_carry on the device: the tables' key references are gathered from the old generation in HBM, k_b_find_keys looks the keys
up in the new generation where they lie (the old generation's key pool at bmq_compact_swap, a device copy at bmq_compact), k_sh_rekey
rewrites the directory.  The cases of tests/share_carry_cases.py on device 0; the carried state as the engine reports it -- per key the
URLs, and the resolve rows, which depend on each table's ordered flag -- is compared with the host executor's, the rows with
tests/share_ref.py inside the cases."""
import pytest

from tests import share_carry_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tables", ["none", "one", "all"])
def test_compact_carries_the_tables(tables):
    assert T.case_compact(0, tables) == T.case_compact(-1, tables)


@pytest.mark.parametrize("grow", [False, True])
def test_id_space_shrinks_and_grows(grow):
    assert T.case_id_space(0, grow) == T.case_id_space(-1, grow)


@pytest.mark.parametrize("bounded", [False, True])
def test_swap_carries_the_tables(bounded):
    assert T.case_swap(0, bounded=bounded) == T.case_swap(-1, bounded=bounded)


def test_default_engine_drops_the_tables():
    T.case_swap(0, bounded=False, share_carry=0)


def test_two_thousand_tables_among_twenty_thousand_keys():
    m = T.Model(0, 36, shared=0.14, counts=[1, 2, 5, 17], n_filters=22000, n_topics=60)
    eng = m.eng
    keys = sorted(m.ref())
    assert 1700 < len(m.mirror) < 2600 and 18000 < len(keys) <= 22000
    m.apply([(1, k) for k in keys[::9]] + [(0, T.O.route_key_from_mqtt(m.tenants[i % 2], "more/%d" % i, T.O.receiver_url(0, "m%d" % i, "d0"))) for i in range(500)])
    keep, dropped = m.survivors()
    assert dropped > 100 and len(keep) > 1500
    gen = eng.info().generation
    eng.set_kernel_timing(True)
    eng.compact()
    m.generation_changed(keep, dropped, gen)
    ci = eng.share_carry_info()
    assert ci.ms_gather > 0 and ci.ms_find > 0 and ci.ms_rekey > 0
    # ... and through a swap, with the keys read from the old generation's pool
    eng.compact_begin()
    while eng.compact_poll(8192) < 1000:
        pass
    keep2, dropped2 = m.survivors()
    assert keep2 == keep and dropped2 == 0
    gen = eng.info().generation
    eng.compact_swap()
    m.generation_changed(keep2, 0, gen)
    m.close()
