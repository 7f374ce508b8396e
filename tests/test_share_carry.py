"""bmq_config.share_carry on a host-only engine: bmq_compact and bmq_compact_swap carry the member tables of shared subscriptions to the
ids their route KEYS get in the new generation (Share::carry_prepare / carry_finish, bifromq_amd/csrc/bmq_share.h, over the host
executor: the per-key lookup find_key_one and the directory rewrite sh_rekey_one that the gfx950 kernels k_b_find_keys / k_sh_rekey
wrap).  The cases and the model are tests/share_carry_cases.py; tests/test_share_carry_gpu.py runs them on the device."""
import ctypes as C

import pytest

import bifromq_amd as B
from bifromq_amd import _lib
from tests import share_carry_cases as T


@pytest.mark.parametrize("tables", ["none", "one", "all"])
def test_compact_carries_the_tables(tables):
    T.case_compact(-1, tables)


@pytest.mark.parametrize("grow", [False, True])
def test_id_space_shrinks_and_grows(grow):
    T.case_id_space(-1, grow)


def test_swap_carries_tables_given_while_the_next_generation_is_built():
    T.case_swap(-1, bounded=False)


def test_bounded_swap_carries_inside_and_drops_outside():
    T.case_swap(-1, bounded=True)


def test_default_engine_drops_the_tables():
    """share_carry = 0: the same sequence ends without a table, and nothing is reported as carried"""
    T.case_swap(-1, bounded=False, share_carry=0)
    m = T.Model(-1, 34, share_carry=0, n_filters=120)
    assert m.eng.share_info().n_tables > 10
    m.eng.compact()
    assert m.eng.share_info().n_tables == 0 and m.eng.share_carry_info().status == 0
    m.close()


def test_rebuild_drops_the_tables_also_with_the_switch():
    m = T.Model(-1, 35, n_filters=120)
    keys = sorted(m.ref())
    assert m.eng.share_info().n_tables > 10
    m.eng.rebuild(keys)
    assert m.eng.share_info().n_tables == 0 and m.eng.share_carry_info().status == 0
    m.close()


def test_the_switch_is_the_last_word_of_the_config():
    assert C.sizeof(_lib.Config) == 13 * 4 and _lib.Config.share_carry.offset == 12 * 4
    with pytest.raises(B.BmqError) as ex:
        B.Engine(device=-1, share_carry=2)
    assert ex.value.code == -1


def test_share_carry_info_mirror_has_the_layout_of_the_header(tmp_path):
    """_lib.ShareCarryInfo restates bmq_share_carry_info: same size, every field at the same offset"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "bmq.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bmq_share_carry_info));']
    lines += ['printf("%s %%zu\\n", offsetof(bmq_share_carry_info, %s));' % (f, f) for f, _ in _lib.ShareCarryInfo._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ['return 0;', '}']))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.ShareCarryInfo)
    for f, _ in _lib.ShareCarryInfo._fields_:
        assert int(got[f]) == getattr(_lib.ShareCarryInfo, f).offset, f
