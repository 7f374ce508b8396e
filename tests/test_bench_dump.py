"""bench.py --dump-outputs: the files dump_outputs writes from a CSR (row pointers + ids ascending inside a row) hold exactly the rows
they name, in float64, within the size bound, and the same CSR gives the same bytes (CPU tensors: the helper only gathers and copies)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("count_rows", "match_counts", "id_rows", "route_ids")


@pytest.mark.parametrize("n", [1000, 100_000, (1 << 20) + 4321])
def test_dump_outputs_writes_the_rows_it_names(tmp_path, n):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 40, n)
    rp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ids = rng.integers(0, 10_000_000, int(rp[-1])).astype(np.int32)
    d_ids = torch.from_numpy(np.concatenate([ids, np.full(64, -1, np.int32)]))  # (a buffer longer than the result, as the engine's)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), torch.from_numpy(rp), d_ids, n, torch, np)
    f = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in NAMES}
    assert all(v.dtype == np.float64 for v in f.values())
    cr, ir = f["count_rows"].astype(np.int64), f["id_rows"].astype(np.int64)
    assert len(cr) == min(n, 1 << 20) and (np.diff(cr) > 0).all() and (f["match_counts"] == cnt[cr]).all()
    assert len(ir) == min(n, 1 << 16) and (np.diff(ir) > 0).all() and np.isin(ir, cr).all()
    assert (f["route_ids"] == np.concatenate([ids[rp[r]:rp[r + 1]] for r in ir])[:1 << 22]).all()
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in NAMES) <= 64 << 20
    for k in NAMES:
        assert (tmp_path / "a" / (k + ".npy")).read_bytes() == (tmp_path / "b" / (k + ".npy")).read_bytes()
