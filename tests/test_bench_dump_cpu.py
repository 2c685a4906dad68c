"""bench.py --dump-outputs on the host: the rows the device buffers hold, decoded from include/epik_amd.h's layout,
the slots past a read's row count masked, the sample fixed from run to run, every array float32 or float64."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _buffers(n, keep, seed=0):
    """Row buffers shaped as bench.py allocates them (16 bytes per row, n_rows int32), filled like a step's output:
    junk past every read's row count."""
    import torch

    from epik_amd import capi
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, keep), dtype=capi.PLACEMENT)
    rows["branch"] = rng.integers(0, 999, size=(n, keep))
    rows["score"] = rng.standard_normal((n, keep)).astype(np.float32)
    rows["lwr"] = rng.random((n, keep))
    n_rows = rng.integers(0, keep + 1, size=n).astype(np.int32)
    d_rows = torch.from_numpy(rows.reshape(-1).view(np.float64).copy())
    return rows, n_rows, d_rows, torch.from_numpy(n_rows.copy())


def test_dump_outputs_writes_the_rows_of_every_read(tmp_path):
    import bench
    n, keep = 300, 7
    rows, n_rows, d_rows, d_nrows = _buffers(n, keep)
    names = bench.dump_outputs(str(tmp_path), d_rows, d_nrows, n, keep)
    assert names == ["branch", "lwr", "n_rows", "sample_reads", "score"]
    out = {name: np.load(tmp_path / f"{name}.npy") for name in names}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["n_rows"], n_rows) and np.array_equal(out["sample_reads"], np.arange(n))
    valid = np.arange(keep)[None, :] < n_rows[:, None]
    assert np.array_equal(out["branch"][valid], rows["branch"][valid])
    assert np.array_equal(out["score"][valid].view(np.uint32), rows["score"][valid].view(np.uint32))
    assert np.array_equal(out["lwr"][valid], rows["lwr"][valid])
    assert (out["branch"][~valid] == -1).all() and (out["score"][~valid] == 0).all() and (out["lwr"][~valid] == 0).all()


def test_dump_outputs_samples_a_large_step_the_same_way_every_time(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE_READS", 50)
    n, keep = 400, 5
    rows, n_rows, d_rows, d_nrows = _buffers(n, keep, seed=1)
    # (a longer buffer than the reads finished: the rows of the first n_out reads only)
    bench.dump_outputs(str(tmp_path / "a"), d_rows, d_nrows, 300, keep)
    bench.dump_outputs(str(tmp_path / "b"), d_rows, d_nrows, 300, keep)
    for name in ("n_rows", "sample_reads", "branch", "score", "lwr"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))
    sample = np.load(tmp_path / "a" / "sample_reads.npy").astype(np.int64)
    assert len(sample) == 50 and (np.diff(sample) > 0).all() and sample.max() < 300
    assert np.array_equal(np.load(tmp_path / "a" / "n_rows.npy"), n_rows[:300])
    branch = np.load(tmp_path / "a" / "branch.npy")
    valid = np.arange(keep)[None, :] < n_rows[sample][:, None]
    assert np.array_equal(branch[valid], rows["branch"][sample][valid])


def test_dump_outputs_refuses_more_than_64_mb(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    _, _, d_rows, d_nrows = _buffers(100, 7)
    with pytest.raises(SystemExit, match="--dump-outputs"):
        bench.dump_outputs(str(tmp_path), d_rows, d_nrows, 100, 7)
    assert not os.listdir(tmp_path)
