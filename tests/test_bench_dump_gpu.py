"""bench.py --dump-outputs on the device: what the timed path computed in its last step, against the CPU oracle on
the same seeded inputs (bench.py's workload: tree seed 42, database seed 43, reads seed 44)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dumped_outputs_are_the_placements_of_the_step(gpu_available, oracle_lib, tmp_path):
    assert gpu_available
    from epik_amd import synth
    leaves, k, n = 60, 6, 3000
    env = dict(os.environ)
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_TEAM_FRONT", "EPIK_AMD_TEAM_POOL", "EPIK_AMD_MAX_BLOCKS",
                "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(var, None)
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-extras",
           "--cpu-baseline-seconds", "0", "--leaves", str(leaves), "--kmer-size", str(k), "--reads-per-step", str(n),
           "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = {name: np.load(out_dir / f"{name}.npy") for name in ("n_rows", "sample_reads", "branch", "score", "lwr")}
    assert np.array_equal(out["sample_reads"], np.arange(n))   # a step this small is dumped whole

    tree = synth.make_tree(leaves, seed=42)
    db = synth.make_db(tree.num_nodes, kmer_size=k, seed=43)
    data, offs = synth.make_reads(n, 150, seed=44)
    ref_rows, ref_n, _ = oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0)
    assert np.array_equal(out["n_rows"], ref_n)
    valid = np.arange(ref_rows.shape[1])[None, :] < ref_n[:, None]
    assert np.array_equal(out["branch"][valid], ref_rows["branch"][valid])
    assert np.array_equal(out["score"][valid].view(np.uint32), ref_rows["score"][valid].view(np.uint32))
    assert float(np.abs(out["lwr"][valid] - ref_rows["lwr"][valid]).max()) <= 1e-5
    assert (out["branch"][~valid] == -1).all()
