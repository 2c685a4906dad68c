"""A plain bench.py run prints the headline and what the timed steps themselves measured; the CPU baseline and the
other measurements that take runs of their own come with --full only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "build", "cpu_baseline"}


def _line(*extra):
    env = dict(os.environ)
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_TEAM_FRONT", "EPIK_AMD_TEAM_POOL", "EPIK_AMD_MAX_BLOCKS",
                "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(var, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--leaves", "60",
           "--kmer-size", "6", "--reads-per-step", "3000", *extra]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [x for x in run.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_a_plain_run_measures_the_headline_only(gpu_available):
    assert gpu_available
    line = _line()
    assert set(line) == PLAIN_KEYS
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    assert line["roofline"]["achieved"] > 0


@pytest.mark.gpu
def test_full_brings_the_cpu_baseline_back(gpu_available):
    assert gpu_available
    line = _line("--full", "--no-extras", "--cpu-baseline-seconds", "1")
    assert set(line) == PLAIN_KEYS | {"cpu_baseline_1thread"}
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline_1thread"]["value"] > 0
