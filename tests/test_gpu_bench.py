"""bench.py on one GPU as the plain command runs it: the headline line only, none of the `--full` legs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_without_the_full_legs():
    """`bench.py --gpus 1 --steps 1 --warmup 1` at the headline workload (c2, 4096 envs): one JSON line with the headline
    fields and the roofline of its own timed steps; the secondary workloads and the cpu_baseline leg run only with --full"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    j = json.loads(lines[0])
    assert j["unit"] == "env-steps/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["steps"] == 1 and j["warmup"] == 1 and j["n_gpus"] == 1
    assert abs(j["value"] - 4096 * 32 / (j["ms_per_step"] * 1e-3)) < 0.02 * j["value"]
    assert j["roofline"]["launches"] > 0
    assert "secondary" not in j and "cpu_baseline" not in j
