"""A plain `bench.py` run on the GPU: set-up, warm-up, the timed steps and the contract line, nothing else -- the
per-kernel pass, the CPU baseline with its parity legs and the side measurements are left to `--full`."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_bench_line_is_the_timed_steps_only():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--height", "128", "--width", "256"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-6
    assert d["epe_px"] == d["epe_px"] and d["timing"]["ms_per_step_with_kernel_events"] is None
    for k in ("roofline", "roofline_kernels", "kernels_ms_per_step", "cpu_baseline", "parity_vs_oracle",
              "parity_vs_oracle_calibrated", "extras"):
        assert k not in d, k
    # what the run spends outside its warm-up and timed steps: start-up, set-up and the line (a plain run's budget is 30 s
    # at the full size; this small frame needs less)
    assert wall - 3 * d["ms_per_step"] / 1e3 < 30.0, wall
