"""bench.py --dump-outputs on the GPU: what the last timed step of the hot path computed, written after the timed steps;
two runs with the same arguments see the same inputs and write the same arrays (the timed steps' random draws are seeded
after the warm-up, so a second warm-up step changes nothing either)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_bench_dump_outputs_repeat(tmp_path):
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    lines = []
    for run, warmup in (("a", "1"), ("b", "2")):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", warmup, "--batch", "2",
                            "--height", "128", "--width", "256", "--no-cpu-baseline", "--no-extras", "--no-kernel-timer",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=800, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(_json_line(r.stdout))
    d = lines[0]
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    names = {"final_disparity", "ddim_stack", "gwc_volume", "image_metric_sums"}
    assert set(d["dump_outputs"]["arrays"]) == names
    assert d["dump_outputs"]["arrays"]["final_disparity"]["shape"] == [2, 128, 256]
    for n in names:
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all()
        assert np.allclose(a, b, rtol=1e-5, atol=1e-5), n
