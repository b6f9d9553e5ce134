"""IGEV `mixed_precision` off / on, same box, alternating: BASELINE config 5's workload (bench.flavour_workload,
--workload kitti15: the whole IGEVStereo_ddim forward, 1248x384, batch 4, 20 DDIM steps x 32 GRU iterations) timed with
the flag False and True in turn, each forward from the same seed.  Prints one JSON line: per mode the forward times,
pairs/s and ms per GRU iteration (forward / (steps x iterations), the figure config 5's bar is stated in), and the mean /
max |d disparity| of the mixed run against the fp32 run.

    python tools/bench_igev_mixed.py [--rounds 3] [--ddim-steps 20] [--gru-iters 32] [--modes f32,mixed]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1248)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--gru-iters", type=int, default=32)
    ap.add_argument("--modes", default="f32,mixed")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    modes = a.modes.split(",")
    wl = types.SimpleNamespace(workload="kitti15", batch=a.batch, height=a.height, width=a.width,
                               ddim_steps=a.ddim_steps, gru_iters=a.gru_iters)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model, step, what = bench.flavour_workload(wl, 0, dev)

    def run(mode):
        model.args.mixed_precision = mode == "mixed"
        torch.manual_seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            pred, _ = step()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, pred

    preds, times = {}, {m: [] for m in modes}
    for m in modes:                                        # warm-up: plans, packed weights, allocator
        run(m)
    for _ in range(a.rounds):
        for m in modes:
            dt, pred = run(m)
            times[m].append(dt)
            preds[m] = pred
    iters = a.ddim_steps * a.gru_iters
    out = {"tool": "bench_igev_mixed", "workload": what, "rounds": a.rounds, "modes": {}}
    for m in modes:
        best = min(times[m])
        out["modes"][m] = {"forward_s": [round(t, 4) for t in times[m]], "pairs_per_s": round(a.batch / best, 3),
                           "ms_per_gru_iteration": round(1e3 * best / iters, 3)}
    if "f32" in preds and "mixed" in preds:
        d = (preds["mixed"] - preds["f32"]).abs()
        out["mixed_vs_f32_disparity_px"] = {"mean": float(d.mean()), "max": float(d.max())}
        out["speedup"] = round(min(times["f32"]) / min(times["mixed"]), 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
