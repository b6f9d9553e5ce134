"""Time one ACVNet_DDIM training step (forward, model_loss_train, backward, Adam) at the reference's training shape --
B = 4 pairs of 256 x 512 (SceneFlow/datasets/sceneflow_dataset.py:41), a 48 x 64 x 128 cost volume -- on the HIP route
of train3d.py and on the F.conv3d / F.conv_transpose3d route (MIOpen), alternating runs in one process, and time the
weight-gradient kernel (csrc/conv3d_wgrad.hip) alone on every 3-D layer shape of the step, with its fraction of the
157.3 TFLOP/s fp32 MFMA peak.  Writes the record to profiles/train_step_bench.json (or --out).

    python tools/bench_train_step.py [--batch 4] [--runs 3] [--out profiles/train_step_bench.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen route's many 3-D shapes
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from diffuvolume_amd import ACVNet_DDIM, model_loss_train  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402
from diffuvolume_amd.train3d import conv3d_weight_grad  # noqa: E402

PEAK = 157.3e12


def wgrad_layers(b):
    """(name, cin, cout, k, stride, x dims) of every 3-D convolution weight gradient in a step; transposed convs are the
    stride-2 form with x and g exchanged (x = their output gradient)."""
    full, half, quarter = (48, 64, 128), (24, 32, 64), (12, 16, 32)
    return [("dres0.0 64->32", 64, 32, 3, 1, full), ("dres1_att_.0 40->32", 40, 32, 3, 1, full),
            ("32->32 (x11)", 32, 32, 3, 1, full), ("conv1 32->64 s2", 32, 64, 3, 2, full),
            ("conv2 64->64", 64, 64, 3, 1, half), ("conv3 64->128 s2", 64, 128, 3, 2, half),
            ("conv4 128->128", 128, 128, 3, 1, quarter), ("conv5 deconv 128->64", 64, 128, 3, 2, half),
            ("conv6 deconv 64->32", 32, 64, 3, 2, full), ("redir1 32->32 1x1", 32, 32, 1, 1, full),
            ("redir2 64->64 1x1", 64, 64, 1, 1, half), ("final1x1 128->128", 128, 128, 1, 1, quarter),
            ("classif 32->1", 32, 1, 3, 1, full)]


def time_wgrad(b, reps=5):
    rows = []
    for name, cin, cout, k, s, dims in wgrad_layers(b):
        out = [(n + 2 * ((k - 1) // 2) - k) // s + 1 for n in dims]
        x = torch.randn(b, cin, *dims, device="cuda")
        g = torch.randn(b, cout, *out, device="cuda")
        conv3d_weight_grad(x, g, k, s, cout)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            conv3d_weight_grad(x, g, k, s, cout)
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / reps
        flop = 2.0 * cout * cin * k ** 3 * b * out[0] * out[1] * out[2]
        rows.append(dict(layer=name, cin=cin, cout=cout, k=k, stride=s, x_dims=list(dims), ms=round(ms, 4),
                         tflops=round(flop / ms / 1e9, 2), frac_peak=round(flop / ms / 1e9 / (PEAK / 1e12), 3)))
        print(f"  {name:24s} {ms:8.3f} ms  {flop / ms / 1e9:7.1f} TFLOP/s  {rows[-1]['frac_peak']:.3f} of peak", flush=True)
        del x, g
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_step_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    model = ACVNet_DDIM(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    x = synth_stereo_batch(a.batch, a.height, a.width, seed=5)
    left, right, disp, gt = (x[k].cuda() for k in ("left", "right", "disp", "gt"))
    mask = (gt < 192) & (gt > 0)

    def step():
        opt.zero_grad()
        outs = model(left, right, None, disp, None)
        loss = model_loss_train(outs, gt, mask)
        loss.backward()
        opt.step()
        return float(loss.detach())

    times = {"hip": [], "torch": []}
    for route in ("hip", "torch"):
        os.environ["DV_TRAIN_CONV3D"] = route
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
    for _ in range(a.runs):
        for route in ("hip", "torch"):
            os.environ["DV_TRAIN_CONV3D"] = route
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step()
            torch.cuda.synchronize()
            times[route].append((time.perf_counter() - t0) * 1e3)
            print(f"{route:5s} step {times[route][-1]:8.1f} ms  loss {loss:.3f}", flush=True)
    os.environ.pop("DV_TRAIN_CONV3D")
    print("weight-gradient kernel per layer (batch %d):" % a.batch)
    rows = time_wgrad(a.batch)
    med = {r: sorted(v)[len(v) // 2] for r, v in times.items()}
    rec = dict(tool="tools/bench_train_step.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               batch=a.batch, image=[a.height, a.width], runs=a.runs, warmup=a.warmup,
               miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               step_ms={r: [round(t, 2) for t in v] for r, v in times.items()},
               step_ms_median={r: round(v, 2) for r, v in med.items()},
               hip_over_torch=round(med["hip"] / med["torch"], 3), wgrad_layers=rows,
               peak_tflops=PEAK / 1e12)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: rec[k] for k in ("step_ms_median", "hip_over_torch")}))


if __name__ == "__main__":
    main()
