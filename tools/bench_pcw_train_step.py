"""Time one PWCNet_ddim training step (forward, model_loss_kitti12, backward, Adam) at the reference's training shape --
B = 4 pairs of 256 x 512 (KITTI12/datasets/kitti_dataset.py:51) -- on three routes, alternating runs in one process:
  hip      refinenet3 on train2d.py and the 3-D stack on train3d.py (the default)
  torch2d  DV_TRAIN_CONV2D=torch: refinenet3 on F.conv2d (MIOpen), the 3-D stack on HIP
  torch    both switches torch: every convolution on MIOpen
and time the weight-gradient kernel (csrc/conv2d_wgrad.hip) alone on every layer shape of refinenet3, with its fraction
of the 157.3 TFLOP/s fp32 MFMA peak, next to torch.nn.grad.conv2d_weight (MIOpen's backward-weights) on the same shape.
Writes the record to profiles/pcw_train_step_bench.json (or --out).

    python tools/bench_pcw_train_step.py [--batch 4] [--runs 3] [--out profiles/pcw_train_step_bench.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen routes' many shapes
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffuvolume_amd import PWCNet_ddim, model_loss_kitti12  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402
from diffuvolume_amd.train2d import conv2d_weight_grad  # noqa: E402

PEAK = 157.3e12
ROUTES = {"hip": ("hip", "hip"), "torch2d": ("torch", "hip"), "torch": ("torch", "torch")}   # (CONV2D, CONV3D)


def refine_layers():
    """(name, cin, cout, k, dilation) of every convolution of refinenet3 (pwcnet_ddim.py:251-306)."""
    return [("conv1 146->128 d1", 146, 128, 3, 1), ("conv2 128->128 d1", 128, 128, 3, 1),
            ("conv3 128->128 d2", 128, 128, 3, 2), ("conv4 128->128 d4", 128, 128, 3, 4),
            ("conv5.conv1 128->96 d8", 128, 96, 3, 8), ("conv5.conv2 96->96 d8", 96, 96, 3, 8),
            ("conv5.down 128->96 1x1", 128, 96, 1, 1), ("conv6.conv1 96->64 d16", 96, 64, 3, 16),
            ("conv6.conv2 64->64 d16", 64, 64, 3, 16), ("conv6.down 96->64 1x1", 96, 64, 1, 1),
            ("conv7.conv1 64->32 d1", 64, 32, 3, 1), ("conv7.conv2 32->32 d1", 32, 32, 3, 1),
            ("conv7.down 64->32 1x1", 64, 32, 1, 1), ("conv8 32->1 d1", 32, 1, 3, 1)]


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def time_wgrad(b, h, w, reps=5):
    rows = []
    for name, cin, cout, k, d in refine_layers():
        x = torch.randn(b, cin, h, w, device="cuda")
        g = torch.randn(b, cout, h, w, device="cuda")
        ms = _ms(lambda: conv2d_weight_grad(x, g, k, d, cout), reps)
        pad, dil = (d, d) if k == 3 else (0, 1)
        ms_t = _ms(lambda: torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), g, padding=pad, dilation=dil), reps)
        flop = 2.0 * cout * cin * k * k * b * h * w
        rows.append(dict(layer=name, cin=cin, cout=cout, k=k, dilation=d, ms=round(ms, 4),
                         tflops=round(flop / ms / 1e9, 2), frac_peak=round(flop / ms / 1e9 / (PEAK / 1e12), 3),
                         torch_ms=round(ms_t, 4), hip_over_torch=round(ms / ms_t, 3)))
        print(f"  {name:26s} {ms:8.3f} ms  {flop / ms / 1e9:7.1f} TFLOP/s  {rows[-1]['frac_peak']:.3f} of peak   "
              f"torch {ms_t:8.3f} ms", flush=True)
        del x, g
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pcw_train_step_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    model = PWCNet_ddim(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    x = synth_stereo_batch(a.batch, a.height, a.width, seed=5)
    left, right, gt = (x[k].cuda() for k in ("left", "right", "gt"))
    disp_net = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(a.height // 4, a.width // 4),
                             mode="bilinear") / 4                  # KITTI12/main.py:148-150
    mask = (gt < 192) & (gt > 0)

    def use(route):
        os.environ["DV_TRAIN_CONV2D"], os.environ["DV_TRAIN_CONV3D"] = ROUTES[route]

    def step():
        opt.zero_grad()
        outs = model(left, right, None, disp_net, None)
        loss = model_loss_kitti12(outs, gt, mask)
        loss.backward()
        opt.step()
        return float(loss.detach())

    times = {r: [] for r in ROUTES}
    for route in ROUTES:
        use(route)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
    for _ in range(a.runs):
        for route in ROUTES:
            use(route)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step()
            torch.cuda.synchronize()
            times[route].append((time.perf_counter() - t0) * 1e3)
            print(f"{route:7s} step {times[route][-1]:8.1f} ms  loss {loss:.3f}", flush=True)
    os.environ.pop("DV_TRAIN_CONV2D")
    os.environ.pop("DV_TRAIN_CONV3D")
    print("weight-gradient kernel per refinenet3 layer (batch %d, %dx%d):" % (a.batch, a.height, a.width))
    rows = time_wgrad(a.batch, a.height, a.width)
    med = {r: sorted(v)[len(v) // 2] for r, v in times.items()}
    rec = dict(tool="tools/bench_pcw_train_step.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               batch=a.batch, image=[a.height, a.width], runs=a.runs, warmup=a.warmup,
               miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"), routes={r: dict(zip(("DV_TRAIN_CONV2D",
                                                                                     "DV_TRAIN_CONV3D"), v))
                                                                         for r, v in ROUTES.items()},
               step_ms={r: [round(t, 2) for t in v] for r, v in times.items()},
               step_ms_median={r: round(v, 2) for r, v in med.items()},
               hip_over_torch2d=round(med["hip"] / med["torch2d"], 3), hip_over_torch=round(med["hip"] / med["torch"], 3),
               wgrad_layers=rows, peak_tflops=PEAK / 1e12)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: rec[k] for k in ("step_ms_median", "hip_over_torch2d", "hip_over_torch")}))


if __name__ == "__main__":
    main()
