"""Benchmark of the cost-volume front's training route on the MI355X -> profiles/igev_volume_train_bench.json.

  kernels  each new kernel alone on the shapes it meets at batch 4, 80 x 184, D 48 (the reference's 320 x 736 training
           crop at 1/4): the k4 transposed convolution's input gradient (weight packing included) and weight gradient
           on conv3_up / conv2_up / conv1_up, as a fraction of the fp32 MFMA peak (157.3 TFLOP/s), against the backward
           of F.conv_transpose3d on the same tensors (both gradients in one autograd call: MIOpen); the gate's
           backward on the four gate shapes, as a fraction of the HBM bandwidth (8 TB/s; 12 bytes per volume element:
           g and cv read, dcv written), against the backward of the torch expression.  Alternating in one process,
           ROUNDS rounds of REPS launches after a warm-up, median and spread.
  step     IGEVCostVolume forward + synth.igev_volume_train_loss + backward + AdamW at the same size, HIP route and
           DV_TRAIN_CONV3D=torch alternating, with max_memory_allocated of both.
The record is rewritten after every leg, so a run that is cut short keeps what it measured.

    python tools/bench_igev_volume_train.py [--skip-kernels] [--skip-step] [--rounds 5] [--reps 5] [--step-rounds 3]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from diffuvolume_amd import _build, train3d  # noqa: E402
from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume  # noqa: E402
from diffuvolume_amd.synth import igev_volume_train_inputs, igev_volume_train_loss, synth_state_dict  # noqa: E402

PEAK = 157.3e12                # fp32 MFMA peak of the MI355X
HBM = 8.0e12                   # HBM3E bandwidth (specification)


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def med(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def alternate(legs, rounds, reps):
    t = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            t[n].append(_ms(fn, reps))
    return {n: med(v) for n, v in t.items()}


def time_deconv_layers(batch, d, h, w, rounds, reps):
    out = []
    for name, ci, co, div in (("conv3_up", 48, 32, 8), ("conv2_up", 32, 16, 4), ("conv1_up", 16, 8, 2)):
        dims = (d // div, h // div, w // div)
        x = torch.randn(batch, ci, *dims, device="cuda")
        wt = torch.randn(ci, co, 4, 4, 4, device="cuda") * 0.05
        g = torch.randn(batch, co, *[2 * n for n in dims], device="cuda")
        xs, ws = x.clone().requires_grad_(), wt.clone().requires_grad_()
        y = F.conv_transpose3d(xs, ws, None, stride=2, padding=1)
        legs = {"dgrad": lambda: train3d.deconv3d_k4_input_grad(g, wt),
                "wgrad": lambda: train3d.deconv3d_k4_weight_grad(x, g),
                "torch_backward_both": lambda: torch.autograd.grad(y, (xs, ws), g, retain_graph=True)}
        row = dict(layer=name, cin=ci, cout=co, x_dims=list(dims), **alternate(legs, rounds, reps))
        flop = 2.0 * batch * dims[0] * dims[1] * dims[2] * ci * co * 64
        row["gflop_per_gradient"] = round(flop / 1e9, 2)
        for n in ("dgrad", "wgrad"):
            row[n]["frac_peak"] = round(flop / (row[n]["median_ms"] * 1e-3) / PEAK, 3)
        row["hip_both_over_torch"] = round((row["dgrad"]["median_ms"] + row["wgrad"]["median_ms"])
                                           / row["torch_backward_both"]["median_ms"], 3)
        out.append(row)
        print(f"  {name} {ci}->{co} {dims}: dgrad {row['dgrad']['median_ms']:.3f} ms ({row['dgrad']['frac_peak']} of peak)  "
              f"wgrad {row['wgrad']['median_ms']:.3f} ms ({row['wgrad']['frac_peak']} of peak)  "
              f"torch backward {row['torch_backward_both']['median_ms']:.3f} ms", flush=True)
        del x, wt, g, xs, ws, y
    return out


def time_gates(batch, d, h, w, rounds, reps):
    out = []
    for name, c, div in (("corr_feature_att", 8, 1), ("feature_att_8 / up_8", 16, 2), ("feature_att_16 / up_16", 32, 4),
                         ("feature_att_32", 48, 8)):
        shape = (batch, c, d // div, h // div, w // div)
        cv, g = torch.randn(*shape, device="cuda"), torch.randn(*shape, device="cuda")
        logit = torch.randn(batch, c, shape[3], shape[4], device="cuda")
        cvs, ls = cv.clone().requires_grad_(), logit.clone().requires_grad_()
        y = torch.sigmoid(ls).unsqueeze(2) * cvs
        legs = {"hip": lambda: train3d.feature_gate_grads(cv, logit, g),
                "torch_backward": lambda: torch.autograd.grad(y, (cvs, ls), g, retain_graph=True)}
        row = dict(gate=name, shape=list(shape), **alternate(legs, rounds, reps))
        nbytes = 12.0 * cv.numel()
        row["mbytes"] = round(nbytes / 1e6, 2)
        row["hip"]["frac_hbm"] = round(nbytes / (row["hip"]["median_ms"] * 1e-3) / HBM, 3)
        row["hip_over_torch"] = round(row["hip"]["median_ms"] / row["torch_backward"]["median_ms"], 3)
        out.append(row)
        print(f"  gate {name} {shape}: hip {row['hip']['median_ms']:.4f} ms ({row['hip']['frac_hbm']} of HBM)  "
              f"torch {row['torch_backward']['median_ms']:.4f} ms", flush=True)
        del cv, g, logit, cvs, ls, y
    return out


def time_step(batch, h, w, max_disp, rounds, routes):
    model = IGEVCostVolume(max_disp)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=91, logit_gain=1.0), strict=True)
    model = model.cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    x = igev_volume_train_inputs(seed=43, b=batch, h=h, w=w, max_disp=max_disp, device="cuda")
    leaves = [x["match_left"], x["match_right"], *x["features"]]

    def step():
        opt.zero_grad(set_to_none=True)
        for t in leaves:
            t.grad = None
        geo, init = model(x["match_left"], x["match_right"], x["features"])
        loss = igev_volume_train_loss(geo, init, x)
        loss.backward()
        opt.step()
        return loss

    t, mem = {r: [] for r in routes}, {}
    for route in t:                                   # warm-up of every shape on both routes
        os.environ["DV_TRAIN_CONV3D"] = route
        step()
        torch.cuda.synchronize()
        print(f"  warm-up {route} done", flush=True)
    for _ in range(rounds):
        for route in t:
            os.environ["DV_TRAIN_CONV3D"] = route
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(step, 1))
            mem[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop("DV_TRAIN_CONV3D", None)
    rec = dict(batch=batch, plane=[h, w], disparities=max_disp // 4,
               note="_ms runs the step once untimed before every timed one")
    for route in t:
        rec[route] = dict(**med(t[route]), max_memory_allocated_gib=mem[route])
        print(f"  step {route:5s} {rec[route]['median_ms']:9.1f} ms ({rec[route]['min_ms']:.1f}-{rec[route]['max_ms']:.1f})  "
              f"peak memory {mem[route]} GiB", flush=True)
    if "hip" in rec and "torch" in rec:
        rec["hip_over_torch"] = round(rec["hip"]["median_ms"] / rec["torch"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--width", type=int, default=184)
    ap.add_argument("--max-disp", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--routes", default="hip,torch")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "igev_volume_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), peak_tflops=PEAK / 1e12,
               hbm_tbytes_per_s=HBM / 1e12)

    def save():
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")

    d = a.max_disp // 4
    if not a.skip_kernels:
        print("k4 transposed convolution backward, per layer:", flush=True)
        rec["deconv_k4_layers"] = time_deconv_layers(a.batch, d, a.height, a.width, a.rounds, a.reps)
        save()
        print("gate backward:", flush=True)
        rec["gate_backward"] = time_gates(a.batch, d, a.height, a.width, a.rounds, a.reps)
        save()
    if not a.skip_step:
        print("training step:", flush=True)
        rec["step"] = time_step(a.batch, a.height, a.width, a.max_disp, a.step_rounds, tuple(a.routes.split(",")))
        save()
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
