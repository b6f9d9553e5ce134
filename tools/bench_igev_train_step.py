"""Benchmark of IGEVStereo_ddim's training step on the MI355X -> profiles/igev_train_step_bench.json.

  step      forward_train, loss.sequence_loss, backward and an AdamW step at batch 4, 320 x 736, 22 iterations (the
            KITTI15 crop of train_stereo.py), after freeze_bn(); the HIP route and DV_TRAIN_CONV2D=torch (the 2-D
            convolutions, InstanceNorm and the convex upsampling on their torch expressions / MIOpen) alternating in one
            process, median of STEP_ROUNDS, max_memory_allocated per route
  fewin     dv_conv2d_fewin_wgrad_f32 on `stem_2[0]` (3 -> 32, k3, s2) and `cnet.conv1` (3 -> 64, k7, s2) at batch 4,
            320 x 736 against MIOpen's backward-weights (torch.nn.grad.conv2d_weight); counted flop 2 Cout Cin k k B Ho Wo
            and bytes (x + g read once, dw written) over the time
  inorm     dv_instance_norm_act_bwd_f32 on the front's largest planes (32 x 160 x 368, 48 x 80 x 184) at batch 4 against
            torch's instance_norm + leaky_relu backward; counted bytes (x, g read once, dx written: 12 B per element)
No target is fixed: the figures are reported against the torch route.

    python tools/bench_igev_train_step.py [--skip-step] [--skip-kernels] [--batch 4 --height 320 --width 736 --iters 22]"""
import argparse
import json
import os
import statistics
import sys
import types
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from diffuvolume_amd import _build, train2d  # noqa: E402
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim  # noqa: E402
from diffuvolume_amd.loss import sequence_loss  # noqa: E402
from diffuvolume_amd.submodule import ACT_LEAKY  # noqa: E402
from diffuvolume_amd.synth import (IGEV_TRAIN_ARGS, IGEV_TRAIN_WEIGHT_SEED, StubMobileNetV2, igev_train_step_inputs,  # noqa: E402
                                   synth_state_dict)

PEAK = 157.3e12                # fp32 MFMA / VALU peak of the MI355X
STEP_ROUNDS, ROUNDS = 5, 5


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


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def alternate(legs, rounds, reps):
    t = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            t[n].append(_ms(fn, reps))
    return {n: med(v) for n, v in t.items()}


def time_fewin(batch, h, w):
    out = []
    for name, cout, k in (("stem_2.0.conv", 32, 3), ("cnet.conv1", 64, 7)):
        x = torch.randn(batch, 3, h, w, device="cuda")
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        g = torch.randn(batch, cout, ho, wo, device="cuda")
        legs = {"new": lambda: train2d.conv2d_fewin_weight_grad(x, g, k, 2),
                "miopen": lambda: torch.nn.grad.conv2d_weight(x, (cout, 3, k, k), g, stride=2, padding=k // 2)}
        agree = rel(legs["miopen"](), legs["new"]())
        flop = 2.0 * cout * 3 * k * k * batch * ho * wo
        nbytes = 4.0 * (x.numel() + g.numel() + cout * 3 * k * k)
        row = dict(layer=name, cout=cout, k=k, plane=[h, w], gflop=round(flop / 1e9, 2), mbytes=round(nbytes / 1e6, 1),
                   miopen_rel_l2_against_new=float(f"{agree:.3e}"), **alternate(legs, ROUNDS, 20))
        for n in legs:
            row[n]["frac_peak"] = round(flop / (row[n]["median_ms"] * 1e-3) / PEAK, 3)
            row[n]["tb_per_s"] = round(nbytes / (row[n]["median_ms"] * 1e-3) / 1e12, 3)
        row["new_over_miopen"] = round(row["new"]["median_ms"] / row["miopen"]["median_ms"], 3)
        out.append(row)
        print(f"  {name:14s} new {row['new']['median_ms']:.3f} ms ({row['new']['frac_peak']:.3f} of peak, "
              f"{row['new']['tb_per_s']:.2f} TB/s)  MIOpen {row['miopen']['median_ms']:.3f} ms  agreement {agree:.2e}", flush=True)
    return out


def time_inorm(batch, h, w):
    out = []
    for name, c, hh, ww in (("stem_2 (1/2)", 32, h // 2, w // 2), ("stem_4 (1/4)", 48, h // 4, w // 4)):
        x = torch.randn(batch, c, hh, ww, device="cuda").requires_grad_(True)
        cot = torch.randn(batch, c, hh, ww, device="cuda")

        def run(route):
            def fn():
                os.environ["DV_TRAIN_CONV2D"] = route
                x.grad = None
                train2d.instance_norm_act(x, ACT_LEAKY, 1e-5).backward(cot)
            return fn

        def fwd(route):
            def fn():
                os.environ["DV_TRAIN_CONV2D"] = route
                with torch.no_grad():
                    train2d.instance_norm_act(x, ACT_LEAKY, 1e-5)
            return fn

        legs = {"new_fwd_bwd": run("hip"), "torch_fwd_bwd": run("torch"), "new_fwd": fwd("hip"), "torch_fwd": fwd("torch")}
        legs["torch_fwd_bwd"]()
        ref = x.grad.clone()
        legs["new_fwd_bwd"]()
        agree = rel(x.grad, ref)
        row = dict(planes=name, shape=[batch, c, hh, ww], torch_rel_l2_against_new=float(f"{agree:.3e}"),
                   **alternate(legs, ROUNDS, 20))
        nbytes = 12.0 * x.numel()
        for r in ("new", "torch"):
            bwd = row[f"{r}_fwd_bwd"]["median_ms"] - row[f"{r}_fwd"]["median_ms"]
            row[f"{r}_bwd_ms"] = round(bwd, 4)
            row[f"{r}_bwd_tb_per_s"] = round(nbytes / (bwd * 1e-3) / 1e12, 3)
        os.environ.pop("DV_TRAIN_CONV2D", None)
        out.append(row)
        print(f"  {name:14s} backward new {row['new_bwd_ms']:.3f} ms ({row['new_bwd_tb_per_s']:.2f} TB/s counted)  torch "
              f"{row['torch_bwd_ms']:.3f} ms  agreement {agree:.2e}", flush=True)
    return out


def time_step(batch, h, w, iters):
    args = types.SimpleNamespace(**IGEV_TRAIN_ARGS)
    x = igev_train_step_inputs(seed=83, b=batch, h=h, w=w, iters=iters, t=400, device="cuda")
    res = {}
    state = {}
    for route in ("hip", "torch"):
        m = IGEVStereo_ddim(args, feature=Feature(StubMobileNetV2()))
        m.load_state_dict(synth_state_dict(m.state_dict(), seed=IGEV_TRAIN_WEIGHT_SEED), strict=True)
        m = m.cuda().train()
        m.freeze_bn()
        state[route] = (m, torch.optim.AdamW(m.parameters(), lr=1e-6))

    def step(route):
        m, opt = state[route]
        os.environ["DV_TRAIN_CONV2D"] = route
        opt.zero_grad(set_to_none=True)
        init, preds = m.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=iters, t=x["t"],
                                      noise=x["noise"])
        loss, _ = sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=args.max_disp)
        loss.backward()
        opt.step()
        return float(loss)

    t = {"hip": [], "torch": []}
    for route in t:                                                    # warm-up: plans, MIOpen's find
        res[f"{route}_first_loss"] = step(route)
    for _ in range(STEP_ROUNDS):
        for route in t:
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(lambda: step(route), 1))
            res[f"{route}_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop("DV_TRAIN_CONV2D", None)
    for route in t:
        res[route] = med(t[route])
    res["hip_over_torch"] = round(res["hip"]["median_ms"] / res["torch"]["median_ms"], 3)
    print(f"  step: HIP {res['hip']['median_ms']:.1f} ms, {res['hip_peak_gib']} GiB;  torch route "
          f"{res['torch']['median_ms']:.1f} ms, {res['torch_peak_gib']} GiB", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=736)
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = dict(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), batch=a.batch, plane=[a.height, a.width],
               iters=a.iters)
    if not a.skip_kernels:
        print("few-input-channel weight gradient", flush=True)
        out["fewin_wgrad"] = time_fewin(a.batch, a.height, a.width)
        print("InstanceNorm + LeakyReLU backward", flush=True)
        out["instance_norm_bwd"] = time_inorm(a.batch, a.height, a.width)
    if not a.skip_step:
        print("training step", flush=True)
        out["step"] = time_step(a.batch, a.height, a.width, a.iters)
    dest = ROOT / "profiles" / "igev_train_step_bench.json"
    dest.write_text(json.dumps(out, indent=1) + "\n")
    print(f"wrote {dest}")


if __name__ == "__main__":
    main()
