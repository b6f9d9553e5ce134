"""Benchmark of the upsampling head's training route on the MI355X -> profiles/upsample_train_bench.json.

  wgrad     dv_deconv2d_k4s2_wgrad_f32 on `spx_2_gru.conv1` (32 -> 32, 80x184) and `spx_gru` (64 -> 9, 160x368) at batch 4
            against (a) the fallback -- pixel-unshuffle of g + dv_conv2d_wgrad_cat_f32 on the 3x3 parity form + the gather
            of its 16 live taps -- and (b) MIOpen's backward-weights (torch.nn.grad.conv2d_weight of the stride-2
            convolution whose input gradient the layer is); alternating in one process, ROUNDS rounds, median and spread,
            fraction of the fp32 MFMA peak from the counted 2 * 16 * Cin * Cout * B * h * w flop; the three results are
            compared with each other first
  upsample  dv_context_upsample_f32 / dv_context_upsample_bwd_f32 at batch 4, 80x184 against the torch expression
            (forward; forward + backward), with the counted bytes (40 B per output pixel forward; 76 B per output pixel +
            80 B per cell backward) over the time
  step      forward, loss, backward and an AdamW step of the T = 22 step (synth.igev_upsample_train_step) at batch 4,
            80x184, HIP route and DV_TRAIN_CONV2D=torch alternating, median of STEP_ROUNDS, max_memory_allocated
  parity    the errors that tests/test_gpu_igev_upsample_train.py prints for the two fixture cases, both routes

    python tools/bench_upsample_train.py [--skip-wgrad] [--skip-upsample] [--skip-step] [--skip-parity]"""
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
from diffuvolume_amd import _build  # noqa: E402
from diffuvolume_amd.igev_stereo_ddim import IGEVUpsampler, context_upsample  # noqa: E402
from diffuvolume_amd.synth import (igev_upsample_state_dict, igev_upsample_train_inputs, igev_upsample_train_leaves,  # noqa: E402
                                   igev_upsample_train_step)
from diffuvolume_amd.train2d import conv2d_cat_weight_grad, deconv2d_k4_weight_grad  # noqa: E402

PEAK = 157.3e12                # fp32 MFMA peak of the MI355X
TAP = {0: {0: 1, -1: 3}, 1: {1: 0, 0: 2}}          # output parity -> {input offset: kernel index} (Deconv2dK4S2Plan)


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


def fallback_weight_grad(x, g):
    """dW [Cin,Cout,4,4] through the 3x3 parity form: 9 taps x 4 Cout rows are computed, 16 x Cout of them are live."""
    cin, cout = x.shape[1], g.shape[1]
    dwc = conv2d_cat_weight_grad([x], F.pixel_unshuffle(g, 2), 3).view(cout, 2, 2, cin, 3, 3)
    dw = torch.empty((cin, cout, 4, 4), dtype=torch.float32, device=x.device)
    for a in (0, 1):
        for dy, ky in TAP[a].items():
            for b in (0, 1):
                for dx, kx in TAP[b].items():
                    dw[:, :, ky, kx] = dwc[:, a, b, :, dy + 1, dx + 1].t()
    return dw


def time_wgrad(batch, h, w, rounds, reps):
    out = []
    for name, cin, cout, hh, ww in (("spx_2_gru.conv1", 32, 32, h, w), ("spx_gru", 64, 9, 2 * h, 2 * w)):
        x = torch.randn(batch, cin, hh, ww, device="cuda")
        g = torch.randn(batch, cout, 2 * hh, 2 * ww, device="cuda")
        legs = {"new": lambda: deconv2d_k4_weight_grad(x, g), "fallback_unshuffle_wgrad_cat": lambda: fallback_weight_grad(x, g),
                "miopen": lambda: torch.nn.grad.conv2d_weight(g, (cin, cout, 4, 4), x, stride=2, padding=1)}
        res = {n: fn() for n, fn in legs.items()}
        agree = {n: float(f"{rel(res[n], res['new']):.3e}") for n in legs if n != "new"}
        t = {n: [] for n in legs}
        for _ in range(rounds):
            for n, fn in legs.items():
                t[n].append(_ms(fn, reps))
        flop = 2.0 * 16 * cin * cout * batch * hh * ww
        row = dict(layer=name, cin=cin, cout=cout, plane=[hh, ww], gflop=round(flop / 1e9, 2), rel_l2_against_new=agree)
        for n in legs:
            row[n] = med(t[n])
            row[n]["frac_peak"] = round(flop / (row[n]["median_ms"] * 1e-3) / PEAK, 3)
        row["new_over_fallback"] = round(row["new"]["median_ms"] / row["fallback_unshuffle_wgrad_cat"]["median_ms"], 3)
        row["new_over_miopen"] = round(row["new"]["median_ms"] / row["miopen"]["median_ms"], 3)
        out.append(row)
        print(f"  {name:16s} new {row['new']['median_ms']:.3f} ms ({row['new']['frac_peak']:.3f} of peak, "
              f"{row['new']['min_ms']:.3f}-{row['new']['max_ms']:.3f})  fallback "
              f"{row['fallback_unshuffle_wgrad_cat']['median_ms']:.3f}  MIOpen {row['miopen']['median_ms']:.3f}  "
              f"agreement {agree}", flush=True)
    return out


def time_upsample(batch, h, w, rounds, reps):
    disp = (torch.randn(batch, 1, h, w, device="cuda").abs() * 4).requires_grad_(True)
    logits = (torch.randn(batch, 9, 4 * h, 4 * w, device="cuda") * 2).requires_grad_(True)
    cot = torch.randn(batch, 4 * h, 4 * w, device="cuda")
    pix, cells = batch * 16 * h * w, batch * h * w

    def fwd_bwd():
        disp.grad = logits.grad = None
        context_upsample(disp, logits, scale=4.0, apply_softmax=True).backward(cot)

    def fwd():
        with torch.no_grad():
            context_upsample(disp, logits, scale=4.0, apply_softmax=True)

    from diffuvolume_amd import _lib
    d0, l0 = disp.detach(), logits.detach()
    d_w, d_d = torch.empty_like(l0), torch.empty_like(d0)
    sums = torch.empty(batch, 9, h, w, device="cuda")

    def bwd_kernels():                     # the two launches of the backward alone, on preallocated buffers
        _lib.check(_lib.load().dv_context_upsample_bwd_f32(d0.data_ptr(), l0.data_ptr(), cot.data_ptr(), d_w.data_ptr(),
                                                           d_d.data_ptr(), sums.data_ptr(), batch, h, w, 4.0, 1,
                                                           _lib.stream_ptr()), "dv_context_upsample_bwd_f32")

    t = {k: [] for k in ("hip_fwd", "hip_bwd_kernels", "hip_fwd_bwd", "torch_fwd", "torch_fwd_bwd")}
    for _ in range(rounds):
        for route in ("hip", "torch"):
            os.environ["DV_TRAIN_CONV2D"] = route
            if route == "hip":
                t["hip_fwd"].append(_ms(fwd, 5 * reps))
                t["hip_bwd_kernels"].append(_ms(bwd_kernels, 5 * reps))
            else:                          # the torch expression is taken under grad mode without a backward
                t["torch_fwd"].append(_ms(lambda: context_upsample(disp, logits, scale=4.0, apply_softmax=True), reps))
            t[route + "_fwd_bwd"].append(_ms(fwd_bwd, reps))      # through autograd: includes its host overhead
    os.environ.pop("DV_TRAIN_CONV2D", None)
    rec = dict(batch=batch, plane=[h, w], **{k: med(v) for k, v in t.items()})
    fwd_bytes, bwd_bytes = 40.0 * pix + 4.0 * cells, 76.0 * pix + 80.0 * cells      # cells: disp, d_disp, the sums twice
    rec["counted_bytes_per_output_pixel"] = dict(fwd=round(fwd_bytes / pix, 2), bwd=round(bwd_bytes / pix, 2))
    rec["achieved_tb_per_s"] = dict(fwd=round(fwd_bytes / (rec["hip_fwd"]["median_ms"] * 1e-3) / 1e12, 2),
                                    bwd=round(bwd_bytes / (rec["hip_bwd_kernels"]["median_ms"] * 1e-3) / 1e12, 2))
    print("  context_upsample:", {k: v for k, v in rec.items() if k not in ("batch", "plane")}, flush=True)
    return rec


def time_step(batch, h, w, iters, rounds, routes=("hip", "torch")):
    model = IGEVUpsampler()
    model.load_state_dict(igev_upsample_state_dict(model.state_dict(), 93), strict=True)
    model = model.cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    x = igev_upsample_train_inputs(51, batch, h, w, iters, device="cuda")
    pix = batch * h * w
    iter_flop = 3 * 2.0 * pix * (32 * 32 * 16 + 4 * 64 * 64 * 9 + 4 * 64 * 9 * 16)       # forward + both gradients

    def step():
        opt.zero_grad(set_to_none=True)
        for t in igev_upsample_train_leaves(x).values():
            t.grad = None
        loss, *_ = igev_upsample_train_step(model, x)
        loss.backward()
        opt.step()
        return loss

    t, mem = {r: [] for r in routes}, {}
    for route in routes:                              # warm-up of every shape on both routes
        os.environ["DV_TRAIN_CONV2D"] = route
        step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for route in routes:
            os.environ["DV_TRAIN_CONV2D"] = route
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(step, 1))
            mem[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop("DV_TRAIN_CONV2D", None)
    rec = dict(batch=batch, plane=[h, w], iters=iters, counted_gflop_per_iteration=round(iter_flop / 1e9, 1))
    for route in routes:
        rec[route] = dict(**med(t[route]), max_memory_allocated_gib=mem[route])
        print(f"  step {route:5s} {rec[route]['median_ms']:8.1f} ms ({rec[route]['min_ms']:.1f}-{rec[route]['max_ms']:.1f})  "
              f"peak memory {mem[route]} GiB", flush=True)
    if "hip" in rec and "torch" in rec:
        rec["hip_over_torch"] = round(rec["hip"]["median_ms"] / rec["torch"]["median_ms"], 3)
    return rec


def parity():
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import pytest
    import test_gpu_igev_upsample_train as T
    with np.load(ROOT / "tests" / "golden" / "igev_upsample_train.npz") as z:
        gold = {k: z[k] for k in z.files}
    mp, out = pytest.MonkeyPatch(), {}
    try:
        for case in ("even", "odd"):
            out[case] = dict(bar={k: float(f"{2 * float(gold[f'{case}_ref_err'][i]) + 1e-6:.3e}") for i, k in enumerate(T.KINDS)})
            for route in ("hip", "torch"):
                mp.setenv("DV_TRAIN_CONV2D", route)
                rows = T.parity_rows(gold, case, T.train_step(T.fresh_model(gold), T.case_of(gold, case)))
                out[case][route] = {k: float(f"{max(r[1] for r in rows[k]):.3e}") for k in T.KINDS}
    finally:
        mp.undo()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--width", type=int, default=184)
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--skip-wgrad", action="store_true")
    ap.add_argument("--skip-upsample", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--routes", default="hip,torch", help="routes of the step leg (a profiler run wants one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "upsample_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = dict(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), peak_tflops=PEAK / 1e12)
    if not a.skip_parity:
        rec["parity"] = parity()
        print("parity (worst relative L2 against float64 per kind):", rec["parity"], flush=True)
    if not a.skip_wgrad:
        print("weight gradient of the transposed convolutions:", flush=True)
        rec["wgrad"] = time_wgrad(a.batch, a.height, a.width, a.rounds, a.reps)
    if not a.skip_upsample:
        rec["context_upsample"] = time_upsample(a.batch, a.height, a.width, a.rounds, a.reps)
    if not a.skip_step:
        print("training step:", flush=True)
        rec["step"] = time_step(a.batch, a.height, a.width, a.iters, a.step_rounds, tuple(a.routes.split(",")))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
