"""Benchmark of mixed-precision training of IGEV's update block on the MI355X -> profiles/update_train_amp_bench.json.

  kernel   dv_conv2d_wgrad_cat_f16 (csrc/conv2d_wgrad_cat_f16.hip) on the block's largest layer, 384 -> 128, k3, batch 4,
           80 x 184 (three 128-channel sources), against dv_conv2d_wgrad_cat_f32 and against MIOpen's fp16
           backward-weights (torch.nn.grad.conv2d_weight on the materialised concatenation, cast to fp16 BEFORE the
           timed region), alternating in one process, ROUNDS rounds, median and spread; its fraction of the fp16 MFMA
           peak on 2 Cout Cin k^2 B H W flop, and of 8 TB/s on the counted bytes: with 64 x 64 block tiles every x plane
           is read ceil(Cout / 64) times and every g plane ceil(Cin / 64) times as float32, plus the split partials
           written and read once.  The other fifteen layers of the block at their planes follow, f16 against f32.
  block    forward, loss, backward and an AdamW step of the 22-iteration loop (synth.update_train_loop) at batch 4,
           80 x 184: the HIP route at "f32", the HIP route at "f16" and the torch-autocast route (DV_TRAIN_CONV2D=torch
           at "f16") alternating in one process, median of five, time and max_memory_allocated
  step     IGEVStereo_ddim.forward_train + sequence_loss + backward + AdamW at batch 4, 320 x 736, 22 iterations,
           amp=False beside amp=True (loss scaled by 1024), alternating, median of three
No target is fixed.

``--bf16`` adds the bf16 arms and writes profiles/update_train_amp_bf16_bench.json instead:
  kernel   the 384 -> 128 layer alone: dv_conv2d_wgrad_cat_f32, _f16 and _bf16
  block    the HIP route at "f32", "f16" and "bf16" and the torch autocast routes in fp16 and bf16 (no loss scale at bf16)
  step     forward_train with amp False / True / torch.bfloat16
alternating in one process, five runs each, median and min-max.

    python tools/bench_update_train_amp.py [--bf16] [--skip-kernel] [--skip-block] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import types
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from diffuvolume_amd import _build  # noqa: E402
from diffuvolume_amd.synth import (IGEV_TRAIN_ARGS, IGEV_TRAIN_WEIGHT_SEED, UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN,  # noqa: E402
                                   StubMobileNetV2, igev_train_step_inputs, synth_state_dict, update_train_inputs,
                                   update_train_loop)
from diffuvolume_amd.train2d import conv2d_cat_weight_grad  # noqa: E402
from diffuvolume_amd.update import BasicMultiUpdateBlock  # noqa: E402

PEAK16 = 2516.6e12             # dense fp16 MFMA peak of the MI355X (16 x the 157.3 TFLOP/s fp32 matrix peak)
PEAK32 = 157.3e12
HBM = 8.0e12
SCALE = 1024.0


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


def block_layers():
    """(name, scale divisor, source channels, cout, k)"""
    rows = []
    for g, div, src in (("gru04", 1, (128, 128, 128)), ("gru08", 2, (128, 128, 128)), ("gru16", 4, (128, 128))):
        rows += [(f"{g}.{c}", div, src, 128, 3) for c in ("convz", "convr", "convq")]
    rows += [("encoder.convc1", 1, (162,), 64, 1), ("encoder.convc2", 1, (64,), 64, 3), ("encoder.convd2", 1, (64,), 64, 3),
             ("encoder.conv", 1, (64, 64), 127, 3), ("disp_head.conv1", 1, (128,), 256, 3), ("disp_head.conv2", 1, (256,), 1, 3),
             ("mask_feat_4", 1, (128,), 32, 3)]
    return rows


def counted_bytes(src, cout, k, b, h, w, splits):
    cin = sum(src)
    planes = 4.0 * b * h * w
    return planes * (cin * -(-cout // 64) + cout * -(-cin // 64)) + 4.0 * cout * cin * k * k * (2 * splits + 1)


def time_kernel(batch, h, w, rounds, reps, bf16=False):
    import ctypes
    from diffuvolume_amd import _lib
    out = []
    first = True
    for name, div, src, cout, k in [("gru04.convz", 1, (128, 128, 128), 128, 3)] + ([] if bf16 else block_layers()[1:]):
        hh, ww = h // div, w // div
        srcs = [torch.randn(batch, c, hh, ww, device="cuda") for c in src]
        g = torch.randn(batch, cout, hh, ww, device="cuda")
        cin = sum(src)
        legs = {"f16": lambda: conv2d_cat_weight_grad(srcs, g, k, f16=True), "f32": lambda: conv2d_cat_weight_grad(srcs, g, k)}
        if bf16:
            legs["bf16"] = lambda: conv2d_cat_weight_grad(srcs, g, k, elem="bf16")
        elif first:
            x16, g16 = torch.cat(srcs, dim=1).half(), g.half()
            legs["miopen_f16"] = lambda: torch.nn.grad.conv2d_weight(x16, (cout, cin, k, k), g16, padding=k // 2)
        arr = (ctypes.c_int * len(src))(*src)
        splits = _lib.load().dv_conv2d_wgrad_cat_f16_workspace_floats(arr, len(src), batch, hh, ww, cout, k) // (cout * cin * k * k)
        flop = 2.0 * cout * cin * k * k * batch * hh * ww
        nbytes = counted_bytes(src, cout, k, batch, hh, ww, splits)
        row = dict(layer=name, plane=[hh, ww], sources=list(src), cout=cout, k=k, gflop=round(flop / 1e9, 2),
                   counted_mbytes=round(nbytes / 1e6, 1), splits=int(splits), **alternate(legs, rounds, reps))
        row["f16"]["frac_fp16_peak"] = round(flop / (row["f16"]["median_ms"] * 1e-3) / PEAK16, 4)
        row["f16"]["frac_hbm_8tbs"] = round(nbytes / (row["f16"]["median_ms"] * 1e-3) / HBM, 3)
        row["f32"]["frac_fp32_peak"] = round(flop / (row["f32"]["median_ms"] * 1e-3) / PEAK32, 3)
        row["f16_over_f32"] = round(row["f16"]["median_ms"] / row["f32"]["median_ms"], 3)
        if bf16:
            row["bf16"]["frac_bf16_peak"] = round(flop / (row["bf16"]["median_ms"] * 1e-3) / PEAK16, 4)
            row["bf16_over_f16"] = round(row["bf16"]["median_ms"] / row["f16"]["median_ms"], 3)
            row["bf16_over_f32"] = round(row["bf16"]["median_ms"] / row["f32"]["median_ms"], 3)
            row["bf16_median_inside_f16_min_max"] = row["f16"]["min_ms"] <= row["bf16"]["median_ms"] <= row["f16"]["max_ms"]
        elif first:
            row["f16_over_miopen_f16"] = round(row["f16"]["median_ms"] / row["miopen_f16"]["median_ms"], 3)
            a, m = legs["f16"](), legs["miopen_f16"]().float()
            row["miopen_f16_rel_l2_against_f16"] = float(f"{float((m - a).norm() / a.norm()):.3e}")
        out.append(row)
        print(f"  {name:16s} {hh:3d}x{ww:<3d} f16 {row['f16']['median_ms']:.3f} ms ({row['f16']['frac_fp16_peak']:.4f} of the fp16 "
              f"peak, {row['f16']['frac_hbm_8tbs']:.3f} of 8 TB/s)  f32 {row['f32']['median_ms']:.3f} ms"
              + (f"  bf16 {row['bf16']['median_ms']:.3f} ms" if bf16 else "")
              + (f"  MIOpen fp16 {row['miopen_f16']['median_ms']:.3f} ms" if first and not bf16 else ""), flush=True)
        first = False
        del srcs, g
    return out


def time_block(batch, h, w, iters, rounds, bf16=False):
    args = types.SimpleNamespace(**UPDATE_TRAIN_ARGS)
    block = BasicMultiUpdateBlock(args, hidden_dims=UPDATE_TRAIN_HIDDEN)
    block.load_state_dict(synth_state_dict(block.state_dict(), seed=7), strict=True)
    block = block.cuda().train()
    opt = torch.optim.AdamW(block.parameters(), lr=1e-5)
    x = update_train_inputs(41, batch, h, w, iters, device="cuda")
    routes = {"hip_f32": ("hip", "f32", 1.0), "hip_f16": ("hip", "f16", SCALE), "torch_autocast_f16": ("torch", "f16", SCALE)}
    if bf16:
        routes = {"hip_f32": routes["hip_f32"], "hip_f16": routes["hip_f16"], "hip_bf16": ("hip", torch.bfloat16, 1.0),
                  "torch_autocast_f16": routes["torch_autocast_f16"], "torch_autocast_bf16": ("torch", torch.bfloat16, 1.0)}

    def step(route):
        env, precision, scale = routes[route]
        os.environ["DV_TRAIN_CONV2D"] = env
        block.set_train_precision(precision)
        opt.zero_grad(set_to_none=True)
        for t in (*x["net"], *(t for lv in x["inp"] for t in lv)):
            t.grad = None
        loss, *_ = update_train_loop(block, x)
        (loss * scale).backward()
        opt.step()
        return loss

    t, mem, rec = {r: [] for r in routes}, {}, dict(batch=batch, plane=[h, w], iters=iters)
    for route in t:                                   # warm-up of every shape on every route
        rec[f"{route}_first_loss"] = float(step(route).detach())
    torch.cuda.synchronize()
    for _ in range(rounds):
        for route in t:
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(lambda: step(route), 1))
            mem[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop("DV_TRAIN_CONV2D", None)
    block.set_train_precision("f32")
    for route in t:
        rec[route] = dict(**med(t[route]), max_memory_allocated_gib=mem[route])
        print(f"  block step {route:20s} {rec[route]['median_ms']:8.1f} ms ({rec[route]['min_ms']:.1f}-{rec[route]['max_ms']:.1f})  "
              f"peak memory {mem[route]} GiB", flush=True)
    rec["hip_f16_over_hip_f32"] = round(rec["hip_f16"]["median_ms"] / rec["hip_f32"]["median_ms"], 3)
    rec["hip_f16_over_torch_autocast"] = round(rec["hip_f16"]["median_ms"] / rec["torch_autocast_f16"]["median_ms"], 3)
    if bf16:
        rec["hip_bf16_over_hip_f32"] = round(rec["hip_bf16"]["median_ms"] / rec["hip_f32"]["median_ms"], 3)
        rec["hip_bf16_over_hip_f16"] = round(rec["hip_bf16"]["median_ms"] / rec["hip_f16"]["median_ms"], 3)
        rec["hip_bf16_over_torch_autocast_bf16"] = round(rec["hip_bf16"]["median_ms"] / rec["torch_autocast_bf16"]["median_ms"], 3)
        rec["hip_bf16_median_inside_hip_f16_min_max"] = rec["hip_f16"]["min_ms"] <= rec["hip_bf16"]["median_ms"] <= rec["hip_f16"]["max_ms"]
        rec["hip_bf16_and_hip_f32_ranges_apart"] = rec["hip_bf16"]["max_ms"] < rec["hip_f32"]["min_ms"] or \
            rec["hip_f32"]["max_ms"] < rec["hip_bf16"]["min_ms"]
    return rec


def time_step(batch, h, w, iters, rounds, bf16=False):
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    from diffuvolume_amd.loss import sequence_loss
    args = types.SimpleNamespace(**IGEV_TRAIN_ARGS)
    x = igev_train_step_inputs(seed=83, b=batch, h=h, w=w, iters=iters, t=400, device="cuda")
    m = IGEVStereo_ddim(args, feature=Feature(StubMobileNetV2()))
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=IGEV_TRAIN_WEIGHT_SEED), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-6)
    os.environ.pop("DV_TRAIN_CONV2D", None)

    def step(amp):
        opt.zero_grad(set_to_none=True)
        init, preds = m.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=iters, t=x["t"],
                                      noise=x["noise"], amp=amp)
        loss, _ = sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=args.max_disp)
        (loss * (SCALE if amp is True else 1.0)).backward()
        opt.step()
        return float(loss)

    legs = {"amp_false": False, "amp_true": True}
    if bf16:
        legs["amp_bf16"] = torch.bfloat16
    res, t = dict(batch=batch, plane=[h, w], iters=iters), {n: [] for n in legs}
    for n, amp in legs.items():
        res[f"{n}_first_loss"] = step(amp)
    for _ in range(rounds):
        for n, amp in legs.items():
            torch.cuda.reset_peak_memory_stats()
            t[n].append(_ms(lambda: step(amp), 1))
            res[f"{n}_peak_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    for n in legs:
        res[n] = med(t[n])
    res["amp_true_over_amp_false"] = round(res["amp_true"]["median_ms"] / res["amp_false"]["median_ms"], 3)
    print(f"  whole step: amp=False {res['amp_false']['median_ms']:.1f} ms, {res['amp_false_peak_gib']} GiB;  amp=True "
          f"{res['amp_true']['median_ms']:.1f} ms, {res['amp_true_peak_gib']} GiB", flush=True)
    if bf16:
        res["amp_bf16_over_amp_false"] = round(res["amp_bf16"]["median_ms"] / res["amp_false"]["median_ms"], 3)
        res["amp_bf16_over_amp_true"] = round(res["amp_bf16"]["median_ms"] / res["amp_true"]["median_ms"], 3)
        print(f"  whole step: amp=torch.bfloat16 {res['amp_bf16']['median_ms']:.1f} ms ({res['amp_bf16']['min_ms']:.1f}-"
              f"{res['amp_bf16']['max_ms']:.1f}), {res['amp_bf16_peak_gib']} GiB", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--width", type=int, default=184)
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--bf16", action="store_true", help="add the bf16 arms; five runs of every arm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.bf16:
        a.step_rounds = max(a.step_rounds, 5)
    a.out = a.out or str(ROOT / "profiles" / ("update_train_amp_bf16_bench.json" if a.bf16 else "update_train_amp_bench.json"))
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = dict(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), fp16_peak_tflops=PEAK16 / 1e12,
               fp32_peak_tflops=PEAK32 / 1e12)
    if not a.skip_kernel:
        print("weight-gradient kernel, f16 against f32 (and MIOpen fp16 on the largest layer):", flush=True)
        rec["kernel"] = time_kernel(a.batch, a.height, a.width, a.rounds, a.reps, a.bf16)
    if not a.skip_block:
        print("update-block training step:", flush=True)
        rec["block"] = time_block(a.batch, a.height, a.width, a.iters, a.rounds, a.bf16)
    if not a.skip_step:
        print("whole training step:", flush=True)
        rec["step"] = time_step(a.batch, 4 * a.height, 4 * a.width, a.iters, a.step_rounds, a.bf16)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
