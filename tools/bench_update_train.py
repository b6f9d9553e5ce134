"""Benchmark of the update block's training route on the MI355X -> profiles/update_train_bench.json.

  layers   the new weight-gradient kernel (csrc/conv2d_wgrad_cat.hip, virtual concatenation) against its predecessor
           (dv_conv2d_wgrad_f32 on the materialised concatenation, torch.cat included) and MIOpen's backward-weights
           (torch.nn.grad.conv2d_weight on the materialised concatenation), alternating in one process, ROUNDS rounds,
           median and spread: the sixteen 3x3 / 1x1 layers of the block at batch 4, 80x184 / 40x92 / 20x46, and
           refinenet3's 128 -> 128 3x3 dilation-1 and 1x1 at batch 4, 256x512
  step     forward, loss, backward and an AdamW step of the 22-iteration loop (synth.update_train_loop) at batch 4,
           80x184, HIP route and DV_TRAIN_CONV2D=torch alternating, with max_memory_allocated and the counted
           17.7 TFLOP over the step time
  parity   the errors that tests/test_gpu_update_train.py prints for the two fixture cases, both routes (taken first,
           in a process that has run nothing else)
  input_grad   the input gradient of a convolution over a concatenation as ONE forward launch on g (channel views per
           source afterwards) against one launch per source, on gru04's candidate (128 -> 384) and z | r pair (256 -> 384)
  long     (--long) the full-length loop of tests/test_gpu_update_train.py::test_full_length_loop: T = 22 at B 1, 80x184,
           two HIP runs compared bit for bit, the distance to the torch route, peak memory; --full-parity adds both
           routes' errors against the float64 CPU restatement

    python tools/bench_update_train.py [--skip-layers] [--skip-step] [--skip-parity] [--rounds 5] [--step-rounds 3]
The per-kernel split of the HIP route comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_update_train.py --skip-layers --skip-parity \
        --routes hip --step-rounds 1 --out DIR/step.json
    python tools/bench_update_train.py --merge-kernel-stats DIR/..._kernel_stats.csv --profiled-steps 3
which adds `step.hip_kernel_split` to the existing record (--out) and changes nothing else in it."""
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
from diffuvolume_amd.synth import (UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, synth_state_dict, update_train_inputs,  # noqa: E402
                                   update_train_loop)
from diffuvolume_amd.train2d import conv2d_cat_weight_grad, conv2d_weight_grad  # noqa: E402
from diffuvolume_amd.update import BasicMultiUpdateBlock  # noqa: E402

PEAK = 157.3e12                # fp32 MFMA peak of the MI355X
STEP_FLOP = 17.7e12            # counted: 22 iterations x 3 x 268.7 GFLOP at batch 4, 80x184


def block_layers():
    """(name, scale divisor, source channels, cout, k)"""
    rows = []
    for g, div, src in (("gru04", 1, (128, 128, 128)), ("gru08", 2, (128, 128, 128)), ("gru16", 4, (128, 128))):
        rows += [(f"{g}.{c}", div, src, 128, 3) for c in ("convz", "convr", "convq")]
    rows += [("encoder.convc1", 1, (162,), 64, 1), ("encoder.convc2", 1, (64,), 64, 3), ("encoder.convd2", 1, (64,), 64, 3),
             ("encoder.conv", 1, (64, 64), 127, 3), ("disp_head.conv1", 1, (128,), 256, 3), ("disp_head.conv2", 1, (256,), 1, 3),
             ("mask_feat_4", 1, (128,), 32, 3)]
    return rows


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


def time_layers(batch, h, w, rounds, reps):
    out = []
    shapes = [(n, batch, h // d, w // d, src, cout, k) for n, d, src, cout, k in block_layers()]
    shapes += [("refinenet3.128->128.k3d1", batch, 256, 512, (128,), 128, 3), ("refinenet3.128->128.k1", batch, 256, 512, (128,), 128, 1)]
    for name, b, hh, ww, src, cout, k in shapes:
        srcs = [torch.randn(b, c, hh, ww, device="cuda") for c in src]
        g = torch.randn(b, cout, hh, ww, device="cuda")
        cin = sum(src)
        legs = {"new": lambda: conv2d_cat_weight_grad(srcs, g, k),
                "old_with_cat": lambda: conv2d_weight_grad(torch.cat(srcs, dim=1) if len(srcs) > 1 else srcs[0], g, k, 1, cout),
                "miopen_with_cat": lambda: torch.nn.grad.conv2d_weight(torch.cat(srcs, dim=1) if len(srcs) > 1 else srcs[0],
                                                                      (cout, cin, k, k), g, padding=k // 2)}
        t = {n: [] for n in legs}
        for _ in range(rounds):
            for n, fn in legs.items():
                t[n].append(_ms(fn, reps))
        flop = 2.0 * cout * cin * k * k * b * hh * ww
        row = dict(layer=name, plane=[hh, ww], sources=list(src), cout=cout, k=k, gflop=round(flop / 1e9, 2))
        for n in legs:
            row[n] = med(t[n])
            row[n]["frac_peak"] = round(flop / (row[n]["median_ms"] * 1e-3) / PEAK, 3)
        row["new_over_old"] = round(row["new"]["median_ms"] / row["old_with_cat"]["median_ms"], 3)
        row["new_over_miopen"] = round(row["new"]["median_ms"] / row["miopen_with_cat"]["median_ms"], 3)
        out.append(row)
        print(f"  {name:26s} {hh:3d}x{ww:<3d} new {row['new']['median_ms']:7.3f} ms ({row['new']['frac_peak']:.3f} of peak, "
              f"{row['new']['min_ms']:.3f}-{row['new']['max_ms']:.3f})  old+cat {row['old_with_cat']['median_ms']:7.3f} "
              f"({row['old_with_cat']['min_ms']:.3f}-{row['old_with_cat']['max_ms']:.3f})  MIOpen+cat "
              f"{row['miopen_with_cat']['median_ms']:7.3f}", flush=True)
        del srcs, g
    return out


def time_step(batch, h, w, iters, rounds, routes=("hip", "torch")):
    args = types.SimpleNamespace(**UPDATE_TRAIN_ARGS)
    block = BasicMultiUpdateBlock(args, hidden_dims=UPDATE_TRAIN_HIDDEN)
    block.load_state_dict(synth_state_dict(block.state_dict(), seed=7), strict=True)
    block = block.cuda().train()
    opt = torch.optim.AdamW(block.parameters(), lr=1e-5)
    x = update_train_inputs(41, batch, h, w, iters, device="cuda")

    def step():
        opt.zero_grad(set_to_none=True)
        for t in (*x["net"], *(t for lv in x["inp"] for t in lv)):
            t.grad = None
        loss, *_ = update_train_loop(block, x)
        loss.backward()
        opt.step()
        return loss

    t, mem = {r: [] for r in routes}, {}
    for route in t:                                   # warm-up of every shape on both routes
        os.environ["DV_TRAIN_CONV2D"] = route
        step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for route in t:
            os.environ["DV_TRAIN_CONV2D"] = route
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(step, 1))
            mem[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop("DV_TRAIN_CONV2D", None)
    rec = dict(batch=batch, plane=[h, w], iters=iters, counted_tflop=STEP_FLOP / 1e12)
    for route in t:
        m = med(t[route])
        rec[route] = dict(**m, max_memory_allocated_gib=mem[route],
                          counted_tflops=round(STEP_FLOP / (m["median_ms"] * 1e-3) / 1e12, 1))
        print(f"  step {route:5s} {m['median_ms']:8.1f} ms ({m['min_ms']:.1f}-{m['max_ms']:.1f})  "
              f"{rec[route]['counted_tflops']} TFLOP/s counted  peak memory {mem[route]} GiB", flush=True)
    if "hip" in rec and "torch" in rec:
        rec["hip_over_torch"] = round(rec["hip"]["median_ms"] / rec["torch"]["median_ms"], 3)
    return rec


def time_input_grad(batch, h, w, rounds, reps):
    from diffuvolume_amd.submodule import ACT_NONE, Conv2dPlan
    out = []
    for name, cout in (("gru04.convq", 128), ("gru04.convz|convr", 256)):
        wt = torch.randn(384, cout, 3, 3, device="cuda") * 0.05          # flipped / transposed already: [Cin, Cout, 3, 3]
        g = torch.randn(batch, cout, h, w, device="cuda")
        one = Conv2dPlan(wt, None, dilation=1, act=ACT_NONE)
        per = [Conv2dPlan(wt[i * 128:(i + 1) * 128].contiguous(), None, dilation=1, act=ACT_NONE) for i in range(3)]
        legs = {"one_launch": lambda: one(g), "launch_per_source": lambda: [p(g) for p in per]}
        t = {n: [] for n in legs}
        for _ in range(rounds):
            for n, fn in legs.items():
                t[n].append(_ms(fn, reps))
        row = dict(layer=name, plane=[h, w], cout_of_g=cout, sources=[128, 128, 128], **{n: med(t[n]) for n in legs})
        out.append(row)
        print(f"  input gradient {name:18s} one launch {row['one_launch']['median_ms']:.3f} ms  per source "
              f"{row['launch_per_source']['median_ms']:.3f} ms", flush=True)
    return out


def long_loop(full_parity):
    sys.path.insert(0, str(ROOT / "tests"))
    import pytest
    import test_gpu_update_train as T
    mp = pytest.MonkeyPatch()
    r4 = lambda d: {k: float(f"{v:.3e}") for k, v in d.items()}
    try:
        torch.cuda.reset_peak_memory_stats()
        a = T.long_loop("hip", mp)
        mem = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        b = T.long_loop("hip", mp)
        t = T.long_loop("torch", mp)
        rec = dict(shape="T = 22, B 1, 80x184", max_memory_allocated_gib=mem,
                   two_hip_runs_bit_identical=all(torch.equal(u, v) for k in T.KINDS for u, v in zip(a[k], b[k])),
                   hip_vs_torch_route=r4(T.worst_rel(a, t)))
        if full_parity:
            block = T.fresh_block().cpu().double()

            class Ref:
                def __call__(self, net, inp, corr=None, disp=None, **kw):
                    return T.block_f64_cpu(block, net, inp, corr, disp)
            x = update_train_inputs(41, 1, 80, 184, 22, dtype=torch.float64)
            loss, disps, masks, _ = update_train_loop(Ref(), x)
            loss.backward()
            r = T.kinds_of(block, x, disps, masks, loss)
            rec["against_float64_cpu"] = dict(hip=r4(T.worst_rel(a, r)), torch=r4(T.worst_rel(t, r)))
    finally:
        mp.undo()
    print("  full-length loop:", rec, flush=True)
    return rec


def merge_kernel_stats(csv_path, out, steps):
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    top = [dict(share_pct=round(float(r["TotalDurationNs"]) / tot * 100, 1), calls_per_step=int(r["Calls"]) // steps,
                ms_per_step=round(float(r["TotalDurationNs"]) / 1e6 / steps, 2),
                kernel=r["Name"].replace("(anonymous namespace)::", "")[:100])
           for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:28]]
    rec = json.loads(Path(out).read_text())
    rec.setdefault("step", {})["hip_kernel_split"] = dict(
        source=f"rocprofv3 --kernel-trace --stats, a run of its own: {steps} steps of the HIP route, figures per step",
        csrc_sha16=_build.csrc_sha16(), total_kernel_ms_per_step=round(tot / 1e6 / steps, 1), kernels=top)
    Path(out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"merged {len(top)} kernels into {out}")


def parity():
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import pytest
    import test_gpu_update_train as T
    with np.load(ROOT / "tests" / "golden" / "update_train_loop.npz") as z:
        gold = {k: z[k] for k in z.files}
    mp, out = pytest.MonkeyPatch(), {}
    try:
        for case in ("even", "ragged"):
            out[case] = {}
            for route in ("hip", "torch"):
                rows = T.run_case(gold, case, route, mp)
                out[case][route] = {k: float(f"{max(r[1] for r in rows[k]):.3e}") for k in T.KINDS}
            out[case]["reference_f32"] = {k: float(f"{max(r[2] for r in rows[k]):.3e}") for k in T.KINDS}
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--routes", default="hip,torch", help="routes of the step leg (a profiler run wants one)")
    ap.add_argument("--long", action="store_true", help="the full-length loop leg")
    ap.add_argument("--full-parity", action="store_true", help="--long with the float64 CPU restatement")
    ap.add_argument("--merge-kernel-stats", metavar="CSV", default=None)
    ap.add_argument("--profiled-steps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "update_train_bench.json"))
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out, a.profiled_steps)
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = dict(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), peak_tflops=PEAK / 1e12)
    if not a.skip_parity:
        rec["parity"] = parity()
        print("parity (worst relative L2 against float64 per kind):", rec["parity"], flush=True)
    if not a.skip_layers:
        rec["input_grad"] = time_input_grad(a.batch, a.height, a.width, a.rounds, a.reps)
        print("weight-gradient kernels, per layer:", flush=True)
        rec["wgrad_layers"] = time_layers(a.batch, a.height, a.width, a.rounds, a.reps)
    if not a.skip_step:
        print("training step:", flush=True)
        rec["step"] = time_step(a.batch, a.height, a.width, a.iters, a.step_rounds, tuple(a.routes.split(",")))
    if a.long or a.full_parity:
        rec["full_length_loop"] = long_loop(a.full_parity)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
