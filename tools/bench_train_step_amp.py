"""Time the ACVNet_DDIM and PWCNet_ddim training steps (forward, loss, backward, Adam) at the reference's training shape --
B = 4 pairs of 256 x 512, the setup of tools/bench_train_step.py and tools/bench_pcw_train_step.py -- at train precision
"f32", "f16" and "bf16" (``set_train_precision``), alternating the three in one process, and time the three products of
the 3x3x3 stride-1 layers alone (forward, input gradient, weight gradient) on their fp16 kernels (csrc/conv3d_f16.hip,
csrc/conv3d_wgrad_f16.hip), on their bf16 twins (csrc/conv3d_bf16.hip, csrc/conv3d_wgrad_bf16.hip), on the float32
kernels they replace and on MIOpen fp16 (torch, half tensors).

Per product: median and min-max of the runs, the fraction of the 16-bit MFMA peak (16 x 157.3 TFLOP/s) and of 8 TB/s on the
COUNTED bytes -- every operand read once and every result written once as float32 (the weight gradient: its partials
written and read once more), which is what the kernels cannot avoid, not what they move.  Peak memory per step is
torch.cuda.max_memory_allocated around the timed runs.  Writes profiles/train_step_amp_bf16_bench.json (or --out);
profiles/train_step_amp_bench.json is the record of the two-arm tool before "bf16" and is left as it is.

    python tools/bench_train_step_amp.py [--runs 5] [--skip-steps] [--out profiles/train_step_amp_bf16_bench.json]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffuvolume_amd import ACVNet_DDIM, PWCNet_ddim, _lib, model_loss_kitti12, model_loss_train, train3d  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

PEAK_F16 = 16 * 157.3e12
PEAK_HBM = 8.0e12
LAYERS = [("32->32", 32, 32, (48, 64, 128)), ("64->32", 64, 32, (48, 64, 128)), ("64->64", 64, 64, (24, 32, 64)),
          ("128->128", 128, 128, (12, 16, 32))]


def stats(ms):
    s = sorted(ms)
    return dict(median=round(s[len(s) // 2], 4), min=round(s[0], 4), max=round(s[-1], 4))


def timed(fn, reps):
    """ms of each of ``reps`` calls (events around every call, one warm call first)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def products(batch, reps):
    rows = []
    for name, cin, cout, dims in LAYERS:
        x = torch.randn(batch, cin, *dims, device="cuda")
        g = torch.randn(batch, cout, *dims, device="cuda")
        w = torch.randn(cout, cin, 3, 3, 3, device="cuda") * 0.05
        xh, gh, wh = x.half(), g.half(), w.half()
        vox = batch * dims[0] * dims[1] * dims[2]
        flop = 2.0 * cout * cin * 27 * vox
        wbytes = 4.0 * cout * cin * 27
        ws = _lib.load().dv_conv3d_wgrad_f16_workspace_floats(batch, cin, *dims, cout)
        plan32 = train3d._plan(w, 1)
        plan32t = train3d._plan(w.flip(2, 3, 4).transpose(0, 1), 1)
        arms = {
            "forward": (4.0 * vox * (cin + cout) + wbytes,
                        {"f16": lambda: train3d.conv3d_k3s1_f16(x, w), "bf16": lambda: train3d.conv3d_k3s1_bf16(x, w),
                         "f32": lambda: plan32(x),
                         "miopen_f16": lambda: F.conv3d(xh, wh, padding=1)}),
            "input_gradient": (4.0 * vox * (cin + cout) + wbytes,
                               {"f16": lambda: train3d.conv3d_k3s1_f16(g, w, transpose_flip=True),
                                "bf16": lambda: train3d.conv3d_k3s1_bf16(g, w, transpose_flip=True), "f32": lambda: plan32t(g),
                                "miopen_f16": lambda: torch.nn.grad.conv3d_input(xh.shape, wh, gh, padding=1)}),
            "weight_gradient": (4.0 * vox * (cin + cout) + wbytes + 8.0 * ws,
                                {"f16": lambda: train3d.conv3d_weight_grad_f16(x, g),
                                 "bf16": lambda: train3d.conv3d_weight_grad_bf16(x, g),
                                 "f32": lambda: train3d.conv3d_weight_grad(x, g, 3, 1, cout),
                                 "miopen_f16": lambda: torch.nn.grad.conv3d_weight(xh, wh.shape, gh, padding=1)}),
        }
        for product, (nbytes, fns) in arms.items():
            ms = {k: [] for k in fns}
            for k, fn in fns.items():                           # warm every arm, then alternate them
                fn()
            for _ in range(reps):
                for k, fn in fns.items():
                    ms[k] += timed(fn, 1)
            row = dict(layer=name, product=product, cin=cin, cout=cout, dims=list(dims), gflop=round(flop / 1e9, 2),
                       counted_mbytes=round(nbytes / 1e6, 2), ms={k: stats(v) for k, v in ms.items()})
            med = row["ms"]["f16"]["median"]
            row["f16_frac_mfma_peak"] = round(flop / (med * 1e-3) / PEAK_F16, 4)
            row["f16_frac_hbm_peak"] = round(nbytes / (med * 1e-3) / PEAK_HBM, 4)
            row["f32_over_f16"] = round(row["ms"]["f32"]["median"] / med, 3)
            row["miopen_f16_over_f16"] = round(row["ms"]["miopen_f16"]["median"] / med, 3)
            bmed = row["ms"]["bf16"]["median"]
            row["bf16_over_f16"] = round(bmed / med, 3)
            row["bf16_within_f16_range"] = row["ms"]["f16"]["min"] <= bmed <= row["ms"]["f16"]["max"]
            rows.append(row)
            print(f"  {name:9s} {product:16s} f16 {med:7.3f} ms ({row['ms']['f16']['min']:.3f}-{row['ms']['f16']['max']:.3f})  "
                  f"bf16 {bmed:7.3f} ({row['ms']['bf16']['min']:.3f}-{row['ms']['bf16']['max']:.3f})  "
                  f"f32 {row['ms']['f32']['median']:7.3f}  MIOpen f16 {row['ms']['miopen_f16']['median']:7.3f}  "
                  f"{row['f16_frac_mfma_peak']:.3f} of MFMA peak, {row['f16_frac_hbm_peak']:.3f} of 8 TB/s", flush=True)
        del x, g, w, xh, gh, wh, plan32, plan32t
        torch.cuda.empty_cache()
    return rows


def model_steps(kind, batch, height, width, runs, warmup):
    if kind == "acv":
        model, loss_fn = ACVNet_DDIM(192), model_loss_train
    else:
        model, loss_fn = PWCNet_ddim(192), model_loss_kitti12
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    x = synth_stereo_batch(batch, height, width, seed=5)
    left, right, disp, gt = (x[k].cuda() for k in ("left", "right", "disp", "gt"))
    if kind == "pcw":
        disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(height // 4, width // 4), mode="bilinear") / 4
    mask = (gt < 192) & (gt > 0)

    def step():
        opt.zero_grad()
        loss = loss_fn(model(left, right, None, disp, None), gt, mask)
        loss.backward()
        opt.step()
        return float(loss.detach())

    times, peak = {"f32": [], "f16": [], "bf16": []}, {}
    dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    for p in times:
        model.set_train_precision(dtype[p])
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
    for _ in range(runs):
        for p in times:
            model.set_train_precision(dtype[p])
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            loss = step()
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) * 1e3)
            peak[p] = max(peak.get(p, 0), torch.cuda.max_memory_allocated())
            print(f"{kind} {p} step {times[p][-1]:8.1f} ms  loss {loss:.3f}", flush=True)
    rec = dict(step_ms={p: [round(t, 2) for t in v] for p, v in times.items()},
               step_ms_stats={p: stats(v) for p, v in times.items()},
               peak_memory_mib={p: round(v / 2 ** 20, 1) for p, v in peak.items()})
    rec["f32_over_f16"] = round(rec["step_ms_stats"]["f32"]["median"] / rec["step_ms_stats"]["f16"]["median"], 3)
    rec["ranges_apart"] = rec["step_ms_stats"]["f16"]["max"] < rec["step_ms_stats"]["f32"]["min"]
    rec["f32_over_bf16"] = round(rec["step_ms_stats"]["f32"]["median"] / rec["step_ms_stats"]["bf16"]["median"], 3)
    rec["bf16_over_f16"] = round(rec["step_ms_stats"]["bf16"]["median"] / rec["step_ms_stats"]["f16"]["median"], 3)
    rec["bf16_ranges_apart_from_f32"] = rec["step_ms_stats"]["bf16"]["max"] < rec["step_ms_stats"]["f32"]["min"]
    rec["bf16_within_f16_range"] = (rec["step_ms_stats"]["f16"]["min"] <= rec["step_ms_stats"]["bf16"]["median"]
                                    <= rec["step_ms_stats"]["f16"]["max"])
    del model, opt
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_step_amp_bf16_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    os.environ.pop("DV_TRAIN_CONV3D", None)
    rec = dict(tool="tools/bench_train_step_amp.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               batch=a.batch, image=[a.height, a.width], runs=a.runs, warmup=a.warmup,
               miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"), peak_f16_tflops=PEAK_F16 / 1e12, peak_hbm_tbs=PEAK_HBM / 1e12)
    rec["f32_arm_note"] = ("forward / input_gradient 'f32' arms of `products` run on a Conv3dPlan built ONCE (packed weight "
                           "cached); the training route builds and packs one per call, so the per-product f32_over_f16 of "
                           "these two products understates what a step sees -- `steps` pays the repack")
    print("the three products alone:")
    rec["products"] = products(a.batch, a.runs)
    if not a.skip_steps:
        rec["steps"] = {k: model_steps(k, a.batch, a.height, a.width, a.runs, a.warmup) for k in ("acv", "pcw")}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    if "steps" in rec:
        print(json.dumps({k: {"ms": v["step_ms_stats"], "f32_over_f16": v["f32_over_f16"], "ranges_apart": v["ranges_apart"],
                              "f32_over_bf16": v["f32_over_bf16"], "bf16_over_f16": v["bf16_over_f16"],
                              "bf16_within_f16_range": v["bf16_within_f16_range"]}
                          for k, v in rec["steps"].items()}))


if __name__ == "__main__":
    main()
