"""Time the fused BatchNorm3d (batch statistics) + skip + activation of the ACV and PCW training stacks (train_norm.py,
csrc/bn3d_act.hip) on its two routes, alternating in one process, median of --runs with min and max.  DV_TRAIN_NORM=torch
runs the PyTorch statement the stacks ran before the kernels existed, so the torch route is that path measured in the same
process.
  function   forward + backward of batch_norm_act_train (x, weight, bias and, where there is one, skip want a gradient) at
             [4,32,48,64,128] and [4,64,24,32,64], ReLU and Mish, with and without skip: time and peak memory above rest;
  kernels    the three launching entries alone (device events around launches of the C ABI) with the bytes they have to
             move -- each tensor operand read or written once per pass that needs it -- as a fraction of 8 TB/s;
  acv, pcw   whole ACVNet_DDIM / PWCNet_ddim training steps (forward, loss, backward, Adam) at batch 4, 256 x 512, set up
             as tools/bench_train_step.py / tools/bench_pcw_train_step.py set them up, with the switch both ways.
Writes the record to profiles/norm_train_bench.json (or --out), after every part, so that a part can be re-run alone.

    python tools/bench_norm_train.py [--runs 5] [--parts function,kernels,acv,pcw] [--out ...]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen layers of the models
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffuvolume_amd import (ACVNet_DDIM, PWCNet_ddim, _env, _lib, batch_norm_act_train, model_loss_kitti12,  # noqa: E402
                             model_loss_train)
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_NORM"
HBM = 8.0e12
PARTS = ("function", "kernels", "acv", "pcw")
SHAPES = [(32, 48, 64, 128), (64, 24, 32, 64)]          # (C, D, H, W)
ACT_CODE = {"none": 0, "relu": 1, "mish": 2}
# -Rpass-analysis=kernel-resource-usage of csrc/bn3d_act.hip (hipcc, gfx950, the flags of _build.py); 16-byte kernels, the
# scalar ones within 2 VGPRs of them.  256 threads per block except the two combines (one wave per channel).
RESOURCES = {
    "bn3d_stats_kernel": dict(vgprs=12, vgpr_spills=0, scratch_bytes=0, lds_bytes=32, waves_per_simd=8),
    "bn3d_stats_combine_kernel": dict(vgprs=26, vgpr_spills=0, scratch_bytes=0, lds_bytes=0, waves_per_simd=8),
    "bn3d_apply_kernel <none | relu | mish>": dict(vgprs=[16, 16, 23], vgpr_spills=0, scratch_bytes=0, lds_bytes=0,
                                                   waves_per_simd=8),
    "bn3d_bwd_dz_kernel <none | relu | mish> (pass 1)": dict(vgprs=[20, 26, 35], vgpr_spills=0, scratch_bytes=0,
                                                             lds_bytes=32, waves_per_simd=8),
    "bn3d_bwd_combine_kernel": dict(vgprs=16, vgpr_spills=0, scratch_bytes=0, lds_bytes=0, waves_per_simd=8),
    "bn3d_bwd_dx_kernel (pass 2)": dict(vgprs=20, vgpr_spills=0, scratch_bytes=0, lds_bytes=0, waves_per_simd=8),
}


def stats(v):
    return dict(median=round(sorted(v)[len(v) // 2], 4), min=round(min(v), 4), max=round(max(v), 4),
                runs=[round(t, 4) for t in v])


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def alternate(fn, runs, warmup, scale=1.0):
    """fn() timed `runs` times per route, routes alternating -> per route: ms statistics, peak bytes above the resting
    allocation, peak bytes."""
    times, peak, top = {r: [] for r in ROUTES}, {r: 0 for r in ROUTES}, {r: 0 for r in ROUTES}
    for r in ROUTES:
        os.environ[KNOB] = r
        for _ in range(warmup):
            fn()
    for _ in range(runs):
        for r in ROUTES:
            os.environ[KNOB] = r
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            rest = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) * 1e3 / scale)
            peak[r] = max(peak[r], torch.cuda.max_memory_allocated() - rest)
            top[r] = max(top[r], torch.cuda.max_memory_allocated())
    os.environ.pop(KNOB)
    return {r: stats(times[r]) for r in ROUTES}, peak, top


def function(b, runs, inner=3):
    out = []
    for c, d, h, w in SHAPES:
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(b, c, d, h, w, generator=gen).cuda().requires_grad_(True)
        sk = torch.randn(b, c, d, h, w, generator=gen).cuda().requires_grad_(True)
        g = torch.randn(b, c, d, h, w, generator=gen).cuda()
        wt, bs = (1 + 0.1 * torch.randn(c)).cuda().requires_grad_(True), (0.1 * torch.randn(c)).cuda().requires_grad_(True)
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        for act in ("relu", "mish"):
            for skip in (None, sk):

                def fwd_bwd():
                    for _ in range(inner):
                        x.grad = sk.grad = wt.grad = bs.grad = None
                        batch_norm_act_train(x, wt, bs, rm, rv, act=act, skip=skip).backward(g)

                t, peak, _ = alternate(fwd_bwd, runs, warmup=1, scale=inner)
                rec = dict(case=f"batch_norm_act_train [{b},{c},{d},{h},{w}] {act}{', skip' if skip is not None else ''}",
                           fwd_bwd_ms=t, peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                           one_tensor_mib=round(4 * x.numel() / (1 << 20), 1),
                           hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4))
                print(json.dumps(rec), flush=True)
                out.append(rec)
        del x, sk, g
        torch.cuda.empty_cache()
    return out


def kernels(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    out = []

    def record(name, fn, needed, note=""):
        ms = [events_ms(fn, reps) for _ in range(runs)]
        med = sorted(ms)[len(ms) // 2]
        rec = dict(kernel=name, ms=stats(ms), bytes_counted=int(needed),
                   fraction_of_8_tb_s=round(needed / (med * 1e-3) / HBM, 3), counted=note)
        print(json.dumps(rec), flush=True)
        out.append(rec)

    for c, d, h, w in SHAPES:
        s = d * h * w
        n = 4 * b * c * s                                   # bytes of one tensor
        x, sk, g = (torch.randn(b, c, d, h, w, device="cuda") for _ in range(3))
        y, dx, dsk = (torch.empty_like(x) for _ in range(3))
        wt, bs = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        mean, invstd, dg, db = (torch.empty(c, device="cuda") for _ in range(4))
        ws = torch.empty(lib.dv_bn3d_train_workspace_floats(b, c, s), device="cuda")
        shape = f"[{b},{c},{d},{h},{w}]"
        record(f"dv_bn3d_stats_f32 {shape}",
               lambda: _lib.check(lib.dv_bn3d_stats_f32(x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), None, None,
                                                        ws.data_ptr(), b, c, s, 0.1, 1e-5, st), "stats"), n, "x read")
        for act in ("relu", "mish"):
            for skip in (None, sk):
                k = 0 if skip is None else 1
                tag = f"{shape} {act}{', skip' if k else ''}"
                record(f"dv_bn3d_apply_act_f32 {tag}",
                       lambda: _lib.check(lib.dv_bn3d_apply_act_f32(x.data_ptr(), _lib.ptr(skip), mean.data_ptr(),
                                                                    invstd.data_ptr(), wt.data_ptr(), bs.data_ptr(),
                                                                    y.data_ptr(), b, c, s, ACT_CODE[act], st), "apply"),
                       (2 + k) * n, "x (+ skip) read, y written")
                record(f"dv_bn3d_act_bwd_f32 {tag}, every gradient",
                       lambda: _lib.check(lib.dv_bn3d_act_bwd_f32(g.data_ptr(), x.data_ptr(), _lib.ptr(skip), mean.data_ptr(),
                                                                  invstd.data_ptr(), wt.data_ptr(), bs.data_ptr(),
                                                                  dx.data_ptr(), dsk.data_ptr() if k else None,
                                                                  dg.data_ptr(), db.data_ptr(), ws.data_ptr(), b, c, s,
                                                                  ACT_CODE[act], st), "bwd"),
                       (6 + k) * n, "pass 1: dy, x (+ skip) read, dz written; pass 2: dz, x read, dx written")
        del x, sk, g, y, dx, dsk, ws
        torch.cuda.empty_cache()
    return out


def acv_step(b, h, w):
    """ACVNet_DDIM: the step of tools/bench_train_step.py."""
    model = ACVNet_DDIM(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    x = synth_stereo_batch(b, h, w, seed=5)
    left, right, disp, gt = (x[k].cuda() for k in ("left", "right", "disp", "gt"))
    mask = (gt < 192) & (gt > 0)

    def step():
        opt.zero_grad()
        model_loss_train(model(left, right, None, disp, None), gt, mask).backward()
        opt.step()

    return step


def pcw_step(b, h, w):
    """PWCNet_ddim: the step of tools/bench_pcw_train_step.py."""
    model = PWCNet_ddim(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    x = synth_stereo_batch(b, h, w, seed=5)
    left, right, gt = (x[k].cuda() for k in ("left", "right", "gt"))
    disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    mask = (gt < 192) & (gt > 0)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        model_loss_kitti12(model(left, right, None, disp, None), gt, mask).backward()
        opt.step()

    return step


def whole_step(name, step, runs, **what):
    t, peak, top = alternate(step, runs, warmup=2)
    apart = bool(t["hip"]["max"] < t["torch"]["min"])
    rec = dict(model=name, **what, step_ms=t, peak_gib={r: round(p / 2 ** 30, 3) for r, p in top.items()},
               peak_gib_above_rest={r: round(p / 2 ** 30, 3) for r, p in peak.items()},
               hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4),
               hip_faster_with_ranges_apart=apart)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "norm_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_norm_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               default_route=_env.KNOBS[KNOB][0], kernel_resources=RESOURCES)

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "function" in parts:
        save("function", function(a.batch, a.runs))
    if "kernels" in parts:
        save("kernels", kernels(a.batch, a.runs))
    if "acv" in parts:
        save("acv_step", whole_step("ACVNet_DDIM", acv_step(a.batch, 256, 512), a.runs, image=[256, 512]))
    if "pcw" in parts:
        save("pcw_step", whole_step("PWCNet_ddim", pcw_step(a.batch, 256, 512), a.runs, image=[256, 512]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
