"""Time the differentiable warp + correlation of PWCNet_ddim's refinement input (train_refine.py, csrc/warp_corr.hip) on
its two routes, alternating in one process, median of --runs with min and max.  DV_TRAIN_REFINE=torch runs the PyTorch
statements train_forward ran before the kernels existed, so the torch route is that path measured in the same process.
  function   forward + backward of warp_corr_train at [4,32,256,512] and [4,32,384,1248] (all three inputs want a
             gradient; the disparity is a smooth field in [0, 64) -- a regressed disparity is one): time and peak memory
             above rest;
  kernels    the forward entry and the backward entry alone (device events around launches of the C ABI), the backward
             also with dleft + ddisp only (pass 1) and on a disparity of uniform noise, with the bytes they have to
             move -- every input read once, every output written once -- as a fraction of 8 TB/s; the workspace traffic
             (m dF written by pass 1, read by pass 2) is listed apart;
  pcw        whole PWCNet_ddim training steps (forward, loss, backward, Adam) at batch 4, 256 x 512, set up as
             tools/bench_pcw_train_step.py sets them up, with the switch both ways.
Writes the record to profiles/train_refine_bench.json (or --out; not a name matching profiles/r*_bench.json, which
tests/test_bench_contract.py takes for the round's bench line), after every part, so that a part can be re-run alone.

    python tools/bench_refine_train.py [--runs 5] [--parts function,kernels,pcw] [--out ...]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen layers of the model
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffuvolume_amd import PWCNet_ddim, _lib, model_loss_kitti12, warp_corr_train  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_REFINE"
HBM = 8.0e12
PARTS = ("function", "kernels", "pcw")
SHAPES = [(32, 256, 512), (32, 384, 1248)]          # (C, H, W)
# -Rpass-analysis=kernel-resource-usage of csrc/warp_corr.hip (hipcc, gfx950, the flags of _build.py)
RESOURCES = {
    "warp_corr_kernel (forward)": dict(vgprs=46, vgpr_spills=0, scratch_bytes=0, lds_bytes=25600, waves_per_simd=6),
    "warp_corr_bwd_kernel (pass 1: dleft, ddisp, m dF)": dict(vgprs=104, vgpr_spills=0, scratch_bytes=0, lds_bytes=24832,
                                                               waves_per_simd=4),
    "warp_scatter_rows_kernel (pass 2: dright)": dict(vgprs=91, vgpr_spills=0, scratch_bytes=0, lds_bytes=11520,
                                                       waves_per_simd=5),
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


def not_slower(t):
    """The rule of the default: hip is not slower than torch by more than the spread of the runs."""
    spread = max(t[r]["max"] - t[r]["min"] for r in ROUTES)
    return bool(t["hip"]["median"] <= t["torch"]["median"] + spread), round(spread, 4)


def smooth_disp(b, h, w, seed=3):
    """A smooth disparity in [0, 64): coarse uniform noise, bilinearly enlarged."""
    gen = torch.Generator().manual_seed(seed)
    coarse = 64 * torch.rand(b, 1, h // 32, w // 32, generator=gen)
    return F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).cuda().contiguous()


def function(b, runs, inner=3):
    out = []
    for c, h, w in SHAPES:
        gen = torch.Generator().manual_seed(1)
        left = torch.randn(b, c, h, w, generator=gen).cuda().requires_grad_(True)
        right = torch.randn(b, c, h, w, generator=gen).cuda().requires_grad_(True)
        disp = smooth_disp(b, h, w).requires_grad_(True)
        cots = [torch.randn(b, c, h, w, device="cuda"), torch.randn(b, 49, h, w, device="cuda")]

        def fwd_bwd():
            for _ in range(inner):
                left.grad = right.grad = disp.grad = None
                torch.autograd.backward(list(warp_corr_train(left, right, disp)), cots)

        t, peak, _ = alternate(fwd_bwd, runs, warmup=1, scale=inner)
        rec = dict(case=f"warp_corr_train [{b},{c},{h},{w}], three gradients", fwd_bwd_ms=t,
                   peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   one_feature_map_mib=round(4 * left.numel() / (1 << 20), 1),
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del left, right, disp, cots
        torch.cuda.empty_cache()
    return out


def kernels(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    out = []

    def record(name, fn, needed, extra=0):
        ms = [events_ms(fn, reps) for _ in range(runs)]
        med = sorted(ms)[len(ms) // 2]
        rec = dict(kernel=name, ms=stats(ms), bytes_counted=int(needed), fraction_of_8_tb_s=round(needed / (med * 1e-3) / HBM, 3),
                   workspace_bytes_written_and_read=int(extra))
        print(json.dumps(rec), flush=True)
        out.append(rec)

    for c, h, w in SHAPES:
        n, px = b * c * h * w, b * h * w
        left, right = torch.randn(b, c, h, w, device="cuda"), torch.randn(b, c, h, w, device="cuda")
        g_diff, g_corr = torch.randn(b, c, h, w, device="cuda"), torch.randn(b, 49, h, w, device="cuda")
        diff, corr = torch.empty_like(left), torch.empty_like(g_corr)
        dleft, dright = torch.empty_like(left), torch.empty_like(right)
        ws = torch.empty(lib.dv_warp_corr_bwd_workspace_floats(b, c, h, w), device="cuda")
        for tag, disp in (("smooth disparity", smooth_disp(b, h, w)),
                          ("uniform noise in [0, 64)", 64 * torch.rand(b, 1, h, w, device="cuda"))):
            ddisp = torch.empty_like(disp)
            shape = f"[{b},{c},{h},{w}] {tag}"
            record(f"dv_warp_corr_f32 {shape}",
                   lambda: _lib.check(lib.dv_warp_corr_f32(left.data_ptr(), right.data_ptr(), disp.data_ptr(), diff.data_ptr(),
                                                           corr.data_ptr(), b, c, h, w, 24, st), "warp_corr"),
                   4 * (3 * n + 50 * px))
            record(f"dv_warp_corr_bwd_f32 {shape}, dleft + dright + ddisp",
                   lambda: _lib.check(lib.dv_warp_corr_bwd_f32(left.data_ptr(), right.data_ptr(), disp.data_ptr(),
                                                               g_diff.data_ptr(), g_corr.data_ptr(), dleft.data_ptr(),
                                                               dright.data_ptr(), ddisp.data_ptr(), ws.data_ptr(), b, c, h, w,
                                                               24, st), "warp_corr bwd"),
                   4 * (5 * n + 51 * px), 4 * 2 * n)
            record(f"dv_warp_corr_bwd_f32 {shape}, dleft + ddisp (pass 1 alone)",
                   lambda: _lib.check(lib.dv_warp_corr_bwd_f32(left.data_ptr(), right.data_ptr(), disp.data_ptr(),
                                                               g_diff.data_ptr(), g_corr.data_ptr(), dleft.data_ptr(), None,
                                                               ddisp.data_ptr(), None, b, c, h, w, 24, st), "warp_corr bwd"),
                   4 * (4 * n + 51 * px))
        del left, right, g_diff, g_corr, diff, corr, dleft, dright, ws
        torch.cuda.empty_cache()
    return out


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

    def fwd_bwd():
        loss = model_loss_kitti12(model(left, right, None, disp, None), gt, mask)
        loss.backward()

    def step():
        opt.zero_grad()
        fwd_bwd()
        opt.step()

    return model, fwd_bwd, step


def whole_step(name, step, runs, **what):
    t, peak, top = alternate(step, runs, warmup=2)
    ok, spread = not_slower(t)
    rec = dict(model=name, **what, step_ms=t, peak_gib={r: round(p / 2 ** 30, 3) for r, p in top.items()},
               peak_gib_above_rest={r: round(p / 2 ** 30, 3) for r, p in peak.items()},
               hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4), spread_ms=spread,
               hip_not_slower_than_torch_by_more_than_the_spread=ok)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_refine_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_refine_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               kernel_resources=RESOURCES)

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "function" in parts:
        save("function", function(a.batch, a.runs))
    if "kernels" in parts:
        save("kernels", kernels(a.batch, a.runs))
    if "pcw" in parts:
        save("pcw_step", whole_step("PWCNet_ddim", pcw_step(a.batch, 256, 512)[2], a.runs, image=[256, 512]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
