"""Time the patch stencils of ACVNet_DDIM's attention branch in training (train_patch.py, csrc/patch_volume.hip forward,
csrc/patch_volume_bwd.hip backward) on their two routes, alternating in one process, median of --runs with min and max.
DV_TRAIN_PATCH=torch runs the four nn.Conv3d calls the call site ran before the backward kernel existed, so the torch route
is that path measured in the same process.
  function   forward + backward of the call site's expression at [4,40,48,64,128] with all three gradients (the hip route
             through patch_volume_train, the torch route through the four modules, slices and cat): time and peak memory
             above rest; and the hip route with frozen stencils (dgwc only);
  kernels    dv_patch_volume_bwd_f32 alone (device events around launches of the C ABI) on the 12 B per element it has to
             move (gwc and dout read, dgwc written), and with frozen stencils on 8 B, beside the forward
             dv_patch_volume_runs_f32 on its 8 B per element, as fractions of 8 TB/s;
  acv        whole ACVNet_DDIM training steps (forward, loss, backward, Adam) at batch 4, 256 x 512, set up as
             tools/bench_train_step.py sets them up, with the switch both ways.
Writes the record to profiles/patch_train_bench.json (or --out), after every part, so that a part can be re-run alone.

    python tools/bench_patch_train.py [--runs 5] [--parts function,kernels,acv] [--out ...]"""
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
from torch import nn  # noqa: E402

from diffuvolume_amd import ACVNet_DDIM, _env, _lib, model_loss_train, patch_volume_train, train_patch  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.acv_ddim import PATCH_DILATION  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_PATCH"
HBM = 8.0e12
PARTS = ("function", "kernels", "acv")
SHAPE = (40, 48, 64, 128)                               # (G, D, H, W): the volume of a 256 x 512 pair
# -Rpass-analysis=kernel-resource-usage of csrc/patch_volume_bwd.hip (hipcc, gfx950, the flags of _build.py).  256 threads
# per block except the combine (one wave per group).  LDS by dilation 1 / 2 / 3; three blocks per CU fit in 160 KiB.
RESOURCES = {
    "patch_bwd_kernel<dilation 1 | 2 | 3, 16-byte accesses>": dict(vgprs=46, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0,
                                                                   lds_bytes=[42912, 46304, 49696], waves_per_simd=3),
    "patch_bwd_kernel<dilation 1 | 2 | 3, element-wise accesses>": dict(vgprs=60, vgpr_spills=0, sgpr_spills=0,
                                                                        scratch_bytes=0, lds_bytes=[42912, 46304, 49696],
                                                                        waves_per_simd=3),
    "patch_bwd_combine_kernel": dict(vgprs=16, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0, lds_bytes=0, waves_per_simd=8),
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


def alternate(fn, runs, warmup, scale=1.0, routes=ROUTES):
    """fn() timed `runs` times per route, routes alternating -> per route: ms statistics, peak bytes above the resting
    allocation, peak bytes."""
    times, peak, top = {r: [] for r in routes}, {r: 0 for r in routes}, {r: 0 for r in routes}
    for r in routes:
        os.environ[KNOB] = r
        for _ in range(warmup):
            fn()
    for _ in range(runs):
        for r in routes:
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
    return {r: stats(times[r]) for r in routes}, peak, top


def patch_modules():
    """The four modules of ACVNet_DDIM's attention branch (acv_ddim.py), on the GPU."""
    mods = [nn.Conv3d(40, 40, (1, 3, 3), 1, (0, 1, 1), 1, groups=40, bias=False),
            nn.Conv3d(8, 8, (1, 3, 3), 1, (0, 1, 1), 1, groups=8, bias=False),
            nn.Conv3d(16, 16, (1, 3, 3), 1, (0, 2, 2), 2, groups=16, bias=False),
            nn.Conv3d(16, 16, (1, 3, 3), 1, (0, 3, 3), 3, groups=16, bias=False)]
    return [m.cuda() for m in mods]


def call_site(x, patch, l1, l2, l3):
    """The expression of ACVNet_DDIM.train_forward on the route of the switch."""
    if train_patch.route() == "hip":
        return patch_volume_train(x, patch.weight.reshape(40, 9),
                                  torch.cat([m.weight.reshape(-1, 9) for m in (l1, l2, l3)]), PATCH_DILATION)
    y = patch(x)
    return torch.cat((l1(y[:, :8]), l2(y[:, 8:24]), l3(y[:, 24:40])), dim=1)


def function(b, runs, inner=3):
    g_, d, h, w = SHAPE
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(b, g_, d, h, w, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(b, g_, d, h, w, generator=gen).cuda()
    mods = patch_modules()
    out = []
    for frozen in (False, True):
        for m in mods:
            m.weight.requires_grad_(not frozen)

        def fwd_bwd():
            for _ in range(inner):
                x.grad = None
                for m in mods:
                    m.weight.grad = None
                call_site(x, *mods).backward(g)

        t, peak, _ = alternate(fwd_bwd, runs, warmup=1, scale=inner)
        rec = dict(case=f"patch stencils [{b},{g_},{d},{h},{w}], " + ("frozen stencils: dgwc only" if frozen else
                                                                      "all three gradients"),
                   fwd_bwd_ms=t, peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   one_tensor_mib=round(4 * x.numel() / (1 << 20), 1),
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernels(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    g_, d, h, w = SHAPE
    n, g0, ng, dl, _ = train_patch._runs(PATCH_DILATION)
    elems = b * g_ * d * h * w
    x, go = (torch.randn(b, g_, d, h, w, device="cuda") for _ in range(2))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    w1, w2 = (torch.randn(g_, 9, device="cuda") / 3 for _ in range(2))
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    table = torch.tensor(PATCH_DILATION, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.dv_patch_volume_bwd_workspace_floats(b, g_, d, h, w), device="cuda")
    shape = f"[{b},{g_},{d},{h},{w}]"
    out = []

    def record(name, fn, needed, note):
        ms = [events_ms(fn, reps) for _ in range(runs)]
        med = sorted(ms)[len(ms) // 2]
        rec = dict(kernel=name, ms=stats(ms), bytes_counted=int(needed),
                   fraction_of_8_tb_s=round(needed / (med * 1e-3) / HBM, 3), counted=note)
        print(json.dumps(rec), flush=True)
        out.append(rec)

    record(f"dv_patch_volume_runs_f32 {shape} (forward)",
           lambda: _lib.check(lib.dv_patch_volume_runs_f32(x.data_ptr(), w1.data_ptr(), w2.data_ptr(), table.data_ptr(),
                                                           y.data_ptr(), b, g_, d, h, w, n, g0, ng, dl, st), "forward"),
           8 * elems, "gwc read, out written")
    record(f"dv_patch_volume_bwd_f32 {shape}, every gradient",
           lambda: _lib.check(lib.dv_patch_volume_bwd_f32(x.data_ptr(), w1.data_ptr(), w2.data_ptr(), go.data_ptr(),
                                                          dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), ws.data_ptr(), b, g_,
                                                          d, h, w, n, g0, ng, dl, st), "backward"),
           12 * elems, "gwc and dout read, dgwc written (the partials and their merge are not counted)")
    record(f"dv_patch_volume_bwd_f32 {shape}, dgwc only",
           lambda: _lib.check(lib.dv_patch_volume_bwd_f32(x.data_ptr(), w1.data_ptr(), w2.data_ptr(), go.data_ptr(),
                                                          dx.data_ptr(), None, None, None, b, g_, d, h, w, n, g0, ng, dl, st),
                              "backward, dgwc only"),
           8 * elems, "dout read, dgwc written")
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "patch_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_patch_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
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
    print("wrote", a.out)


if __name__ == "__main__":
    main()
