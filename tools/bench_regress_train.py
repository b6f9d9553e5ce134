"""Time the differentiable regression tail (train_tail.py, csrc/regress_bwd.hip) on its two routes, alternating in one
process, median of --runs:
  1. the function alone at cost [4,48,64,128] (the bench shape 4 x 256 x 512 at quarter resolution), align_corners 0 and 1:
     forward + backward time and peak memory on DV_TRAIN_TAIL=hip against =torch, and the backward kernel's time next to
     the forward kernel's (device events around launches of the C ABI);
  2. whole training steps (forward, loss, backward, Adam) of ACVNet_DDIM and PWCNet_ddim at batch 4, 256 x 512 on both
     routes: step time and peak memory.  The torch route is what the heads ran on before the HIP backward existed;
  3. whether two whole ACVNet_DDIM steps from the same state give the same gradient bits on each route.
Writes the record to profiles/train_tail_bench.json (or --out; not a name matching profiles/r*_bench.json, which
tests/test_bench_contract.py takes for the round's bench line).

    python tools/bench_regress_train.py [--runs 5] [--skip-models] [--out profiles/train_tail_bench.json]"""
import argparse
import copy
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

from diffuvolume_amd import (ACVNet_DDIM, PWCNet_ddim, _lib, model_loss_kitti12, model_loss_train,  # noqa: E402
                             upsample_softmax_regress_train)
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
GIB = float(1 << 30)


def median(v):
    return sorted(v)[len(v) // 2]


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


def alternate(fn, runs, warmup):
    """fn() timed `runs` times per route, routes alternating; (ms lists, peak bytes above the resting allocation, peak bytes)."""
    times, peak, top = {r: [] for r in ROUTES}, {r: 0 for r in ROUTES}, {r: 0 for r in ROUTES}
    for r in ROUTES:
        os.environ["DV_TRAIN_TAIL"] = r
        for _ in range(warmup):
            fn()
    for _ in range(runs):
        for r in ROUTES:
            os.environ["DV_TRAIN_TAIL"] = r
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            rest = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[r].append((time.perf_counter() - t0) * 1e3)
            peak[r] = max(peak[r], torch.cuda.max_memory_allocated() - rest)
            top[r] = max(top[r], torch.cuda.max_memory_allocated())
    os.environ.pop("DV_TRAIN_TAIL")
    return times, peak, top


def function_alone(shape, ac, runs, inner=10):
    b, d, h, w = shape
    cost = torch.randn(*shape, device="cuda").requires_grad_(True)
    g = torch.randn(b, 4 * h, 4 * w, device="cuda")

    def fwd_bwd():
        for _ in range(inner):
            cost.grad = None
            upsample_softmax_regress_train(cost, align_corners=ac).backward(g)

    times, peak, _ = alternate(fwd_bwd, runs, warmup=1)
    lib = _lib.load()
    c = cost.detach()
    disp, dcost = torch.empty_like(g), torch.empty_like(c)
    s = _lib.stream_ptr()
    fwd = events_ms(lambda: _lib.check(lib.dv_upsample_softmax_regress_f32(c.data_ptr(), disp.data_ptr(), None, b, d, h, w,
                                                                           int(ac), s), "forward"), 20)
    bwd = events_ms(lambda: _lib.check(lib.dv_upsample_softmax_regress_bwd_f32(c.data_ptr(), disp.data_ptr(), g.data_ptr(),
                                                                               dcost.data_ptr(), None, b, d, h, w, int(ac),
                                                                               s), "backward"), 20)
    rec = dict(shape=list(shape), align_corners=int(ac),
               fwd_bwd_ms={r: [round(t / inner, 4) for t in v] for r, v in times.items()},
               fwd_bwd_ms_median={r: round(median(v) / inner, 4) for r, v in times.items()},
               peak_mib={r: round(p / (1 << 20), 2) for r, p in peak.items()},
               forward_kernel_ms=round(fwd, 4), backward_kernel_ms=round(bwd, 4), backward_over_forward=round(bwd / fwd, 3))
    rec["hip_over_torch"] = round(rec["fwd_bwd_ms_median"]["hip"] / rec["fwd_bwd_ms_median"]["torch"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def model_setup(which, batch, height, width):
    model = (ACVNet_DDIM if which == "acv" else PWCNet_ddim)(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    x = synth_stereo_batch(batch, height, width, seed=5)
    left, right, disp, gt = (x[k].cuda() for k in ("left", "right", "disp", "gt"))
    if which == "pcw":
        disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(height // 4, width // 4), mode="bilinear") / 4
    mask = (gt < 192) & (gt > 0)
    loss_fn = model_loss_train if which == "acv" else model_loss_kitti12

    def fwd_bwd(m):
        outs = m(left, right, None, disp, None)
        loss = loss_fn(outs, gt, mask)
        loss.backward()
        return float(loss.detach())

    return model, fwd_bwd


def whole_step(which, batch, height, width, runs):
    model, fwd_bwd = model_setup(which, batch, height, width)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))

    def step():
        opt.zero_grad()
        fwd_bwd(model)
        opt.step()

    times, peak, top = alternate(step, runs, warmup=2)
    rec = dict(model=which, batch=batch, image=[height, width],
               step_ms={r: [round(t, 2) for t in v] for r, v in times.items()},
               step_ms_median={r: round(median(v), 2) for r, v in times.items()},
               peak_gib={r: round(p / GIB, 3) for r, p in top.items()},
               peak_gib_above_rest={r: round(p / GIB, 3) for r, p in peak.items()})
    rec["hip_over_torch"] = round(rec["step_ms_median"]["hip"] / rec["step_ms_median"]["torch"], 4)
    print(json.dumps(rec), flush=True)
    return rec


def acv_gradient_bits(batch, height, width):
    """Two forward + backward passes of ACVNet_DDIM from the same weights, BatchNorm state and random draws, per route:
    the parameters whose gradients differ in any bit."""
    model, fwd_bwd = model_setup("acv", batch, height, width)
    state = copy.deepcopy(model.state_dict())
    out = {}
    for r in ROUTES:
        os.environ["DV_TRAIN_TAIL"] = r
        grads = []
        for _ in range(2):
            model.load_state_dict(state, strict=True)
            model.zero_grad(set_to_none=True)
            torch.manual_seed(3)
            fwd_bwd(model)
            grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        differ = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
        out[r] = dict(parameters_with_gradient=len(grads[0]), parameters_that_differ=len(differ), first=differ[:8])
    os.environ.pop("DV_TRAIN_TAIL")
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_tail_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    shape = (a.batch, 48, a.height // 4, a.width // 4)
    rec = dict(tool="tools/bench_regress_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               function=[function_alone(shape, ac, a.runs) for ac in (False, True)])
    if not a.skip_models:
        rec["steps"] = [whole_step(which, a.batch, a.height, a.width, a.runs) for which in ("acv", "pcw")]
        torch.cuda.empty_cache()
        rec["acv_two_steps_same_gradient_bits"] = acv_gradient_bits(a.batch, a.height, a.width)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
