"""Time the differentiable cost-volume builders (train_volume.py, csrc/volume_bwd.hip) on their two routes, alternating in
one process, median of --runs with min and max.  DV_TRAIN_VOLUME=torch runs the PyTorch statements the builders ran
before the HIP backward existed, so the torch route is that path measured in the same process.
  functions  forward + backward of each builder at the models' training shapes: time and peak memory above rest.
             ACV gwc [4,320,64,128] D 48 G 40; ACV scaled concat [4,32,64,128] D 48 (the scale wants a gradient too);
             IGEV gwc [4,96,80,184] D 48 G 8; PCW: gwc (320 channels, 40 groups) + zero_left concat (12 channels) at
             the four scales of a 256 x 512 crop, as one function;
  kernels    each backward entry alone (device events around launches of the C ABI) with the bytes it has to move --
             the volume's gradient, the feature maps and the scale read once, every gradient written once -- as a
             fraction of 8 TB/s; the workspace traffic of ds is listed apart;
  acv / pcw  whole training steps (forward, loss, backward, Adam) set up as tools/bench_train_step.py and
             tools/bench_pcw_train_step.py set them up, with the switch both ways.  IGEV's step has no such pair: its call
             site stays on the statement (igev_volume._cost_volume_train), so the switch does not reach it;
  bits       of ACVNet_DDIM's parameter gradients, how many repeat bit for bit on two steps from the same state.
Writes the record to profiles/volume_train_bench.json (or --out; not a name matching profiles/r*_bench.json, which
tests/test_bench_contract.py takes for the round's bench line), after every part, so that a part can be re-run alone.

    python tools/bench_volume_train.py [--runs 5] [--parts functions,kernels,acv,pcw,bits] [--out ...]"""
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

from diffuvolume_amd import (ACVNet_DDIM, PWCNet_ddim, _lib, build_concat_volume_train, build_gwc_volume_train,  # noqa: E402
                             model_loss_kitti12, model_loss_train)
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_VOLUME"
HBM = 8.0e12
PARTS = ("functions", "kernels", "acv", "pcw", "bits")
PCW_SCALES = [(64, 128, 48), (32, 64, 24), (16, 32, 12), (8, 16, 6)]          # (h, w, D) of a 256 x 512 crop


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
    """The rule of the call sites' default: hip is not slower than torch by more than the spread of the runs."""
    spread = max(t[r]["max"] - t[r]["min"] for r in ROUTES)
    return bool(t["hip"]["median"] <= t["torch"]["median"] + spread), round(spread, 4)


def leaf(*shape):
    return torch.randn(*shape, device="cuda").requires_grad_(True)


def function_cases(b):
    """name -> (leaves, forward): forward() builds the volumes of the case from the leaves."""
    cases = {}
    fl, fr = leaf(b, 320, 64, 128), leaf(b, 320, 64, 128)
    cases["acv_gwc [%d,320,64,128] D48 G40" % b] = ([fl, fr], lambda: [build_gwc_volume_train(fl, fr, 48, 40)])
    cl, cr, s = leaf(b, 32, 64, 128), leaf(b, 32, 64, 128), torch.rand(b, 48, 64, 128, device="cuda").requires_grad_(True)
    cases["acv_scaled_concat [%d,32,64,128] D48" % b] = ([cl, cr, s], lambda: [build_concat_volume_train(cl, cr, 48, scale=s)])
    ml, mr = leaf(b, 96, 80, 184), leaf(b, 96, 80, 184)
    cases["igev_gwc [%d,96,80,184] D48 G8" % b] = ([ml, mr], lambda: [build_gwc_volume_train(ml, mr, 48, 8)])
    pcw = [(leaf(b, 320, h, w), leaf(b, 320, h, w), leaf(b, 12, h, w), leaf(b, 12, h, w), d) for h, w, d in PCW_SCALES]
    cases["pcw_four_scales gwc 320/40 + zero_left concat 12, 256x512"] = (
        [t for row in pcw for t in row[:4]],
        lambda: [v for gl, gr, kl, kr, d in pcw for v in (build_gwc_volume_train(gl, gr, d, 40),
                                                            build_concat_volume_train(kl, kr, d, zero_left=True))])
    return cases


def functions(b, runs, inner=3):
    out = []
    for name, (ins, forward) in function_cases(b).items():
        os.environ[KNOB] = "hip"
        cots = [torch.randn_like(v) for v in forward()]
        os.environ.pop(KNOB)

        def fwd_bwd():
            for _ in range(inner):
                for t in ins:
                    t.grad = None
                vols = forward()
                torch.autograd.backward(vols, cots)

        t, peak, _ = alternate(fwd_bwd, runs, warmup=1, scale=inner)
        rec = dict(case=name, fwd_bwd_ms=t, peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   volume_mib=round(sum(4 * c.numel() for c in cots) / (1 << 20), 1),
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del cots
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

    for tag, (c, h, w, d, g) in (("acv (= pcw 1/4)", (320, 64, 128, 48, 40)), ("igev", (96, 80, 184, 48, 8))):
        ref = torch.randn(b, c, h, w, device="cuda")
        tgt = torch.randn(b, c, h, w, device="cuda")
        dvol = torch.randn(b, g, d, h, w, device="cuda")
        dref, dtgt = torch.empty_like(ref), torch.empty_like(tgt)
        record(f"dv_gwc_volume_bwd_f32 {tag} [{b},{c},{h},{w}] D{d} G{g}",
               lambda: _lib.check(lib.dv_gwc_volume_bwd_f32(ref.data_ptr(), tgt.data_ptr(), dvol.data_ptr(), dref.data_ptr(),
                                                            dtgt.data_ptr(), b, c, h, w, d, g, st), "gwc bwd"),
               4 * (dvol.numel() + 4 * ref.numel()))
        del ref, tgt, dvol, dref, dtgt
    c, h, w, d = 32, 64, 128, 48
    ref, tgt = torch.randn(b, c, h, w, device="cuda"), torch.randn(b, c, h, w, device="cuda")
    s, dvol = torch.rand(b, d, h, w, device="cuda"), torch.randn(b, 2 * c, d, h, w, device="cuda")
    dref, dtgt, ds = torch.empty_like(ref), torch.empty_like(tgt), torch.empty_like(s)
    n_ws = lib.dv_concat_volume_bwd_workspace_floats(b, c, h, w, d)
    ws = torch.empty(n_ws, device="cuda")
    record(f"dv_concat_volume_bwd_f32 acv scaled [{b},{c},{h},{w}] D{d}, dref + dtgt + ds",
           lambda: _lib.check(lib.dv_concat_volume_bwd_f32(ref.data_ptr(), tgt.data_ptr(), s.data_ptr(), dvol.data_ptr(),
                                                           dref.data_ptr(), dtgt.data_ptr(), ds.data_ptr(), _lib.ptr(ws), b, c,
                                                           h, w, d, 0, st), "concat bwd"),
           4 * (dvol.numel() + 4 * ref.numel() + 2 * s.numel()), 4 * 2 * n_ws)
    del ref, tgt, s, dvol, dref, dtgt, ds, ws
    c = 12
    for h, w, d in PCW_SCALES[:2]:
        dvol = torch.randn(b, 2 * c, d, h, w, device="cuda")
        dref, dtgt = (torch.empty(b, c, h, w, device="cuda") for _ in range(2))
        record(f"dv_concat_volume_bwd_f32 pcw zero_left [{b},{c},{h},{w}] D{d}, dref + dtgt",
               lambda: _lib.check(lib.dv_concat_volume_bwd_f32(None, None, None, dvol.data_ptr(), dref.data_ptr(),
                                                               dtgt.data_ptr(), None, None, b, c, h, w, d, 1, st), "concat bwd"),
               4 * (dvol.numel() + 2 * dref.numel()))
    return out


def pair_step(which, b, h, w):
    """ACVNet_DDIM / PWCNet_ddim: the step of tools/bench_train_step.py / tools/bench_pcw_train_step.py."""
    model = (ACVNet_DDIM if which == "acv" else PWCNet_ddim)(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
    model = model.cuda().train()
    x = synth_stereo_batch(b, h, w, seed=5)
    left, right, disp, gt = (x[k].cuda() for k in ("left", "right", "disp", "gt"))
    if which == "pcw":
        disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    mask = (gt < 192) & (gt > 0)
    loss_fn = model_loss_train if which == "acv" else model_loss_kitti12
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))

    def fwd_bwd():
        loss = loss_fn(model(left, right, None, disp, None), gt, mask)
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


def acv_gradient_bits(b, h, w):
    """Two forward + backward passes of ACVNet_DDIM from the same weights, BatchNorm state and random draws, per route:
    the parameters whose gradients differ in any bit."""
    model, fwd_bwd, _ = pair_step("acv", b, h, w)
    state = copy.deepcopy(model.state_dict())
    out = {}
    for r in ROUTES:
        os.environ[KNOB] = r
        grads = []
        for _ in range(2):
            model.load_state_dict(state, strict=True)
            model.zero_grad(set_to_none=True)
            torch.manual_seed(3)
            fwd_bwd()
            grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        differ = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
        out[r] = dict(parameters_with_gradient=len(grads[0]), parameters_that_repeat=len(grads[0]) - len(differ),
                      parameters_that_differ=len(differ), first=differ[:8])
    os.environ.pop(KNOB)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "volume_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_volume_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"))

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "functions" in parts:
        save("functions", functions(a.batch, a.runs))
    if "kernels" in parts:
        save("backward_kernels", kernels(a.batch, a.runs))
    if "acv" in parts:
        save("acv_step", whole_step("ACVNet_DDIM", pair_step("acv", a.batch, 256, 512)[2], a.runs, image=[256, 512]))
    if "pcw" in parts:
        save("pcw_step", whole_step("PWCNet_ddim", pair_step("pcw", a.batch, 256, 512)[2], a.runs, image=[256, 512]))
    if "bits" in parts:
        save("acv_two_steps_same_gradient_bits", acv_gradient_bits(a.batch, 256, 512))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
