"""Time the 2-D networks of ACVNet_DDIM / PWCNet_ddim training (train_net2d.py) on their two routes, DV_TRAIN_NET2D=hip and
=torch (the nn.Modules: MIOpen convolutions and BatchNorm, ATen's resize backward), alternating in one process, median of
--runs with min and max.
  nets       each feature CNN alone at [4,3,256,512] and `concatconv` alone at [4,320,64,128], forward + backward (every
             parameter wants a gradient; concatconv's input too): time and peak memory above rest;
  layers     one convolution per layer class of the feature CNNs, batch 4: forward, input gradient and weight gradient
             alone (device events), the route's kernels against MIOpen (F.conv2d under autograd);
  resize     dv_resize_bilinear_ac_bwd_f32 against ATen's backward of F.interpolate at [4,32,64,128] -> [4,32,256,512], with
             the bytes it has to move (dy read once, dx written once) as a fraction of 8 TB/s;
  acv, pcw   whole training steps (forward, loss, backward, Adam) at batch 4, 256 x 512, set up as
             tools/bench_train_step.py / tools/bench_pcw_train_step.py set them up, with the switch both ways.
Writes the record to profiles/net2d_train_bench.json (or --out), after every part, so that a part can be re-run alone.

    python tools/bench_net2d_train.py [--runs 5] [--parts nets,layers,resize,acv,pcw] [--out ...]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen layers
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

from bench_norm_train import acv_step, events_ms, pcw_step, stats  # noqa: E402
from diffuvolume_amd import ACVNet_DDIM, _env, _lib, acv_ddim, pwcnet_ddim, train2d, train_net2d  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.submodule import ACT_NONE  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_NET2D"
HBM = 8.0e12
PARTS = ("nets", "layers", "resize", "acv", "pcw")
# (name, Cin, Cout, k, stride, dilation, H, W of the input)
LAYERS = [("32 -> 32 3x3 at 128x256 (firstconv, layer1)", 32, 32, 3, 1, 1, 128, 256),
          ("64 -> 64 3x3 at 64x128 (layer2)", 64, 64, 3, 1, 1, 64, 128),
          ("128 -> 128 3x3 at 64x128 (layer3)", 128, 128, 3, 1, 1, 64, 128),
          ("128 -> 128 3x3 dilation 2 at 64x128 (layer4)", 128, 128, 3, 1, 2, 64, 128),
          ("320 -> 128 3x3 at 64x128 (concatconv, layer_refine, lastconv)", 320, 128, 3, 1, 1, 64, 128),
          ("32 -> 64 3x3 stride 2 at 128x256 (layer2.0.conv1)", 32, 64, 3, 2, 1, 128, 256),
          ("32 -> 64 1x1 stride 2 at 128x256 (layer2.0.downsample)", 32, 64, 1, 2, 1, 128, 256),
          ("128 -> 32 1x1 at 64x128 (concatconv, layer_refine)", 128, 32, 1, 1, 1, 64, 128),
          ("320 -> 320 1x1 at 64x128 (layer11)", 320, 320, 1, 1, 1, 64, 128)]
# -Rpass-analysis=kernel-resource-usage of csrc/resize_bwd.hip (hipcc, gfx950, the flags of _build.py); 256 threads per block
RESOURCES = {
    "resize_bilinear_ac_bwd_kernel<16-byte loads>": dict(vgprs=38, sgprs=54, vgpr_spills=0, sgpr_spills=0, lds_bytes=12288,
                                                         waves_per_simd=8),
    "resize_bilinear_ac_bwd_kernel<element loads>": dict(vgprs=61, sgprs=67, vgpr_spills=0, sgpr_spills=0, lds_bytes=12288,
                                                         waves_per_simd=8),
}


def alternate(fn, runs, warmup, scale=1.0):
    """fn() timed `runs` times per route, routes alternating -> per route: ms statistics, peak bytes above rest, peak."""
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


def nets(b, runs):
    out = []
    gen = torch.Generator().manual_seed(3)

    def one(name, model, call, x, params):
        model.load_state_dict(synth_state_dict(model.state_dict(), seed=1), strict=True)
        model.cuda().train()
        with torch.no_grad():
            os.environ[KNOB] = "torch"
            cot = {k: torch.randn_like(v) for k, v in call(model, x).items()}

        def fwd_bwd():
            for p in params(model):
                p.grad = None
            x.grad = None
            outs = call(model, x)
            torch.autograd.backward([outs[k] for k in cot], [cot[k] for k in cot])

        t, peak, _ = alternate(fwd_bwd, runs, warmup=2)
        rec = dict(net=name, input=list(x.shape), fwd_bwd_ms=t,
                   peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4),
                   hip_faster_with_ranges_apart=bool(t["hip"]["max"] < t["torch"]["min"]))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        model.cpu()
        torch.cuda.empty_cache()

    image = torch.rand(b, 3, 256, 512, generator=gen).cuda()
    one("ACVNet_DDIM.feature_extraction", acv_ddim.FeatureExtraction(), lambda m, x: m(x), image,
        lambda m: m.parameters())
    one("PWCNet_ddim.feature_extraction", pwcnet_ddim.FeatureExtraction(True, 12), lambda m, x: m(x), image,
        lambda m: m.parameters())

    def concat(m, x):
        if train_net2d.route() == "hip":
            return {"concat": train_net2d.Net2d(m, ("concatconv.",)).seq(m.concatconv, x)}
        return {"concat": m.concatconv(x)}

    feat = torch.randn(b, 320, 64, 128, generator=gen).cuda().requires_grad_(True)
    one("ACVNet_DDIM.concatconv", ACVNet_DDIM(192), concat, feat, lambda m: m.concatconv.parameters())
    return out


def layers(b, runs, reps=10):
    out = []
    for name, cin, cout, k, stride, dil, h, w in LAYERS:
        pad = dil if k == 3 else 0
        conv = nn.Conv2d(cin, cout, k, stride, pad, dil, bias=False).cuda()
        x = torch.randn(b, cin, h, w, device="cuda")
        planned = train_net2d._planned(conv)
        plan = train2d.TrainConvPlan(conv, ACT_NONE) if planned else None

        def forward(route, xx, ww):
            if route == "torch":
                return F.conv2d(xx, ww, None, stride, pad, dil)
            if planned:
                return train2d.ConvCatFn.apply(plan, ww, None, xx)
            conv.weight.requires_grad_(ww.requires_grad)
            return train2d.conv2d_any(conv, xx)

        rec = dict(layer=name, batch=b, hip_route="TrainConvPlan / ConvCatFn (dv_conv2d_wgrad_cat_f32)" if planned
                   else "train2d.conv2d_any", ms={})
        for what in ("forward", "input_gradient", "weight_gradient"):
            rec["ms"][what] = {}
            for route in ROUTES:
                xx = x.detach().requires_grad_(what == "input_gradient")
                ww = conv.weight.detach().requires_grad_(what == "weight_gradient")
                if what == "forward":
                    with torch.no_grad():
                        ms = [events_ms(lambda: forward(route, xx, ww), reps) for _ in range(runs)]
                else:
                    y = forward(route, xx, ww)
                    g = torch.randn_like(y)
                    leaf = xx if what == "input_gradient" else (ww if route == "torch" or planned else conv.weight)
                    ms = [events_ms(lambda: torch.autograd.grad(y, leaf, g, retain_graph=True), reps) for _ in range(runs)]
                    del y, g
                rec["ms"][what][route] = stats(ms)
            rec["ms"][what]["hip_over_torch"] = round(rec["ms"][what]["hip"]["median"] / rec["ms"][what]["torch"]["median"], 3)
        conv.weight.requires_grad_(True)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        torch.cuda.empty_cache()
    return out


def resize(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    c, h, w, hh, ww = 32, 64, 128, 256, 512
    dy = torch.randn(b, c, hh, ww, device="cuda")
    dx = torch.empty(b, c, h, w, device="cuda")
    x = torch.randn(b, c, h, w, device="cuda", requires_grad=True)
    y = F.interpolate(x, [hh, ww], mode="bilinear", align_corners=True)
    needed = 4 * (dy.numel() + dx.numel())
    hip = [events_ms(lambda: _lib.check(lib.dv_resize_bilinear_ac_bwd_f32(dy.data_ptr(), dx.data_ptr(), b * c, h, w, hh, ww,
                                                                          st), "resize bwd"), reps) for _ in range(runs)]
    aten = [events_ms(lambda: torch.autograd.grad(y, x, dy, retain_graph=True), reps) for _ in range(runs)]
    med = sorted(hip)[len(hip) // 2]
    rec = dict(case=f"[{b},{c},{h},{w}] -> [{b},{c},{hh},{ww}]", dv_resize_bilinear_ac_bwd_f32_ms=stats(hip),
               aten_upsample_bilinear2d_backward_ms=stats(aten), bytes_counted=int(needed),
               counted="dy read once, dx written once",
               fraction_of_8_tb_s=round(needed / (med * 1e-3) / HBM, 3),
               hip_over_aten=round(med / sorted(aten)[len(aten) // 2], 3), kernel_resources=RESOURCES)
    print(json.dumps(rec), flush=True)
    return rec


def whole_step(name, step, runs, **what):
    t, peak, top = alternate(step, runs, warmup=2)
    rec = dict(model=name, **what, step_ms=t, peak_gib={r: round(p / 2 ** 30, 3) for r, p in top.items()},
               peak_gib_above_rest={r: round(p / 2 ** 30, 3) for r, p in peak.items()},
               hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4),
               hip_not_slower_with_ranges_apart=bool(t["hip"]["max"] <= t["torch"]["min"]),
               hip_slower_with_ranges_apart=bool(t["hip"]["min"] > t["torch"]["max"]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "net2d_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_net2d_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               default_route=_env.KNOBS[KNOB][0])

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "resize" in parts:
        save("resize", resize(a.batch, a.runs))
    if "layers" in parts:
        save("layers", layers(a.batch, a.runs))
    if "nets" in parts:
        save("nets", nets(a.batch, a.runs))
    if "acv" in parts:
        save("acv_step", whole_step("ACVNet_DDIM", acv_step(a.batch, 256, 512), a.runs, image=[256, 512]))
    if "pcw" in parts:
        save("pcw_step", whole_step("PWCNet_ddim", pcw_step(a.batch, 256, 512), a.runs, image=[256, 512]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
