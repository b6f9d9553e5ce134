"""Time IGEV's real MobileNetV2 backbone (diffuvolume_amd/mobilenetv2.py) on the HIP kernels against the same module on
PyTorch / MIOpen, alternating in one process, median of --runs with min and max.
  pyramid   `Feature(MobileNetV2Features())` in eval at [4,3,384,1248]: the HIP walk against the TORCH route;
  train     forward + backward of the pyramid (every parameter wants a gradient, BatchNorm frozen): TRAIN against TORCH;
  layers    one layer per class at batch 4, eval, conv + BatchNorm + activation: depthwise stride 1, depthwise stride 2,
            1x1 expand (+ ReLU6), 1x1 project with the skip;
  entries   dv_dwconv3x3_f32 and dv_dwconv3x3_bwd_f32 alone with the bytes they have to move as a fraction of 8 TB/s.
            Counted: forward x read once + out written once; dx launch dy read once + dx written once; dw launch x and dy
            read once (the weights, scale, shift and the dw partials are below 0.1 % of that);
  model     one whole `IGEVStereo_ddim` forward at KITTI15 size (bench.py's kitti15 workload) with the real backbone beside
            the stub's.
Writes the record to profiles/mobilenetv2_bench.json (or --out) after every part, so that a part can be re-run alone.

    python tools/bench_mobilenetv2.py [--runs 5] [--parts pyramid,train,layers,entries,model] [--out ...]"""
import argparse
import json
import os
import sys
import time
import types
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search for the MIOpen layers
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402
from torch import nn  # noqa: E402

import bench  # noqa: E402
from bench_norm_train import events_ms, stats  # noqa: E402
from diffuvolume_amd import _lib  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.igev_front2d import Feature, feature_pyramid  # noqa: E402
from diffuvolume_amd.igev_layers import ACT_NONE, ACT_RELU6, HIP, TORCH, TRAIN, freeze_bn  # noqa: E402
from diffuvolume_amd.mobilenetv2 import MobileNetV2Features  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict  # noqa: E402

HBM = 8.0e12
PARTS = ("pyramid", "train", "layers", "entries", "model")
# -Rpass-analysis=kernel-resource-usage of csrc/dwconv2d.hip (hipcc, gfx950, the flags of _build.py); 256 threads per block,
# no LDS anywhere; "vec" = 16-byte loads and stores, "elem" = the element path
RESOURCES = {
    "dwconv_fwd_kernel<stride 1>": dict(vgprs=dict(vec=56, elem=60), lds_bytes=0, vgpr_spills=0, sgpr_spills=0, waves_per_simd=8),
    "dwconv_fwd_kernel<stride 2>": dict(vgprs=dict(vec=59, elem=70), lds_bytes=0, vgpr_spills=0, sgpr_spills=0,
                                        waves_per_simd=dict(vec=8, elem=7)),
    "dwconv_dx_s2_kernel": dict(vgprs=dict(vec=30, elem=34), lds_bytes=0, vgpr_spills=0, sgpr_spills=0, waves_per_simd=8),
    "dwconv_dw_kernel<stride 1>": dict(vgprs=dict(vec=56, elem=66), lds_bytes=0, vgpr_spills=0, sgpr_spills=0,
                                       waves_per_simd=dict(vec=8, elem=7)),
    "dwconv_dw_kernel<stride 2>": dict(vgprs=dict(vec=66, elem=82), lds_bytes=0, vgpr_spills=0, sgpr_spills=0,
                                       waves_per_simd=dict(vec=7, elem=5)),
    "dwconv_dw_combine_kernel": dict(vgprs=18, lds_bytes=0, vgpr_spills=0, sgpr_spills=0, waves_per_simd=8),
}


def alternate(fns, runs, warmup=2):
    """{name: fn} timed `runs` times each, alternating -> {name: ms statistics}."""
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    for _ in range(runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in times.items()}


def verdict(t, a, b):
    return dict(ratio=round(t[a]["median"] / t[b]["median"], 4), faster_with_ranges_apart=bool(t[a]["max"] < t[b]["min"]),
                slower_with_ranges_apart=bool(t[a]["min"] > t[b]["max"]))


def feature(train):
    f = Feature(MobileNetV2Features())
    f.load_state_dict(synth_state_dict(f.state_dict(), seed=21), strict=True)
    f = f.cuda()
    if train:
        f.train()
        freeze_bn(f)
        return f
    return f.eval()


def pyramid(b, h, w, runs):
    f, x = feature(False), torch.rand(b, 3, h, w, device="cuda") * 2 - 1

    def run(route):
        with torch.no_grad():
            return feature_pyramid(route, f, x)

    t = alternate({"hip": lambda: run(HIP), "torch": lambda: run(TORCH)}, runs)
    rec = dict(input=[b, 3, h, w], forward_ms=t, hip_over_torch=verdict(t, "hip", "torch"))
    print(json.dumps(rec), flush=True)
    return rec


def train(b, h, w, runs):
    f, x = feature(True), torch.rand(b, 3, h, w, device="cuda") * 2 - 1
    with torch.no_grad():
        cots = [torch.randn_like(o) for o in feature_pyramid(TORCH, f, x)]

    def run(route):
        f.zero_grad(set_to_none=True)
        torch.autograd.backward(feature_pyramid(route, f, x), cots)

    t = alternate({"hip": lambda: run(TRAIN), "torch": lambda: run(TORCH)}, runs)
    rec = dict(input=[b, 3, h, w], fwd_bwd_ms=t, hip_over_torch=verdict(t, "hip", "torch"))
    print(json.dumps(rec), flush=True)
    return rec


# (class, Cin, Cout, depthwise, stride, activation, skip, H, W of the input): the 1/4 level of a 384 x 1248 image and the
# stride-2 layer that produces it
LAYERS = [("depthwise 3x3 stride 1 + BN + ReLU6, 144 ch at 96x312 (blocks.1.1)", 144, 144, True, 1, ACT_RELU6, False, 96, 312),
          ("depthwise 3x3 stride 2 + BN + ReLU6, 96 ch at 192x624 (blocks.1.0)", 96, 96, True, 2, ACT_RELU6, False, 192, 624),
          ("1x1 expand + BN + ReLU6, 24 -> 144 at 96x312 (blocks.1.1)", 24, 144, False, 1, ACT_RELU6, False, 96, 312),
          ("1x1 project + BN + skip, 144 -> 24 at 96x312 (blocks.1.1)", 144, 24, False, 1, ACT_NONE, True, 96, 312)]


def layers(b, runs, reps=20):
    out = []
    for name, cin, cout, dw, stride, act, skip, h, w in LAYERS:
        conv = (nn.Conv2d(cin, cin, 3, stride, 1, groups=cin, bias=False) if dw else nn.Conv2d(cin, cout, 1, bias=False)).cuda()
        bn = nn.BatchNorm2d(cout).cuda().eval()
        bn.load_state_dict(synth_state_dict(bn.state_dict(), seed=3))
        x = torch.randn(b, cin, h, w, device="cuda")
        res = torch.randn(b, cout, h, w, device="cuda") if skip else None

        def run(route):
            with torch.no_grad():
                return route.dwconv(conv, x, bn, act) if dw else route.conv(conv, x, bn, act, residual=res)

        ms = {}
        for _ in range(runs):
            for k, route in (("hip", HIP), ("torch", TORCH)):
                ms.setdefault(k, []).append(events_ms(lambda: run(route), reps))
        t = {k: stats(v) for k, v in ms.items()}
        rec = dict(layer=name, batch=b, forward_ms=t, hip_over_torch=verdict(t, "hip", "torch"))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        torch.cuda.empty_cache()
    return out


def entries(b, runs, reps=20):
    lib, st, out = _lib.load(), _lib.stream_ptr(), []
    for c, h, w, stride in ((144, 96, 312, 1), (96, 192, 624, 2), (32, 192, 624, 1)):
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        x, wt = torch.randn(b, c, h, w, device="cuda"), torch.randn(c, 9, device="cuda")
        sc, sh = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda")
        y, dy = torch.empty(b, c, ho, wo, device="cuda"), torch.randn(b, c, ho, wo, device="cuda")
        dx, dw = torch.empty_like(x), torch.empty_like(wt)
        ws = _lib.workspace("dv_dwconv3x3_bwd_workspace_floats", x.device, b, c, h, w, stride)
        p = lambda t: 0 if t is None else t.data_ptr()                                            # noqa: E731
        calls = {
            "forward (BN + ReLU6 inside)": (lambda: _lib.check(lib.dv_dwconv3x3_f32(
                p(x), p(wt), p(sc), p(sh), p(y), b, c, h, w, stride, 1, 6.0, st), "fwd"), 4 * (x.numel() + y.numel())),
            "backward, dx alone": (lambda: _lib.check(lib.dv_dwconv3x3_bwd_f32(
                0, p(wt), p(dy), p(dx), 0, 0, b, c, h, w, stride, st), "dx"), 4 * (dy.numel() + dx.numel())),
            "backward, dw alone": (lambda: _lib.check(lib.dv_dwconv3x3_bwd_f32(
                p(x), 0, p(dy), 0, p(dw), p(ws), b, c, h, w, stride, st), "dw"), 4 * (x.numel() + dy.numel())),
        }
        for what, (fn, nbytes) in calls.items():
            ms = [events_ms(fn, reps) for _ in range(runs)]
            med = sorted(ms)[len(ms) // 2]
            rec = dict(entry=what, case=f"[{b},{c},{h},{w}] stride {stride}", ms=stats(ms), bytes_counted=int(nbytes),
                       fraction_of_8_tb_s=round(nbytes / (med * 1e-3) / HBM, 3))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return dict(cases=out, kernel_resources=RESOURCES)


def model(runs, ddim_steps, gru_iters):
    """bench.py's kitti15 workload, and the same model with the real backbone in place of the stub's."""
    wl = types.SimpleNamespace(workload="kitti15", batch=4, height=384, width=1248, ddim_steps=ddim_steps, gru_iters=gru_iters)
    dev = torch.device("cuda:0")
    stub, stub_step, what = bench.flavour_workload(wl, 0, dev)
    real, real_step, _ = bench.flavour_workload(wl, 0, dev)
    real.feature = Feature(MobileNetV2Features())
    real.feature.load_state_dict(synth_state_dict(real.feature.state_dict(), seed=7), strict=True)
    real.to(dev).eval()

    def run(step):
        torch.manual_seed(1234)
        with torch.no_grad():
            step()

    t = alternate({"real": lambda: run(real_step), "stub": lambda: run(stub_step)}, runs, warmup=1)
    rec = dict(workload=what, forward_ms=t, pairs_per_s={k: round(4e3 / v["median"], 3) for k, v in t.items()},
               real_over_stub=verdict(t, "real", "stub"))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1248)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ddim-steps", type=int, default=20)
    ap.add_argument("--gru-iters", type=int, default=32)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mobilenetv2_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_mobilenetv2.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0), runs=a.runs,
               batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"))

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "entries" in parts:
        save("entries", entries(a.batch, a.runs))
    if "layers" in parts:
        save("layers", layers(a.batch, a.runs))
    if "pyramid" in parts:
        save("pyramid", pyramid(a.batch, a.height, a.width, a.runs))
    if "train" in parts:
        save("train", train(a.batch, a.height, a.width, a.runs))
    if "model" in parts:
        save("model", model(a.runs, a.ddim_steps, a.gru_iters))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
