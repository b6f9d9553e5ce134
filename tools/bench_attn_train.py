"""Time the bottleneck window attention of ACVNet_DDIM's hourglasses in training (train_attn.py, csrc/window_attn.hip
forward, csrc/window_attn_bwd.hip backward) on its two routes, alternating in one process, median of --runs with min and
max.  DV_TRAIN_ATTN=torch runs the PyTorch statements the call site ran before the backward kernel existed, so the torch
route is that path measured in the same process.
  function   forward + backward of window_attention_train at [4,128,12,16,32] (the bottleneck of a 256 x 512 pair at batch
             4) with every gradient: time and peak memory above rest; and the hip route with frozen parameters (dx only);
  kernels    dv_window_attn3d_bwd_f32 alone (device events around launches of the C ABI) with every gradient, its stage 1
             alone (dx only: one block per window) against the 12 B per element it has to move (x and dout read, dx
             written) as a fraction of 8 TB/s, its GEMM stage (the entry with every gradient less the entry without dqkv_w
             and dproj_w, so including stage 1's stores of Om and dQKV) against the 157.3 TFLOP/s fp32 MFMA
             peak, beside the same two products on dv_conv3d_wgrad_f32 at k = 1 (what the stage ran on at first) and the
             forward dv_window_attn3d_f32;
  acv        whole ACVNet_DDIM training steps (forward, loss, backward, Adam) at batch 4, 256 x 512, set up as
             tools/bench_train_step.py sets them up, with the switch both ways.
Writes the record to profiles/attn_train_bench.json (or --out), after every part, so that a part can be re-run alone.

    python tools/bench_attn_train.py [--runs 5] [--parts function,kernels,acv] [--out ...]"""
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

from diffuvolume_amd import ACVNet_DDIM, _env, _lib, model_loss_train, window_attention_train  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.acv_ddim import _WindowAttention  # noqa: E402
from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch  # noqa: E402

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_ATTN"
HBM = 8.0e12
PEAK = 157.3e12                                         # fp32 MFMA peak of the MI355X
PARTS = ("function", "kernels", "acv")
SHAPE = (128, 12, 16, 32)                               # (C, D, H, W): the bottleneck of a 256 x 512 pair
# -Rpass-analysis=kernel-resource-usage of csrc/window_attn_bwd.hip and, for the split sum, csrc/splitk_reduce.hip (hipcc,
# gfx950, the flags of _build.py).
RESOURCES = {
    "window_attn_bwd_kernel (256 threads, one block per window)": dict(
        vgprs=255, agprs=52, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0, lds_bytes=106112, waves_per_simd=1),
    "attn_wgrad_kernel (256 threads, 128 x 128 tile of one split)": dict(vgprs=151, agprs=0, vgpr_spills=0, sgpr_spills=0,
                                                                         scratch_bytes=0, lds_bytes=34816, waves_per_simd=3),
    "splitk_sum_kernel": dict(vgprs=8, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0, lds_bytes=0, waves_per_simd=8),
    "attn_bwd_bias_kernel (one wave per feature)": dict(vgprs=10, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0, lds_bytes=0,
                                                        waves_per_simd=8),
    "attn_bwd_dbp_kernel (256 threads, one block per channel)": dict(vgprs=12, vgpr_spills=0, sgpr_spills=0, scratch_bytes=0,
                                                                     lds_bytes=32, waves_per_simd=8),
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


def attention_module():
    ab = _WindowAttention(128, 16)
    ab.load_state_dict(synth_state_dict(ab.state_dict(), seed=3), strict=True)
    return ab.cuda()


def function(b, runs, inner=3):
    c, d, h, w = SHAPE
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(b, c, d, h, w, generator=gen).cuda().requires_grad_(True)
    g = torch.randn(b, c, d, h, w, generator=gen).cuda()
    ab = attention_module()
    params = [ab.qkv_3d.weight, ab.qkv_3d.bias, ab.final1x1.weight, ab.final1x1.bias]
    out = []
    for frozen in (False, True):
        for p in params:
            p.requires_grad_(not frozen)

        def fwd_bwd():
            for _ in range(inner):
                x.grad = None
                for p in params:
                    p.grad = None
                window_attention_train(x, *params, ab.num_heads).backward(g)

        t, peak, _ = alternate(fwd_bwd, runs, warmup=1, scale=inner)
        rec = dict(case=f"window attention [{b},{c},{d},{h},{w}], " + ("frozen parameters: dx only" if frozen else
                                                                       "every gradient"),
                   fwd_bwd_ms=t, peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   one_tensor_mib=round(4 * x.numel() / (1 << 20), 1),
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def kernels(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    c, d, h, w = SHAPE
    size = (b, c, d, h, w, 16)
    elems = b * c * d * h * w
    tokens = b * d * h * w
    x, go = (torch.randn(b, c, d, h, w, device="cuda") for _ in range(2))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    ab = attention_module()
    wq, bq, bp = (t.detach().contiguous() for t in (ab.qkv_3d.weight, ab.qkv_3d.bias, ab.final1x1.bias))
    wp = ab.final1x1.weight.detach().reshape(c, c).contiguous()
    dwq, dbq, dwp, dbp = (torch.empty_like(t) for t in (wq, bq, wp, bp))
    ws = torch.empty(lib.dv_window_attn3d_bwd_workspace_floats(*size), device="cuda")
    big = torch.randn(b, 3 * c, d, h, w, device="cuda")                       # stands for dQKV in the GEMM stage alone
    wg = [torch.empty(lib.dv_conv3d_wgrad_workspace_floats(b, c, d, h, w, co, 1, 1), device="cuda") for co in (3 * c, c)]
    shape = f"[{b},{c},{d},{h},{w}]"
    out = []

    def record(name, fn, note, nbytes=None, flop=None):
        ms = [events_ms(fn, reps) for _ in range(runs)]
        med = sorted(ms)[len(ms) // 2]
        rec = dict(kernel=name, ms=stats(ms), counted=note)
        if nbytes is not None:
            rec.update(bytes_counted=int(nbytes), fraction_of_8_tb_s=round(nbytes / (med * 1e-3) / HBM, 4))
        if flop is not None:
            rec.update(flop_counted=int(flop), tflops=round(flop / (med * 1e-3) / 1e12, 2),
                       fraction_of_fp32_mfma_peak=round(flop / (med * 1e-3) / PEAK, 4))
        print(json.dumps(rec), flush=True)
        out.append(rec)

    ins = (x.data_ptr(), wq.data_ptr(), bq.data_ptr(), wp.data_ptr())
    attn_flop = tokens * (2.0 * c * 3 * c + 2.0 * c * c + 4.0 * 64 * c)        # the forward's count (submodule.window_attention)
    record(f"dv_window_attn3d_f32 {shape} (forward)",
           lambda: _lib.check(lib.dv_window_attn3d_f32(*ins, bp.data_ptr(), y.data_ptr(), *size, st), "forward"),
           "x read, out written; qkv GEMM, attention and projection", nbytes=8 * elems, flop=attn_flop)
    record(f"dv_window_attn3d_bwd_f32 {shape}, every gradient",
           lambda: _lib.check(lib.dv_window_attn3d_bwd_f32(*ins, go.data_ptr(), dx.data_ptr(), dwq.data_ptr(), dbq.data_ptr(),
                                                           dwp.data_ptr(), dbp.data_ptr(), ws.data_ptr(), *size, st),
                              "backward"),
           "x and dout read, dx written (Om and dQKV through the workspace and the sums are not counted)", nbytes=12 * elems)
    record(f"dv_window_attn3d_bwd_f32 {shape}, dx only (stage 1 without its workspace stores)",
           lambda: _lib.check(lib.dv_window_attn3d_bwd_f32(*ins, go.data_ptr(), dx.data_ptr(), None, None, None, None, None,
                                                           *size, st), "backward, dx only"),
           "x and dout read, dx written; recomputed forward (without the projection's output) + 2x its GEMMs backward",
           nbytes=12 * elems, flop=tokens * (2.0 * c * 3 * c + 2.0 * c * c + 2.0 * c * 3 * c + 10.0 * 64 * c))
    record(f"dv_window_attn3d_bwd_f32 {shape}, dx + dqkv_b + dproj_b (no GEMM stage, no Om / dQKV stores)",
           lambda: _lib.check(lib.dv_window_attn3d_bwd_f32(*ins, go.data_ptr(), dx.data_ptr(), None, dbq.data_ptr(), None,
                                                           dbp.data_ptr(), ws.data_ptr(), *size, st), "backward, no weights"),
           "x and dout read, dx written", nbytes=12 * elems)
    gemm_flop = 2.0 * tokens * c * (3 * c + c)
    every, rest = (out[i]["ms"]["median"] for i in (1, 3))
    rec = dict(kernel=f"GEMM stage: every gradient less the entry without dqkv_w / dproj_w, over {tokens} tokens",
               ms=round(every - rest, 4), counted="dWqkv = dQKV^T X and dWp = dY^T Om as split-K GEMMs with their split sums; the "
               "difference also holds stage 1's stores of Om and dQKV (4 x 12 MiB)", flop_counted=int(gemm_flop),
               tflops=round(gemm_flop / ((every - rest) * 1e-3) / 1e12, 2),
               fraction_of_fp32_mfma_peak=round(gemm_flop / ((every - rest) * 1e-3) / PEAK, 4))
    print(json.dumps(rec), flush=True)
    out.append(rec)
    record(f"the same two products on dv_conv3d_wgrad_f32 at k = 1 (32 x 32 tiles; what the stage ran on at first)",
           lambda: (_lib.check(lib.dv_conv3d_wgrad_f32(x.data_ptr(), big.data_ptr(), dwq.data_ptr(), wg[0].data_ptr(), b, c, d, h,
                                                       w, 3 * c, 1, 1, st), "wgrad qkv"),
                    _lib.check(lib.dv_conv3d_wgrad_f32(y.data_ptr(), go.data_ptr(), dwp.data_ptr(), wg[1].data_ptr(), b, c, d, h,
                                                       w, c, 1, 1, st), "wgrad proj")),
           "128 -> 384 and 128 -> 128 over the tokens, with their split sums", flop=gemm_flop)
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_attn_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE"),
               default_route=_env.KNOBS[KNOB][0], peak_tflops=PEAK / 1e12, kernel_resources=RESOURCES)

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
