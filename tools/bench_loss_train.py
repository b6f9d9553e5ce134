"""Time the masked training losses on their two routes, DV_TRAIN_LOSS=hip (csrc/masked_loss.hip) and =torch (the reference's
expression: a boolean gather per prediction), alternating in one process, median of --runs with min and max.
  function   the loss alone, forward + backward, at the three workloads' shapes -- model_loss_train (4 predictions) and
             model_loss_kitti12 (6) at [4,256,512], sequence_loss (22 + 1) at [4,1,320,736]: time, peak memory above rest
             and host synchronisations per call (torch.cuda.set_sync_debug_mode) on each route;
  kernels    dv_masked_loss_fwd_f32 (both launches) and dv_masked_loss_bwd_f32 alone (device events), with the counted
             bytes -- forward 4K + 5 per pixel, backward 8K + 5 (every prediction read once, gt and a byte of mask read
             once, every gradient written once) -- as a fraction of 8 TB/s, and the kernels' resources;
  acv, pcw, igev   whole training steps (forward, loss, backward, optimizer) of ACVNet_DDIM and PWCNet_ddim at batch 4,
             256 x 512 and of IGEVStereo_ddim at batch 4, 320 x 736, 22 iterations, with the switch both ways, and the
             share of the step the loss takes on each route (the function's time over the step's).
Writes the record to profiles/loss_train_bench.json (or --out) after every part, so that a part can be re-run alone.

    python tools/bench_loss_train.py [--runs 5] [--parts function,kernels,acv,pcw,igev] [--out ...]"""
import argparse
import ctypes
import json
import os
import sys
import time
import types
import warnings
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import torch  # noqa: E402

from bench_norm_train import acv_step, events_ms, pcw_step, stats  # noqa: E402
from diffuvolume_amd import _env, _lib, loss as L, train_loss  # noqa: E402
from diffuvolume_amd._build import csrc_sha16  # noqa: E402
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim  # noqa: E402
from diffuvolume_amd.synth import (IGEV_TRAIN_ARGS, IGEV_TRAIN_WEIGHT_SEED, StubMobileNetV2, igev_train_step_inputs,  # noqa: E402
                                   synth_state_dict)

ROUTES = ("hip", "torch")
KNOB = "DV_TRAIN_LOSS"
HBM = 8.0e12
PARTS = ("function", "kernels", "acv", "pcw", "igev")
# .vgpr_count / .sgpr_spill_count / .group_segment_fixed_size / .private_segment_fixed_size of the code object (hipcc, gfx950,
# the flags of _build.py); 256 threads per block.  The forward is instantiated per accumulator count KT >= K; the scalar
# registers that do not fit (the by-value table of K pointers) are kept in vector-register lanes, not in memory.
RESOURCES = {
    "masked_loss_fwd_kernel<KT = 1 | 4 | 8 | 16 | 24>": dict(vgprs=[37, 42, 53, 82, 85], sgpr_spills=[0, 0, 26, 90, 146],
                                                             vgpr_spills=0, scratch_bytes=0,
                                                             lds_bytes=[224, 320, 448, 704, 960]),
    "masked_loss_merge_kernel": dict(vgprs=46, sgpr_spills=0, vgpr_spills=0, scratch_bytes=0, lds_bytes=240),
    "masked_loss_bwd_kernel": dict(vgprs=21, sgpr_spills=0, vgpr_spills=0, scratch_bytes=0, lds_bytes=0),
}


def alternate(fn, runs, warmup):
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
            times[r].append((time.perf_counter() - t0) * 1e3)
            peak[r] = max(peak[r], torch.cuda.max_memory_allocated() - rest)
            top[r] = max(top[r], torch.cuda.max_memory_allocated())
    os.environ.pop(KNOB)
    return {r: stats(times[r]) for r in ROUTES}, peak, top


def host_syncs(fn):
    """Synchronising calls PyTorch reports during fn() per route (None where the debug mode is not available)."""
    out = {}
    for r in ROUTES:
        os.environ[KNOB] = r
        fn()
        torch.cuda.synchronize()
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                fn()
            out[r] = sum("synchroniz" in str(w.message).lower() for w in seen)
        except Exception as e:                                            # noqa: BLE001
            out[r] = None
            print("sync debug mode:", e)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    os.environ.pop(KNOB)
    return out


def cases(b):
    gen = torch.Generator().manual_seed(11)

    def around(gt, k):
        return [(gt + torch.randn(gt.shape, generator=gen) * (3.0 / (i % 6 + 1))).cuda() for i in range(k)]

    gt = torch.rand(b, 256, 512, generator=gen) * 200
    gt[torch.rand(b, 256, 512, generator=gen) < 0.05] = 0.0
    flow = torch.rand(b, 1, 320, 736, generator=gen) * 230
    valid = (torch.rand(b, 320, 736, generator=gen) > 0.1).float()
    return [("model_loss_train", "smooth_l1", around(gt, 4), gt.cuda(), ((gt < 192) & (gt > 0)).cuda(), None),
            ("model_loss_kitti12", "smooth_l1", around(gt, 6), gt.cuda(), ((gt < 192) & (gt > 0)).cuda(), None),
            ("sequence_loss", "smooth_l1 + 22 l1", around(flow, 23), flow.cuda(), None, valid.cuda())]


def call(name, preds, gt, mask, valid):
    if name == "sequence_loss":
        return L.sequence_loss(preds[1:], preds[0], gt, valid, max_disp=192)[0]
    return getattr(L, name)(preds, gt, mask)


def function(b, runs):
    out = []
    for name, kind, preds, gt, mask, valid in cases(b):
        leaves = [p.requires_grad_(True) for p in preds]

        def fwd_bwd():
            for p in leaves:
                p.grad = None
            call(name, leaves, gt, mask, valid).backward()

        t, peak, _ = alternate(fwd_bwd, runs, warmup=3)
        rec = dict(function=name, kind=kind, shape=list(gt.shape), predictions=len(preds), fwd_bwd_ms=t,
                   peak_mib_above_rest={r: round(p / (1 << 20), 1) for r, p in peak.items()},
                   host_synchronisations_per_call=host_syncs(fwd_bwd),
                   hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4),
                   hip_faster_with_ranges_apart=bool(t["hip"]["max"] < t["torch"]["min"]))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del leaves
        torch.cuda.empty_cache()
    return out


def kernels(b, runs, reps=20):
    lib, st = _lib.load(), _lib.stream_ptr()
    out = []
    for name, kind, preds, gt, mask, valid in cases(b):
        k, n = len(preds), gt.numel()
        seq = name == "sequence_loss"
        m = valid if seq else mask.view(torch.uint8)
        mode, max_disp, metric = (train_loss.MASK_VALID_F32, 192.0, k - 1) if seq else (train_loss.MASK_U8, 0.0, -1)
        kinds = [train_loss.SMOOTH_L1] + [train_loss.L1 if seq else train_loss.SMOOTH_L1] * (k - 1)
        pa = (ctypes.c_void_p * k)(*[p.data_ptr() for p in preds])
        wa = (ctypes.c_double * k)(*[1.0] * k)
        ka = (ctypes.c_int * k)(*kinds)
        ws = _lib.workspace("dv_masked_loss_workspace_floats", gt.device, k, n)
        stats_t = torch.zeros(k + 6, dtype=torch.float64, device="cuda")
        loss = torch.zeros(1, device="cuda")
        gout = torch.ones(1, device="cuda")
        grads = [torch.empty_like(p) for p in preds]
        ga = (ctypes.c_void_p * k)(*[g.data_ptr() for g in grads])

        def fwd():
            _lib.check(lib.dv_masked_loss_fwd_f32(pa, wa, ka, gt.data_ptr(), m.data_ptr(), mode, max_disp, k, n, metric,
                                                  ws.data_ptr(), stats_t.data_ptr(), loss.data_ptr(), st), "fwd")

        def bwd():
            _lib.check(lib.dv_masked_loss_bwd_f32(pa, wa, ka, gt.data_ptr(), m.data_ptr(), mode, max_disp,
                                                  stats_t.data_ptr(), gout.data_ptr(), ga, k, n, st), "bwd")

        f = [events_ms(fwd, reps) for _ in range(runs)]
        g = [events_ms(bwd, reps) for _ in range(runs)]
        mask_bytes = 4 if seq else 1
        rec = dict(case=name, shape=list(gt.shape), predictions=k, mask="valid_f32" if seq else "u8",
                   forward_ms=stats(f), backward_ms=stats(g),
                   counted_bytes=dict(forward=(4 * k + 5) * n, backward=(8 * k + 5) * n,
                                      counted="4K + 5 and 8K + 5 per pixel (a float32 `valid` adds 3 per pixel, not counted)"
                                      if seq else "4K + 5 and 8K + 5 per pixel"),
                   moved_bytes=dict(forward=(4 * k + 4 + mask_bytes) * n, backward=(8 * k + 4 + mask_bytes) * n),
                   forward_fraction_of_8_tb_s=round((4 * k + 5) * n / (stats(f)["median"] * 1e-3) / HBM, 3),
                   backward_fraction_of_8_tb_s=round((8 * k + 5) * n / (stats(g)["median"] * 1e-3) / HBM, 3))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del grads
        torch.cuda.empty_cache()
    return dict(cases=out, kernel_resources=RESOURCES)


def igev_step(b, h, w, iters):
    """IGEVStereo_ddim: the step of tools/bench_igev_train_step.py."""
    args = types.SimpleNamespace(**IGEV_TRAIN_ARGS)
    x = igev_train_step_inputs(seed=83, b=b, h=h, w=w, iters=iters, t=400, device="cuda")
    m = IGEVStereo_ddim(args, feature=Feature(StubMobileNetV2()))
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=IGEV_TRAIN_WEIGHT_SEED), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        init, preds = m.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=iters, t=x["t"],
                                      noise=x["noise"])
        loss, _ = L.sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=args.max_disp)
        loss.backward()
        opt.step()

    return step


def whole_step(name, step, runs, loss_alone, **what):
    t, peak, top = alternate(step, runs, warmup=2)
    rec = dict(model=name, **what, step_ms=t, peak_gib={r: round(p / 2 ** 30, 3) for r, p in top.items()},
               peak_gib_above_rest={r: round(p / 2 ** 30, 3) for r, p in peak.items()},
               hip_over_torch=round(t["hip"]["median"] / t["torch"]["median"], 4),
               hip_not_slower_with_ranges_apart=bool(t["hip"]["max"] <= t["torch"]["min"]),
               hip_slower_with_ranges_apart=bool(t["hip"]["min"] > t["torch"]["max"]),
               ranges_overlap=bool(t["hip"]["min"] <= t["torch"]["max"] and t["torch"]["min"] <= t["hip"]["max"]))
    if loss_alone:
        rec["loss_share_of_step"] = {r: round(loss_alone["fwd_bwd_ms"][r]["median"] / t[r]["median"], 4) for r in ROUTES}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "loss_train_bench.json"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    assert set(parts) <= set(PARTS), f"--parts takes {PARTS}"
    assert torch.cuda.is_available(), "needs the MI355X"
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else {}
    rec.update(tool="tools/bench_loss_train.py", csrc_sha16=csrc_sha16(), device=torch.cuda.get_device_name(0),
               runs=a.runs, batch=a.batch, default_route=_env.KNOBS[KNOB][0])

    def save(key, value):
        rec[key] = value
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(rec, indent=1) + "\n")
        torch.cuda.empty_cache()

    if "kernels" in parts:
        save("kernels", kernels(a.batch, a.runs))
    if "function" in parts:
        save("function", function(a.batch, a.runs))
    alone = {f["function"]: f for f in rec.get("function", [])}
    if "acv" in parts:
        save("acv_step", whole_step("ACVNet_DDIM", acv_step(a.batch, 256, 512), a.runs, alone.get("model_loss_train"),
                                    image=[256, 512]))
    if "pcw" in parts:
        save("pcw_step", whole_step("PWCNet_ddim", pcw_step(a.batch, 256, 512), a.runs, alone.get("model_loss_kitti12"),
                                    image=[256, 512]))
    if "igev" in parts:
        save("igev_step", whole_step("IGEVStereo_ddim", igev_step(a.batch, 320, 736, 22), a.runs, alone.get("sequence_loss"),
                                     image=[320, 736], iters=22))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
