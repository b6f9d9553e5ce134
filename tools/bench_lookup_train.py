"""Benchmark of the geometry lookup's training route on the MI355X -> profiles/lookup_train_bench.json.

  kernels   each new kernel alone at batch 4, 80x184, C 8, D 48, 96 feature channels, on preallocated buffers, with its
            counted bytes (every operand once) and flop over the time:
              dv_geo_filter_lookup_bwd_f32   dgeo only / dcorr0 only / both
              dv_allpairs_corr_bwd_f32       dfmap1 only / dfmap2 only / both (2 * B * h * W1 * W2 * C flop each)
  lookups   one volume, T = 22 lookups (synth.igev_lookup_train_step) + backward, HIP route and DV_TRAIN_LOOKUP=torch
            alternating in one process, median of ROUNDS, max_memory_allocated
  chain     the chained step of tests/test_gpu_igev_lookup_train.py (IGEVCostVolume -> lookup -> update block ->
            upsampler, T iterations, forward + backward) at that size on both lookup routes, with the share of autograd's
            sum of the T dense volume gradients (T - 1 adds of a [B,8,48,h,w] tensor, timed alone)
  parity    the errors that tests/test_gpu_igev_lookup_train.py prints for the two fixture cases, both routes

    python tools/bench_lookup_train.py [--skip-kernels] [--skip-lookups] [--skip-chain] [--skip-parity]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from diffuvolume_amd import _build, _lib  # noqa: E402
from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume  # noqa: E402
from diffuvolume_amd.synth import igev_lookup_train_inputs, igev_lookup_train_leaves, igev_lookup_train_step  # noqa: E402

PEAK = 157.3e12                # fp32 MFMA peak of the MI355X


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def med(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def time_kernels(b, c, d, h, w, feat, rounds, reps):
    lib = _lib.load()
    dev = "cuda"
    go = torch.randn(b, 2 * (9 * c + 9), h, w, device=dev)
    disp = torch.rand(b, 1, h, w, device=dev) * (d + 6) - 3
    coords = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w).expand(b, 1, h, w).contiguous()
    noisy = torch.rand(b, d, h, w, device=dev)
    dgeo, dcorr = torch.empty(b, c, d, h, w, device=dev), torch.randn(b, h, w, w, device=dev)
    f1, f2 = torch.randn(b, feat, h, w, device=dev), torch.randn(b, feat, h, w, device=dev)
    d1, d2 = torch.empty_like(f1), torch.empty_like(f2)

    def lookup(pg, pc):
        return lambda: _lib.check(lib.dv_geo_filter_lookup_bwd_f32(go.data_ptr(), disp.data_ptr(), coords.data_ptr(),
                                                                   noisy.data_ptr(), pg, pc, b, c, d, h, w, w, 4,
                                                                   _lib.stream_ptr()), "dv_geo_filter_lookup_bwd_f32")

    def corr(p1, p2):
        return lambda: _lib.check(lib.dv_allpairs_corr_bwd_f32(dcorr.data_ptr(), f1.data_ptr(), f2.data_ptr(), p1, p2, b,
                                                               feat, h, w, w, _lib.stream_ptr()), "dv_allpairs_corr_bwd_f32")
    pix = b * h * w
    geo_bytes = 4.0 * (pix * 2 * 9 * c + 2 * pix + dgeo.numel() + noisy.numel())     # its grad_out channels, disp, noise, dgeo
    corr_bytes = 4.0 * (pix * 18 + 2 * pix + dcorr.numel())
    gemm = 2.0 * b * h * w * w * feat
    side = 4.0 * (dcorr.numel() + 2 * f1.numel())
    legs = {"lookup_bwd_dgeo_only": (lookup(dgeo.data_ptr(), None), geo_bytes, 0.0),
            "lookup_bwd_dcorr0_only": (lookup(None, dcorr.data_ptr()), corr_bytes, 0.0),
            "lookup_bwd_both": (lookup(dgeo.data_ptr(), dcorr.data_ptr()), geo_bytes + corr_bytes, 0.0),
            "corr_bwd_dfmap1_only": (corr(d1.data_ptr(), None), side, gemm),
            "corr_bwd_dfmap2_only": (corr(None, d2.data_ptr()), side, gemm),
            "corr_bwd_both": (corr(d1.data_ptr(), d2.data_ptr()), 2 * side, 2 * gemm)}
    t = {n: [] for n in legs}
    for _ in range(rounds):
        for n, (fn, _, _) in legs.items():
            t[n].append(_ms(fn, reps))
    out = dict(batch=b, channels=c, disparities=d, plane=[h, w], feature_channels=feat)
    for n, (_, nbytes, flop) in legs.items():
        row = med(t[n])
        row["counted_mb"] = round(nbytes / 1e6, 1)
        row["achieved_tb_per_s"] = round(nbytes / (row["median_ms"] * 1e-3) / 1e12, 3)
        if flop:
            row["gflop"] = round(flop / 1e9, 2)
            row["frac_peak"] = round(flop / (row["median_ms"] * 1e-3) / PEAK, 4)
        out[n] = row
        print(f"  {n:24s} {row['median_ms']:.4f} ms ({row['min_ms']:.4f}-{row['max_ms']:.4f})  {row['counted_mb']} MB  "
              f"{row['achieved_tb_per_s']} TB/s" + (f"  {row['frac_peak']} of peak" if flop else ""), flush=True)
    return out


def _alternate(step, rounds, env="DV_TRAIN_LOOKUP", routes=("hip", "torch")):
    t, mem = {r: [] for r in routes}, {}
    for route in routes:                              # warm-up on both routes
        os.environ[env] = route
        step()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for route in routes:
            os.environ[env] = route
            torch.cuda.reset_peak_memory_stats()
            t[route].append(_ms(step, 1))
            mem[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    os.environ.pop(env, None)
    rec = {}
    for route in routes:
        rec[route] = dict(**med(t[route]), max_memory_allocated_gib=mem[route])
        print(f"  {route:5s} {rec[route]['median_ms']:8.2f} ms ({rec[route]['min_ms']:.2f}-{rec[route]['max_ms']:.2f})  "
              f"peak memory {mem[route]} GiB", flush=True)
    rec["hip_over_torch"] = round(rec["hip"]["median_ms"] / rec["torch"]["median_ms"], 3)
    return rec


def time_lookups(b, c, d, h, w, feat, iters, rounds):
    x = igev_lookup_train_inputs(71, b, c, d, h, w, iters, feat=feat, device="cuda")

    def step():
        for t in igev_lookup_train_leaves(x).values():
            t.grad = None
        loss, _ = igev_lookup_train_step(Combined_Geo_Encoding_Volume, x)
        loss.backward()
    return dict(batch=b, plane=[h, w], iters=iters, **_alternate(step, rounds))


def time_chain(b, h, w, iters, rounds):
    sys.path.insert(0, str(ROOT / "tests"))
    import test_gpu_igev_lookup_train as T
    s = T.chain_setup(dict(b=b, h=h, w=w, max_disp=192, iters=iters, seed=81))
    rec = dict(batch=b, plane=[h, w], iters=iters, **_alternate(lambda: T.chain_step(s), rounds))
    parts = [torch.randn(b, 8, 48, h, w, device="cuda") for _ in range(2)]
    add = _ms(lambda: parts[0].add_(parts[1]), 20)
    rec["volume_gradient_sum"] = dict(one_add_ms=round(add, 4), adds=iters - 1, total_ms=round(add * (iters - 1), 3),
                                      share_of_hip_step=round(add * (iters - 1) / rec["hip"]["median_ms"], 4))
    print(f"  autograd's sum of the volume gradients: {iters - 1} x {add:.4f} ms = "
          f"{rec['volume_gradient_sum']['share_of_hip_step']:.2%} of the HIP step", flush=True)
    return rec


def parity():
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import test_gpu_igev_lookup_train as T
    with np.load(ROOT / "tests" / "golden" / "igev_lookup_train.npz") as z:
        gold = {k: z[k] for k in z.files}
    out = {}
    for case in ("even", "odd"):
        out[case] = dict(bar={k: float(f"{2 * float(gold[f'{case}_ref_err'][i]) + 1e-6:.3e}") for i, k in enumerate(T.KINDS)})
        for route in ("hip", "torch"):
            os.environ["DV_TRAIN_LOOKUP"] = route
            T.assert_parity(gold, case, T.train_step(T.case_of(gold, case)), route)
    os.environ.pop("DV_TRAIN_LOOKUP", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--width", type=int, default=184)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--disparities", type=int, default=48)
    ap.add_argument("--feature-channels", type=int, default=96)
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-lookups", action="store_true")
    ap.add_argument("--skip-chain", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lookup_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = dict(device=torch.cuda.get_device_name(0), csrc_sha16=_build.csrc_sha16(), peak_tflops=PEAK / 1e12)
    dims = (a.batch, a.channels, a.disparities, a.height, a.width, a.feature_channels)
    if not a.skip_parity:
        print("parity (fixture cases, both routes; asserted against the tests' bar):", flush=True)
        rec["parity_bars"] = parity()
    if not a.skip_kernels:
        print("kernels alone:", flush=True)
        rec["kernels"] = time_kernels(*dims, a.rounds, a.reps)
    if not a.skip_lookups:
        print(f"T = {a.iters} lookups + backward:", flush=True)
        rec["lookups"] = time_lookups(*dims, a.iters, a.rounds)
    if not a.skip_chain:
        print(f"chained step, T = {a.iters}:", flush=True)
        rec["chain"] = time_chain(a.batch, a.height, a.width, a.iters, a.rounds)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
