"""IGEV's geometry lookup (Combined_Geo_Encoding_Volume) on its training route on the MI355X: the correlation and every
lookup autograd functions on the HIP kernels (geometry_ddim.AllPairsCorrFn / GeoLookupFn).

Parity with the reference (tests/golden/igev_lookup_train.npz, tools/make_golden_igev_lookup_train.py: the imported
reference class in float32 and float64 on one training step, cases `even` B 2, C 8, D 48, 8 x 24, T 3 and `odd` B 1,
5 x 7, T 2).  Bar per kind of gradient (df1, df2, dgeo), as relative L2 against the fixture's float64 (sampled entries
and the norm):
    rel(hip, f64) <= 2 * ref_err[kind] + 1e-6
with ref_err the reference's own float32 error for that kind (stored in the fixture).  The chain test uses the same bar
with err32 = the float32 error of the oracle's vjp on the test's own inputs.

Measured on the MI355X (df1 / df2 / dgeo, the worse of sampled entries and norm; bars 2.26e-6 / 2.25e-6 / 2.91e-6 for
`even`, 1.47e-6 / 1.43e-6 / 2.82e-6 for `odd`):
    HIP   even 6.3e-7 / 6.2e-7 / 8.2e-7,   odd 2.5e-7 / 2.0e-7 / 4.4e-7
    torch even 7.7e-7 / 6.7e-7 / 2.13e-6,  odd 2.8e-7 / 2.3e-7 / 2.12e-6   (DV_TRAIN_LOOKUP=torch)
Chain test (cost volume -> lookup -> update block -> upsampler, two iterations): the lookup's share against the float64
oracle's vjp is printed as `PARITY chain lookup share ...` lines."""
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
from diffuvolume_amd.synth import (IGEV_LOOKUP_LEAVES, UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, _gen,
                                   igev_lookup_train_inputs, igev_lookup_train_leaves, igev_lookup_train_step,
                                   igev_upsample_state_dict, igev_volume_train_inputs, synth_state_dict,
                                   update_train_inputs)

pytestmark = pytest.mark.gpu
KINDS = ("df1", "df2", "dgeo")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_lookup_train.npz") as z:
        return {k: z[k] for k in z.files}


def case_of(gold, case):
    b, c, d, h, w, iters = (int(v) for v in gold[f"{case}_shape"])
    return dict(seed=int(gold[f"{case}_seed"]), b=b, c=c, d=d, h=h, w=w, iters=iters)


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def train_step(case, requires_grad=True):
    x = igev_lookup_train_inputs(device="cuda", requires_grad=requires_grad, **case)
    loss, outs = igev_lookup_train_step(Combined_Geo_Encoding_Volume, x)
    if requires_grad:
        loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach(), outs=[o.detach() for o in outs],
                grads={n: t.grad for n, t in igev_lookup_train_leaves(x).items()})


def assert_parity(gold, case, run, label):
    bad = []
    for i, (kind, name) in enumerate(zip(KINDS, IGEV_LOOKUP_LEAVES)):
        g = run["grads"][name]
        assert g is not None and torch.isfinite(g).all(), name
        idx = torch.from_numpy(gold[f"{case}_grad_idx"][i]).cuda()
        e_val = rel(g.reshape(-1)[idx].cpu().numpy(), gold[f"{case}_grad_val_f64"][i])
        e_norm = rel(float(g.double().norm()), gold[f"{case}_grad_norm_f64"][i])
        bar = 2 * float(gold[f"{case}_ref_err"][i]) + 1e-6
        print(f"PARITY {label} {case} {kind}: samples {e_val:.3e}  norm {e_norm:.3e}  bar {bar:.2e}")
        if not (e_val <= bar and e_norm <= bar):
            bad.append((kind, e_val, e_norm, bar))
    assert not bad, f"{label} route over the bar: {bad}"


@pytest.mark.parametrize("case", ["even", "odd"])
def test_step_matches_reference_and_repeats(gold, case, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_LOOKUP", raising=False)
    run = train_step(case_of(gold, case))
    assert_parity(gold, case, run, "hip")
    again = train_step(case_of(gold, case))
    assert torch.equal(run["loss"], again["loss"])
    for n in IGEV_LOOKUP_LEAVES:
        assert torch.equal(run["grads"][n], again["grads"][n]), n
    frozen = train_step(case_of(gold, case), requires_grad=False)             # no input requires grad: the inference route
    assert not frozen["loss"].requires_grad and all(torch.equal(a, b) for a, b in zip(frozen["outs"], run["outs"]))


@pytest.mark.parametrize("case", ["even", "odd"])
def test_torch_route_is_within_the_same_bar(gold, case, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_LOOKUP", "torch")
    assert_parity(gold, case, train_step(case_of(gold, case)), "torch")


def test_refusals(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_LOOKUP", raising=False)
    c = case_of(gold, "odd")
    x = igev_lookup_train_inputs(device="cuda", **c)
    vol = Combined_Geo_Encoding_Volume(x["fmap1"], x["fmap2"], x["geo"])
    assert vol.training_route
    disp, coords, noisy = x["disp"][0], x["coords"], x["noisy"][0]
    with pytest.raises(DiffuVolumeError, match=r"noisy requires grad.*igev_stereo_ddim\.py:436"):
        vol(disp, coords, noisy.clone().requires_grad_(True))
    with pytest.raises(DiffuVolumeError, match=r"disp requires grad.*:442"):
        vol(disp.clone().requires_grad_(True), coords, noisy)
    with pytest.raises(DiffuVolumeError, match=r"disp requires grad"):
        vol.request(disp.clone().requires_grad_(True), coords, noisy).materialize()
    with pytest.raises(DiffuVolumeError, match="inference-only"):
        vol.lookup_conv1x1(disp, coords, noisy, torch.zeros(9 * 20 * 64, device="cuda"), None, 1)
    with pytest.raises(DiffuVolumeError, match="inference-only"):
        vol.request(disp, coords, noisy).conv1x1(torch.zeros(9 * 20 * 64, device="cuda"), None, 1)
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        vol(disp.cpu(), coords, noisy)
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        Combined_Geo_Encoding_Volume(x["fmap1"].cpu(), x["fmap2"], x["geo"])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        Combined_Geo_Encoding_Volume(x["fmap1"], x["fmap2"], x["geo"].detach().cpu().requires_grad_(True))
    # outside the training route nothing changed: a tensor that requires grad is still refused as inference-only
    plain = Combined_Geo_Encoding_Volume(x["fmap1"].detach(), x["fmap2"].detach(), x["geo"].detach())
    assert not plain.training_route
    with pytest.raises(NotImplementedError, match="inference-only"):
        plain(disp.clone().requires_grad_(True), coords, noisy)
    with torch.no_grad():                                                     # grad mode off: the inference route, same bits
        quiet = Combined_Geo_Encoding_Volume(x["fmap1"], x["fmap2"], x["geo"])
        assert not quiet.training_route and torch.equal(quiet(disp, coords, noisy), plain(disp, coords, noisy))
        assert torch.equal(vol(disp, coords, noisy), plain(disp, coords, noisy))


# ---- the chain: cost-volume front -> lookup -> update block -> upsampling head ---------------------------------------

CHAIN = dict(b=2, h=8, w=24, max_disp=192, iters=2, seed=81)


def chain_setup(cfg=CHAIN):
    """The modules (train mode, seeded weights) and seeded inputs of the chain; tools/bench_lookup_train.py times the same
    step at batch 4, 80 x 184."""
    from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume, IGEVUpsampler
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    b, h, w, iters, seed = (cfg[k] for k in ("b", "h", "w", "iters", "seed"))
    front = IGEVCostVolume(cfg["max_disp"])
    front.load_state_dict(synth_state_dict(front.state_dict(), seed=91), strict=True)
    block = BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)
    block.load_state_dict(synth_state_dict(block.state_dict(), seed=7), strict=True)
    ups = IGEVUpsampler()
    ups.load_state_dict(igev_upsample_state_dict(ups.state_dict(), 93, 1.0), strict=True)
    x = igev_volume_train_inputs(seed, b, h, w, cfg["max_disp"], device="cuda", requires_grad=False)
    return dict(front=front.cuda().train(), block=block.cuda().train(), ups=ups.cuda().train(), iters=iters,
                ml=x["match_left"].requires_grad_(True), mr=x["match_right"].requires_grad_(True), features=x["features"],
                u=update_train_inputs(seed, b, h, w, 1, device="cuda"),
                stem_2x=torch.randn(b, 32, 2 * h, 2 * w, generator=_gen(seed, "stem_2x")).cuda(),
                gt=(torch.rand(b, 1, 4 * h, 4 * w, generator=_gen(seed, "gt")) * 160 + 4).cuda(),
                noisy=torch.rand(b, cfg["max_disp"] // 4, h, w, generator=_gen(seed, "noisy")).cuda(),
                coords=torch.arange(w, dtype=torch.float32, device="cuda").view(1, 1, 1, w).expand(b, 1, h, w).contiguous())


def chain_step(s=None):
    """T iterations of the reference's train loop (KITTI15/core/igev_stereo_ddim.py:441-457, `disp.detach()` before
    every lookup) on IGEVCostVolume -> Combined_Geo_Encoding_Volume -> BasicMultiUpdateBlock -> IGEVUpsampler, all in
    train mode; loss = sum_i mean|disp_up_i - gt| + mean|init_disp - gt / 4|.  The lookup is fed identity views of the
    volume and of the two feature leaves, so that the views' retained gradients are the lookup's share alone (the volume
    also reaches the loss through `init_disp`, the features through the group-wise correlation volume)."""
    s = s or chain_setup()
    front, block, ups, ml, mr, u = (s[k] for k in ("front", "block", "ups", "ml", "mr", "u"))
    for t in (ml, mr, *front.parameters(), *block.parameters(), *ups.parameters(), *u["net"], *(t for i in u["inp"] for t in i)):
        t.grad = None
    geo, init_disp = front(ml, mr, s["features"])
    f1, f2, geo_v = ml.view_as(ml), mr.view_as(mr), geo.view_as(geo)
    f1.retain_grad(), f2.retain_grad(), geo_v.retain_grad()
    geo_fn = Combined_Geo_Encoding_Volume(f1, f2, geo_v)
    loss = (init_disp - torch.nn.functional.avg_pool2d(s["gt"], 4) / 4).abs().mean()
    net, disp, feats, disps = list(u["net"]), init_disp, [], []
    for _ in range(s["iters"]):
        disp = disp.detach()
        geo_feat = geo_fn(disp, s["coords"], s["noisy"])
        geo_feat.retain_grad()
        feats.append(geo_feat)
        disps.append(disp)
        net, mask_feat_4, delta = block(net, u["inp"], geo_feat, disp, iter16=True, iter08=True)
        disp = disp + delta
        loss = loss + (ups(disp, mask_feat_4, s["stem_2x"]) - s["gt"]).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    # the convolution weights (conv1_up is built without BatchNorm but keeps an unused `bn` of parameters, as in the reference)
    weights = {n: p.grad for n, p in front.named_parameters() if n.startswith(("corr_stem", "cost_agg")) and p.dim() > 1}
    return dict(loss=loss.detach(), ml=ml.grad, mr=mr.grad, weights=weights, geo_grad=geo_v.grad, f1_grad=f1.grad,
                f2_grad=f2.grad, grad_outs=[f.grad for f in feats], disps=disps, geo=geo.detach(),
                ml_val=ml.detach(), mr_val=mr.detach(), coords=s["coords"], noisy=s["noisy"])


def test_chain_trains_through_the_lookup(monkeypatch):
    from oracle.igev_oracle import geo_filter_lookup
    for k in ("DV_TRAIN_LOOKUP", "DV_TRAIN_CONV2D", "DV_TRAIN_CONV3D"):
        monkeypatch.delenv(k, raising=False)
    run, again = chain_step(), chain_step()
    for name in ("ml", "mr"):
        g = run[name]
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, name
        assert torch.equal(g, again[name]), name
    assert run["weights"]
    for n, g in run["weights"].items():
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, n
        assert torch.equal(g, again["weights"][n]), n
    assert torch.equal(run["loss"], again["loss"]) and torch.equal(run["geo_grad"], again["geo_grad"])
    assert all(g is not None and float(g.abs().max()) > 0 for g in run["grad_outs"])

    # the lookup's share, exactly: the captured grad_outs through the float64 oracle's vjp
    def oracle_vjp(dtype):
        leaves = [run[k].cpu().to(dtype).requires_grad_(True) for k in ("geo", "ml_val", "mr_val")]
        total = 0.0
        for g, d in zip(run["grad_outs"], run["disps"]):
            out = geo_filter_lookup(*leaves, d.cpu().to(dtype), run["coords"].cpu().to(dtype), run["noisy"].cpu().to(dtype))
            total = total + (out * g.cpu()).sum()
        total.backward()
        return [t.grad.double() for t in leaves]
    want, w32 = oracle_vjp(torch.float64), oracle_vjp(torch.float32)
    got = [run[k].double().cpu() for k in ("geo_grad", "f1_grad", "f2_grad")]
    bad = []
    for name, g, ref, r32 in zip(("dgeo", "df1", "df2"), got, want, w32):
        err32 = float((r32 - ref).norm() / ref.norm())
        e, bar = float((g - ref).norm() / ref.norm()), 2 * err32 + 1e-6
        print(f"PARITY chain lookup share {name}: {e:.3e}  err32 {err32:.3e}  bar {bar:.2e}")
        if not e <= bar:
            bad.append((name, e, bar))
    assert not bad, bad
