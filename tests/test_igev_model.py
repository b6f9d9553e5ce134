"""IGEVStereo_ddim drop-in (KITTI15/core/igev_stereo_ddim.py:118-463): state_dict layout and constructor contract on
CPU; on the GPU the whole eval forward against the output of the REFERENCE class itself (tests/golden/igev_model.npz,
oracle/make_golden_igev_model.py: timm stubbed with synth.StubMobileNetV2), the convex upsampling kernel, and a
config-5-sized run (1248x384, 20 DDIM steps x 32 GRU iterations through the real update block)."""
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from diffuvolume_amd.synth import NoiseTape, StubMobileNetV2, _gen, synth_state_dict

ARGS = dict(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2, corr_radius=4,
            slow_fast_gru=False, max_disp=192, mixed_precision=False)
DEV = "cuda:0"


def build(steps=2, cof=None):
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    return IGEVStereo_ddim(types.SimpleNamespace(**ARGS), feature=Feature(StubMobileNetV2()), sampling_timesteps=steps,
                           ensemble_cof=cof)


def golden_inputs(seed, h=64, w=128):
    g = _gen(seed, "igev_model")
    img1 = torch.rand(1, 3, h, w, generator=g) * 255
    img2 = torch.roll(img1, -6, dims=-1)
    flow_full = (6 + torch.randn(1, 1, h, w, generator=g)).clamp(0.5, 47)
    flow_gt = F.interpolate(flow_full, size=(h // 4, w // 4), mode="bilinear") / 4
    return img1, img2, flow_full, flow_gt


def test_state_dict_layout_and_contract():
    from diffuvolume_amd import _lib
    from diffuvolume_amd.igev_stereo_ddim import IGEVStereo_ddim
    g = load_golden("igev_model")
    m = build()
    sd = m.state_dict()
    assert len(sd) == g["n_keys"]                                   # the reference's own key count (checked key by key
    for k in ("cnet.layer2.0.downsample.1.weight", "cnet.layer2.0.norm3.weight", "update_block.gru04.convz.weight",   # in the generator)
              "context_zqr_convs.2.bias", "time_embedding.time_mlp.1.weight", "feature.deconv32_16.conv1.conv.weight",
              "stem_2.0.conv.weight", "spx_gru.0.weight", "spx_2_gru.conv2.bn.running_var", "corr_stem.bn.weight",
              "corr_feature_att.feat_att.1.bias", "cost_agg.feature_att_up_8.feat_att.0.conv.weight",
              "classifier.weight", "sqrt_recipm1_alphas_cumprod"):
        assert k in sd, k
    assert sd["alphas_cumprod"].dtype == torch.float64
    m.load_state_dict(synth_state_dict(sd, seed=3), strict=True)
    # IGEVStereo_ddim(args) as the reference constructs it (core/igev_stereo_ddim.py:118-121, extractor.py:331): the
    # backbone comes from timm when timm is importable, and only otherwise is feature= asked for
    import sys
    had = sys.modules.get("timm")
    try:
        sys.modules["timm"] = None                                    # import timm -> ImportError
        with pytest.raises(_lib.DiffuVolumeError, match="feature="):
            IGEVStereo_ddim(types.SimpleNamespace(**ARGS))
        calls = []

        def create_model(name, pretrained=False, features_only=False):
            calls.append((name, pretrained, features_only))
            return StubMobileNetV2()

        sys.modules["timm"] = types.SimpleNamespace(create_model=create_model)
        m2 = IGEVStereo_ddim(types.SimpleNamespace(**ARGS))
        assert calls == [("mobilenetv2_100", True, True)]
        assert list(m2.state_dict().keys()) == list(sd.keys())
    finally:
        if had is None:
            sys.modules.pop("timm", None)
        else:
            sys.modules["timm"] = had
    with pytest.raises(ValueError):
        build(steps=20)                                              # ensemble weights must be given for S != 2
    m.train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 64, 128), torch.zeros(1, 3, 64, 128), torch.zeros(1, 1, 64, 128), torch.zeros(1, 1, 16, 32))


def test_context_upsample_oracle_matches_reference():
    from oracle import igev_oracle as IO
    g = load_golden("igev_model")
    out = IO.context_upsample(g["ctx_disp"] * 4.0, F.softmax(g["ctx_logits"], 1))
    torch.testing.assert_close(out, g["ctx_out"], atol=1e-6, rtol=1e-6)
    assert IO.upsample_disp(g["ctx_disp"], g["ctx_logits"]).shape == (2, 1, 20, 28)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 96, 312), (3, 1, 1)])
def test_context_upsample_kernel(shape):
    from diffuvolume_amd.igev_stereo_ddim import context_upsample
    from oracle import igev_oracle as IO
    g = load_golden("igev_model")
    if shape == (2, 5, 7):
        disp, logits, want = g["ctx_disp"], g["ctx_logits"], g["ctx_out"]
    else:
        b, h, w = shape
        gen = _gen(9, str(shape))
        disp, logits = torch.rand(b, 1, h, w, generator=gen) * 47, torch.randn(b, 9, 4 * h, 4 * w, generator=gen) * 3
        want = IO.context_upsample(disp * 4.0, F.softmax(logits, 1))
    out = context_upsample(disp.to(DEV), logits.to(DEV), scale=4.0, apply_softmax=True)
    torch.testing.assert_close(out.cpu(), want, atol=2e-5, rtol=1e-5)
    probs = F.softmax(logits, 1)
    out2 = context_upsample((disp * 4.0).to(DEV), probs.to(DEV))                # the reference's own call form
    torch.testing.assert_close(out2.cpu(), want, atol=2e-5, rtol=1e-5)


@pytest.mark.gpu
def test_forward_matches_the_reference_class():
    from diffuvolume_amd import igev_stereo_ddim as M
    g = load_golden("igev_model")
    scale = {str(k): float(v) for k, v in zip(g["scale_keys"].tolist(), g["scale_vals"].tolist())}
    m = build()
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=g["seed"], scale=scale), strict=True)
    m = m.to(DEV).eval()
    img1, img2, flow_full, flow_gt = (t.to(DEV) for t in golden_inputs(g["seed"]))
    seen = []
    inner = M.IGEVDiffusionLoop._update

    def spy(self, pred, *a, **k):
        seen.append(pred.clone())
        return inner(self, pred, *a, **k)

    M.IGEVDiffusionLoop._update = spy
    try:
        pred, pred2 = m(img1, img2, flow_full, flow_gt, iters=g["iters"], test_mode=True, noise=NoiseTape(g["tape_seed"]))
    finally:
        M.IGEVDiffusionLoop._update = inner
    assert pred is pred2 and tuple(pred.shape) == tuple(g["pred"].shape)
    steps = torch.stack([s.reshape(g["step_disp"].shape[1:]) for s in seen]).cpu()
    d1 = (steps[0] - g["step_disp"][0]).abs()
    # step 1 (before any renewal decision is fed back): the contract's bar against the reference's own output
    # (measured: mean 6.4e-5 px, max 4.9e-4 px)
    assert float(d1.mean()) < 2e-4 and float(d1.max()) < 1e-3, (float(d1.mean()), float(d1.max()))
    d = (pred.cpu() - g["pred"]).abs()
    print("igev model vs reference class: step1 mean", float(d1.mean()), "max", float(d1.max()), "frac>1e-3",
          float((d1 > 1e-3).float().mean()), "| final mean", float(d.mean()), "max", float(d.max()), "frac>1e-3",
          float((d > 1e-3).float().mean()))
    # final output: every pixel within 1e-3 px of the reference class's output, EPE within 1e-4 (measured: mean
    # 1.8e-6 px, max 2.0e-4 px)
    assert float(d.max()) < 1e-3 and float(d.mean()) < 1e-4, (float(d.max()), float(d.mean()))
    gt = flow_full[0].cpu()
    assert abs(float((pred.cpu() - gt).abs().mean()) - float((g["pred"] - gt).abs().mean())) < 1e-4


@pytest.mark.gpu
def test_config5_size_20_steps_32_iterations():
    """BASELINE config 5 geometry on one GPU: 1248x384, 20 DDIM steps, 32 GRU iterations per step through the real
    BasicMultiUpdateBlock (640 filtered lookups + update-block passes per pair).  Checked: the step / iteration
    counts really run, the result is finite and inside the disparity range, bit-reproducible, and independent of
    what else is in the batch (pair 0 alone / pairs 2-3 alone == the same pairs inside the batch of 4 -- BASELINE's 4 pairs
    per GPU: the data-parallel sharding property)."""
    from diffuvolume_amd import update as U
    steps, iters = 20, 32
    cof = [0.5] + [0.0] * (steps - 1) + [0.5]
    m = build(steps=steps, cof=cof)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=7, scale={"update_block.disp_head.conv2.weight": 0.05,
                                                                      "update_block.disp_head.conv2.bias": 0.0,
                                                                      "classifier.weight": 20.0}), strict=True)
    m = m.to(DEV).eval()
    g = _gen(77, "cfg5")
    B = 4
    img1 = torch.rand(B, 3, 384, 1248, generator=g) * 255
    img2 = torch.roll(img1, -9, dims=-1)
    flow_full = (9 + torch.randn(B, 1, 384, 1248, generator=g)).clamp(0.5, 47)
    flow_gt = F.interpolate(flow_full, size=(96, 312), mode="bilinear") / 4
    calls = {"n": 0}
    inner = U.BasicMultiUpdateBlock.forward

    def counting(self, *a, **k):
        calls["n"] += 1
        return inner(self, *a, **k)

    def run(lo, hi):
        tape = NoiseTape(5)

        def draw(kind, shape, dtype):
            return tape(kind, (B,) + tuple(shape[1:]), dtype)[lo:hi]

        sl = slice(lo, hi)
        return m(img1[sl].to(DEV), img2[sl].to(DEV), flow_full[sl].to(DEV), flow_gt[sl].to(DEV), iters=iters,
                 test_mode=True, noise=draw)[0]

    U.BasicMultiUpdateBlock.forward = counting
    try:
        both = run(0, B)
    finally:
        U.BasicMultiUpdateBlock.forward = inner
    assert calls["n"] == steps * iters
    assert tuple(both.shape) == (B, 384, 1248) and bool(torch.isfinite(both).all())
    assert float(both.min()) >= 0.0 and float(both.max()) <= 4 * 47 + 1e-3
    # round 5: the 2-D front (feature pyramid on the stub backbone, stems, context encoder, spx heads) runs on the in-tree
    # kernels too -- no MIOpen solver choice anywhere on the path -- so a rerun and the shards of the batch carry the bits
    # the batch has (what the N-rank sharding of config 5 rests on)
    again, alone, pair = run(0, B), run(0, 1), run(2, 4)
    for name, x, y in (("rerun", again, both), ("shard [0,1)", alone, both[:1]), ("shard [2,4)", pair, both[2:4])):
        assert torch.equal(x, y), (name, float((x - y).abs().max()))


# ---- the origin network (KITTI15/core/igev_stereo.py): what evaluate_stereo.py:88 runs first for `flow_pr` ----------
def build_origin():
    from diffuvolume_amd.igev_stereo import IGEVStereo
    from diffuvolume_amd.igev_stereo_ddim import Feature
    return IGEVStereo(types.SimpleNamespace(**ARGS), feature=Feature(StubMobileNetV2()))


def test_origin_state_dict_layout():
    g = load_golden("igev_origin")
    m = build_origin()
    sd = m.state_dict()
    assert len(sd) == g["n_keys"]                  # the reference class's own key count (checked key by key in the generator)
    assert not any(k.startswith("time_embedding") or "alphas" in k or k == "betas" for k in sd)
    for k in ("update_block.gru04.convz.weight", "context_zqr_convs.2.bias", "spx.0.weight", "spx_2.conv2.conv.weight",
              "spx_4.0.conv.weight", "cost_agg.feature_att_up_8.feat_att.0.conv.weight", "classifier.weight"):
        assert k in sd, k
    m.load_state_dict(synth_state_dict(sd, seed=3), strict=True)
    with pytest.raises(NotImplementedError):
        m.train()(torch.zeros(1, 3, 64, 128), torch.zeros(1, 3, 64, 128))


@pytest.mark.gpu
def test_origin_forward_vs_the_reference_class():
    """Both eval modes of igev_stereo.py:151-221 against the reference class's own outputs: the disparity after the
    last GRU iteration (test_mode=True, evaluate_stereo.py:88), and the upsampled initial disparity + every iteration's
    prediction (test_mode=False) -- the contract's bars on each map: <= 1e-3 px on 99.9 % of the pixels, mean
    difference below 1e-4 px."""
    g = load_golden("igev_origin")
    scale = {str(k): float(v) for k, v in zip(g["scale_keys"].tolist(), g["scale_vals"].tolist())}
    m = build_origin()
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=g["seed"], scale=scale), strict=True)
    m = m.to(DEV).eval()
    gen = _gen(g["seed"], "igev_origin")
    img1 = torch.rand(1, 3, 64, 128, generator=gen) * 255
    img2 = torch.roll(img1, -6, dims=-1)
    pred = m(img1.to(DEV), img2.to(DEV), iters=g["iters"], test_mode=True)
    init_disp, preds = m(img1.to(DEV), img2.to(DEV), iters=g["iters"], test_mode=False)
    assert tuple(pred.shape) == tuple(g["pred"].shape) and len(preds) == g["iters"]

    rows = {}

    def measure(name, a, b):
        d = (a.cpu().reshape(b.shape) - b).abs()
        rows[name] = (float(d.mean()), float(d.max()), float((d > 1e-3).float().mean()))
        print(f"igev origin {name}: mean {rows[name][0]:.2e} px, max {rows[name][1]:.2e} px, beyond 1e-3 px {rows[name][2]:.2e}")

    measure("test_mode=True", pred, g["pred"])
    measure("init_disp", init_disp, g["init_disp"])
    for i, p in enumerate(preds):
        measure(f"iteration {i + 1}", p, g["preds"][i:i + 1])
    # No recurrence yet (the cost-volume front + convex upsampling; one pass through the update block): the contract's
    # bars.  From the second iteration on the untrained GRU feeds its own output back (the disparity moves ~1.2 px per
    # iteration on a 30-120 px range) and two fp32 evaluations drift apart at fp32 level -- relative to the disparity
    # the difference stays below 1e-5; it is bounded here so that a defect (1e-2 px and up) cannot hide.
    for name in ("init_disp", "iteration 1"):
        assert rows[name][2] <= 1e-3 and rows[name][0] < 1e-4, (name, rows[name])
    for name, (mean, mx, frac) in rows.items():
        assert mean < 5e-4 and mx < 2e-2, (name, mean, mx, frac)
    # the two modes run the same iterations; the PyTorch 2-D modules around the HIP kernels (MIOpen) may pick another solver
    # on the second call, so the two results agree to fp32 re-association, not necessarily bit for bit
    dd = (preds[-1] - pred).abs()
    assert float(dd.mean()) < 5e-4 and float(dd.max()) < 2e-2, (float(dd.mean()), float(dd.max()))


@pytest.mark.gpu
def test_validate_kitti_sample_runs_the_two_networks_back_to_back():
    """KITTI15/evaluate_stereo.py:80-117 on one synthetic item of a size that needs padding (370 x 1226 -> 384 x 1248):
    origin network -> flow_pr / flow_4 -> DiffuVolume network -> unpadded disparity -> EPE / D1."""
    from diffuvolume_amd.pipeline import _sintel_pad, validate_kitti_sample
    assert _sintel_pad(370, 1226) == [11, 11, 7, 7] and _sintel_pad(384, 1248) == [0, 0, 0, 0]
    scale = {"update_block.disp_head.conv2.weight": 0.05, "update_block.disp_head.conv2.bias": 0.0, "classifier.weight": 20.0}
    origin, ddim = build_origin(), build()
    origin.load_state_dict(synth_state_dict(origin.state_dict(), seed=8, scale=scale), strict=True)
    ddim.load_state_dict(synth_state_dict(ddim.state_dict(), seed=7, scale=scale), strict=True)
    origin, ddim = origin.to(DEV).eval(), ddim.to(DEV).eval()
    g = _gen(78, "kitti")
    img1 = torch.rand(3, 370, 1226, generator=g) * 255
    img2 = torch.roll(img1, -9, dims=-1)
    gt = (36 + torch.randn(1, 370, 1226, generator=g)).clamp(1, 190)
    valid = (torch.rand(370, 1226, generator=g) > 0.3).float()
    out = validate_kitti_sample(origin, ddim, img1, img2, gt, valid, iters=4)
    assert set(out) == {"epe", "d1"} and 0.0 <= out["d1"] <= 1.0 and out["epe"] >= 0.0 and out["epe"] == out["epe"]


@pytest.mark.gpu
def test_gru_iterations_as_a_hipgraph_give_the_eager_bits():
    """IGEVDiffusionLoop.use_graph (opt-in, DV_IGEV_GRAPH=1): the GRU iterations of a DDIM step captured once per forward
    and replayed for the later steps -- same launches, same order, same bits as the eager loop."""
    from diffuvolume_amd.igev_stereo_ddim import IGEVDiffusionLoop
    m = build(steps=4, cof=[0.4, 0.1, 0.1, 0.1, 0.3])
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=3, scale={"update_block.disp_head.conv2.weight": 0.05,
                                                                      "update_block.disp_head.conv2.bias": 0.0}), strict=True)
    m = m.to(DEV).eval()
    img1, img2, flow_full, flow_gt = (t.to(DEV) for t in golden_inputs(11, 64, 160))
    outs = {}
    old = IGEVDiffusionLoop.use_graph
    try:
        for flag in (False, True, True):
            IGEVDiffusionLoop.use_graph = flag
            outs.setdefault(flag, []).append(m(img1, img2, flow_full, flow_gt, iters=5, test_mode=True, noise=NoiseTape(9))[0].clone())
    finally:
        IGEVDiffusionLoop.use_graph = old
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[True][0], outs[True][1])


@pytest.mark.gpu
def test_weights_written_in_place_rebuild_the_plans():
    """An update-block conv weight and a BatchNorm statistic of hourglass(8) overwritten in place between two forwards
    (no hook fires): the next forward folds / packs the new values, bit for bit what a model loaded with them gives."""
    m = build()
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=3, scale={"update_block.disp_head.conv2.weight": 0.05,
                                                                      "update_block.disp_head.conv2.bias": 0.0}), strict=True)
    m = m.to(DEV).eval()
    ins = [t.to(DEV) for t in golden_inputs(11)]

    def run(model):
        return model(*ins, iters=3, test_mode=True, noise=NoiseTape(9))[0].clone()

    before = run(m)
    with torch.no_grad():
        m.update_block.gru04.convq.weight.mul_(1.5)
        m.cost_agg.conv1[0].bn.running_var.mul_(2.0)
    after = run(m)
    fresh = build()
    fresh.load_state_dict(m.state_dict(), strict=True)
    assert not torch.equal(after, before)
    assert torch.equal(after, run(fresh.to(DEV).eval()))
