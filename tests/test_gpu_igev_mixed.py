"""IGEV with `mixed_precision=True`: the update block under fp16 autocast (csrc/conv2d_f16.hip) against the reference's
own semantics -- the oracle's update block run on the GPU under the same real `torch.autocast` (MIOpen fp16) -- with both
triangulated against the float64 / float32 oracle; the loop, and the whole model's mode switch."""
import types

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib
from diffuvolume_amd.synth import NoiseTape, StubMobileNetV2, _gen, synth_state_dict
from oracle import igev_oracle as I
from test_igev_update_oracle import ARGS, update_inputs, update_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return t.to(DEV)


def f16_values(net, inp):
    """What the reference's autocast front hands to the loop: fp16 hidden states and context terms."""
    return [t.half().float() for t in net], [[t.half().float() for t in l] for l in inp]


def make_block(sd):
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    m = BasicMultiUpdateBlock(ARGS, hidden_dims=[128, 128, 128])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def autocast_oracle(sd):
    """The oracle's update block on the GPU under real fp16 autocast; CPU float32 in and out (fp16-valued outputs)."""
    sd_gpu = {k: dev(v) for k, v in sd.items()}

    def call(net, inp, corr, disp, **kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            # hidden states and context terms are fp16 tensors in the reference (its front runs under autocast too);
            # the lookup and the disparity are float32 (they are computed outside the autocast region)
            out = I.update_block(sd_gpu, [dev(t).half() for t in net], [[dev(t).half() for t in l] for l in inp],
                                 dev(corr), dev(disp),
                                 iter04=kw.get("iter04", True), iter08=kw.get("iter08", True),
                                 iter16=kw.get("iter16", True))
        nets, mask, delta = out
        return [t.float().cpu() for t in nets], mask.float().cpu(), delta.float().cpu()
    return call


def test_update_block_call_vs_reference_autocast():
    sd = update_state_dict(401)
    m = make_block(sd)
    net, inp, corr, disp = update_inputs(402, 2, 24, 312)
    net, inp = f16_values(net, inp)
    with torch.autocast("cuda", dtype=torch.float16):
        hn, hmask, hdelta = m([dev(t) for t in net], [[dev(t) for t in l] for l in inp], dev(corr), dev(disp))
    an, amask, adelta = autocast_oracle(sd)(net, inp, corr, disp)
    sd64 = {k: v.double() for k, v in sd.items()}
    rn, rmask, rdelta = I.update_block(sd64, [t.double() for t in net], [[t.double() for t in l] for l in inp],
                                       corr.double(), disp.double())
    for name, h, a, r in (("net0", hn[0], an[0], rn[0]), ("net1", hn[1], an[1], rn[1]), ("net2", hn[2], an[2], rn[2]),
                          ("delta", hdelta, adelta, rdelta), ("mask", hmask, amask, rmask)):
        h = h.cpu().double()
        assert h.dtype == torch.float64 and torch.equal(h, h.float().half().double()), f"{name}: not fp16-exact"
        eh, ea = (h - r).abs(), (a.double() - r).abs()
        print(f"{name}: mean |hip - f64| {float(eh.mean()):.3e} (autocast {float(ea.mean()):.3e}), "
              f"max {float(eh.max()):.3e} (autocast {float(ea.max()):.3e})")
        assert float(eh.mean()) <= 1.25 * float(ea.mean()) and float(eh.max()) <= 2 * float(ea.max()), name


def test_update_block_accepts_fp16_inputs_and_refuses_bf16():
    sd = update_state_dict(403)
    m = make_block(sd)
    net, inp, corr, disp = update_inputs(404, 1, 16, 24)
    net, inp = f16_values(net, inp)
    with torch.autocast("cuda", dtype=torch.float16):
        a = m([dev(t) for t in net], [[dev(t) for t in l] for l in inp], dev(corr), dev(disp))
        b = m([dev(t).half() for t in net], [[dev(t).half() for t in l] for l in inp], dev(corr).half(), dev(disp))
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert x.dtype == torch.float32 and torch.equal(x, y)
    with pytest.raises(_lib.DiffuVolumeError, match="fp16"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            m([dev(t) for t in net], [[dev(t) for t in l] for l in inp], dev(corr), dev(disp))


def _loop_fixture(seed, b, h, w, steps, cof=None):
    from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
    from diffuvolume_amd.igev_stereo_ddim import DynamicHead180, IGEVDiffusionLoop
    from diffuvolume_amd.synth import toy_upsample_disp
    sd = update_state_dict(seed)
    sd["disp_head.conv2.weight"] = sd["disp_head.conv2.weight"] * 0.05      # keep the per-iteration step ~1 bin
    m = make_block(sd)
    head = DynamicHead180()
    head.load_state_dict(synth_state_dict(head.state_dict(), seed=seed + 1), strict=True)
    head = head.eval()
    net, inp, _, _ = update_inputs(seed + 2, b, h, w)
    net, inp = f16_values(net, inp)
    geo = torch.randn(b, 8, 48, h, w, generator=_gen(seed + 3, "geo"))
    f1, f2 = torch.randn(b, 16, h, w, generator=_gen(seed + 3, "f1")), torch.randn(b, 16, h, w, generator=_gen(seed + 3, "f2"))
    init = torch.rand(b, 1, h, w, generator=_gen(seed + 3, "init")) * 40
    kw = {} if cof is None else {"cof": cof}
    orcs = {mode: I.IGEVLoopOracle(head.state_dict(), fn, toy_upsample_disp, geo, f1, f2, sampling_timesteps=steps,
                                   net_list=net, inp_list=inp, **kw)
            for mode, fn in (("f32", lambda n, i, c, f, **k: I.update_block(sd, n, i, c, f)), ("amp", autocast_oracle(sd)))}
    geo_fn = Combined_Geo_Encoding_Volume(dev(f1), dev(f2), dev(geo), radius=4, num_levels=2)
    loop = IGEVDiffusionLoop(head.to(DEV), m, toy_upsample_disp, n_gru_layers=3, slow_fast_gru=False,
                             sampling_timesteps=steps, mixed_precision=True,
                             **({} if cof is None else {"ensemble_cof": cof}))
    return orcs, loop, geo_fn, net, inp, init


def _bar(hip, amp, f32, what):
    eh, ea = float((hip - f32).abs().mean()), float((amp - f32).abs().mean())
    print(f"{what}: mean |hip - oracle f32| {eh:.3e} px, mean |oracle autocast - oracle f32| {ea:.3e} px")
    assert eh <= 1.5 * ea + 1e-3, (what, eh, ea)


def test_ddim_step_teacher_forced_at_config5_size_mixed():
    """One DDIM step (t = 999, 32 GRU iterations) at config 5's quarter resolution 96 x 312."""
    steps = 20
    cof = (0.6,) + (0.0,) * (steps - 2) + (0.1, 0.3)
    orcs, loop, geo_fn, net, inp, init = _loop_fixture(411, 1, 96, 312, steps, cof)
    x_t = torch.randn(1, 48, 96, 312, generator=_gen(415, "xt"))
    t = torch.full((1,), 999, dtype=torch.long)
    preds = {mode: o.model_predictions(init, init, 32, x_t, t)[2] for mode, o in orcs.items()}
    _, _, pred, _ = loop.model_predictions(dev(init), dev(init), None, 32, [dev(x) for x in net],
                                           [[dev(x) for x in l] for l in inp], geo_fn, dev(x_t), dev(t), None)
    _bar(pred.cpu(), preds["amp"], preds["f32"], "config-5 size step")


def test_free_run_2_steps_32_iterations_mixed():
    orcs, loop, geo_fn, net, inp, init = _loop_fixture(421, 1, 16, 24, 2)
    used = F.interpolate(init * 4, scale_factor=4, mode="bilinear") + 1.5
    asd = torch.rand(1, 48, 16, 24, generator=_gen(425, "asd")) * 2 - 1
    finals = {mode: o.ddim_sample(init, init, 32, used, asd, NoiseTape(426)) for mode, o in orcs.items()}
    final = loop.ddim_sample(dev(init), dev(init), None, 32, [dev(x) for x in net], [[dev(x) for x in l] for l in inp],
                             geo_fn, dev(used), dev(asd), None, noise=NoiseTape(426))
    shape = finals["f32"].shape
    _bar(final.cpu().reshape(shape), finals["amp"].reshape(shape), finals["f32"], "free run")


def test_whole_model_mode_switch_and_graph_replay():
    """IGEVStereo_ddim.forward at 1248x384 with the flag read per forward: mixed differs from fp32, a hipGraph replay of
    the mixed GRU iterations gives the eager bits, and flipping back gives the bits of the fp32 run before."""
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVDiffusionLoop, IGEVStereo_ddim
    args = types.SimpleNamespace(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2,
                                 corr_radius=4, slow_fast_gru=False, max_disp=192, mixed_precision=False)
    m = IGEVStereo_ddim(args, feature=Feature(StubMobileNetV2()), sampling_timesteps=3, ensemble_cof=(0.4, 0.2, 0.1, 0.3))
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=431, scale={"update_block.disp_head.conv2.weight": 0.05,
                                                                        "update_block.disp_head.conv2.bias": 0.0,
                                                                        "classifier.weight": 20.0}), strict=True)
    m = m.to(DEV).eval()
    g = _gen(432, "img")
    img1 = torch.rand(1, 3, 384, 1248, generator=g) * 255
    img2 = torch.roll(img1, -9, dims=-1)
    flow_full = (9 + torch.randn(1, 1, 384, 1248, generator=g)).clamp(0.5, 47)
    flow_gt = F.interpolate(flow_full, size=(96, 312), mode="bilinear") / 4
    ins = [dev(t) for t in (img1, img2, flow_full, flow_gt)]

    def run(mixed, graph=False):
        m.args.mixed_precision = mixed
        old = IGEVDiffusionLoop.use_graph
        IGEVDiffusionLoop.use_graph = graph
        try:
            return m(*ins, iters=6, test_mode=True, noise=NoiseTape(433))[0].clone()
        finally:
            IGEVDiffusionLoop.use_graph = old

    fp32_before = run(False)
    mixed_eager = run(True)
    mixed_graph = run(True, graph=True)
    fp32_after = run(False)
    d = (mixed_eager - fp32_before).abs()
    print(f"mixed vs fp32 at 1248x384: mean {float(d.mean()):.3e} px, max {float(d.max()):.3e} px")
    assert bool(torch.isfinite(mixed_eager).all()) and float(d.max()) > 0 and float(d.mean()) < 0.5
    assert torch.equal(mixed_graph, mixed_eager)
    assert torch.equal(fp32_after, fp32_before)
