"""Mixed-precision training of IGEVStereo_ddim on the MI355X: ``forward_train(..., amp=True)`` (the update block at train
precision "f16", everything else float32) stepped through ``torch.amp.GradScaler`` -- the replacement of the reference's
``--mixed_precision`` loop (KITTI15/train_stereo.py:146-173).  Smallest plane of the whole-step workload (B 1, 64 x 128),
2 iterations."""
import types

import pytest
import torch

from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
from diffuvolume_amd.loss import sequence_loss
from diffuvolume_amd.synth import (IGEV_TRAIN_ARGS, IGEV_TRAIN_WEIGHT_SEED, StubMobileNetV2, igev_train_step_inputs,
                                   synth_state_dict)

pytestmark = pytest.mark.gpu
CASE = dict(seed=83, b=1, h=64, w=128, iters=2, t=400)


def fresh_model():
    m = IGEVStereo_ddim(types.SimpleNamespace(**IGEV_TRAIN_ARGS), feature=Feature(StubMobileNetV2()))
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=IGEV_TRAIN_WEIGHT_SEED), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    return m


def forward_loss(model, x, **kw):
    init, preds = model.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=x["iters"], t=x["t"],
                                      noise=x["noise"], **kw)
    loss, _ = sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=IGEV_TRAIN_ARGS["max_disp"])
    return loss, init, preds


@pytest.fixture(scope="module")
def x():
    return igev_train_step_inputs(device="cuda", **CASE)


def test_basic_call_and_precision_restored(x, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    runs = {}
    for amp in (False, True):
        model = fresh_model()
        loss, init, preds = forward_loss(model, x, amp=amp)
        assert model.update_block.train_precision == "f32"           # back to the default after the call
        assert all(m.train_precision == "f32" for m in (model.update_block.gru04, model.update_block.encoder))
        loss.backward()
        assert init.dtype == torch.float32 and tuple(init.shape) == (CASE["b"], 1, CASE["h"], CASE["w"])
        assert len(preds) == CASE["iters"]
        for p in preds:
            assert p.dtype == torch.float32 and tuple(p.shape) == (CASE["b"], 1, CASE["h"], CASE["w"])
            assert torch.isfinite(p).all()
        runs[amp] = dict(preds=[p.detach() for p in preds], loss=loss.detach(),
                         none=sorted(n for n, p in model.named_parameters() if p.grad is None),
                         grads={n: p.grad for n, p in model.named_parameters() if p.grad is not None})
    assert not torch.equal(runs[True]["preds"][-1], runs[False]["preds"][-1])       # the fp16 block computes other values
    d = (runs[True]["preds"][-1] - runs[False]["preds"][-1]).double()
    print(f"AMP last prediction against float32: relative L2 {float(d.norm() / runs[False]['preds'][-1].double().norm()):.3e}")
    assert runs[True]["none"] == runs[False]["none"]
    assert all(g.dtype == torch.float32 and torch.isfinite(g).all() for g in runs[True]["grads"].values())
    # after an exception inside the call, too
    model = fresh_model()
    with pytest.raises(RuntimeError):
        model.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"][:, :, :3], iters=1, amp=True)
    assert model.update_block.train_precision == "f32" and model.update_block.disp_head.train_precision == "f32"


def scaler_step(model, x, scaler, opt):
    opt.zero_grad(set_to_none=True)
    loss, _, _ = forward_loss(model, x, amp=True)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    scaler.step(opt)
    scaler.update()
    return grads


def test_full_step_with_the_grad_scaler(x, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    scaler = torch.amp.GradScaler("cuda")
    scale0 = scaler.get_scale()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = scaler_step(model, x, scaler, opt)
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert scaler.get_scale() == scale0
    changed = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert any(n.startswith("update_block.") for n in changed) and any(not n.startswith("update_block.") for n in changed)


def test_overflowing_scale_skips_the_step(x, monkeypatch):
    """init_scale 2^40: the scaled gradients leave the fp16 range inside the block (numeric infinities only), the scaler
    skips the step -- every parameter keeps its bits -- and halves its scale."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 40)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = scaler_step(model, x, scaler, opt)
    assert not all(torch.isfinite(g).all() for g in grads)
    assert all(torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())
    assert scaler.get_scale() == 2.0 ** 39


def test_refusals_that_stay(x, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    args = (x["image1"], x["image2"], x["flow_full"], x["flow_gt"])
    model.args.mixed_precision = True
    try:
        with pytest.raises(DiffuVolumeError, match="amp=True"):
            model.forward_train(*args, iters=1)
    finally:
        model.args.mixed_precision = False
    for amp in (False, True):
        with torch.autocast("cuda", dtype=torch.float16), pytest.raises(DiffuVolumeError, match="amp=True"):
            model.forward_train(*args, iters=1, amp=amp)
    assert model.update_block.train_precision == "f32"
