"""bfloat16 training of IGEVStereo_ddim on the MI355X: ``forward_train(..., amp=torch.bfloat16)`` (the update block at
train precision "bf16", everything else float32) stepped with the plain optimizer -- no ``GradScaler``, no skipped step.
The case is tests/test_gpu_igev_train_amp.py's: the smallest plane of the whole-step workload (B 1, 64 x 128), 2
iterations."""
import pytest
import torch

from diffuvolume_amd import DiffuVolumeError
from test_gpu_igev_train_amp import CASE, forward_loss, fresh_model
from diffuvolume_amd.synth import igev_train_step_inputs

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def x():
    return igev_train_step_inputs(device="cuda", **CASE)


@pytest.fixture(scope="module")
def runs(x):
    """One forward and backward per value of ``amp``, shared by the tests below (never modified)."""
    out = {}
    for amp in (False, True, torch.float16, BF16):
        model = fresh_model()
        loss, init, preds = forward_loss(model, x, amp=amp)
        precision_after = [m.train_precision for m in (model.update_block, model.update_block.gru04, model.update_block.encoder)]
        loss.backward()
        out[amp] = dict(init=init.detach(), preds=[p.detach() for p in preds], loss=loss.detach(), after=precision_after,
                        none=sorted(n for n, p in model.named_parameters() if p.grad is None),
                        grads={n: p.grad for n, p in model.named_parameters() if p.grad is not None})
    return out


def test_basic_call_and_precision_restored(x, runs, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    r = runs[BF16]
    assert r["after"] == ["f32"] * 3                                     # back to the default after the call
    assert r["init"].dtype == torch.float32 and tuple(r["init"].shape) == (CASE["b"], 1, CASE["h"], CASE["w"])
    assert len(r["preds"]) == CASE["iters"]
    for p in r["preds"]:
        assert p.dtype == torch.float32 and tuple(p.shape) == (CASE["b"], 1, CASE["h"], CASE["w"])
        assert torch.isfinite(p).all()
    assert r["none"] == runs[False]["none"]                              # the same parameters stay without a gradient
    assert all(g.dtype == torch.float32 and torch.isfinite(g).all() for g in r["grads"].values())
    last = r["preds"][-1]
    assert not torch.equal(last, runs[False]["preds"][-1]) and not torch.equal(last, runs[True]["preds"][-1])
    d = (last - runs[False]["preds"][-1]).double()
    print(f"BF16 last prediction against float32: relative L2 {float(d.norm() / runs[False]['preds'][-1].double().norm()):.3e}")
    # after an exception inside the call, too
    model = fresh_model()
    with pytest.raises(RuntimeError):
        model.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"][:, :, :3], iters=1, amp=BF16)
    assert model.update_block.train_precision == "f32" and model.update_block.disp_head.train_precision == "f32"
    # a block the caller has set keeps the caller's precision after the call
    model.update_block.set_train_precision(BF16)
    forward_loss(model, x, amp=True)
    assert model.update_block.train_precision == "bf16" and model.update_block.gru08.train_precision == "bf16"


def test_amp_float16_is_amp_true(runs):
    a, b = runs[torch.float16], runs[True]
    assert all(torch.equal(p, q) for p, q in zip(a["preds"], b["preds"])) and torch.equal(a["init"], b["init"])
    assert a["grads"].keys() == b["grads"].keys() and all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])


def test_a_plain_adamw_step_without_a_scaler(x, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss, _, _ = forward_loss(model, x, amp=BF16)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    changed = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert any(n.startswith("update_block.") for n in changed) and any(not n.startswith("update_block.") for n in changed)
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_three_sgd_steps_on_a_loss_scaled_by_2_to_the_20_stay_finite(x, monkeypatch):
    """The scale that overflows fp16 inside the block (tests/test_gpu_igev_train_amp.py skips its step at 2^40; 2^20
    already passes 65504 in the block's gradients) is in range at bf16: no gradient leaves float32."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4 / 2.0 ** 20)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss, _, _ = forward_loss(model, x, amp=BF16)
        (loss * 2.0 ** 20).backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads)
        opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_values_of_amp_and_refusals_that_stay(x, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    model = fresh_model()
    args = (x["image1"], x["image2"], x["flow_full"], x["flow_gt"])
    for bad in ("bf16", torch.float64, 1.5, "f16", None, 1):
        with pytest.raises(ValueError):
            model.forward_train(*args, iters=1, amp=bad)
    with pytest.raises(TypeError):
        model.forward_train(*args, 1, None, False, None, None, BF16)           # amp stays keyword-only
    for dt in (torch.float16, BF16):                                           # a caller's autocast of either dtype
        for amp in (False, True, BF16):
            with torch.autocast("cuda", dtype=dt), pytest.raises(DiffuVolumeError, match="amp=True"):
                model.forward_train(*args, iters=1, amp=amp)
    model.args.mixed_precision = True
    try:
        with pytest.raises(DiffuVolumeError, match="amp=True"):
            model.forward_train(*args, iters=1)
    finally:
        model.args.mixed_precision = False
    assert model.update_block.train_precision == "f32"
