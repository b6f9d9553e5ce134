"""Backward of the convex upsampling on the MI355X (dv_context_upsample_bwd_f32 through igev_stereo_ddim.context_upsample).

Both gradients against float64 autograd of the oracle's `context_upsample` (oracle/igev_oracle.py: the reference's
expression) on the CPU.  Bar per gradient, as relative L2 against float64:
    rel(hip, f64) <= 2 * err32 + 1e-6
with err32 the error of that same expression run in float32 on the CPU, computed here.  Shapes (B, h, w): (3, 1, 1) a
single cell, all taps but the centre outside; (2, 5, 7) odd planes; (1, 2, 70) a cell row longer than a wave and no
multiple of it (two blocks per row, the second partly idle).

Measured on the MI355X: logits gradient at most 1.8e-7, disparity gradient 1.1e-7, forward 8.0e-8 (bars 1.0e-6 to 1.4e-6)."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd.igev_stereo_ddim import context_upsample
from diffuvolume_amd.synth import _gen
from oracle import igev_oracle as IO

pytestmark = pytest.mark.gpu
SHAPES = [(3, 1, 1), (2, 5, 7), (1, 2, 70)]


def inputs(shape, softmax):
    b, h, w = shape
    key = f"{b}x{h}x{w}"
    disp = torch.randn(b, 1, h, w, generator=_gen(3, "disp" + key)).abs() * 4
    wts = torch.randn(b, 9, 4 * h, 4 * w, generator=_gen(3, "w" + key)) * (2.0 if softmax else 1.0)
    cot = torch.randn(b, 4 * h, 4 * w, generator=_gen(3, "cot" + key))
    return disp, wts, cot


def oracle_grads(disp, wts, cot, scale, softmax, dtype):
    d = disp.to(dtype).clone().requires_grad_(True)
    w = wts.to(dtype).clone().requires_grad_(True)
    out = IO.context_upsample(d * scale, F.softmax(w, 1) if softmax else w)
    out.backward(cot.to(dtype))
    return out.detach(), d.grad, w.grad


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


_REF = {}


def reference(shape, scale, softmax):
    """float64 gradients and the float32 expression's own error, once per case."""
    key = (shape, scale, softmax)
    if key not in _REF:
        disp, wts, cot = inputs(shape, softmax)
        o64, d64, w64 = oracle_grads(disp, wts, cot, scale, softmax, torch.float64)
        o32, d32, w32 = oracle_grads(disp, wts, cot, scale, softmax, torch.float32)
        _REF[key] = dict(out=o64, d=d64, w=w64, err=dict(out=rel(o32, o64), d=rel(d32, d64), w=rel(w32, w64)))
    return _REF[key]


def hip_grads(shape, scale, softmax, need_d=True, need_w=True):
    disp, wts, cot = (t.cuda() for t in inputs(shape, softmax))
    d, w = disp.requires_grad_(need_d), wts.requires_grad_(need_w)
    out = context_upsample(d, w, scale=scale, apply_softmax=softmax)
    out.backward(cot)
    torch.cuda.synchronize()
    return out.detach(), d.grad, w.grad


@pytest.mark.parametrize("scale", [4.0, 1.0])
@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_gradients_match_float64_autograd(shape, softmax, scale):
    ref = reference(shape, scale, softmax)
    out, dd, dw = hip_grads(shape, scale, softmax)
    assert dd.shape == ref["d"].shape and dw.shape == ref["w"].shape
    for name, ours in (("out", out), ("d", dd), ("w", dw)):
        e, bar = rel(ours, ref[name]), 2 * ref["err"][name] + 1e-6
        print(f"PARITY context_upsample {shape} softmax={softmax} scale={scale} {name}: {e:.3e}  bar {bar:.2e}")
        assert e <= bar, (name, e, bar)


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_sided_gradients_and_repeatability(shape, softmax):
    out, dd, dw = hip_grads(shape, 4.0, softmax)
    out2, dd2, dw2 = hip_grads(shape, 4.0, softmax)
    assert torch.equal(out, out2) and torch.equal(dd, dd2) and torch.equal(dw, dw2)          # two calls: the same bits
    out_d, dd_only, none_w = hip_grads(shape, 4.0, softmax, need_w=False)
    out_w, none_d, dw_only = hip_grads(shape, 4.0, softmax, need_d=False)
    assert none_w is None and none_d is None
    assert torch.equal(dd_only, dd) and torch.equal(dw_only, dw)
    disp, wts, _ = (t.cuda() for t in inputs(shape, softmax))
    with torch.no_grad():
        plain = context_upsample(disp, wts, scale=4.0, apply_softmax=softmax)
    assert torch.equal(plain, out) and torch.equal(plain, out_d) and torch.equal(plain, out_w)  # the inference launch's bits
    assert not plain.requires_grad and not context_upsample(disp, wts, scale=4.0, apply_softmax=softmax).requires_grad


def test_torch_route_and_bad_logit_shapes(monkeypatch):
    shape = (2, 5, 7)
    ref = reference(shape, 4.0, True)
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    out, dd, dw = hip_grads(shape, 4.0, True)
    for name, ours in (("out", out), ("d", dd), ("w", dw)):
        assert rel(ours, ref[name]) <= 2 * ref["err"][name] + 1e-6, name
    monkeypatch.delenv("DV_TRAIN_CONV2D")
    disp = torch.zeros(2, 1, 5, 7, device="cuda", requires_grad=True)
    for bad in ((2, 9, 20, 27), (2, 8, 20, 28), (1, 9, 20, 28)):
        with pytest.raises(RuntimeError, match="up_weights"):
            context_upsample(disp, torch.zeros(bad, device="cuda"), scale=4.0, apply_softmax=True)
