"""ConvTranspose2d(kernel 4, stride 2, padding 1) on the differentiable HIP route (train2d.conv_transpose2d_k4):
weight gradient on dv_deconv2d_k4s2_wgrad_f32, input gradient on the forward 3x3 kernels, bias gradient a sum.

dW, dx and db against float64 `F.conv_transpose2d` autograd on the CPU.  Bar per gradient, as relative L2:
    rel(hip, f64) <= 2 * err32 + 1e-6
with err32 the error of the same torch expression run in float32 on the CPU, computed here.  Channel pairs: (32, 32)
`spx_2_gru.conv1`, (64, 9) `spx_gru` (three blocks of three output channels, four N tiles), (8, 3) one partly filled N
tile and one block of three waves.  Planes 1 x 3 (a single brick, every tap row meets a border), 5 x 7 (odd, under one
brick wide), 8 x 16 (two bricks), 13 x 3 (four bricks per item: the smallest plane of that width whose split count at batch
3 is at least 5 and no multiple of 4); batch 1 and 3 (bricks of several batch items in one split sequence).  Split counts
(the workspace size over numel(dW)): 1 or 3 on the first three planes, and on 13 x 3 two at batch 1 (two of the four quarters of the split
sum are empty) and six at batch 3 (quarters of 1, 2, 1 and 2 splits).

Measured on the MI355X: at most 2.4e-7 over out / dx / dW / db of all cases (bars 1.1e-6 to 3.0e-6)."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import DiffuVolumeError, train2d
from diffuvolume_amd.submodule import Deconv2dK4S2Plan
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu
CHANNELS = [(32, 32), (64, 9), (8, 3)]
PLANES = [(1, 3), (5, 7), (8, 16), (13, 3)]


def inputs(cin, cout, h, w, b):
    key = f"{cin}x{cout}x{h}x{w}x{b}"
    x = torch.randn(b, cin, h, w, generator=_gen(5, "x" + key))
    wt = torch.randn(cin, cout, 4, 4, generator=_gen(5, "w" + key)) * (2.0 / (16 * cin)) ** 0.5
    bias = torch.randn(cout, generator=_gen(5, "b" + key)) * 0.1
    cot = torch.randn(b, cout, 2 * h, 2 * w, generator=_gen(5, "g" + key))
    return x, wt, bias, cot


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def torch_grads(x, wt, bias, cot, dtype):
    x, wt, bias = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, wt, bias))
    out = F.conv_transpose2d(x, wt, bias, stride=2, padding=1)
    out.backward(cot.to(dtype))
    return dict(out=out.detach(), dx=x.grad, dw=wt.grad, db=bias.grad)


def hip_grads(x, wt, bias, cot):
    x, wt, bias = (t.detach().cuda().requires_grad_(True) for t in (x, wt, bias))
    out = train2d.conv_transpose2d_k4(x, wt, bias)
    out.backward(cot.cuda())
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad, dw=wt.grad, db=bias.grad)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("channels", CHANNELS)
def test_gradients_match_float64_autograd(channels, plane, b, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    data = inputs(*channels, *plane, b)
    r64, r32 = torch_grads(*data, torch.float64), torch_grads(*data, torch.float32)
    ours = hip_grads(*data)
    again = hip_grads(*data)
    for name in ("out", "dx", "dw", "db"):
        assert ours[name].shape == r64[name].shape, name
        e, bar = rel(ours[name], r64[name]), 2 * rel(r32[name], r64[name]) + 1e-6
        print(f"PARITY deconv2d_k4 {channels} {plane} B{b} {name}: {e:.3e}  bar {bar:.2e}")
        assert e <= bar, (name, e, bar)
        assert torch.equal(ours[name], again[name]), name                            # the same bits twice
    x, wt, bias, _ = (t.cuda() for t in data)
    with torch.no_grad():
        assert torch.equal(ours["out"], Deconv2dK4S2Plan(wt, None, bias=bias)(x))    # the inference plan's bits


def test_no_bias_frozen_input_and_cached_plan(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x, wt, _, cot = (t.cuda() for t in inputs(8, 3, 5, 7, 3))
    full = hip_grads(x.cpu(), wt.cpu(), torch.zeros(3), cot.cpu())
    w = wt.clone().requires_grad_(True)
    plan = train2d.TrainDeconvPlan(w)
    calls = []
    out = train2d.conv_transpose2d_k4(x, w, None, lambda: calls.append(1) or plan)   # x asks for no gradient
    out.backward(cot)
    assert calls == [1] and torch.equal(out.detach(), full["out"]) and torch.equal(w.grad, full["dw"])
    m = torch.nn.ConvTranspose2d(8, 3, 4, 2, 1).cuda()
    xg = x.clone().requires_grad_(True)
    train2d.conv_transpose2d_module(m, xg).backward(cot)
    assert m.weight.grad is not None and m.bias.grad is not None and xg.grad.shape == x.shape
    assert torch.equal(m.bias.grad, cot.sum((0, 2, 3)))


def test_torch_route_and_unsupported_geometry(monkeypatch):
    data = inputs(8, 3, 5, 7, 1)
    r64, r32 = torch_grads(*data, torch.float64), torch_grads(*data, torch.float32)
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    ours = hip_grads(*data)
    for name in ("out", "dx", "dw", "db"):
        assert rel(ours[name], r64[name]) <= 2 * rel(r32[name], r64[name]) + 1e-6, name
    monkeypatch.delenv("DV_TRAIN_CONV2D")
    x = torch.zeros(1, 8, 2, 2, device="cuda")
    for m in (torch.nn.ConvTranspose2d(8, 3, 4, 2, 0), torch.nn.ConvTranspose2d(8, 3, 3, 2, 1),
              torch.nn.ConvTranspose2d(8, 3, 4, 1, 1), torch.nn.ConvTranspose2d(8, 4, 4, 2, 1, groups=2),
              torch.nn.ConvTranspose2d(8, 3, 4, 2, 1, output_padding=1)):
        with pytest.raises(DiffuVolumeError):
            train2d.conv_transpose2d_module(m.cuda(), x)
    with pytest.raises(DiffuVolumeError):
        train2d.conv_transpose2d_k4(x, torch.zeros(8, 3, 3, 3, device="cuda"))
    with pytest.raises(DiffuVolumeError):                                            # channel mismatch
        train2d.conv_transpose2d_k4(x, torch.zeros(16, 3, 4, 4, device="cuda", requires_grad=True))
