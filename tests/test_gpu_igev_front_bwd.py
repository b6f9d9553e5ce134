"""The backward pieces of IGEV's 2-D front (csrc/igev_front_bwd.hip and the train2d functions on top of them):
  * dv_instance_norm_act_bwd_f32 through train2d.instance_norm_act (none / ReLU / LeakyReLU 0.01);
  * dv_conv2d_fewin_wgrad_f32 through train2d.conv2d_fewin (Cin 1 / 3 / 4, k 3 / 5 / 7, stride 1 / 2);
  * train2d.conv2d_s2 (k3 s2 p1: backward on the k4 transposed-convolution kernels) and train2d.conv2d_k1s2.

Everything against float64 torch autograd on the CPU.  Bar per tensor, as relative L2 (the project's convention,
tests/test_gpu_igev_upsample_train.py):
    rel(hip, f64) <= 2 * rel(torch float32, f64) + 1e-6
with the float32 error of the same torch expression computed here; and two launches give the same bits.

Shapes.  InstanceNorm: planes of 1 (must give zeros: torch itself refuses a single-element plane in training, so that
case is checked against the analytic zero), 5 x 7 (scalar body, under one pass of the 1024 threads), 16 x 24 (float4
body), 33 x 31 = 1023 (one short of the 1024-thread stride, scalar).  Few-in: planes 5 x 7 (under one 8 x 16 brick), 16 x 16
(two bricks per item at stride 1, one at stride 2), 17 x 33 (odd, partial bricks in both directions); Cout 5 (a partly filled
group of 16) and 64 (four groups); batch 2 (bricks of two items in one split sequence).  conv2d_s2: 7 x 9 (both odd: padded
for dW, cropped for dx), 8 x 10 (even), 1 x 1, 5 x 6 (mixed), channels 5 -> 6 and 32 -> 48.

Measured on the MI355X: at most 3.8e-7 over every tensor of every case (bars 1.0e-6 to 3.1e-6)."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import DiffuVolumeError, train2d
from diffuvolume_amd.submodule import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_TANH
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu


def rel(a, ref):
    a, ref = a.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def check(tag, ours, again, r32, r64):
    for name in r64:
        assert ours[name].shape == r64[name].shape, (tag, name)
        e, bar = rel(ours[name], r64[name]), 2 * rel(r32[name], r64[name]) + 1e-6
        print(f"PARITY {tag} {name}: {e:.3e}  bar {bar:.2e}")
        assert e <= bar, (tag, name, e, bar)
        assert torch.equal(ours[name], again[name]), (tag, name)                     # the same bits twice


# ---- InstanceNorm + activation ----------------------------------------------------------------------------------------
ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "leaky": ACT_LEAKY}


def _act(y, name):
    return y if name == "none" else (F.relu(y) if name == "relu" else F.leaky_relu(y, 0.01))


def in_torch(x, cot, name, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    out = _act(F.instance_norm(x, eps=1e-5), name)
    out.backward(cot.to(dtype))
    return dict(out=out.detach(), dx=x.grad)


def in_hip(x, cot, name):
    x = x.cuda().requires_grad_(True)
    out = train2d.instance_norm_act(x, ACTS[name], 1e-5)
    out.backward(cot.cuda())
    torch.cuda.synchronize()
    return dict(out=out.detach(), dx=x.grad)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("plane", [(5, 7), (16, 24), (33, 31)])
def test_instance_norm_act_backward(plane, act, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    key = f"in{plane}{act}"
    x = torch.randn(2, 3, *plane, generator=_gen(61, "x" + key)) * 1.7 + 0.3
    cot = torch.randn(2, 3, *plane, generator=_gen(61, "g" + key))
    ours, again = in_hip(x, cot, act), in_hip(x, cot, act)
    check(f"instance_norm {plane} {act}", ours, again, in_torch(x, cot, act, torch.float32), in_torch(x, cot, act, torch.float64))
    from diffuvolume_amd.igev_stereo_ddim import instance_norm_act
    with torch.no_grad():                                                            # the inference launch's bits
        assert torch.equal(ours["out"], instance_norm_act(x.cuda(), ACTS[act], 1e-5, inplace=False))


@pytest.mark.parametrize("act", list(ACTS))
def test_instance_norm_single_element_plane_gives_zeros(act, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = torch.randn(2, 5, 1, 1, generator=_gen(61, "x1"))
    cot = torch.randn(2, 5, 1, 1, generator=_gen(61, "g1"))
    ours = in_hip(x, cot, act)
    assert torch.equal(ours["dx"], torch.zeros_like(ours["dx"])) and torch.equal(ours["out"], torch.zeros_like(ours["out"]))


def test_instance_norm_refusals_and_torch_route(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = torch.randn(1, 2, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(DiffuVolumeError):
        train2d.instance_norm_act(x, ACT_TANH)
    with pytest.raises(DiffuVolumeError):
        train2d.instance_norm_act(x.detach().cpu().requires_grad_(True), ACT_RELU)
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    xs, cot = torch.randn(2, 3, 5, 7, generator=_gen(61, "xt")), torch.randn(2, 3, 5, 7, generator=_gen(61, "gt"))
    ours = in_hip(xs, cot, "leaky")
    check("instance_norm torch route", ours, ours, in_torch(xs, cot, "leaky", torch.float32), in_torch(xs, cot, "leaky", torch.float64))


# ---- few-input-channel convolution ------------------------------------------------------------------------------------
def conv_torch(x, w, bias, cot, stride, dtype, x_grad):
    x = x.to(dtype).clone().requires_grad_(x_grad)
    w, bias = (t.to(dtype).clone().requires_grad_(True) for t in (w, bias))
    out = F.conv2d(x, w, bias, stride=stride, padding=w.shape[-1] // 2)
    out.backward(cot.to(dtype))
    r = dict(out=out.detach(), dw=w.grad, db=bias.grad)
    if x_grad:
        r["dx"] = x.grad
    return r


def conv_hip(fn, x, w, bias, cot, x_grad):
    x = x.cuda().requires_grad_(x_grad)
    w, bias = (t.cuda().requires_grad_(True) for t in (w, bias))
    out = fn(x, w, bias)
    out.backward(cot.cuda())
    torch.cuda.synchronize()
    r = dict(out=out.detach(), dw=w.grad, db=bias.grad)
    if x_grad:
        r["dx"] = x.grad
    return r


def conv_inputs(cin, cout, k, stride, h, w, b, seed):
    key = f"{cin}x{cout}k{k}s{stride}x{h}x{w}x{b}"
    x = torch.randn(b, cin, h, w, generator=_gen(seed, "x" + key))
    wt = torch.randn(cout, cin, k, k, generator=_gen(seed, "w" + key)) * (2.0 / (k * k * cin)) ** 0.5
    bias = torch.randn(cout, generator=_gen(seed, "b" + key)) * 0.1
    cot = torch.randn(b, cout, (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1,
                      generator=_gen(seed, "g" + key))
    return x, wt, bias, cot


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("cin", [1, 3, 4])
def test_fewin_weight_gradient(cin, k, stride, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    fn = lambda x, w, b: train2d.conv2d_fewin(x, w, b, stride)
    for plane in ((5, 7), (16, 16), (17, 33)):
        for cout in (5, 64):
            data = conv_inputs(cin, cout, k, stride, *plane, 2, 62)
            ours, again = conv_hip(fn, *data, False), conv_hip(fn, *data, False)
            check(f"fewin Cin{cin} k{k} s{stride} {plane} Cout{cout}", ours, again,
                  conv_torch(*data, stride, torch.float32, False), conv_torch(*data, stride, torch.float64, False))


def test_fewin_refusals_and_torch_route(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x, wt, bias, cot = conv_inputs(3, 5, 3, 2, 5, 7, 2, 62)
    with pytest.raises(DiffuVolumeError):                                            # images are data
        train2d.conv2d_fewin(x.cuda().requires_grad_(True), wt.cuda(), None, 2)
    with pytest.raises(DiffuVolumeError):
        train2d.conv2d_fewin(x, wt.requires_grad_(True), None, 2)                    # CPU tensors
    with pytest.raises(DiffuVolumeError):
        train2d.conv2d_fewin(torch.zeros(1, 5, 4, 4, device="cuda"), torch.zeros(2, 5, 3, 3, device="cuda", requires_grad=True))
    with pytest.raises(DiffuVolumeError):
        train2d.conv2d_fewin_weight_grad(x.cuda(), cot.cuda(), 3, 1)                 # g does not belong to stride 1
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    fn = lambda a, w, b: train2d.conv2d_fewin(a, w, b, 2)
    data = (x, wt.detach(), bias, cot)
    ours = conv_hip(fn, *data, False)
    check("fewin torch route", ours, ours, conv_torch(*data, 2, torch.float32, False), conv_torch(*data, 2, torch.float64, False))


# ---- stride-2 convolutions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [(5, 6), (32, 48)])
@pytest.mark.parametrize("plane", [(7, 9), (8, 10), (1, 1), (5, 6)])
def test_conv2d_s2(plane, channels, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    data = conv_inputs(*channels, 3, 2, *plane, 2, 63)
    ours, again = conv_hip(train2d.conv2d_s2, *data, True), conv_hip(train2d.conv2d_s2, *data, True)
    check(f"conv2d_s2 {channels} {plane}", ours, again, conv_torch(*data, 2, torch.float32, True),
          conv_torch(*data, 2, torch.float64, True))


@pytest.mark.parametrize("plane", [(7, 9), (8, 10)])
def test_conv2d_k1s2(plane, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    data = conv_inputs(12, 20, 1, 2, *plane, 2, 64)
    ours, again = conv_hip(train2d.conv2d_k1s2, *data, True), conv_hip(train2d.conv2d_k1s2, *data, True)
    check(f"conv2d_k1s2 {plane}", ours, again, conv_torch(*data, 2, torch.float32, True), conv_torch(*data, 2, torch.float64, True))


def test_conv2d_any_dispatch(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    nn = torch.nn
    for m, cin, x_grad in ((nn.Conv2d(3, 8, 7, 2, 3), 3, False), (nn.Conv2d(6, 8, 3, 1, 1), 6, True), (nn.Conv2d(6, 8, 1), 6, True),
                           (nn.Conv2d(6, 8, 3, 2, 1, bias=False), 6, True), (nn.Conv2d(6, 8, 1, 2), 6, True)):
        m = m.cuda()
        x = torch.randn(2, cin, 9, 12, generator=_gen(65, "x")).cuda().requires_grad_(x_grad)
        out = train2d.conv2d_any(m, x)
        ref = m(x.detach())
        assert out.shape == ref.shape and rel(out, ref) < 1e-5, m
        out.sum().backward()
        assert m.weight.grad is not None and (x.grad is not None) == x_grad, m
    x = torch.zeros(1, 6, 8, 8, device="cuda")
    for m in (nn.Conv2d(6, 8, 5, 1, 2), nn.Conv2d(6, 8, 3, 2, 0), nn.Conv2d(6, 6, 3, 1, 1, groups=2), nn.Conv2d(6, 8, 3, 3, 1),
              nn.ConvTranspose2d(6, 8, 4, 2, 1)):
        with pytest.raises(DiffuVolumeError):
            train2d.conv2d_any(m.cuda(), x)
