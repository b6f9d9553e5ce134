"""The differentiable HIP 2-D convolution of train2d.py against float64 CPU autograd, for every dilation of refinenet3
(1, 2, 4, 8, 16), for its 1x1 down-sampling layers and for the two shapes whose input gradient needs care: Cout = 146
(conv1's input gradient has 146 output channels) and Cout = 1 (conv8's output gradient has a single channel).

Weight gradients: the per-element bar of tests/test_gpu_conv2d_wgrad.py.  Input gradients run on the forward kernels
(Winograd / direct): |dx_hip - dx_f64| <= C_DX * 2^-24 * sum |g * w| per element, C_DX = 4 * (terms of the sum), as for
the 3-D functions.  The routes are checked by counting calls into the library's entry points."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib, train2d
from test_gpu_conv2d_wgrad import U, depth_c, rand

pytestmark = pytest.mark.gpu
FORWARD = ("dv_conv2d_f32", "dv_conv2d_gated_f32", "dv_conv2d_cat_f32", "dv_conv2d_cat_ksplit_f32", "dv_conv2d_wino_dil_cat_f32",
           "dv_conv2d_wino_cat_ksplit_f32", "dv_conv2d_1in_f32")


@pytest.fixture
def calls(monkeypatch):
    lib = _lib.load()
    counts = {}
    for name in FORWARD + ("dv_conv2d_wgrad_f32",):
        real = getattr(lib, name)

        def counting(*args, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(lib, name, counting)
    return counts


def run_both(fn_hip, fn_ref, x, w, bias=None):
    """-> (hip grads, f64 grads, f64 grads of |.| for the bars), for a fixed random output gradient."""
    gy = None
    outs = []
    for dev, dtype, fn, absval in (("cuda", torch.float32, fn_hip, False), ("cpu", torch.float64, fn_ref, False),
                                   ("cpu", torch.float64, fn_ref, True)):
        xs = (x.abs() if absval else x).to(dev, dtype).requires_grad_()
        ws = (w.abs() if absval else w).to(dev, dtype).requires_grad_()
        bs = None if bias is None else bias.to(dev, dtype).requires_grad_()
        y = fn(xs, ws, bs)
        if gy is None:
            gy = rand(*y.shape, seed=77)
        y.backward((gy.abs() if absval else gy).to(dev, dtype))
        outs.append((y.detach().cpu().double(), xs.grad.cpu().double(), ws.grad.cpu().double(),
                     None if bs is None else bs.grad.cpu().double()))
    return outs


def assert_bars(hip, ref, mag, c_dx, c_dw):
    assert torch.all((hip[1] - ref[1]).abs() <= c_dx * U * mag[1] + 1e-30), "input gradient"
    assert torch.all((hip[2] - ref[2]).abs() <= c_dw * U * mag[2] + 1e-30), "weight gradient"


def ref_conv(d, k):
    return lambda x, w, b: F.conv2d(x, w, b, padding=d if k == 3 else 0, dilation=d if k == 3 else 1)


@pytest.mark.parametrize("cin,cout,k,d,b,h,w", [
    (146, 128, 3, 1, 2, 32, 64), (128, 128, 3, 2, 2, 32, 64), (128, 128, 3, 4, 1, 40, 72), (128, 96, 3, 8, 2, 40, 72),
    (96, 64, 3, 16, 2, 40, 72), (64, 32, 3, 1, 2, 33, 47), (32, 1, 3, 1, 2, 32, 64), (128, 96, 1, 1, 2, 32, 64),
    (64, 32, 1, 1, 1, 21, 35)])
def test_conv2d_function(monkeypatch, calls, cin, cout, k, d, b, h, w):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x, wt = rand(b, cin, h, w, seed=cin + k + d), rand(cout, cin, k, k, seed=cout + d) * 0.1
    hip, ref, mag = run_both(lambda x, w, _: train2d.conv2d(x, w, None, d), ref_conv(d, k), x, wt)
    assert hip[1].shape == ref[1].shape and hip[2].shape == ref[2].shape
    torch.testing.assert_close(hip[0], ref[0], rtol=0, atol=float(1e-5 * ref[0].abs().max()))
    assert_bars(hip, ref, mag, 4 * cout * k * k, depth_c(b, cin, h, w, cout, k, d))
    assert calls.get("dv_conv2d_wgrad_f32") == 1
    assert sum(calls.get(n, 0) for n in FORWARD) == 2                    # the forward and the input gradient
    if cout == 1:
        assert calls.get("dv_conv2d_1in_f32") == 1                       # conv8's single-channel output gradient


def test_conv2d_with_bias(monkeypatch, calls):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x, w, bias = rand(2, 64, 24, 40, seed=1), rand(32, 64, 3, 3, seed=2) * 0.1, rand(32, seed=3)
    hip, ref, mag = run_both(lambda x, w, b: train2d.conv2d(x, w, b, 2), lambda x, w, b: F.conv2d(x, w, b, padding=2,
                                                                                                 dilation=2), x, w, bias)
    assert_bars(hip, ref, mag, 4 * 32 * 9, depth_c(2, 64, 24, 40, 32, 3, 2))
    torch.testing.assert_close(hip[3], ref[3], rtol=1e-5, atol=1e-4)


def test_conv2d_module_routes(monkeypatch, calls):
    m = torch.nn.Conv2d(32, 16, 3, 1, 4, 4, bias=False).cuda()
    x = rand(1, 32, 24, 40, seed=4).cuda().requires_grad_()
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    train2d.conv2d_module(m, x).sum().backward()
    assert not calls                                                     # F.conv2d: neither entry point
    ref_dx, ref_dw = x.grad.clone(), m.weight.grad.clone()
    x.grad = m.weight.grad = None
    monkeypatch.setenv("DV_TRAIN_CONV2D", "hip")
    train2d.conv2d_module(m, x).sum().backward()
    assert calls.get("dv_conv2d_wgrad_f32") == 1 and sum(calls.get(n, 0) for n in FORWARD) == 2
    torch.testing.assert_close(x.grad, ref_dx, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(m.weight.grad, ref_dw, rtol=1e-4, atol=1e-3)
    with pytest.raises(_lib.DiffuVolumeError):
        train2d.conv2d_module(torch.nn.Conv2d(32, 16, 3, 2, 1).cuda(), x)        # stride 2: not this route


def test_functions_give_the_same_bits_twice(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x, w = rand(2, 96, 32, 64, seed=9).cuda(), (rand(64, 96, 3, 3, seed=10) * 0.1).cuda()
    gy = rand(2, 64, 32, 64, seed=11).cuda()
    res = []
    for _ in range(2):
        xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = train2d.conv2d(xs, ws, None, 16)
        y.backward(gy)
        res.append((y, xs.grad, ws.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
