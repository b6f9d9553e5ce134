"""The differentiable HIP 3-D convolutions of train3d.py against float64 CPU autograd.

Weight gradients: the per-element bar of tests/test_gpu_conv3d_wgrad.py.  Input gradients run on the forward kernels
(Winograd / polyphase / transposed): |dx_hip - dx_f64| <= C_DX * 2^-24 * sum |g * w| per element, C_DX = 4 * (terms of
the sum) -- the minimal-filtering transforms add and subtract neighbouring taps before the products, which a handful of
extra roundings per term covers.  The routes are checked by counting calls into the library's entry points."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib, train3d
from test_gpu_conv3d_wgrad import U, depth_c, rand

pytestmark = pytest.mark.gpu


@pytest.fixture
def calls(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    lib = _lib.load()
    counts = {}
    for name in ("dv_conv3d_wino_f32", "dv_conv3d_wino3_f32", "dv_conv3d_s2pp_f32", "dv_conv3d_f32",
                 "dv_deconv3d_k3s2_f32", "dv_conv3d_wgrad_f32"):
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


@pytest.mark.parametrize("cin,cout,k,s,b,dims", [(40, 32, 3, 1, 2, (6, 8, 20)), (64, 64, 3, 1, 1, (6, 8, 20)),
                                                 (32, 64, 3, 2, 2, (6, 8, 20)), (64, 128, 3, 2, 1, (6, 8, 20)),
                                                 (32, 32, 1, 1, 2, (6, 8, 20)), (32, 1, 3, 1, 2, (6, 8, 20))])
def test_conv3d_function(calls, cin, cout, k, s, b, dims):
    x, w = rand(b, cin, *dims, seed=cin + k), rand(cout, cin, k, k, k, seed=cout + s) * 0.1
    hip, ref, mag = run_both(lambda x, w, _: train3d.conv3d(x, w, None, s),
                             lambda x, w, _: F.conv3d(x, w, None, stride=s, padding=(k - 1) // 2), x, w)
    assert_bars(hip, ref, mag, 4 * cout * k ** 3, depth_c(b, cin, dims, cout, k, s))
    assert calls.get("dv_conv3d_wgrad_f32") == 1
    if k == 3 and s == 1:
        assert calls.get("dv_conv3d_wino_f32", 0) + calls.get("dv_conv3d_wino3_f32", 0) >= 1 + (cout > 1)
    if s == 2:
        assert calls.get("dv_deconv3d_k3s2_f32") == 1                  # the input gradient
        assert calls.get("dv_conv3d_s2pp_f32", 0) + calls.get("dv_conv3d_f32", 0) >= 1


def test_conv3d_1x1_with_bias(calls):
    x, w, bias = rand(2, 128, 3, 4, 10, seed=1), rand(128, 128, 1, 1, 1, seed=2) * 0.1, rand(128, seed=3)
    hip, ref, mag = run_both(train3d.conv3d, lambda x, w, b: F.conv3d(x, w, b), x, w, bias)
    assert_bars(hip, ref, mag, 4 * 128, depth_c(2, 128, (3, 4, 10), 128, 1, 1))
    torch.testing.assert_close(hip[3], ref[3], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("cin_t,cout_t,b,dims", [(128, 64, 2, (3, 4, 10)), (64, 32, 1, (6, 8, 20))])
def test_conv_transpose3d_function(calls, cin_t, cout_t, b, dims):
    x, w = rand(b, cin_t, *dims, seed=cin_t), rand(cin_t, cout_t, 3, 3, 3, seed=cout_t) * 0.1
    hip, ref, mag = run_both(lambda x, w, _: train3d.conv_transpose3d(x, w),
                             lambda x, w, _: F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1), x, w)
    assert_bars(hip, ref, mag, 4 * cout_t * 27, depth_c(b, cout_t, [2 * n for n in dims], cin_t, 3, 2))
    assert calls.get("dv_deconv3d_k3s2_f32") == 1 and calls.get("dv_conv3d_wgrad_f32") == 1
    assert calls.get("dv_conv3d_s2pp_f32", 0) + calls.get("dv_conv3d_f32", 0) == 1       # the input gradient


def test_functions_give_the_same_bits_twice(calls):
    x, w = rand(2, 32, 6, 8, 20, seed=9).cuda(), (rand(64, 32, 3, 3, 3, seed=10) * 0.1).cuda()
    gy = rand(2, 64, 3, 4, 10, seed=11).cuda()
    res = []
    for _ in range(2):
        xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = train3d.conv3d(xs, ws, None, 2)
        y.backward(gy)
        res.append((y, xs.grad, ws.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
