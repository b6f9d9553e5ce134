"""dv_conv3d_wgrad_f32 (csrc/conv3d_wgrad.hip) against float64 for every layer kind of ACVNet_DDIM's aggregation stack.

Bar, per element: |dW_hip - dW_f64| <= c * 2^-24 * sum |g * x| over that element's sum.  The kernel adds each element's
products in one fp32 fma chain per K split (the split's bricks, TZ*TY*TX positions each, padding positions included as
exact zeros) and then the S split partials one after the other, so every product passes through at most
c = ceil(bricks / S) * positions_per_brick + S roundings: the standard recursive-summation bound gamma_c."""
import math

import pytest
import torch

from diffuvolume_amd import _lib
from diffuvolume_amd.train3d import conv3d_weight_grad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (k, stride) -> output brick of the kernel (TZ, TY, TX)
BRICK = {(3, 1): (2, 4, 16), (3, 2): (2, 2, 8), (1, 1): (2, 4, 16)}


def depth_c(b, cin, dims, cout, k, s):
    pad = (k - 1) // 2
    out = [(n + 2 * pad - k) // s + 1 for n in dims]
    brick = BRICK[(k, s)]
    nbricks = b * math.prod(-(-o // t) for o, t in zip(out, brick))
    splits = _lib.load().dv_conv3d_wgrad_workspace_floats(b, cin, *dims, cout, k, s) // (cout * cin * k ** 3)
    return -(-nbricks // splits) * math.prod(brick) + splits


def ref_wgrad(x, g, k, s):
    pad = (k - 1) // 2
    return torch.nn.grad.conv3d_weight(x, (g.shape[1], x.shape[1], k, k, k), g, stride=s, padding=pad)


def check(x, g, k, s, cout):
    dw = conv3d_weight_grad(x.cuda(), g.cuda(), k, s, cout).cpu().double()
    x64, g64 = x.double(), g.double()
    ref = ref_wgrad(x64, g64, k, s)
    mag = ref_wgrad(x64.abs(), g64.abs(), k, s)
    c = depth_c(x.shape[0], x.shape[1], x.shape[2:], cout, k, s)
    err = (dw - ref).abs()
    assert torch.all(err <= c * U * mag), (float((err / (mag * U)).max()), c)
    return dw


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


CONV = [  # (cin, cout, k, stride, batch, dims)
    (64, 32, 3, 1, 1, (12, 8, 20)), (40, 32, 3, 1, 3, (5, 7, 18)), (32, 32, 3, 1, 3, (6, 9, 33)),
    (64, 64, 3, 1, 1, (6, 5, 21)), (128, 128, 3, 1, 3, (3, 4, 10)),
    (32, 64, 3, 2, 3, (6, 8, 20)), (64, 128, 3, 2, 1, (7, 9, 19)),
    (32, 32, 1, 1, 3, (6, 8, 20)), (64, 64, 1, 1, 1, (5, 7, 11)),
    (32, 1, 3, 1, 3, (6, 8, 20)),
]


@pytest.mark.parametrize("cin,cout,k,s,b,dims", CONV)
def test_conv_weight_gradient(cin, cout, k, s, b, dims):
    pad = (k - 1) // 2
    x = rand(b, cin, *dims, seed=cin * 7 + cout)
    out = [(n + 2 * pad - k) // s + 1 for n in dims]
    g = rand(b, cout, *out, seed=cin + cout * 13 + s)
    check(x, g, k, s, cout)


@pytest.mark.parametrize("cin_t,cout_t,b,dims", [(128, 64, 3, (3, 4, 5)), (64, 32, 1, (6, 4, 10))])
def test_transposed_conv_weight_gradient(cin_t, cout_t, b, dims):
    """ConvTranspose3d(k3, s2, p1, op1): the stride-2 weight gradient with x and g exchanged."""
    x = rand(b, cin_t, *dims, seed=cin_t)
    gy = rand(b, cout_t, *[2 * n for n in dims], seed=cout_t + 1)
    w = torch.zeros(cin_t, cout_t, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv_transpose3d(x.double(), w, stride=2, padding=1, output_padding=1).backward(gy.double())
    dw = check(gy, x, 3, 2, cin_t)                 # the conv form is checked at its own bar ...
    torch.testing.assert_close(dw, w.grad, rtol=0, atol=float(1e-4 * w.grad.abs().max()))   # ... and is the deconv's


def test_two_launches_same_bits():
    x, g = rand(3, 32, 6, 8, 20, seed=1).cuda(), rand(3, 32, 6, 8, 20, seed=2).cuda()
    assert torch.equal(conv3d_weight_grad(x, g, 3, 1, 32), conv3d_weight_grad(x, g, 3, 1, 32))
    x2, g2 = rand(2, 32, 8, 8, 20, seed=3).cuda(), rand(2, 64, 4, 4, 10, seed=4).cuda()
    assert torch.equal(conv3d_weight_grad(x2, g2, 3, 2, 64), conv3d_weight_grad(x2, g2, 3, 2, 64))


def test_nan_stays_in_its_input_channel():
    x, g = rand(2, 40, 5, 8, 20, seed=5), rand(2, 32, 5, 8, 20, seed=6)
    x[1, 17, 3, 2, 7] = float("nan")
    dw = conv3d_weight_grad(x.cuda(), g.cuda(), 3, 1, 32).cpu()
    nan = torch.isnan(dw)
    assert nan[:, 17].any() and not nan[:, :17].any() and not nan[:, 18:].any()
