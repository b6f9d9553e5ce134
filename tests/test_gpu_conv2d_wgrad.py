"""dv_conv2d_wgrad_f32 (csrc/conv2d_wgrad.hip) against float64 for every layer shape of PWCNet_ddim's refinement network
refinenet3 (at reduced image size) and for edge shapes.

Bar, per element: |dW_hip - dW_f64| <= c * 2^-24 * sum |g * x| over that element's sum.  The kernel adds each element's
products in one fp32 fma chain per K split (the split's bricks, TY*TX positions each, padding positions included as
exact zeros) and then the S split partials one after the other, so every product passes through at most
c = ceil(bricks / S) * positions_per_brick + S roundings: the standard recursive-summation bound gamma_c."""
import pytest
import torch

from diffuvolume_amd import _lib
from diffuvolume_amd.train2d import conv2d_weight_grad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def brick(k, d):
    """The kernel's output brick (TY, TX) for this layer kind."""
    return (2, 32) if (k == 3 and d > 4) else (4, 32)


def depth_c(b, cin, h, w, cout, k, d):
    ty, tx = brick(k, d)
    nbricks = b * -(-h // ty) * -(-w // tx)
    splits = _lib.load().dv_conv2d_wgrad_workspace_floats(b, cin, h, w, cout, k, d) // (cout * cin * k * k)
    return -(-nbricks // splits) * ty * tx + splits


def ref_wgrad(x, g, k, d):
    return torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], k, k), g, padding=d if k == 3 else 0,
                                       dilation=d if k == 3 else 1)


def check(x, g, k, d, cout):
    dw = conv2d_weight_grad(x.cuda(), g.cuda(), k, d, cout).cpu().double()
    x64, g64 = x.double(), g.double()
    ref = ref_wgrad(x64, g64, k, d)
    mag = ref_wgrad(x64.abs(), g64.abs(), k, d)
    c = depth_c(*x.shape[:1], x.shape[1], *x.shape[2:], cout, k, d)
    err = (dw - ref).abs()
    assert torch.all(err <= c * U * mag), (float((err / (mag * U)).max()), c)
    return dw


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


LAYERS = [  # (cin, cout, k, dilation, batch, h, w): refinenet3's layers at 48 x 96, then edge shapes
    (146, 128, 3, 1, 2, 48, 96), (128, 128, 3, 1, 2, 48, 96), (128, 128, 3, 2, 2, 48, 96), (128, 128, 3, 4, 2, 48, 96),
    (128, 96, 3, 8, 2, 48, 96), (96, 96, 3, 8, 2, 48, 96), (128, 96, 1, 1, 2, 48, 96),
    (96, 64, 3, 16, 2, 48, 96), (64, 64, 3, 16, 2, 48, 96), (96, 64, 1, 1, 2, 48, 96),
    (64, 32, 3, 1, 2, 48, 96), (32, 32, 3, 1, 2, 48, 96), (64, 32, 1, 1, 2, 48, 96), (32, 1, 3, 1, 2, 48, 96),
    # edges: Cin 1, Cout 1, odd H and W, B = 1 and 3, k = 1, dilation larger than H/2, odd channel counts
    (1, 32, 3, 1, 3, 17, 41), (32, 1, 3, 2, 1, 19, 37), (5, 7, 1, 1, 3, 13, 35), (146, 146, 3, 1, 1, 9, 45),
    (33, 17, 3, 16, 3, 21, 50), (16, 16, 3, 12, 1, 11, 70), (3, 5, 3, 5, 1, 7, 9),
]


@pytest.mark.parametrize("cin,cout,k,d,b,h,w", LAYERS)
def test_weight_gradient(cin, cout, k, d, b, h, w):
    x = rand(b, cin, h, w, seed=cin * 7 + cout + d)
    g = rand(b, cout, h, w, seed=cin + cout * 13 + d)
    check(x, g, k, d, cout)


def test_two_launches_same_bits_and_workspace_reuse():
    x, g = rand(2, 128, 40, 72, seed=1).cuda(), rand(2, 96, 40, 72, seed=2).cuda()
    a = conv2d_weight_grad(x, g, 3, 8, 96)
    assert torch.equal(a, conv2d_weight_grad(x, g, 3, 8, 96))
    lib = _lib.load()
    n = lib.dv_conv2d_wgrad_workspace_floats(2, 128, 40, 72, 96, 3, 8)
    ws = torch.full((n,), float("nan"), device="cuda")                # stale contents must not leak into the result
    out = []
    for _ in range(2):
        dw = torch.empty(96, 128, 3, 3, device="cuda")
        _lib.check(lib.dv_conv2d_wgrad_f32(x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), 2, 128, 40, 72,
                                           96, 3, 8, _lib.stream_ptr()), "dv_conv2d_wgrad_f32")
        out.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(out[0], a) and torch.equal(out[1], a)


def test_nan_stays_in_its_input_channel():
    x, g = rand(2, 40, 12, 40, seed=5), rand(2, 32, 12, 40, seed=6)
    x[1, 17, 3, 7] = float("nan")
    dw = conv2d_weight_grad(x.cuda(), g.cuda(), 3, 2, 32).cpu()
    nan = torch.isnan(dw)
    assert nan[:, 17].any() and not nan[:, :17].any() and not nan[:, 18:].any()
