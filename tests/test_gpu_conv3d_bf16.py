"""dv_conv3d_k3s1_bf16_f32 (csrc/conv3d_bf16.hip, the bf16 instantiation of csrc/conv3d_mp.h): the forward and the input
gradient of the 3x3x3 stride-1 convolutions at train precision "bf16".  tests/test_gpu_conv3d_f16.py restated with
``rb16 = t.bfloat16().float()``; its shape list is used as it is.

Exact contract: y = conv(rb16(x), rb16(w)) with exact products, fp32 accumulation and an unrounded float32 y, so the
reference is the CPU float64 ``F.conv3d`` of ``x.bfloat16().double()`` and ``w.bfloat16().double()`` and the only difference
is the fp32 accumulation.  Bar, per element, the derived one of the fp16 test unchanged (the kernel body, its K chunking
and its summation order are the same; only the element type of the operands differs, and the reference rounds them the
same way):
    |y - ref| <= c * 2^-24 * conv(|rb16 x|, |rb16 w|),    c = 32 * 7 * ceil(Cin / 8)   (+ 1 with a bias).
(Measured: the worst ratio is 0.6 .. 2.1 against c = 224 .. 3584 on the shapes here, the relative L2 error 3.6e-8 .. 2.6e-7.)

Operands below 2^-126 (bf16 subnormals) may be flushed to zero: no test here asserts either behaviour."""
import pytest
import torch
import torch.nn.functional as F

import arena as A
from diffuvolume_amd import _lib, train3d
from test_gpu_conv3d_f16 import SHAPES, U, depth_c, rand

pytestmark = pytest.mark.gpu


def rb16(t):
    return t.bfloat16().float()


def reference(x, w, bias=None):
    """(float64 convolution of the rounded operands, the same of their magnitudes)."""
    x64, w64 = rb16(x).double(), rb16(w).double()
    ref = F.conv3d(x64, w64, None if bias is None else bias.double(), padding=1)
    mag = F.conv3d(x64.abs(), w64.abs(), None if bias is None else bias.double().abs(), padding=1)
    return ref, mag


def check(x, w, bias=None, flip=False, what="fwd"):
    """``flip``: ``w`` is the layer's weight [Cin,Cout,3,3,3] and ``x`` its output gradient (the input-gradient view)."""
    y = train3d.conv3d_k3s1_bf16(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), transpose_flip=flip)
    assert y.dtype == torch.float32
    y = y.cpu().double()
    ref, mag = reference(x, w.flip(2, 3, 4).transpose(0, 1) if flip else w, bias)
    assert y.shape == ref.shape
    c = depth_c(x.shape[1], bias is not None)
    err = (y - ref).abs()
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((y - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"CONV3DBF16 {what} {tuple(x.shape)} -> {ref.shape[1]}: worst {worst:.2f} of c = {c}, relative L2 {rel:.2e}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return y


def test_the_shape_list_holds_every_tile_edge():
    """W 47, 48 and 49; H 4 and 5; D 2 and 3; Cout 31 and 33; Cin 5 and 9 (65 is in the weight-gradient list)."""
    ws, hs, ds = {s[5] for s in SHAPES}, {s[4] for s in SHAPES}, {s[3] for s in SHAPES}
    assert {47, 48, 49} <= ws and {4, 5} <= hs and {2, 3} <= ds
    assert {31, 33} <= {s[2] for s in SHAPES} and {5, 9} <= {s[1] for s in SHAPES}


@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_forward(b, cin, cout, d, h, w):
    check(rand(b, cin, d, h, w, seed=cin + w), rand(cout, cin, 3, 3, 3, seed=cout + d, scale=0.1))


@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_input_gradient(b, cin, cout, d, h, w):
    """The same entry on g with transpose_flip: here g has ``cin`` channels and the layer's weight is [cin, cout, 3,3,3]."""
    check(rand(b, cin, d, h, w, seed=cin + 2 * w), rand(cin, cout, 3, 3, 3, seed=cout + h, scale=0.1), flip=True, what="dgrad")


def test_bias():
    check(rand(2, 12, 3, 5, 19, seed=1), rand(10, 12, 3, 3, 3, seed=2, scale=0.1), bias=rand(10, seed=3))


def test_reruns_and_batch_shards_give_the_same_bits():
    x, w = rand(3, 40, 3, 5, 50, seed=4).cuda(), rand(32, 40, 3, 3, 3, seed=5, scale=0.1).cuda()
    y = train3d.conv3d_k3s1_bf16(x, w)
    assert torch.equal(y, train3d.conv3d_k3s1_bf16(x, w))
    for i in range(3):
        assert torch.equal(y[i:i + 1], train3d.conv3d_k3s1_bf16(x[i:i + 1], w))
    g = train3d.conv3d_k3s1_bf16(y, w, transpose_flip=True)
    assert torch.equal(g, train3d.conv3d_k3s1_bf16(y, w, transpose_flip=True))
    assert torch.equal(g[1:2], train3d.conv3d_k3s1_bf16(y[1:2], w, transpose_flip=True))
    assert not torch.equal(y, train3d.conv3d_k3s1_f16(x, w))       # another rounding than the fp16 entry's


def test_operands_beyond_the_fp16_range_stay_finite_at_bf16():
    """The point of the precision: x scaled so that entries pass 7e4.  Through the fp16 entry they are Inf and reach the
    output; through the bf16 entry every output is finite and within the bar."""
    x, w = rand(2, 12, 4, 6, 52, seed=6, scale=3e4), rand(9, 12, 3, 3, 3, seed=7, scale=0.1)
    assert int((x.abs() > 7e4).sum()) > 10
    y16 = train3d.conv3d_k3s1_f16(x.cuda(), w.cuda())
    assert not torch.isfinite(y16).all()
    y = check(x, w, what="beyond fp16")
    assert torch.isfinite(y).all()
    g = check(x, rand(12, 9, 3, 3, 3, seed=8, scale=0.1), flip=True, what="beyond fp16, dgrad")
    assert torch.isfinite(g).all()


def test_a_float32_that_rounds_to_inf_reaches_exactly_its_window():
    """One x at 3.4e38 rounds to Inf (3.39e38 would stay finite): the outputs the emulation makes non-finite are
    non-finite, all others within the bar."""
    x, w = rand(2, 12, 4, 6, 52, seed=6), rand(9, 12, 3, 3, 3, seed=7, scale=0.1)
    x[1, 5, 2, 3, 47] = 3.4e38
    assert torch.isinf(rb16(x)[1, 5, 2, 3, 47]) and torch.isfinite(rb16(torch.tensor(3.39e38)))
    y = train3d.conv3d_k3s1_bf16(x.cuda(), w.cuda()).cpu().double()
    ref, mag = reference(x, w)
    bad = ~torch.isfinite(ref)
    assert int(bad.sum()) == 9 * 27                                # its 3x3x3 window in every output channel
    assert torch.equal(~torch.isfinite(y), bad)
    ok = ~bad
    assert torch.all((y - ref).abs()[ok] <= depth_c(12) * U * mag[ok])


def test_nan_stays_nan():
    x, w = rand(1, 8, 2, 4, 20, seed=15), rand(4, 8, 3, 3, 3, seed=16, scale=0.1)
    x[0, 3, 1, 2, 9] = float("nan")
    y = train3d.conv3d_k3s1_bf16(x.cuda(), w.cuda()).cpu()
    bad = torch.isnan(F.conv3d(x.double(), w.double(), padding=1))
    assert int(bad.sum()) == 4 * 2 * 3 * 3 and torch.equal(torch.isnan(y), bad)


def test_refusals_launch_nothing():
    lib = _lib.load()
    x, w = rand(1, 8, 2, 3, 8, seed=10).cuda(), rand(4, 8, 3, 3, 3, seed=11).cuda()
    out = A.place(torch.empty(1, 4, 2, 3, 8), kind="out", device="cuda", name="out")
    s = _lib.stream_ptr()
    call = lambda cout, k, xp=x.data_ptr(): lib.dv_conv3d_k3s1_bf16_f32(xp, w.data_ptr(), None, out.data_ptr(), 1, 8, 2, 3,
                                                                      8, cout, k, 0, s)
    assert call(1, 3) == -3                                        # Cout == 1: DV_ERR_UNSUPPORTED
    assert call(4, 1) == -3 and call(4, 5) == -3                   # k != 3
    assert call(4, 3, None) == -1                                  # null input
    assert call(0, 3) == -2
    torch.cuda.synchronize()
    A.check_untouched(out)
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.conv3d_k3s1_bf16(x, rand(4, 9, 3, 3, 3, seed=1).cuda())


def test_a_single_input_channel_layer_trains_at_bf16():
    """Cin == 1, Cout > 1: the forward and the weight gradient run on the bf16 kernels, the one-channel input gradient
    (which the bf16 entry refuses, as it does the 32 -> 1 heads) on the float32 kernel -- backward must not raise."""
    x = rand(2, 1, 3, 5, 20, seed=12).cuda().requires_grad_(True)
    w = rand(6, 1, 3, 3, 3, seed=13, scale=0.3).cuda().requires_grad_(True)
    g = rand(2, 6, 3, 5, 20, seed=14).cuda()
    y = train3d.conv3d(x, w, None, 1, precision="bf16")
    y.backward(g)
    ref, mag = reference(x.detach().cpu(), w.detach().cpu())
    assert torch.all((y.detach().cpu().double() - ref).abs() <= depth_c(1) * U * mag)
    dx = F.conv3d(g.cpu().double(), w.detach().cpu().double().flip(2, 3, 4).transpose(0, 1), padding=1)   # unrounded operands
    assert x.grad.shape == x.shape and float((x.grad.cpu().double() - dx).norm() / dx.norm()) < 1e-5
    assert torch.equal(w.grad, train3d.conv3d_weight_grad_bf16(x.detach(), g))


def test_autograd_uses_the_precision_the_forward_saved():
    """A "bf16" forward followed by a backward outside any scope: all three products are the bf16 entries'."""
    x = rand(1, 9, 3, 5, 20, seed=17).cuda().requires_grad_(True)
    w = rand(6, 9, 3, 3, 3, seed=18, scale=0.1).cuda().requires_grad_(True)
    g = rand(1, 6, 3, 5, 20, seed=19).cuda()
    with train3d.precision_scope("bf16"):
        y = train3d.conv3d(x, w, None, 1)
    with train3d.precision_scope("f16"):
        y.backward(g)
    assert torch.equal(y.detach(), train3d.conv3d_k3s1_bf16(x.detach(), w.detach()))
    assert torch.equal(x.grad, train3d.conv3d_k3s1_bf16(g, w.detach(), transpose_flip=True))
    assert torch.equal(w.grad, train3d.conv3d_weight_grad_bf16(x.detach(), g))
