"""dv_conv3d_k3s1_f16_f32 (csrc/conv3d_f16.hip): the forward and the input gradient of the 3x3x3 stride-1 convolutions at
train precision "f16".

Exact contract: y = conv(r16(x), r16(w)) with exact products, fp32 accumulation and an unrounded float32 y, so the
reference is the CPU float64 ``F.conv3d`` of ``x.half().double()`` and ``w.half().double()`` and the only difference is the
fp32 accumulation.  Bar, per element:  |y - ref| <= c * 2^-24 * conv(|r16 x|, |r16 w|).

c from the kernel's K chunking: an output is the sum over ceil(Cin / 8) chunks of 8 input channels, each chunk 7 matrix
instructions (K-blocks of 4 tap slots x 8 channels = 32 products; 28 slots = 27 taps + 1 with zero weights), each
instruction adding its 32 products to the running fp32 accumulator.  The order inside an instruction is not documented,
so it is taken at its worst -- the accumulator first, then the 32 products one by one, a rounding each: a product passes
through at most 32 roundings per instruction it has been part of the accumulator for,
    c = 32 * 7 * ceil(Cin / 8)      (+ 1 for the rounding of the bias addition where there is a bias).
(Measured: the worst ratio is 0.5 .. 3.0 against c = 224 .. 3584 on the shapes here, the relative L2 error 5e-8 .. 2.7e-7.)"""
import pytest
import torch
import torch.nn.functional as F

import arena as A
from diffuvolume_amd import _lib, train3d

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TD, TH, TW, TN, KC = 2, 4, 48, 32, 8          # the kernel's tile: output brick, cout per block, channels per chunk


def r16(t):
    return t.half().float()


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def depth_c(cin, bias=False):
    return 32 * 7 * -(-cin // KC) + (1 if bias else 0)


def reference(x, w, bias=None):
    """(float64 convolution of the rounded operands, the same of their magnitudes)."""
    x64, w64 = r16(x).double(), r16(w).double()
    ref = F.conv3d(x64, w64, None if bias is None else bias.double(), padding=1)
    mag = F.conv3d(x64.abs(), w64.abs(), None if bias is None else bias.double().abs(), padding=1)
    return ref, mag


def check(x, w, bias=None, flip=False, what="fwd"):
    """``flip``: ``w`` is the layer's weight [Cin,Cout,3,3,3] and ``x`` its output gradient (the input-gradient view)."""
    y = train3d.conv3d_k3s1_f16(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), transpose_flip=flip)
    assert y.dtype == torch.float32
    y = y.cpu().double()
    ref, mag = reference(x, w.flip(2, 3, 4).transpose(0, 1) if flip else w, bias)
    assert y.shape == ref.shape
    c = depth_c(x.shape[1], bias is not None)
    err = (y - ref).abs()
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((y - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"CONV3D16 {what} {tuple(x.shape)} -> {ref.shape[1]}: worst {worst:.2f} of c = {c}, relative L2 {rel:.2e}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return y


SHAPES = [  # (B, Cin, Cout, D, H, W)
    (2, 40, 32, 3, 5, 50),        # ACV's 40 -> 32, tails on every axis
    (1, 32, 32, 2, 4, 48),
    (1, 64, 32, 1, 1, 1),
    (1, 5, 7, 2, 3, 17),
    (1, 32, 33, 2, 2, 16),
    (2, 64, 64, 4, 6, 20),
    (1, 128, 128, 2, 3, 8),
    # both sides of every edge of the tile: W 48, H 4, D 2, 32 cout per block, 8 channels per chunk
    (1, 8, 16, 2, 4, 47),
    (1, 9, 16, 3, 5, 49),
    (1, 7, 2, 1, 3, 48),
    (1, 16, 31, 2, 4, 4),
]


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
    y = train3d.conv3d_k3s1_f16(x, w)
    assert torch.equal(y, train3d.conv3d_k3s1_f16(x, w))
    for i in range(3):
        assert torch.equal(y[i:i + 1], train3d.conv3d_k3s1_f16(x[i:i + 1], w))
    g = train3d.conv3d_k3s1_f16(y, w, transpose_flip=True)
    assert torch.equal(g, train3d.conv3d_k3s1_f16(y, w, transpose_flip=True))
    assert torch.equal(g[1:2], train3d.conv3d_k3s1_f16(y[1:2], w, transpose_flip=True))


def test_an_operand_beyond_the_fp16_range_reaches_exactly_its_window():
    """One x at 7e4 rounds to Inf: the outputs the emulation makes non-finite are non-finite, all others within the bar."""
    x, w = rand(2, 12, 4, 6, 52, seed=6), rand(9, 12, 3, 3, 3, seed=7, scale=0.1)
    x[1, 5, 2, 3, 47] = 7e4
    y = train3d.conv3d_k3s1_f16(x.cuda(), w.cuda()).cpu().double()
    ref, mag = reference(x, w)
    bad = ~torch.isfinite(ref)
    assert int(bad.sum()) == 9 * 27                                # its 3x3x3 window in every output channel
    assert torch.equal(~torch.isfinite(y), bad)
    ok = ~bad
    assert torch.all((y - ref).abs()[ok] <= depth_c(12) * U * mag[ok])


def test_subnormal_operands_are_kept():
    """x spread over 2^-26 .. 2^-12: most of r16(x) is subnormal (below 2^-14).  A kernel that flushed them would miss
    the bar by orders of magnitude (the bar is relative to the sum of the rounded operands' products)."""
    gen = torch.Generator().manual_seed(8)
    x = torch.exp2(torch.rand(1, 16, 2, 4, 40, generator=gen) * 14 - 26) * torch.where(torch.rand(1, 16, 2, 4, 40, generator=gen) < 0.5, -1.0, 1.0)
    w = rand(8, 16, 3, 3, 3, seed=9)
    x16 = r16(x)
    sub = (x16 != 0) & (x16.abs() < 2.0 ** -14)
    assert float(sub.float().mean()) > 0.5
    y = check(x, w, what="subnormal")
    only_sub = F.conv3d(torch.where(sub, x16, torch.zeros(())).double(), r16(w).double(), padding=1)
    assert float(only_sub.abs().max()) > 0 and float(y.abs().max()) > 0


def test_refusals_launch_nothing():
    lib = _lib.load()
    x, w = rand(1, 8, 2, 3, 8, seed=10).cuda(), rand(4, 8, 3, 3, 3, seed=11).cuda()
    out = A.place(torch.empty(1, 4, 2, 3, 8), kind="out", device="cuda", name="out")
    s = _lib.stream_ptr()
    call = lambda cout, k, xp=x.data_ptr(): lib.dv_conv3d_k3s1_f16_f32(xp, w.data_ptr(), None, out.data_ptr(), 1, 8, 2, 3, 8,
                                                                     cout, k, 0, s)
    assert call(1, 3) == -3                                        # Cout == 1: DV_ERR_UNSUPPORTED
    assert call(4, 1) == -3 and call(4, 5) == -3                   # k != 3
    assert call(4, 3, None) == -1                                  # null input
    assert call(0, 3) == -2
    torch.cuda.synchronize()
    A.check_untouched(out)
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.conv3d_k3s1_f16(x, rand(4, 9, 3, 3, 3, seed=1).cuda())


def test_a_single_input_channel_layer_trains_at_f16():
    """Cin == 1, Cout > 1: the forward and the weight gradient run on the fp16 kernels, the one-channel input gradient
    (which the fp16 entry refuses, as it does the 32 -> 1 heads) on the float32 kernel -- backward must not raise."""
    x = rand(2, 1, 3, 5, 20, seed=12).cuda().requires_grad_(True)
    w = rand(6, 1, 3, 3, 3, seed=13, scale=0.3).cuda().requires_grad_(True)
    g = rand(2, 6, 3, 5, 20, seed=14).cuda()
    y = train3d.conv3d(x, w, None, 1, precision="f16")
    y.backward(g)
    ref, mag = reference(x.detach().cpu(), w.detach().cpu())
    assert torch.all((y.detach().cpu().double() - ref).abs() <= depth_c(1) * U * mag)
    dx = F.conv3d(g.cpu().double(), w.detach().cpu().double().flip(2, 3, 4).transpose(0, 1), padding=1)   # unrounded operands
    assert x.grad.shape == x.shape and float((x.grad.cpu().double() - dx).norm() / dx.norm()) < 1e-5
    assert torch.equal(w.grad, train3d.conv3d_weight_grad_f16(x.detach(), g))
