"""The 16-bit training kernels held to their per-element bars AWAY from amplitude 1: fp16 subnormals, exact rounding
ties, the edge of the fp16 range, operands whose channels span three decades, and bf16's exponent range.

Entries: dv_conv3d_k3s1_{f16,bf16}_f32 forward and ``transpose_flip`` (csrc/conv3d_mp.h), dv_conv3d_wgrad_{f16,bf16}_f32
(csrc/conv3d_wgrad_mp.h: a half-wave loads a row, a quad permute fetches the neighbour, two halves are packed into a
dword -- not the forward's staging), dv_conv2d_wgrad_cat_f16 and dv_conv2d_f16_cat.

Reference and bars are the sibling tests', imported and unchanged: the float64 expression on ``t.half().double()`` /
``t.bfloat16().double()`` and, per element, c * 2^-24 * sum |operands| with c = depth_c(...) of the entry's own file
(224 .. 1120 for the forward here, 129 .. 152 for the weight gradient); ``emulate`` / ``check`` of
tests/test_gpu_conv2d_f16.py for the 2-D forward.  No constant is introduced here.  The operands come from
tests/magnitudes.py, and tests/test_amp_magnitudes_host.py shows on the CPU that a kernel which flushed the subnormals or
rounded the ties away from zero would miss these bars at more than 90 % of the output elements.

Shapes: the smallest of the sibling lists that cross each tile edge once."""
import pytest
import torch

import magnitudes as M
import test_gpu_conv2d_f16 as P16
import test_gpu_conv2d_wgrad_cat_f16 as WC16
import test_gpu_conv3d_bf16 as CB16
import test_gpu_conv3d_f16 as C16
import test_gpu_conv3d_wgrad_bf16 as WB16
import test_gpu_conv3d_wgrad_f16 as W16
from diffuvolume_amd import submodule as S
from diffuvolume_amd import train3d
from test_gpu_conv3d_f16 import U, rand

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 8, 2, 2, 32), (1, 5, 7, 2, 3, 17), (2, 40, 32, 3, 5, 50), (1, 9, 16, 3, 5, 49)]     # (B, Cin, Cout, D, H, W)
ELEMS = ["f16", "bf16"]
DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}
CONV = {"f16": C16, "bf16": CB16}                 # check(x, w, flip=, what=), reference(x, w)
WGRAD = {"f16": W16, "bf16": WB16}                # check(x, g), depth_c(...)
CAT2D = WC16.EDGES[:2]                            # ((8,), 8, 3, 1, 1, 1) and ((16, 8), 24, 3, 3, 2, 3)


def nonzero(t):
    assert float(t.abs().max()) > 0
    return t


# ------------------------------------------------------------------ 1. subnormal gradients (fp16)
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_subnormal_gradient(b, cin, cout, d, h, w):
    """What loss scaling is there for: g spread over 2^-26 .. 2^-12, 78 .. 81 % of r16(g) subnormal and not zero.  The weight
    gradient with a subnormal g, with a subnormal x, with both (products down to 2^-50, exact in fp32), and the input
    gradient with a subnormal g: each within the sibling bar, each non-zero.
    Measured (worst ratio against c): dW 1.0 .. 2.8 of c = 129 .. 152 over the three forms; dx 1.7 .. 2.6 of c = 224 .. 896."""
    g, gs = rand(b, cout, d, h, w, seed=1), M.subnormal16((b, cout, d, h, w), seed=2)
    x, xs = rand(b, cin, d, h, w, seed=3), M.subnormal16((b, cin, d, h, w), seed=4)
    assert float(M.is_subnormal16(gs).float().mean()) > 0.5 and float(M.is_subnormal16(xs).float().mean()) > 0.5
    nonzero(W16.check(x, gs))
    nonzero(W16.check(xs, g))
    nonzero(W16.check(xs, gs))
    # the input gradient: the entry's "x" is the layer's output gradient [B,Cout,...], its weight [Cout,Cin,3,3,3] read flipped
    nonzero(C16.check(gs, rand(cout, cin, 3, 3, 3, seed=5, scale=0.1), flip=True, what="dgrad, g subnormal"))


@pytest.mark.parametrize("chans,cout,k,b,h,w", CAT2D)
def test_subnormal_gradient_2d_weight_gradient(chans, cout, k, b, h, w):
    """dv_conv2d_wgrad_cat_f16 with a subnormal g, then with subnormal sources.  Measured: 1 x 1 exact; 2 x 3 worst 48 (g
    subnormal) and 56 (sources subnormal) of c = 385 -- 18 products four decades apart inside ONE matrix instruction, where
    its internal sum costs more than the one rounding per product of an fp32 chain; the largest figure in this file."""
    srcs = [rand(b, c, h, w, seed=6 + i) for i, c in enumerate(chans)]
    nonzero(WC16.check(srcs, M.subnormal16((b, cout, h, w), seed=9), k))
    subs = [M.subnormal16((b, c, h, w), seed=10 + i) for i, c in enumerate(chans)]
    nonzero(WC16.check(subs, rand(b, cout, h, w, seed=14), k))


# ------------------------------------------------------------------ 2. ties
def tie_pairs(tie_shape, other_shape, dtype, seed, other_scale=1.0):
    """(ties, ordinary) twice: signed -- both signs on both operands, where a wrong tie rule on one sign shows -- and
    sign-coherent (|ties|, |ordinary|), where the errors of a wrong rule add up instead of cancelling."""
    t, o = M.ties16(tie_shape, seed=seed, dtype=dtype), rand(*other_shape, seed=seed + 1, scale=other_scale)
    return [("signed", t, o), ("coherent", t.abs(), o.abs())]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_ties_forward_and_input_gradient(b, cin, cout, d, h, w, elem):
    """Every x, then every w, exactly between two neighbours of the 16-bit type: round to nearest even on the activation
    staging and on the weight staging, forward and ``transpose_flip``.
    Measured: worst 0.8 .. 11.9 of c = 224 .. 1120 at fp16 and 0.6 .. 13.0 at bf16; the signed cases stay near 1, the
    sign-coherent ones reach 12 (every product positive: a one-sided rounding inside the matrix instruction adds up)."""
    check, dt = CONV[elem].check, DTYPE[elem]
    xs, ws, wts = (b, cin, d, h, w), (cout, cin, 3, 3, 3), (cin, cout, 3, 3, 3)
    for mode, x, wt in tie_pairs(xs, ws, dt, 20, 0.1):
        check(x, wt, what=f"ties in x, {mode}")
    for mode, wt, x in tie_pairs(ws, xs, dt, 22):
        check(x, wt, what=f"ties in w, {mode}")
    for mode, g, wt in tie_pairs(xs, wts, dt, 24, 0.1):
        check(g, wt, flip=True, what=f"dgrad, ties in g, {mode}")
    for mode, wt, g in tie_pairs(wts, xs, dt, 26):
        check(g, wt, flip=True, what=f"dgrad, ties in w, {mode}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_ties_weight_gradient(b, cin, cout, d, h, w, elem):
    """The packed staging of the weight-gradient kernels: ties in x, then in g.
    Measured: worst 0.5 .. 5.3 of c = 129 .. 152 at fp16 and 0.5 .. 5.1 at bf16 (the larger figures are the coherent cases)."""
    check, dt = WGRAD[elem].check, DTYPE[elem]
    for mode, x, g in tie_pairs((b, cin, d, h, w), (b, cout, d, h, w), dt, 30):
        check(x, g)
    for mode, g, x in tie_pairs((b, cout, d, h, w), (b, cin, d, h, w), dt, 32):
        check(x, g)


@pytest.mark.parametrize("chans,cout,k,b,h,w", CAT2D)
def test_ties_2d_weight_gradient(chans, cout, k, b, h, w):
    """dv_conv2d_wgrad_cat_f16: ties in every source of the virtual concatenation (one source, then two), then in g.
    Measured: 1 x 1 exact; 2 x 3 worst 1.8 .. 2.6 of c = 385."""
    for mode, f in (("signed", lambda t: t), ("coherent", torch.abs)):
        ties = [f(M.ties16((b, c, h, w), seed=40 + i)) for i, c in enumerate(chans)]
        WC16.check(ties, f(rand(b, cout, h, w, seed=44)), k)
        srcs = [f(rand(b, c, h, w, seed=45 + i)) for i, c in enumerate(chans)]
        WC16.check(srcs, f(M.ties16((b, cout, h, w), seed=49)), k)


def test_ties_2d_forward_two_sources():
    """dv_conv2d_f16_cat through ``Conv2dF16Plan``: ties in both sources of a two-source call (channel counts that are no
    multiples of the 32-channel chunk), then in the weights; ``emulate`` / ``check`` of tests/test_gpu_conv2d_f16.py,
    outputs fp16-exact, at most 2 % of them off the emulation.  Measured: 0 .. 7.1e-4 of the outputs differ from the
    emulation, the closest to its bound 5e-6 inside it."""
    b, h, w, chans, cout = 2, 5, 35, (5, 27), 20
    cin = sum(chans)
    for mode, f in (("signed", lambda t: t), ("coherent", torch.abs)):
        parts = [f(M.ties16((b, c, h, w), seed=50 + i)) for i, c in enumerate(chans)]
        wt, bias = f(rand(cout, cin, 3, 3, seed=53, scale=(cin * 9) ** -0.5)), rand(cout, seed=54, scale=0.1)
        plan = S.Conv2dF16Plan(wt.to(P16.DEV), bias.to(P16.DEV), act=S.ACT_NONE)
        P16.check(plan([p.to(P16.DEV) for p in parts]), P16.emulate(parts, wt, bias, "none"))
        parts = [f(rand(b, c, h, w, seed=55 + i)) for i, c in enumerate(chans)]
        wt = f(M.ties16((cout, cin, 3, 3), seed=58)) * 2.0 ** -4          # a power of two: the ties stay ties
        plan = S.Conv2dF16Plan(wt.to(P16.DEV), bias.to(P16.DEV), act=S.ACT_NONE)
        P16.check(plan([p.to(P16.DEV) for p in parts]), P16.emulate(parts, wt, bias, "none"))


# ------------------------------------------------------------------ 3. the edge of the fp16 range
EDGE_SHAPE = (1, 9, 16, 3, 5, 49)
AT = (0, 4, 1, 2, 47)                             # interior in D and H, next to the 48-wide tile's edge in W


def test_range_edge_forward_and_input_gradient():
    """One operand at nextafter(65520, 0) rounds to 65504: every output finite and within the bar.  At 65520.0 it rounds to
    Inf: exactly the outputs that the emulation makes non-finite are non-finite (its 3x3x3 window in every output
    channel), all others within the bar.  Forward, then ``transpose_flip``.
    Measured: worst 7.7 / 7.9 of c = 448 just below the edge."""
    b, cin, cout, d, h, w = EDGE_SHAPE
    for flip in (False, True):
        x = rand(b, cin, d, h, w, seed=60 + flip)
        wt = rand(*((cin, cout) if flip else (cout, cin)), 3, 3, 3, seed=62 + flip, scale=0.1)
        x[AT] = M.below_edge16()
        y = C16.check(x, wt, flip=flip, what=f"below the edge, flip {flip}")
        assert torch.isfinite(y).all()
        x[AT] = M.EDGE16
        y = train3d.conv3d_k3s1_f16(x.cuda(), wt.cuda(), transpose_flip=flip).cpu().double()
        ref, mag = C16.reference(x, wt.flip(2, 3, 4).transpose(0, 1) if flip else wt)
        bad = ~torch.isfinite(ref)
        assert int(bad.sum()) == cout * 27
        assert torch.equal(~torch.isfinite(y), bad)
        ok = ~bad
        assert torch.all((y - ref).abs()[ok] <= C16.depth_c(cin) * U * mag[ok])


@pytest.mark.parametrize("which", ["g", "x"])
def test_range_edge_weight_gradient(which):
    """The same for g and for x of the weight gradient, at the granularity of the sibling overflow tests: just below the
    edge dW is finite and within the bar; at 65520 the operand's channel of dW is not finite and every other channel has
    the bits it has without it.  Measured: worst 4.8 (g) / 5.1 (x) of c = 140 just below the edge."""
    b, cin, cout, d, h, w = EDGE_SHAPE
    x, g = rand(b, cin, d, h, w, seed=64), rand(b, cout, d, h, w, seed=65)
    clean = train3d.conv3d_weight_grad_f16(x.cuda(), g.cuda())
    t = g if which == "g" else x
    ch = AT[1]
    t[AT] = M.below_edge16()
    assert torch.isfinite(W16.check(x, g)).all()
    t[AT] = M.EDGE16
    dw = train3d.conv3d_weight_grad_f16(x.cuda(), g.cuda())
    if which == "x":                               # dW is [Cout, Cin, 3, 3, 3]: put the operand's channel first
        dw, clean = dw.transpose(0, 1), clean.transpose(0, 1)
    assert torch.isfinite(clean).all() and not torch.isfinite(dw[ch]).all()
    keep = [c for c in range(dw.shape[0]) if c != ch]
    assert torch.equal(dw[keep], clean[keep])


# ------------------------------------------------------------------ 4. channels three decades apart
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_channel_ramp(b, cin, cout, d, h, w, elem):
    """Channel c scaled by 2^-min(2c, 10): a max-norm bar would see channel 0 alone, the per-element bar holds the rows of
    dW and the taps of y that the small channels feed.  Forward, input gradient, weight gradient (x ramped, then g).
    Measured: worst 1.5 .. 12.0 of c = 224 .. 1120 (y, dx) and 0.5 .. 1.3 of c = 129 .. 152 (dW), both types."""
    conv, wg = CONV[elem].check, WGRAD[elem].check
    conv(M.ramp((b, cin, d, h, w), seed=70), rand(cout, cin, 3, 3, 3, seed=71, scale=0.1), what="ramp")
    conv(M.ramp((b, cin, d, h, w), seed=72), rand(cin, cout, 3, 3, 3, seed=73, scale=0.1), flip=True, what="dgrad, ramp")
    wg(M.ramp((b, cin, d, h, w), seed=74), rand(b, cout, d, h, w, seed=75))
    wg(rand(b, cin, d, h, w, seed=76), M.ramp((b, cout, d, h, w), seed=77))


# ------------------------------------------------------------------ 5. bf16: the exponent range fp16 does not have
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_bf16_exponent_range(b, cin, cout, d, h, w):
    """g ~ 2^-60, x ~ 2^-40 (and weights at the other's scale): products about 2^-100, far below fp16's range and still
    normal in fp32.  bf16 subnormals (below 2^-126) stay unasserted, as DESIGN.md says.
    Measured: worst 0.5 .. 1.5 of c = 224 .. 1120 (y, dx) and 0.6 .. 1.1 of c = 129 .. 152 (dW)."""
    lo, hi = 2.0 ** -60, 2.0 ** -40
    x, g = rand(b, cin, d, h, w, seed=80, scale=hi), rand(b, cout, d, h, w, seed=81, scale=lo)
    nonzero(CB16.check(x, rand(cout, cin, 3, 3, 3, seed=82, scale=lo), what="2^-40 x 2^-60"))
    nonzero(CB16.check(g, rand(cout, cin, 3, 3, 3, seed=83, scale=hi), flip=True, what="dgrad, 2^-60 x 2^-40"))
    nonzero(WB16.check(x, g, "2^-40 x 2^-60 "))


# ------------------------------------------------------------------ 6. autograd hands the subnormal cotangent on unchanged
def test_autograd_with_a_subnormal_cotangent():
    """``train3d.conv3d(..., precision="f16")`` backward with a cotangent from ``subnormal16``: x.grad and w.grad have the
    bits of the direct entry calls (nothing on the way rescales, clamps or flushes the cotangent)."""
    b, cin, cout, d, h, w = SHAPES[3]
    x = rand(b, cin, d, h, w, seed=90).cuda().requires_grad_(True)
    wt = rand(cout, cin, 3, 3, 3, seed=91, scale=0.1).cuda().requires_grad_(True)
    g = M.subnormal16((b, cout, d, h, w), seed=92).cuda()
    train3d.conv3d(x, wt, None, 1, precision="f16").backward(g)
    assert torch.equal(x.grad, train3d.conv3d_k3s1_f16(g, wt.detach(), transpose_flip=True))
    assert torch.equal(wt.grad, train3d.conv3d_weight_grad_f16(x.detach(), g))
    assert float(x.grad.abs().max()) > 0 and float(wt.grad.abs().max()) > 0
