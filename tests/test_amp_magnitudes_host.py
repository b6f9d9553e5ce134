"""tests/magnitudes.py on the CPU: each builder has the property that keeps the GPU tests of tests/test_gpu_amp_magnitudes.py
from passing vacuously.  Everything here is computed on the float64 reference alone: a WRONG rounding of the operands
(subnormals flushed, ties rounded away from zero) is put into the reference, and the share of output elements that then
miss the sibling tests' per-element bar c * 2^-24 * sum |operands| is printed and asserted.

Shares measured on the four shapes below (pytest -s prints them):
  subnormal16    0.78 .. 0.81 of the rounded operand is subnormal and not zero;
                 flushed g: 0.9997 .. 1.0 of dW and 0.9987 .. 1.0 of dx miss the bar; flushed x: 0.9996 .. 1.0 of dW
  ties16         sign-coherent operands (|ties| against |randn|), round-half-away: 1.0 of y and of dW miss the bar, at
                 fp16 and at bf16;  signed operands (printed, asserted non-zero only): fp16 0.03 .. 0.88 of y and
                 0.72 .. 0.96 of dW, bf16 0.78 .. 0.99 and 0.96 .. 1.0
The signed share is low where the sum is long: half of the ties move by one unit of the last place, with the sign of the
operand, so against a signed second operand the errors add up like sqrt(N) while the bar grows like N (at 40 input
channels, c = 1120, 3 % of y).  With both operands positive they add up like N -- 2^-11.5 of the sum against the bar's
c * 2^-24, a factor 5800 / c -- which is why the GPU tests run the ties both ways: signed for the sign handling, coherent
for the power this file asserts."""
import pytest
import torch
import torch.nn.functional as F

import magnitudes as M
from test_gpu_conv3d_f16 import depth_c as fwd_c
from test_gpu_conv3d_wgrad_f16 import depth_c as wgrad_c, ref_wgrad

U = 2.0 ** -24
SHAPES = [(1, 8, 8, 2, 2, 32), (1, 5, 7, 2, 3, 17), (2, 40, 32, 3, 5, 50), (1, 9, 16, 3, 5, 49)]     # (B, Cin, Cout, D, H, W)
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def built():
    """The weight-gradient bar reads its split count from the library's workspace query (host code)."""
    from diffuvolume_amd import _build
    return _build.build()


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def conv(x, w):
    return F.conv3d(x.double(), w.double(), padding=1)


def dgrad(g, w):
    return conv(g, w.flip(2, 3, 4).transpose(0, 1))


def wgrad(x, g):
    return ref_wgrad(x.double(), g.double())


def missed(op, a, a_wrong, b, c):
    """Share of the elements of op(a, b) that op(a_wrong, b) misses by more than the bar c * 2^-24 * op(|a|, |b|)."""
    ref, mag = op(a, b), op(a.abs(), b.abs())
    return float(((op(a_wrong, b) - ref).abs() > c * U * mag).double().mean())


@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_subnormal16_is_mostly_subnormal_and_flushing_it_misses_the_bar(b, cin, cout, d, h, w):
    r16 = lambda t: M.rounded(t, torch.float16)
    g, x = M.subnormal16((b, cout, d, h, w), seed=1), rand(b, cin, d, h, w, seed=2)
    assert float(g.abs().max()) <= 2.0 ** -12 and float(g.abs().min()) >= 2.0 ** -26
    sub = M.is_subnormal16(g)
    share = float(sub.float().mean())
    flushed = torch.where(sub, torch.zeros(()), r16(g))
    cw = wgrad_c(b, cin, d, h, w, cout)
    dw = missed(lambda gg, xx: wgrad(xx, gg), r16(g), flushed, r16(x), cw)
    wt = rand(cout, cin, 3, 3, 3, seed=3, scale=0.1)
    dx = missed(dgrad, r16(g), flushed, r16(wt), fwd_c(cout))
    xs = M.subnormal16((b, cin, d, h, w), seed=4)
    xsub = M.is_subnormal16(xs)
    dw_x = missed(wgrad, r16(xs), torch.where(xsub, torch.zeros(()), r16(xs)), r16(rand(b, cout, d, h, w, seed=5)), cw)
    print(f"MAGHOST subnormal {(b, cin, cout, d, h, w)}: subnormal share {share:.3f}; flushed g misses dW {dw:.4f}, dx {dx:.4f}; "
          f"flushed x misses dW {dw_x:.4f}")
    assert share > 0.5 and float(xsub.float().mean()) > 0.5
    assert dw > 0.9 and dx > 0.9 and dw_x > 0.9


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_ties16_are_exact_midpoints_that_round_to_even(b, cin, cout, d, h, w, dtype):
    t = M.ties16((b, cin, d, h, w), seed=6, dtype=dtype)
    r = M.rounded(t, dtype)
    bits = r.to(dtype).view(torch.int16).int()
    assert torch.all(bits & 1 == 0)                                     # round to nearest even
    toward, away = r.abs() < t.abs(), r.abs() > t.abs()
    assert torch.all(toward | away)                                     # no value is representable: all were rounded
    # each value is the float64 midpoint of its two 16-bit neighbours, so float32 held it exactly
    other = torch.where(toward, bits + 1, bits - 1).to(torch.int16).view(dtype)
    assert torch.equal(t.double(), (r.double() + other.double()) / 2)
    up = float(away.float().mean())
    assert 0.4 < up < 0.6, up                                           # half of the a had an odd last bit
    assert float((t < 0).float().mean()) > 0.3 and float((t > 0).float().mean()) > 0.3
    assert float(t.abs().min()) >= 2.0 ** -6 and torch.isfinite(t).all()
    ha = M.half_away(t, dtype)
    assert torch.equal(ha[away], r[away]) and torch.all(ha[toward].abs() > t[toward].abs())
    assert torch.equal(M.rounded(ha, dtype), ha)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_round_half_away_on_the_ties_misses_the_bar(b, cin, cout, d, h, w, dtype):
    rd = lambda t: M.rounded(t, dtype)
    cf, cw = fwd_c(cin), wgrad_c(b, cin, d, h, w, cout)
    shares = {}
    for mode, f in (("signed", lambda t: t), ("coherent", torch.abs)):
        tx, tw, tg = (f(M.ties16(s, seed=7 + i, dtype=dtype)) for i, s in
                      enumerate([(b, cin, d, h, w), (cout, cin, 3, 3, 3), (b, cout, d, h, w)]))
        x, wt, g = f(rand(b, cin, d, h, w, seed=10)), f(rand(cout, cin, 3, 3, 3, seed=11)), f(rand(b, cout, d, h, w, seed=12))
        ha = lambda t: M.half_away(t, dtype)
        shares[mode] = {
            "y, ties in x": missed(conv, rd(tx), ha(tx), rd(wt), cf),
            "y, ties in w": missed(lambda ww, xx: conv(xx, ww), rd(tw), ha(tw), rd(x), cf),
            "dW, ties in x": missed(wgrad, rd(tx), ha(tx), rd(g), cw),
            "dW, ties in g": missed(lambda gg, xx: wgrad(xx, gg), rd(tg), ha(tg), rd(x), cw),
        }
        print(f"MAGHOST ties {mode} {dtype} {(b, cin, cout, d, h, w)}: " + ", ".join(f"{k} {v:.4f}" for k, v in shares[mode].items()))
    assert all(v > 0.9 for v in shares["coherent"].values()), shares["coherent"]
    assert all(v > 0 for v in shares["signed"].values()), shares["signed"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_ramp_has_no_zero_and_no_subnormal_after_rounding(dtype):
    for b, cin, cout, d, h, w in SHAPES:
        x = M.ramp((b, cin, d, h, w), seed=13)
        r = M.rounded(x, dtype)
        assert float(r.abs().min()) >= 2.0 ** -13 > 2.0 ** -14          # 2^-14: the smallest fp16 normal
        per_channel = x.abs().amax(dim=(0, 2, 3, 4))
        assert per_channel[0] > 1 and per_channel[-1] < 2.0 ** -(min(2 * (cin - 1), M.RAMP_CAP) - 3)
        assert float(per_channel[0] / per_channel[-1]) > 2.0 ** 6       # a max-norm bar would see channel 0 alone


def test_the_fp16_range_edge():
    assert M.EDGE16 == 65520.0 and M.below_edge16() < M.EDGE16
    assert torch.isinf(torch.tensor(M.EDGE16).half()) and float(torch.tensor(M.below_edge16()).half()) == 65504.0
