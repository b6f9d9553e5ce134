"""The split-fp16 inference convolution (csrc/conv3d_f16x3.hip, ``Conv3dPlan(..., precision="f16x3")``) at low amplitude.

The kernel carries every activation as hi + lo, hi = fp16(v), lo = fp16(v - hi), v = x * in_scale * kActScale (2^-2).  While
lo is an fp16 NORMAL number the pair holds v to 2^-22 |v|.  lo is at most 2^-11 |v|, so below |v| = 2^-3 -- |x * in_scale|
below 0.5 -- it is subnormal, its spacing is 2^-24 whatever v is, and the pair carries an ABSOLUTE error of up to 2^-25 in
v, 2^-25 / kActScale = 2^-23 in x * in_scale.  (A hi that is itself subnormal, |v| < 2^-14, leaves the same 2^-25.)  The
noise prologue multiplies the volume by a factor in [0, 1], so the network's own activations reach this regime.

Per element, against the float64 convolution of the unrounded operands (no BatchNorm, no residual, no activation: the
epilogue is then one exact multiplication by kOutScale = 2^-8):

    |y - ref| <= c * 2^-24 * conv(|x s|, |w|)  +  2^-23 * conv([lo subnormal], |w|)

* the fp32 term, counted as tests/test_gpu_conv3d_f16.py counts it: per chunk of 8 input channels 7 K-blocks, here THREE
  matrix instructions each (hi*hi', hi*lo', lo*hi'), each adding 32 products to the fp32 accumulator at one rounding per
  product at worst: 3 * 32 * 7 * ceil(Cin / 8); plus 4 units for each of the two 22-bit splits (2^-22 = 4 * 2^-24) and 4 for
  the dropped lo*lo' (2^-11 * 2^-11), plus 1 for the rounding of x * (in_scale * 2^-2) where there is an in_scale:
      c = 672 * ceil(Cin / 8) + 12 (+ 1)         -- 684 (685) at 8 channels, 3372 (3373) at 40
* the floor: 2^-23 for every activation under the tap whose lo the emulation of the kernel's split finds subnormal, times
  |w| (the weight image is scaled by kWScale = 2^10 and the accumulator by kOutScale, which cancel).

Both terms are derived; neither was fitted.  The weight image has a floor of its own (2^-35 per weight below 2^-13); it is
given no term.

The header used to say the 2^-2 pre-scale keeps "lo parts out of the fp16 subnormal range", i.e. that the fp32 term alone
holds.  ``test_the_fp32_term_alone`` asserts that at k = 0 and records where it stops.

Measured on the MI355X, x = randn * 2^-k; "worst" is max |y - ref| / (2^-24 conv(|x s|, |w|)), to be read against c; the
CPU emulation of the split (float64 sums of the three products) gives the same figures to three digits:

                                  k = 0     k = 4     k = 8     k = 12      the fp32 term alone
  8 -> 32, no in_scale   (c 684)    2.8      12.4     180.8     3051.3      holds to k = 8, fails at 12 (31 % of y)
  8 -> 32, in_scale      (c 685)    3.8      34.3     719.1    10317.3      holds to k = 4, fails at 8 (one output), 12 (61 %)
  40 -> 32, no in_scale  (c 3372)   2.1       5.7      75.8     1740.8      holds at every k here
  40 -> 32, in_scale     (c 3373)   2.9      13.0     194.3     3464.5      holds to k = 8, fails at 12 (one output)

The error per unit of sum |x w| grows 16-fold for every 2^-4 in amplitude: it is absolute, as the floor says, and the GPU
confirms the emulation.  That the fp32 term alone survives to 2^-8 is the slack of its worst-case c (the accumulation
itself stays at 2 .. 4), not the split.  Against the whole bar the worst output is at 0.27 (8 channels, in_scale,
k = 12); what is beyond the fp32 term is at most 0.25 of the floor.  lo is subnormal for 83 % (95 % with in_scale) of the
activations at k = 0 -- by |v| < 2^-3 or by the chance of v lying close to an fp16 number -- and for all of them from
k = 4 on.
"""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
K_ACT = 0.25                          # kActScale
FLOOR = 2.0 ** -25 / K_ACT            # per activation with a subnormal lo, in units of x * in_scale
ROWS = [(8, 32, (1, 2, 4, 96)), (40, 32, (1, 4, 4, 32))]          # of test_conv_f16x3_oracle (tests/test_gpu_parity.py)
KS = [0, 4, 8, 12]


def depth_c(cin, in_scale):
    return 3 * 32 * 7 * -(-cin // 8) + 12 + (1 if in_scale else 0)


def lo_is_subnormal(x, scale):
    """The kernel's split (csrc/conv3d_f16x3.hip, ``commit``) in float32 on the CPU: where lo = fp16(v - fp16(v)) is below
    the smallest fp16 normal, zero included."""
    v = x * (K_ACT if scale is None else (scale * K_ACT).unsqueeze(1))
    return ((v - v.half().float()).half().float().abs() < 2.0 ** -14)


_CASES = {}


def case(cfg, k, with_scale):
    """-> (|y - ref|, fp32 term per unit of c, floor term), computed once per case and shared by the two tests."""
    key = (cfg, k, with_scale)
    if key not in _CASES:
        cin, cout, dims = cfg
        g = _gen(23, f"{cfg}{k}")
        x = torch.randn(dims[0], cin, *dims[1:], generator=g) * 2.0 ** -k
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
        scale = torch.rand(dims[0], *dims[1:], generator=g) if with_scale else None
        plan = S.Conv3dPlan(w.to(DEV), None, stride=1, act=S.ACT_NONE, precision="f16x3")
        y = plan(x.to(DEV), in_scale=None if scale is None else scale.to(DEV)).cpu().double()
        xs = x.double() if scale is None else x.double() * scale.double().unsqueeze(1)
        ref = F.conv3d(xs, w.double(), padding=1)
        unit = U * F.conv3d(xs.abs(), w.double().abs(), padding=1)
        sub = lo_is_subnormal(x, scale)
        floor = FLOOR * F.conv3d(sub.double(), w.double().abs(), padding=1)
        assert y.shape == ref.shape and float(ref.abs().max()) > 0
        _CASES[key] = ((y - ref).abs(), unit, floor, float(sub.double().mean()))
    return _CASES[key]


@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "in_scale"])
@pytest.mark.parametrize("cfg", ROWS)
def test_low_amplitude_within_the_fp32_term_plus_the_floor(cfg, with_scale):
    c = depth_c(cfg[0], with_scale)
    for k in KS:
        err, unit, floor, share = case(cfg, k, with_scale)
        against_c = float((err / unit.clamp_min(1e-300)).max())
        against_floor = float(((err - c * unit).clamp_min(0) / floor.clamp_min(1e-300)).max())
        both = float((err / (c * unit + floor).clamp_min(1e-300)).max())
        print(f"F16X3 {cfg} in_scale {with_scale} k {k}: lo subnormal {share:.3f}; worst {against_c:.1f} of c = {c}; "
              f"beyond the fp32 term {against_floor:.3f} of the floor; {both:.3f} of the whole bar")
        assert torch.all(err <= c * unit + floor), (k, both)


@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "in_scale"])
@pytest.mark.parametrize("cfg", ROWS)
def test_the_fp32_term_alone(cfg, with_scale):
    """What the header claimed: no floor.  It holds at unit amplitude; the amplitudes at which it does not are printed
    (and written into the module docstring)."""
    c = depth_c(cfg[0], with_scale)
    held = {}
    for k in KS:
        err, unit, _, _ = case(cfg, k, with_scale)
        held[k] = bool(torch.all(err <= c * unit))
        over = float((err > c * unit).double().mean())
        print(f"F16X3 {cfg} in_scale {with_scale} k {k}: the fp32 term alone {'holds' if held[k] else 'FAILS'} "
              f"({over:.4f} of the outputs beyond it)")
    assert held[0]
