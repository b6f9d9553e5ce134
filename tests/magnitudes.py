"""Operands for the tests that hold the 16-bit kernels to their bars away from amplitude 1 (tests/test_gpu_amp_magnitudes.py;
tests/test_amp_magnitudes_host.py checks on the CPU that each builder has the property its GPU tests rest on).

Every builder returns float32 on the CPU and is a pure function of its arguments."""
import torch

EDGE16 = 65520.0                      # the first float32 that torch.half() rounds to Inf (the tie between 65504 and 2^16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(t, dtype):
    """``t`` rounded to ``dtype`` (round to nearest even), back as float32."""
    return t.to(dtype).float()


def subnormal16(shape, seed):
    """+-2^U(-26, -12): most of ``t.half()`` is subnormal (below 2^-14) and not zero; the rest are the smallest normals
    and values that round to zero (below 2^-25)."""
    g = _gen(seed)
    mag = torch.exp2(torch.rand(*shape, generator=g) * 14 - 26)
    return mag * torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)


def is_subnormal16(t):
    """Elements of ``t`` whose fp16 rounding is subnormal and not zero."""
    h = rounded(t, torch.float16)
    return (h != 0) & (h.abs() < 2.0 ** -14)


def ties16(shape, seed, dtype=torch.float16):
    """(a + next(a)) / 2 for random ``a`` of the 16-bit type ``dtype`` (unit normal draws kept away from zero and, at fp16,
    away from the subnormals), ``next`` the neighbour away from zero, taken by incrementing the bit pattern.  The last
    bit of ``a`` is drawn on its own, so half of the ``a`` are odd: round to nearest even sends those to next(a) and the
    others back to ``a``.  Every midpoint needs one significand bit more than the type has, so it is exact in float32."""
    g = _gen(seed)
    a = torch.randn(*shape, generator=g)
    a = torch.where(a.abs() < 2.0 ** -6, torch.full_like(a, 2.0 ** -6).copysign(a), a).to(dtype)
    bits = a.view(torch.int16)
    odd = (torch.rand(*shape, generator=g) < 0.5).to(bits.dtype)
    bits = (bits & ~1) | odd
    lo, hi = bits.view(dtype).float(), (bits + 1).view(dtype).float()
    return (lo + hi) / 2


def half_away(t, dtype):
    """``t`` rounded to ``dtype`` with ties AWAY from zero (what a kernel must not do), as float32: for the host test."""
    r = rounded(t, dtype)
    bits = r.view(torch.int32)                                     # the 16-bit value sits in float32: its neighbour away
    step = 1 << (23 - (10 if dtype == torch.float16 else 7))       # from zero is one unit of its last kept bit further
    up = (bits + step).view(torch.float32)
    tie = (t - r).abs() == (up - t).abs()
    return torch.where(tie & (r.abs() < t.abs()), up, r)


RAMP_CAP = 10                         # 2^-10 * 2^-3 = 2^-13: still an fp16 normal (the smallest is 2^-14)


def ramp(shape, seed):
    """Unit normal draws (magnitudes kept at or above 2^-3) with channel c (dim 1) scaled by 2^-min(2c, RAMP_CAP): the
    channels span three decades and none of them rounds to an fp16 subnormal or to zero."""
    x = torch.randn(*shape, generator=_gen(seed))
    x = torch.where(x.abs() < 2.0 ** -3, torch.full_like(x, 2.0 ** -3).copysign(x), x)
    e = torch.clamp(2 * torch.arange(shape[1]), max=RAMP_CAP).float()
    return x * torch.exp2(-e).reshape(1, -1, *([1] * (len(shape) - 2)))


def below_edge16():
    """The last float32 that stays finite at fp16: nextafter(65520, 0) (it rounds to 65504)."""
    return float(torch.nextafter(torch.tensor(EDGE16), torch.tensor(0.0)))
