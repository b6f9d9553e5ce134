"""dv_conv3d_wgrad_f32 (csrc/conv3d_wgrad.hip) against float64 for every layer kind of ACVNet_DDIM's aggregation stack.

Bar, per element: |dW_hip - dW_f64| <= c * 2^-24 * sum |g * x| over that element's sum.  The kernel adds each element's
products in one fp32 fma chain per K split (the split's bricks, TZ*TY*TX positions each, padding positions included as
exact zeros) and then the S split partials one after the other, so every product passes through at most
c = ceil(bricks / S) * positions_per_brick + S roundings: the standard recursive-summation bound gamma_c.

The split count is min(512 / channel tiles, 48 MB / numel(dW), bricks).  CONV has few channel tiles, so there every split is
ONE brick; the LONG cases have 16 channel tiles (28 to 32 splits) under 54 to 81 bricks, so that the brick loop of a block
runs two or three times, over a batch boundary in one of the splits (`assert_long_splits`, also held without a GPU by
tests/test_wgrad_split_cases_host.py)."""
import functools
import math

import pytest
import torch

from diffuvolume_amd import _lib
from diffuvolume_amd.train3d import conv3d_weight_grad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
# (k, stride) -> output brick of the kernel (TZ, TY, TX)
BRICK = {(3, 1): (2, 4, 16), (3, 2): (2, 2, 8), (1, 1): (2, 4, 16)}


def out_dims(dims, k, s):
    pad = (k - 1) // 2
    return [(n + 2 * pad - k) // s + 1 for n in dims]


def split_plan(b, cin, dims, cout, k, s):
    """(bricks, splits, bricks of one batch item): the bricks from the kernel's brick, the splits from the size entry."""
    per_item = math.prod(-(-o // t) for o, t in zip(out_dims(dims, k, s), BRICK[(k, s)]))
    splits = _lib.load().dv_conv3d_wgrad_workspace_floats(b, cin, *dims, cout, k, s) // (cout * cin * k ** 3)
    return b * per_item, splits, per_item


def split_ranges(nbricks, splits):
    """The bricks [first, last) of every split, as both kernels cut them."""
    return [(nbricks * s // splits, nbricks * (s + 1) // splits) for s in range(splits)]


def assert_long_splits(nbricks, splits, per_item):
    """What makes a case a long-split case; a case that stops meeting it fails here and does not quietly stop covering
    the brick loop.  Returns the splits that hold bricks of two batch items."""
    ranges = split_ranges(nbricks, splits)
    assert splits >= 1 and all(b1 > b0 for b0, b1 in ranges), (nbricks, splits)
    assert any(b1 - b0 >= 2 for b0, b1 in ranges), f"no split holds two bricks: {nbricks} bricks over {splits} splits"
    assert nbricks % splits != 0, f"{nbricks} bricks divide evenly over {splits} splits"
    straddling = [(b0, b1) for b0, b1 in ranges if b0 // per_item != (b1 - 1) // per_item]
    assert straddling, f"no split holds bricks of two batch items: {nbricks} bricks, {per_item} per item, {splits} splits"
    return straddling


def depth_c(b, cin, dims, cout, k, s):
    nbricks, splits, _ = split_plan(b, cin, dims, cout, k, s)
    return -(-nbricks // splits) * math.prod(BRICK[(k, s)]) + splits


def ref_wgrad(x, g, k, s):
    pad = (k - 1) // 2
    return torch.nn.grad.conv3d_weight(x, (g.shape[1], x.shape[1], k, k, k), g, stride=s, padding=pad)


def check(x, g, k, s, cout, ref=None, mag=None):
    dw = conv3d_weight_grad(x.cuda(), g.cuda(), k, s, cout).cpu().double()
    if ref is None:
        x64, g64 = x.double(), g.double()
        ref = ref_wgrad(x64, g64, k, s)
        mag = ref_wgrad(x64.abs(), g64.abs(), k, s)
    c = depth_c(x.shape[0], x.shape[1], x.shape[2:], cout, k, s)
    err = (dw - ref).abs()
    worst = float((err / (mag * U).clamp(min=1e-300)).max())
    assert torch.all(err <= c * U * mag), (worst, c)
    return dw, worst, c


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


# more bricks than splits (see the module docstring): k3 s1, k1 and k3 s2, the three geometries of the kernel
LONG = [  # (cin, cout, k, stride, batch, dims)
    (128, 128, 3, 1, 3, (6, 9, 33)), (128, 128, 1, 1, 3, (6, 9, 33)), (128, 128, 3, 2, 3, (8, 10, 36)),
]


@functools.lru_cache(maxsize=None)
def long_case(cin, cout, k, s, b, dims):
    """Inputs and the float64 references of a LONG case: computed once, shared, left unchanged."""
    x = rand(b, cin, *dims, seed=cin * 7 + cout + k)
    g = rand(b, cout, *out_dims(dims, k, s), seed=cin + cout * 13 + s)
    x64, g64 = x.double(), g.double()
    return x, g, ref_wgrad(x64, g64, k, s), ref_wgrad(x64.abs(), g64.abs(), k, s)


@pytest.mark.parametrize("cin,cout,k,s,b,dims", LONG)
def test_conv_weight_gradient_long_splits(cin, cout, k, s, b, dims):
    """A block walks several bricks: the barrier before the re-staging, the overwrite of the LDS tiles, the brick index
    taken apart across y, z and batch boundaries inside one split, and the accumulation over the bricks."""
    nbricks, splits, per_item = split_plan(b, cin, dims, cout, k, s)
    straddling = assert_long_splits(nbricks, splits, per_item)
    x, g, ref, mag = long_case(cin, cout, k, s, b, dims)
    _, worst, c = check(x, g, k, s, cout, ref, mag)
    sizes = sorted({b1 - b0 for b0, b1 in split_ranges(nbricks, splits)})
    print(f"LONG conv3d wgrad {cin}->{cout} k{k} s{s} B{b} {dims}: nbricks {nbricks}, splits {splits}, bricks per split {sizes}, "
          f"two batch items in splits {straddling}, worst err / (u * mag) = {worst:.1f}, c = {c}")


@pytest.mark.parametrize("cin_t,cout_t,b,dims", [(128, 64, 3, (3, 4, 5)), (64, 32, 1, (6, 4, 10))])
def test_transposed_conv_weight_gradient(cin_t, cout_t, b, dims):
    """ConvTranspose3d(k3, s2, p1, op1): the stride-2 weight gradient with x and g exchanged."""
    x = rand(b, cin_t, *dims, seed=cin_t)
    gy = rand(b, cout_t, *[2 * n for n in dims], seed=cout_t + 1)
    w = torch.zeros(cin_t, cout_t, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv_transpose3d(x.double(), w, stride=2, padding=1, output_padding=1).backward(gy.double())
    dw = check(gy, x, 3, 2, cin_t)[0]              # the conv form is checked at its own bar ...
    torch.testing.assert_close(dw, w.grad, rtol=0, atol=float(1e-4 * w.grad.abs().max()))   # ... and is the deconv's


def test_two_launches_same_bits():
    x, g = rand(3, 32, 6, 8, 20, seed=1).cuda(), rand(3, 32, 6, 8, 20, seed=2).cuda()
    assert torch.equal(conv3d_weight_grad(x, g, 3, 1, 32), conv3d_weight_grad(x, g, 3, 1, 32))
    x2, g2 = rand(2, 32, 8, 8, 20, seed=3).cuda(), rand(2, 64, 4, 4, 10, seed=4).cuda()
    assert torch.equal(conv3d_weight_grad(x2, g2, 3, 2, 64), conv3d_weight_grad(x2, g2, 3, 2, 64))
    cin, cout, k, s, b, dims = LONG[0]                                   # several bricks per block
    assert_long_splits(*split_plan(b, cin, dims, cout, k, s))
    x3, g3 = (t.cuda() for t in long_case(*LONG[0])[:2])
    assert torch.equal(conv3d_weight_grad(x3, g3, k, s, cout), conv3d_weight_grad(x3, g3, k, s, cout))


def test_nan_stays_in_its_input_channel():
    x, g = rand(2, 40, 5, 8, 20, seed=5), rand(2, 32, 5, 8, 20, seed=6)
    x[1, 17, 3, 2, 7] = float("nan")
    dw = conv3d_weight_grad(x.cuda(), g.cuda(), 3, 1, 32).cpu()
    nan = torch.isnan(dw)
    assert nan[:, 17].any() and not nan[:, :17].any() and not nan[:, 18:].any()
    # ... and in the SECOND brick of a split: k = 1, so that only the brick that holds the position reads the NaN
    cin, cout, k, s, b, dims = LONG[1]
    assert k == 1 and s == 1
    nbricks, splits, per_item = split_plan(b, cin, dims, cout, k, s)
    assert_long_splits(nbricks, splits, per_item)
    second = next(b0 for b0, b1 in split_ranges(nbricks, splits) if b1 - b0 >= 2) + 1
    nb = [-(-o // t) for o, t in zip(dims, BRICK[(k, s)])]
    item, r = divmod(second, per_item)
    origin = [i * t for i, t in zip((r // (nb[1] * nb[2]), (r // nb[2]) % nb[1], r % nb[2]), BRICK[(k, s)])]
    x, g = long_case(*LONG[1])[:2]
    x = x.clone()
    x[(item, 77, *origin)] = float("nan")
    nan = torch.isnan(conv3d_weight_grad(x.cuda(), g.cuda(), k, s, cout).cpu())
    assert nan[:, 77].any() and not nan[:, :77].any() and not nan[:, 78:].any()
