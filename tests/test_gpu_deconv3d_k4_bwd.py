"""dv_deconv3d_k4s2_dgrad_f32 / dv_deconv3d_k4s2_wgrad_f32 (csrc/deconv3d_k4_bwd.hip) against the float64 backward of
F.conv_transpose3d(kernel 4, stride 2, padding 1) on the CPU, for the IGEV hourglass's transposed layers.

Bar, per element (the one tests/test_gpu_conv3d_wgrad.py derives): |err| <= c * 2^-24 * sum |a * b| over that element's
sum, c = the number of roundings the kernel's own summation order imposes on a product.
  weight gradient: per K split, KW waves each run one fp32 fma chain over their rows (64 / KW of the 2 x 4 x 8 positions
      of x) of the split's bricks (padding positions as exact zeros); the KW chains are added in wave order, then the S
      split partials one after the other: c = ceil(bricks / S) * 64 / KW + (KW - 1) + S, with KW = 4 / (MW * NW) waves
      per 16 x 16 channel tile for blocks of fewer than four tiles (the launcher's rule, restated in k_waves)
  input gradient:  one fp32 fma chain over Co * 64 products (taps outside the volume and padded channels are exact
      zeros): c = Co * 64
The autograd function's forward runs on the inference kernel: 4 * (terms of the sum), the forward-kernel convention of
tests/test_gpu_conv3d_autograd.py, with Ci * 8 terms (2 x 2 x 2 taps reach an output position)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib, train3d
from test_gpu_conv3d_wgrad import assert_long_splits, split_ranges

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BRICK = (2, 4, 8)                   # x positions per brick of the weight-gradient kernel (WG_TZ, WG_TY, WG_TX)

SHAPES = [  # (Ci, Co, B, dims of x)
    (16, 8, 2, (6, 5, 12)),         # conv1_up pair
    (32, 16, 1, (3, 4, 7)),         # odd W: scalar path
    (48, 32, 3, (2, 3, 5)),         # 48 is no tile multiple; three batch items over the K split
    (16, 8, 1, (1, 1, 1)),          # every tap is border
]
# The split count is min(2048 / waves of the channel tiles, 48 MB / numel(dW), bricks): in SHAPES every split is one brick.
# These have more bricks than splits, so that a block walks two bricks and, in one split, bricks of two batch items
# (assert_long_splits; tests/test_wgrad_split_cases_host.py holds the same without a GPU), on every wave layout.
LONG = [  # (Ci, Co, B, dims of x)
    (64, 64, 3, (5, 9, 9)),         # 2 x 2 tiles, one K wave: 54 bricks over 32 splits, a tail in every brick dimension
    (32, 16, 3, (8, 16, 32)),       # 2 x 1 tiles, two K waves: 192 bricks over 128 splits
    (16, 8, 3, (8, 16, 32)),        # one tile, four K waves: the accumulators pass through the tiles' LDS after two bricks
]


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def k_waves(ci, co):
    """Waves that share one channel tile's brick (wg_plan in csrc/deconv3d_k4_bwd.hip)."""
    nm, nn = -(-ci // 16), -(-co // 16)
    tiles = (3 if nm % 3 == 0 else min(nm, 2)) * min(nn, 2)
    return 1 if tiles >= 4 else 4 // tiles


def split_plan(ci, co, b, dims):
    """(bricks, splits, bricks of one batch item): the bricks from the kernel's brick, the splits from the size entry."""
    per_item = math.prod(-(-n // t) for n, t in zip(dims, BRICK))
    splits = _lib.load().dv_deconv3d_k4s2_wgrad_workspace_floats(b, ci, *dims, co) // (ci * co * 64)
    assert splits >= 1
    return b * per_item, splits, per_item


def wgrad_c(ci, co, b, dims):
    nbricks, splits, _ = split_plan(ci, co, b, dims)
    kw = k_waves(ci, co)
    return -(-nbricks // splits) * math.prod(BRICK) // kw + (kw - 1) + splits


def f64_backward(x, w, g):
    xs, ws = x.double().requires_grad_(), w.double().requires_grad_()
    F.conv_transpose3d(xs, ws, None, stride=2, padding=1).backward(g.double())
    return xs.grad, ws.grad


@functools.lru_cache(maxsize=None)
def case(ci, co, b, dims):
    """Inputs and the float64 references (gradients, and the gradients of |.| for the bars): computed once, shared."""
    x, w = rand(b, ci, *dims, seed=ci * 7 + co), rand(ci, co, 4, 4, 4, seed=ci + co * 13) * 0.1
    g = rand(b, co, *[2 * n for n in dims], seed=ci + co + b)
    dx, dw = f64_backward(x, w, g)
    mx, mw = f64_backward(x.abs(), w.abs(), g.abs())
    return x, w, g, dx, dw, mx, mw


@pytest.mark.parametrize("ci,co,b,dims", SHAPES)
def test_input_gradient(ci, co, b, dims):
    x, w, g, dx, _, mx, _ = case(ci, co, b, dims)
    out = train3d.deconv3d_k4_input_grad(g.cuda(), w.cuda()).cpu().double()
    err = (out - dx).abs()
    print(f"dgrad {ci}->{co} {dims}: worst err / (u * mag) = {float((err / (mx * U)).max()):.1f}, c = {co * 64}")
    assert torch.all(err <= co * 64 * U * mx)


@pytest.mark.parametrize("ci,co,b,dims", SHAPES)
def test_weight_gradient(ci, co, b, dims):
    x, w, g, _, dw, _, mw = case(ci, co, b, dims)
    out = train3d.deconv3d_k4_weight_grad(x.cuda(), g.cuda()).cpu().double()
    c = wgrad_c(ci, co, b, dims)
    err = (out - dw).abs()
    print(f"wgrad {ci}->{co} {dims}: worst err / (u * mag) = {float((err / (mw * U).clamp(min=1e-300)).max()):.1f}, c = {c}")
    assert torch.all(err <= c * U * mw)


@pytest.mark.parametrize("ci,co,b,dims", LONG)
def test_weight_gradient_long_splits(ci, co, b, dims):
    """A block walks several bricks: the barrier before the re-staging, the overwrite of the LDS tiles, the brick index
    taken apart across y, z and batch boundaries inside one split, the accumulation over the bricks, and for KW > 1 the
    hand-over of the K waves' accumulators through the LDS of the tiles after the last brick."""
    nbricks, splits, per_item = split_plan(ci, co, b, dims)
    straddling = assert_long_splits(nbricks, splits, per_item)
    x, w, g, _, dw, _, mw = case(ci, co, b, dims)
    out = train3d.deconv3d_k4_weight_grad(x.cuda(), g.cuda()).cpu().double()
    c = wgrad_c(ci, co, b, dims)
    err = (out - dw).abs()
    sizes = sorted({b1 - b0 for b0, b1 in split_ranges(nbricks, splits)})
    print(f"LONG k4 wgrad {ci}->{co} B{b} {dims}: K waves {k_waves(ci, co)}, nbricks {nbricks}, splits {splits}, bricks per split "
          f"{sizes}, two batch items in splits {straddling}, worst err / (u * mag) = "
          f"{float((err / (mw * U).clamp(min=1e-300)).max()):.1f}, c = {c}")
    assert torch.all(err <= c * U * mw)


def test_misaligned_pointers_take_the_scalar_path():
    """W % 4 == 0 but g starts 4 bytes off a 16-byte boundary: no error, and the same bits as the vector path."""
    ci, co, b, dims = SHAPES[0]
    x, w, g, dx, _, mx, _ = case(ci, co, b, dims)
    buf = torch.empty(g.numel() + 1, device="cuda")
    g_off = buf[1:].view(g.shape).copy_(g)
    assert g_off.data_ptr() % 16 == 4
    out = train3d.deconv3d_k4_input_grad(g_off, w.cuda())
    assert torch.all((out.cpu().double() - dx).abs() <= co * 64 * U * mx)
    assert torch.equal(out, train3d.deconv3d_k4_input_grad(g.cuda(), w.cuda()))      # the same chain on both paths


def test_two_launches_same_bits():
    for ci, co, b, dims in SHAPES[:3]:
        x, w, g = (t.cuda() for t in case(ci, co, b, dims)[:3])
        assert torch.equal(train3d.deconv3d_k4_weight_grad(x, g), train3d.deconv3d_k4_weight_grad(x, g))
        assert torch.equal(train3d.deconv3d_k4_input_grad(g, w), train3d.deconv3d_k4_input_grad(g, w))
    ci, co, b, dims = LONG[2]                                            # several bricks per block, four K waves
    assert_long_splits(*split_plan(ci, co, b, dims))
    x, g = case(ci, co, b, dims)[0].cuda(), case(ci, co, b, dims)[2].cuda()
    assert torch.equal(train3d.deconv3d_k4_weight_grad(x, g), train3d.deconv3d_k4_weight_grad(x, g))


def test_nan_stays_in_its_input_channel():
    ci, co, b, dims = SHAPES[2]
    x, _, g = (t.clone() for t in case(ci, co, b, dims)[:3])
    x[1, 37, 1, 2, 3] = float("nan")
    nan = torch.isnan(train3d.deconv3d_k4_weight_grad(x.cuda(), g.cuda()).cpu())
    assert nan[37].any() and not nan[:37].any() and not nan[38:].any()
    # ... and in the SECOND brick of a split (a position of x is read by the one brick that holds it)
    ci, co, b, dims = LONG[0]
    nbricks, splits, per_item = split_plan(ci, co, b, dims)
    assert_long_splits(nbricks, splits, per_item)
    second = next(b0 for b0, b1 in split_ranges(nbricks, splits) if b1 - b0 >= 2) + 1
    nb = [-(-n // t) for n, t in zip(dims, BRICK)]
    item, r = divmod(second, per_item)
    origin = [i * t for i, t in zip((r // (nb[1] * nb[2]), (r // nb[2]) % nb[1], r % nb[2]), BRICK)]
    x, g = case(ci, co, b, dims)[0].clone(), case(ci, co, b, dims)[2]
    x[(item, 37, *origin)] = float("nan")
    nan = torch.isnan(train3d.deconv3d_k4_weight_grad(x.cuda(), g.cuda()).cpu())
    assert nan[37].any() and not nan[:37].any() and not nan[38:].any()


def test_bad_arguments_return_error_codes():
    lib = _lib.load()
    t = torch.zeros(4096, device="cuda")
    p, s = t.data_ptr(), _lib.stream_ptr()
    assert lib.dv_deconv3d_k4s2_dgrad_f32(None, p, p, 1, 16, 1, 1, 1, 8, s) == -1
    assert lib.dv_deconv3d_k4s2_dgrad_f32(p, None, p, 1, 16, 1, 1, 1, 8, s) == -1
    assert lib.dv_deconv3d_k4s2_dgrad_f32(p, p, None, 1, 16, 1, 1, 1, 8, s) == -1
    assert lib.dv_deconv3d_k4s2_dgrad_f32(p, p, p, 1, 16, 0, 1, 1, 8, s) == -2
    assert lib.dv_deconv3d_k4s2_dgrad_f32(p, p, p, 1, 16, 1, 1, 1, -8, s) == -2
    assert lib.dv_deconv3d_k4s2_dgrad_pack_weights_f32(None, p, 16, 8, s) == -1
    assert lib.dv_deconv3d_k4s2_dgrad_pack_weights_f32(p, p, 0, 8, s) == -2
    assert lib.dv_deconv3d_k4s2_dgrad_packed_floats(0, 8) == 0
    assert lib.dv_deconv3d_k4s2_dgrad_packed_floats(16, 8) == 64 * 8 * 16
    assert lib.dv_deconv3d_k4s2_dgrad_packed_floats(48, 30) == 64 * 32 * 48
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        assert lib.dv_deconv3d_k4s2_wgrad_f32(*args, 1, 16, 1, 1, 1, 8, s) == -1
    assert lib.dv_deconv3d_k4s2_wgrad_f32(p, p, p, p, 0, 16, 1, 1, 1, 8, s) == -2
    assert lib.dv_deconv3d_k4s2_wgrad_f32(p, p, p, p, 1, 16, 1, -1, 1, 8, s) == -2
    assert lib.dv_deconv3d_k4s2_wgrad_workspace_floats(1, 16, 1, 0, 1, 8) == 0
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0                                     # nothing was launched on the buffers


@pytest.fixture
def calls(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    lib = _lib.load()
    counts = {}
    for name in ("dv_deconv3d_k4s2_f32", "dv_deconv3d_k4s2_dgrad_f32", "dv_deconv3d_k4s2_wgrad_f32"):
        real = getattr(lib, name)

        def counting(*args, _real=real, _name=name):
            counts[_name] = counts.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(lib, name, counting)
    return counts


@pytest.mark.parametrize("ci,co,b,dims", SHAPES[:3])
def test_conv_transpose3d_k4_function(calls, monkeypatch, ci, co, b, dims):
    """The autograd function against float64, at the kernels' bars, and against its own torch route."""
    x, w, g, dx, dw, mx, mw = case(ci, co, b, dims)
    res = {}
    for r in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_CONV3D", r)
        xs, ws = x.cuda().requires_grad_(), w.cuda().requires_grad_()
        y = train3d.conv_transpose3d_k4(xs, ws)
        y.backward(g.cuda())
        res[r] = (y.detach().cpu().double(), xs.grad.cpu().double(), ws.grad.cpu().double())
    y64 = F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1)
    y, gx, gw = res["hip"]
    ymag = F.conv_transpose3d(x.double().abs(), w.double().abs(), None, stride=2, padding=1)
    assert torch.all((y - y64).abs() <= 4 * ci * 8 * U * ymag)              # 8 taps x Ci products per output
    assert torch.all((gx - dx).abs() <= co * 64 * U * mx)
    assert torch.all((gw - dw).abs() <= wgrad_c(ci, co, b, dims) * U * mw)
    assert calls == {"dv_deconv3d_k4s2_f32": 1, "dv_deconv3d_k4s2_dgrad_f32": 1, "dv_deconv3d_k4s2_wgrad_f32": 1}
    for a, t in zip(res["hip"], res["torch"]):
        torch.testing.assert_close(a, t, rtol=1e-4, atol=1e-4 * float(t.abs().max()))


def test_module_dispatch_and_cpu_tensors():
    m4 = torch.nn.ConvTranspose3d(16, 8, (4, 4, 4), stride=2, padding=1, bias=False).cuda()
    x = rand(1, 16, 2, 3, 4, seed=5).cuda()
    assert train3d.conv_transpose3d_module(m4, x).shape == (1, 8, 4, 6, 8)
    m3 = torch.nn.ConvTranspose3d(16, 8, 3, stride=2, padding=1, output_padding=1, bias=False).cuda()
    assert train3d.conv_transpose3d_module(m3, x).shape == (1, 8, 4, 6, 8)
    with pytest.raises(_lib.DiffuVolumeError):                                # conv_transpose3d keeps its k3 contract
        train3d.conv_transpose3d(x, m4.weight)
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.conv_transpose3d_k4(x.cpu(), m4.weight.detach().cpu())
