"""dv_dwconv3x3_f32 / dv_dwconv3x3_bwd_f32 (csrc/dwconv2d.hip): the depthwise 3x3 convolution of MobileNetV2's blocks,
forward with folded BatchNorm and ReLU / ReLU6 inside the launch, and the backward of the bare convolution.

Reference: the PyTorch expression in float64 on the CPU -- F.conv2d(groups=C) [* scale + shift] [clamp], autograd for the
gradients.  Yardstick: the same expression in float32.  Bar per tensor, as relative L2 error against float64:
    rel(hip) <= 2 * rel(float32) + 1e-6

Shapes (H, W): a single pixel, a single row, 2 x 3, odd and even sizes (at stride 2 the last output's right and bottom taps
fall on padding only for odd sizes), W % 4 != 0 and W % 4 == 0 (the 16-byte path), planes narrow enough that a wave folds
several row bands (7 x 9: 16 bands of one row; 35 x 100: two bands of 16 rows, twice), more than one band in H (33 rows:
three bands of 16, at stride 2 three of 8) and more than one tile of 256 output columns in W (5 x 300, and 3 x 259 whose second
tile holds three columns).  B in {1, 3}, C in {1, 5, 96}, both strides.

The inputs are scaled (`operands`: the convolution's standard deviation is about 6, the shift around 3) so that ReLU6
clamps on both sides.  A tensor with fewer than 40
outputs cannot be asked to hold 5 % of them at each end (5 % of it is less than two elements, 1 x 1 with C = 1 is ONE
output), so `test_relu6_inputs_clamp_on_both_sides` asserts the two fractions on the float64 reference per case for the
tensors with at least 40 outputs and over the pooled outputs of the smaller ones."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (2, 3), (7, 9), (8, 10), (33, 130), (8, 12), (35, 100), (5, 300), (3, 259)]
BWD_SHAPES = SHAPES
CHANNELS = (1, 5, 96)
ACTS = {"none": (0, 0.0), "relu": (1, 0.0), "relu6": (1, 6.0)}
SENT, PAD = -777.0, 1025


def rel(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


def out_size(n, stride):
    return (n - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def operands(c, shape):
    """x [3,C,H,W], w [C,1,3,3], scale, shift [C] on the CPU."""
    h, w = shape
    gen = torch.Generator().manual_seed(7919 * c + 131 * h + w)
    # every channel's nine taps have norm 1 and x ~ N(0, s^2) with s = 18 / sqrt(taps inside the image): the convolution has
    # a standard deviation of about 6 whatever the plane's size and however few channels there are, so that without the
    # affine map ~50 % of the outputs are <= 0 and ~16 % >= 6, and with it (centre 3) ~30 % on each side
    x = torch.randn(3, c, h, w, generator=gen) * (18.0 / (min(h, 3) * min(w, 3)) ** 0.5)
    wt = torch.randn(c, 1, 3, 3, generator=gen)
    wt = wt / wt.flatten(1).norm(dim=1).view(c, 1, 1, 1)
    scale = torch.rand(c, generator=gen) * 0.4 + 0.8
    shift = torch.randn(c, generator=gen) * 0.5 + 3.0
    return x, wt, scale, shift


def expression(x, wt, scale, shift, stride, act, dtype):
    y = F.conv2d(x.to(dtype), wt.to(dtype), None, stride, 1, 1, x.shape[1])
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return {"none": y, "relu": y.clamp(min=0), "relu6": y.clamp(0, 6)}[act]


@functools.lru_cache(maxsize=None)
def forward_refs(c, shape, stride, act, affine):
    """(float64, float32) of the batch of three, computed once per case."""
    x, wt, scale, shift = operands(c, shape)
    sc, sh = (scale, shift) if affine else (None, None)
    return expression(x, wt, sc, sh, stride, act, torch.float64), expression(x, wt, sc, sh, stride, act, torch.float32)


def hip_forward(x, wt, scale, shift, stride, act, fill=float("nan")):
    x, wt = x.cuda().contiguous(), wt.cuda().contiguous()
    scale, shift = (None, None) if scale is None else (scale.cuda(), shift.cuda())
    b, c, h, w = x.shape
    out = torch.full((b, c, out_size(h, stride), out_size(w, stride)), fill, device="cuda")
    code, cap = ACTS[act]
    assert _lib.load().dv_dwconv3x3_f32(x.data_ptr(), wt.data_ptr(), _lib.ptr(scale), _lib.ptr(shift), out.data_ptr(), b, c, h,
                                        w, stride, code, cap, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", CHANNELS)
def test_forward_against_float64(c, stride, shape, act):
    x, wt, scale, shift = operands(c, shape)
    for affine in (True, False):
        f64, f32 = forward_refs(c, shape, stride, act, affine)
        sc, sh = (scale, shift) if affine else (None, None)
        for b in (1, 3):
            out = hip_forward(x[:b], wt, sc, sh, stride, act)
            assert out.shape == f64[:b].shape
            assert bool(torch.isfinite(out).all())                   # pre-filled with NaN: every element is written
            e, y = rel(out, f64[:b]), rel(f32[:b], f64[:b])
            print(f"C={c} s={stride} {shape} {act} affine={affine} B={b}: hip {e:.3g}  float32 {y:.3g}")
            assert e <= 2 * y + 1e-6


def test_relu6_inputs_clamp_on_both_sides():
    small_lo = small_hi = small_n = 0
    for c in CHANNELS:
        for stride in (1, 2):
            for shape in SHAPES:
                for affine in (True, False):
                    f64, _ = forward_refs(c, shape, stride, "relu6", affine)
                    for b in (1, 3):
                        r = f64[:b]
                        lo, hi, n = int((r == 0).sum()), int((r == 6).sum()), r.numel()
                        if n >= 40:
                            assert lo >= 0.05 * n and hi >= 0.05 * n, (c, stride, shape, affine, b, lo, hi, n)
                        else:
                            small_lo, small_hi, small_n = small_lo + lo, small_hi + hi, small_n + n
    assert small_n > 0 and small_lo >= 0.05 * small_n and small_hi >= 0.05 * small_n, (small_lo, small_hi, small_n)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_forward_bits_repeat_and_do_not_depend_on_the_batch(stride, shape):
    x, wt, scale, shift = operands(5, shape)
    a = hip_forward(x, wt, scale, shift, stride, "relu6")
    assert torch.equal(a, hip_forward(x, wt, scale, shift, stride, "relu6", fill=0.0))
    for i in range(3):
        assert torch.equal(a[i:i + 1], hip_forward(x[i:i + 1], wt, scale, shift, stride, "relu6")), i


def carve(t, fill=None, off=1):
    """t's values (or `fill`) in the middle of a sentinel-filled arena -> (arena, view, start); the view lies `off` floats
    off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD + 4,), SENT, device="cuda")
    start = PAD + (off - PAD) % 4
    v = arena[start:start + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return arena, v, start


def intact(arena, start, n):
    return bool((arena[:start] == SENT).all()) and bool((arena[start + n:] == SENT).all())


@pytest.mark.parametrize("shape", [(8, 12), (35, 100), (5, 300), (33, 130), (1, 7)])
@pytest.mark.parametrize("stride", [1, 2])
def test_vector_and_element_paths_give_the_same_bits(stride, shape):
    """The same tensors once on 16-byte lines and once through views one float off them, input and output separately.
    (8,12), (35,100), (5,300): W % 4 == 0, so the aligned run takes 16-byte loads; (1,7) at stride 2: Wo = 4, 16-byte stores."""
    lib, st = _lib.load(), _lib.stream_ptr()
    x, wt, scale, shift = operands(5, shape)
    want = hip_forward(x, wt, scale, shift, stride, "relu6")
    b, c, h, w = x.shape
    wd, sc, sh = wt.cuda(), scale.cuda(), shift.cuda()
    for off_in in (0, 1):
        for off_out in (0, 1):
            _, xv, _ = carve(x, off=off_in)
            arena, out, start = carve(torch.empty_like(want), fill=float("nan"), off=off_out)
            assert lib.dv_dwconv3x3_f32(xv.data_ptr(), wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(), b, c, h, w,
                                        stride, 1, 6.0, st) == 0
            torch.cuda.synchronize()
            assert intact(arena, start, out.numel()) and torch.equal(out, want), (off_in, off_out)


# ---- backward -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def backward_refs(c, shape, stride):
    """dy and (dx, dw) of the batch of three and of its first item alone, by autograd in float64 and float32."""
    x, wt, _, _ = operands(c, shape)
    h, w = shape
    gen = torch.Generator().manual_seed(31 * c + 7 * h + w + stride)
    dy = torch.randn(3, c, out_size(h, stride), out_size(w, stride), generator=gen)
    out = {}
    for b in (1, 3):
        for dtype in (torch.float64, torch.float32):
            xg, wg = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x[:b], wt))
            F.conv2d(xg, wg, None, stride, 1, 1, c).backward(dy[:b].to(dtype))
            out[b, dtype] = (xg.grad, wg.grad)
    return dy, out


def hip_backward(x, wt, dy, stride, want_dx=True, want_dw=True, fill=float("nan")):
    lib = _lib.load()
    x, wt, dy = x.cuda().contiguous(), wt.cuda().contiguous(), dy.cuda().contiguous()
    b, c, h, w = x.shape
    dx = torch.full_like(x, fill) if want_dx else None
    dw = torch.full_like(wt, fill) if want_dw else None
    n = lib.dv_dwconv3x3_bwd_workspace_floats(b, c, h, w, stride)
    assert n > 0
    ws = torch.full((n,), float("nan"), device="cuda") if want_dw else None
    assert lib.dv_dwconv3x3_bwd_f32(x.data_ptr(), wt.data_ptr(), dy.data_ptr(), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(ws), b, c,
                                    h, w, stride, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    return dx, dw


@pytest.mark.parametrize("shape", BWD_SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", CHANNELS)
def test_backward_against_float64(c, stride, shape):
    x, wt, _, _ = operands(c, shape)
    dy, refs = backward_refs(c, shape, stride)
    for b in (1, 3):
        dx, dw = hip_backward(x[:b], wt, dy[:b], stride)
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all())     # every element is written
        for name, got, f64, f32 in (("dx", dx, refs[b, torch.float64][0], refs[b, torch.float32][0]),
                                    ("dw", dw, refs[b, torch.float64][1], refs[b, torch.float32][1])):
            e, y = rel(got, f64), rel(f32, f64)
            print(f"C={c} s={stride} {shape} B={b} {name}: hip {e:.3g}  float32 {y:.3g}")
            assert e <= 2 * y + 1e-6, name


@pytest.mark.parametrize("shape", BWD_SHAPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_backward_bits_repeat_null_subsets_and_batch_split(stride, shape):
    x, wt, _, _ = operands(5, shape)
    dy, _ = backward_refs(5, shape, stride)
    dx, dw = hip_backward(x, wt, dy, stride)
    dx2, dw2 = hip_backward(x, wt, dy, stride, fill=0.0)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    only_dx, none = hip_backward(x, wt, dy, stride, want_dw=False)
    assert none is None and torch.equal(only_dx, dx)
    none, only_dw = hip_backward(x, wt, dy, stride, want_dx=False)
    assert none is None and torch.equal(only_dw, dw)
    for i in range(3):
        one, _ = hip_backward(x[i:i + 1], wt, dy[i:i + 1], stride)
        assert torch.equal(one, dx[i:i + 1]), i


def test_autograd_function_and_module_route():
    """train2d.dwconv2d: forward = the entry without scale, shift or activation; backward = the backward entry."""
    from diffuvolume_amd import train2d
    for stride in (1, 2):
        x, wt, _, _ = operands(5, (8, 10))
        dy, refs = backward_refs(5, (8, 10), stride)
        xg, wg = x.cuda().requires_grad_(True), wt.cuda().requires_grad_(True)
        y = train2d.dwconv2d(xg, wg, stride)
        assert "DepthwiseConv2dFn" in y.grad_fn.name()
        assert torch.equal(y, hip_forward(x, wt, None, None, stride, "none"))
        y.backward(dy.cuda())
        dx, dw = hip_backward(x, wt, dy, stride)
        assert torch.equal(xg.grad, dx) and torch.equal(wg.grad, dw)
        frozen = train2d.dwconv2d(x.cuda(), wt.cuda(), stride)
        assert not frozen.requires_grad


# ---- the entries as a C caller sees them ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,stride", [((8, 12), 1), ((8, 12), 2), ((33, 130), 1), ((33, 130), 2), ((3, 259), 1),
                                          ((5, 300), 2), ((1, 1), 2)])
def test_dwconv_abi_offset_views_bounds_and_refusals(shape, stride):
    """dv_dwconv3x3_f32, dv_dwconv3x3_bwd_workspace_floats and dv_dwconv3x3_bwd_f32 as a C caller sees them: every input a
    view one float off a 16-byte line, every output (and the workspace) between sentinels that survive, pre-filled with NaN
    and finite afterwards, with the bits of the aligned run; refused calls return their code and write nothing."""
    lib, st = _lib.load(), _lib.stream_ptr()
    x, wt, scale, shift = operands(5, shape)
    dy, _ = backward_refs(5, shape, stride)
    b, c, h, w = x.shape
    want = hip_forward(x, wt, scale, shift, stride, "relu6")
    want_dx, want_dw = hip_backward(x, wt, dy, stride)
    (_, xv, _), (_, wv, _), (_, sc, _), (_, sh, _), (_, gv, _) = (carve(t) for t in (x, wt, scale, shift, dy))
    a_out, out, s_out = carve(torch.empty_like(want), fill=float("nan"))
    a_dx, dx, s_dx = carve(torch.empty(b, c, h, w), fill=float("nan"))
    a_dw, dw, s_dw = carve(torch.empty(c, 1, 3, 3), fill=float("nan"))
    n = lib.dv_dwconv3x3_bwd_workspace_floats(b, c, h, w, stride)
    a_ws, ws, s_ws = carve(torch.empty(n), fill=float("nan"))
    fwd = lambda *a: lib.dv_dwconv3x3_f32(*a, st)                                       # noqa: E731
    bwd = lambda *a: lib.dv_dwconv3x3_bwd_f32(*a, st)                                   # noqa: E731
    p = lambda t: t.data_ptr()                                                          # noqa: E731
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), b, c, h, w, stride, 1, 6.0) == 0
    assert bwd(p(xv), p(wv), p(gv), p(dx), p(dw), p(ws), b, c, h, w, stride) == 0
    torch.cuda.synchronize()
    for arena, t, start in ((a_out, out, s_out), (a_dx, dx, s_dx), (a_dw, dw, s_dw), (a_ws, ws, s_ws)):
        assert intact(arena, start, t.numel())
        assert bool(torch.isfinite(t).all())
    assert torch.equal(out, want) and torch.equal(dx, want_dx) and torch.equal(dw, want_dw)

    # refusals: nothing is launched, nothing is written
    for arena in (a_out, a_dx, a_dw, a_ws):
        arena.fill_(SENT)
    null = ctypes.c_void_p(None)
    dims = (b, c, h, w, stride)
    assert fwd(null, p(wv), p(sc), p(sh), p(out), *dims, 1, 6.0) == -1
    assert fwd(p(xv), null, p(sc), p(sh), p(out), *dims, 1, 6.0) == -1
    assert fwd(p(xv), p(wv), p(sc), p(sh), null, *dims, 1, 6.0) == -1
    assert fwd(p(xv), p(wv), null, p(sh), p(out), *dims, 1, 6.0) == -1                  # scale and shift: both or neither
    assert fwd(p(xv), p(wv), p(sc), null, p(out), *dims, 1, 6.0) == -1
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), b, c, h, w, 3, 1, 6.0) == -3         # stride 3
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), b, c, h, w, 0, 1, 6.0) == -3
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), *dims, 3, 0.0) == -3                 # LeakyReLU is not an activation here
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), *dims, 1, -1.0) == -3
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), *dims, 1, float("nan")) == -3
    assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), *dims, 0, 6.0) == -3                 # a cap without a ReLU
    assert bwd(p(xv), p(wv), null, p(dx), p(dw), p(ws), *dims) == -1
    assert bwd(p(xv), p(wv), p(gv), null, null, p(ws), *dims) == -1                     # no output wanted
    assert bwd(p(xv), p(wv), p(gv), p(dx), p(dw), null, *dims) == -1                    # dw needs the workspace
    assert bwd(null, p(wv), p(gv), p(dx), p(dw), p(ws), *dims) == -1                    # ... and x
    assert bwd(p(xv), null, p(gv), p(dx), p(dw), p(ws), *dims) == -1                    # dx needs w
    assert bwd(p(xv), p(wv), p(gv), p(dx), p(dw), p(ws), b, c, h, w, 3) == -3
    for i in range(4):
        for bad in (0, -1):
            d = [b, c, h, w]
            d[i] = bad
            assert fwd(p(xv), p(wv), p(sc), p(sh), p(out), *d, stride, 1, 6.0) == -2, d
            assert bwd(p(xv), p(wv), p(gv), p(dx), p(dw), p(ws), *d, stride) == -2, d
            assert lib.dv_dwconv3x3_bwd_workspace_floats(*d, stride) == 0
    assert lib.dv_dwconv3x3_bwd_workspace_floats(b, c, h, w, 3) == 0
    torch.cuda.synchronize()
    for arena in (a_out, a_dx, a_dw, a_ws):
        assert bool((arena == SENT).all())
    # what the NULLs above are allowed to be when the output that needs them is not wanted
    assert bwd(null, p(wv), p(gv), p(dx), null, null, *dims) == 0                       # dx alone: no x, no workspace
    assert bwd(p(xv), null, p(gv), null, p(dw), p(ws), *dims) == 0                      # dw alone: no w
    torch.cuda.synchronize()
    assert torch.equal(dx, want_dx) and torch.equal(dw, want_dw)
