"""dv_resize_bilinear_ac_bwd_f32 (csrc/resize_bwd.hip) and `resize_bilinear_train`: the backward of
F.interpolate(x, size, mode="bilinear", align_corners=True).

Reference: float64 CPU autograd of F.interpolate.  Yardstick: the same in float32.  Bar per case, as relative L2 error
against float64:  rel(hip) <= 2 * rel(float32) + 1e-6.

Shapes (h, w) -> (H, W): scale 0 (a single source row / column), the identity, an exact x4, a ratio that is no integer, a
downscale, the 16-byte path (W % 4 == 0) and rows wider than the kernel's 64-column tile (three tiles, the last one
partial); with 1 and 7 planes (7: more than one block per launch everywhere)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib, resize_bilinear_train

pytestmark = pytest.mark.gpu

SHAPES = {"scale0_1": ((1, 1), (1, 1)), "scale0": ((1, 1), (3, 5)), "identity": ((2, 3), (2, 3)), "x4": ((3, 5), (12, 20)),
          "ratio": ((3, 5), (7, 9)), "down": ((5, 7), (3, 4)), "vector": ((4, 8), (16, 32)), "wide": ((3, 130), (5, 517))}
CASES = [(n, bc) for n in SHAPES for bc in (1, 7)]
SENT, PAD = -777.0, 1025


def rel(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


def operands(name, bc):
    (h, w), (hh, ww) = SHAPES[name]
    gen = torch.Generator().manual_seed(1000 * bc + h * 31 + ww)
    return torch.randn(1, bc, h, w, generator=gen), torch.randn(1, bc, hh, ww, generator=gen)


def autograd_bwd(x, dy, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    F.interpolate(x, list(dy.shape[-2:]), mode="bilinear", align_corners=True).backward(dy.to(dtype))
    return x.grad


@pytest.fixture(scope="module")
def refs():
    """(x, dy, dx float64, dx float32) per case, computed once on the CPU."""
    out = {}
    for name, bc in CASES:
        x, dy = operands(name, bc)
        out[name, bc] = (x, dy, autograd_bwd(x, dy, torch.float64), autograd_bwd(x, dy, torch.float32))
    return out


def entry(dy, dx, bc, h, w, hh, ww):
    return _lib.load().dv_resize_bilinear_ac_bwd_f32(dy.data_ptr(), dx.data_ptr(), bc, h, w, hh, ww, _lib.stream_ptr())


def hip_bwd(x, dy, fill=float("nan")):
    dy = dy.cuda().contiguous()
    bc, (h, w), (hh, ww) = x.shape[1], x.shape[-2:], dy.shape[-2:]
    dx = torch.full((1, bc, h, w), fill, device="cuda")
    assert entry(dy, dx, bc, h, w, hh, ww) == 0
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("name,bc", CASES)
def test_backward_against_float64(refs, name, bc):
    x, dy, f64, f32 = refs[name, bc]
    dx = hip_bwd(x, dy)
    assert bool(torch.isfinite(dx).all())                       # pre-filled with NaN: every element is written
    e, y = rel(dx, f64), rel(f32, f64)
    print(f"{name} BC={bc}: hip {e:.3g}  float32 {y:.3g}")
    assert e <= 2 * y + 1e-6


@pytest.mark.parametrize("name,bc", CASES)
def test_adjoint_identity(refs, name, bc, monkeypatch):
    """<resize(x), dy> == <x, bwd(dy)> with the project's own forward, within float32 rounding of the sums."""
    monkeypatch.setenv("DV_TRAIN_NET2D", "hip")
    x, dy, _, _ = refs[name, bc]
    y = resize_bilinear_train(x.cuda(), dy.shape[-2:])
    dx = hip_bwd(x, dy)
    lhs = float((y.double() * dy.cuda().double()).sum())
    rhs = float((x.cuda().double() * dx.double()).sum())
    scale = float((y.double().abs() * dy.cuda().double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-6 * scale + 1e-30, (lhs, rhs, scale)


@pytest.mark.parametrize("name", list(SHAPES))
def test_same_bits_on_every_launch_and_for_every_split(refs, name):
    x, dy, _, _ = refs[name, 7]
    a, b = hip_bwd(x, dy), hip_bwd(x, dy, fill=0.0)
    assert torch.equal(a, b)
    lo, hi = hip_bwd(x[:, :3], dy[:, :3]), hip_bwd(x[:, 3:], dy[:, 3:])
    assert torch.equal(torch.cat((lo, hi), dim=1), a)


def test_autograd_function_on_both_routes(refs, monkeypatch):
    x, dy, f64, f32 = refs["ratio", 7]
    grads = {}
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NET2D", route)
        xg = x.cuda().requires_grad_(True)
        y = resize_bilinear_train(xg, dy.shape[-2:])
        assert ("ResizeBilinearFn" in y.grad_fn.name()) == (route == "hip")
        y.backward(dy.cuda())
        grads[route] = xg.grad
        assert rel(y, F.interpolate(x.double(), list(dy.shape[-2:]), mode="bilinear", align_corners=True)) < 1e-6
    assert torch.equal(grads["hip"], hip_bwd(x, dy))
    assert rel(grads["hip"], f64) <= 2 * rel(f32, f64) + 1e-6
    assert rel(grads["torch"], f64) <= 2 * rel(f32, f64) + 1e-6
    monkeypatch.setenv("DV_TRAIN_NET2D", "hip")
    frozen = resize_bilinear_train(x.cuda(), dy.shape[-2:])
    assert not frozen.requires_grad


def carve(t, fill=None, off=1):
    """t's values (or `fill`) in the middle of a sentinel-filled arena -> (arena, view), `off` floats off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD + 4,), SENT, device="cuda")
    start = PAD + (off - PAD) % 4
    v = arena[start:start + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return arena, v, start


def intact(arena, start, n):
    return bool((arena[:start] == SENT).all()) and bool((arena[start + n:] == SENT).all())


@pytest.mark.parametrize("name", ["vector", "x4", "wide", "down", "scale0"])
def test_resize_bwd_abi_offset_views_bounds_and_refusals(refs, name):
    """dv_resize_bilinear_ac_bwd_f32 as a C caller sees it.  dy and dx one float off a 16-byte line (the element loads) give
    the bits of the run with dy on a line (the 16-byte loads where W % 4 == 0); dx lies between sentinels that survive and,
    pre-filled with NaN, comes back finite; NULL pointers and non-positive sizes return -1 and write nothing."""
    lib, st = _lib.load(), _lib.stream_ptr()
    x, dy, _, _ = refs[name, 7]
    (h, w), (hh, ww), bc = SHAPES[name][0], SHAPES[name][1], 7
    want = hip_bwd(x, dy)
    results = []
    for off in (1, 0):
        _, g, _ = carve(dy, off=off)
        arena, dx, start = carve(torch.empty(1, bc, h, w), fill=float("nan"), off=1)
        assert lib.dv_resize_bilinear_ac_bwd_f32(g.data_ptr(), dx.data_ptr(), bc, h, w, hh, ww, st) == 0
        torch.cuda.synchronize()
        assert intact(arena, start, dx.numel()), off
        assert bool(torch.isfinite(dx).all()), off
        results.append(dx.clone())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], want)

    # refusals: nothing is launched, nothing is written
    arena.fill_(SENT)
    null = ctypes.c_void_p(None)
    assert lib.dv_resize_bilinear_ac_bwd_f32(null, dx.data_ptr(), bc, h, w, hh, ww, st) == -1
    assert lib.dv_resize_bilinear_ac_bwd_f32(g.data_ptr(), null, bc, h, w, hh, ww, st) == -1
    for i in range(5):
        for bad in (0, -1):
            dims = [bc, h, w, hh, ww]
            dims[i] = bad
            assert lib.dv_resize_bilinear_ac_bwd_f32(g.data_ptr(), dx.data_ptr(), *dims, st) == -1, dims
    torch.cuda.synchronize()
    assert bool((arena == SENT).all())
