"""dv_conv2d_wgrad_cat_bf16 (csrc/conv2d_wgrad_cat_bf16.hip, the bf16 instantiation of csrc/conv2d_wgrad_cat_mp.h) and the
bf16 gate kernels (csrc/gru_gates_bf16.hip) of the update block's train precision "bf16".

Exact contract, as tests/test_gpu_conv2d_wgrad_cat_f16.py's: dW = sum rb16(g) * rb16(x) with fp32 accumulation, so the
reference is the float64 weight gradient of ``x.bfloat16().double()`` and ``g.bfloat16().double()`` on the CPU and the
only difference is the fp32 accumulation order (a product of two bf16 values has 16 significant bits: exact in fp32).
Bar: the existing per-element one, |dW - dW_f64| <= c * 2^-24 * sum |g x| with c = ceil(bricks / S) * TY * TX + S, the
brick being 4 x 32 positions and S what the bf16 workspace query implies.  Operands are randn: normal bf16 numbers."""
import ctypes

import pytest
import torch

from diffuvolume_amd import _lib, train2d
from diffuvolume_amd.train2d import conv2d_cat_weight_grad
from test_gpu_conv2d_wgrad_cat import rand, ref_wgrad
from test_gpu_conv2d_wgrad_cat_f16 import BLOCK_LAYERS, EDGES, TX, TY, U

pytestmark = pytest.mark.gpu
ENTRY, SIZE = "dv_conv2d_wgrad_cat_bf16", "dv_conv2d_wgrad_cat_bf16_workspace_floats"


def rb16(t):
    return t.bfloat16().float()


def wgrad(sources, g, k):
    return conv2d_cat_weight_grad(sources, g, k, elem="bf16")


def depth_c(chans, b, h, w, cout, k):
    arr = (ctypes.c_int * len(chans))(*chans)
    n = getattr(_lib.load(), SIZE)(arr, len(chans), b, h, w, cout, k)
    per = cout * sum(chans) * k * k
    assert n > 0 and n % per == 0 and n * 4 <= 48 << 20
    s = n // per
    return -(-(b * -(-h // TY) * -(-w // TX)) // s) * TY * TX + s


def check(sources, g, k, gpu_sources=None):
    gpu_sources = [t.cuda() for t in sources] if gpu_sources is None else gpu_sources
    dw = wgrad(gpu_sources, g.cuda(), k)
    assert dw.dtype == torch.float32
    dw = dw.cpu().double()
    x64, g64 = torch.cat([rb16(t) for t in sources], dim=1).double(), rb16(g).double()
    ref, mag = ref_wgrad(x64, g64, k), ref_wgrad(x64.abs(), g64.abs(), k)
    c = depth_c([t.shape[1] for t in sources], g.shape[0], g.shape[2], g.shape[3], g.shape[1], k)
    err = (dw - ref).abs()
    assert dw.shape == ref.shape and torch.isfinite(dw).all()
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"WGRADBF16 {[t.shape[1] for t in sources]}->{g.shape[1]} k{k} {tuple(g.shape[2:])}: worst {worst:.2f} of c = {c}, "
          f"relative L2 {rel:.2e}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return dw


@pytest.mark.parametrize("chans,cout,k", BLOCK_LAYERS)
def test_update_block_layers(chans, cout, k):
    h, w = 13, 37
    srcs = [rand(2, c, h, w, seed=11 * i + c + h) for i, c in enumerate(chans)]
    check(srcs, rand(2, cout, h, w, seed=cout + 3 * h + k), k)


@pytest.mark.parametrize("chans,cout,k,b,h,w", EDGES)
def test_edge_shapes(chans, cout, k, b, h, w):
    srcs = [rand(b, c, h, w, seed=17 * i + c + w) for i, c in enumerate(chans)]
    check(srcs, rand(b, cout, h, w, seed=cout + w), k)


def test_non_contiguous_channel_view():
    """A source handed over as a channel slice of a wider tensor: the wrapper makes it contiguous."""
    wide, other, g = rand(2, 40, 7, 19, seed=3), rand(2, 11, 7, 19, seed=4), rand(2, 13, 7, 19, seed=5)
    view = wide.cuda()[:, 3:27]
    assert not view.is_contiguous()
    check([wide[:, 3:27], other], g, 3, gpu_sources=[view, other.cuda()])


def test_two_launches_same_bits_dirty_workspace_and_every_element_written():
    chans, b, h, w, cout = (128, 64, 9), 2, 20, 44, 96
    srcs = [rand(b, c, h, w, seed=c).cuda() for c in chans]
    g = rand(b, cout, h, w, seed=2).cuda()
    a = wgrad(srcs, g, 3)
    assert torch.equal(a, wgrad(srcs, g, 3)) and torch.isfinite(a).all()
    assert not torch.equal(a, conv2d_cat_weight_grad(srcs, g, 3, f16=True))         # (another rounding: other bits)
    lib = _lib.load()
    arr = (ctypes.c_int * 3)(*chans)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in srcs])
    n = getattr(lib, SIZE)(arr, 3, b, h, w, cout, 3)
    ws = torch.full((n,), float("nan"), device="cuda")                # stale contents must not leak into the result
    for _ in range(2):
        dw = torch.full((cout, sum(chans), 3, 3), float("nan"), device="cuda")
        _lib.check(getattr(lib, ENTRY)(ptrs, arr, 3, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, h, w, cout, 3,
                                       _lib.stream_ptr()), ENTRY)
        torch.cuda.synchronize()
        assert torch.equal(dw, a)


def test_range_what_overflows_fp16_stays_finite_and_within_the_bar():
    """A g element of 1e6 and an x element of 1e30 -- Inf at fp16 -- are ordinary bf16 numbers: dW finite, inside the bar."""
    srcs = [rand(2, 24, 12, 40, seed=5), rand(2, 16, 12, 40, seed=6)]
    g = rand(2, 32, 12, 40, seed=7)
    g[1, 5, 3, 7] = 1e6
    srcs[1][0, 3, 6, 20] = 1e30
    srcs[0][1, 2, 3, 7] = 1e30                       # (meets the large g in the centre tap: 1e36)
    dw = check(srcs, g, 3)
    assert float(dw.abs().max()) > 1e35
    f16 = conv2d_cat_weight_grad([t.cuda() for t in srcs], g.cuda(), 3, f16=True)
    assert not torch.isfinite(f16).all()             # the same operands at fp16: the overflow GradScaler skips on


def test_a_real_inf_of_the_gradient_stays_in_its_output_channel():
    srcs = [rand(2, 24, 12, 40, seed=5).cuda(), rand(2, 16, 12, 40, seed=6).cuda()]
    g = rand(2, 32, 12, 40, seed=7).cuda()
    clean = wgrad(srcs, g, 3)
    g[1, 5, 3, 7] = float("inf")
    dw = wgrad(srcs, g, 3)
    assert torch.isfinite(clean).all()
    assert not torch.isfinite(dw[5]).all()
    keep = [c for c in range(32) if c != 5]
    assert torch.equal(dw[keep], clean[keep])


def test_refusals():
    lib = _lib.load()
    x, g = rand(1, 8, 4, 4, seed=1).cuda(), rand(1, 8, 4, 4, seed=2).cuda()
    with pytest.raises(_lib.DiffuVolumeError):
        wgrad([x] * 5, g, 3)
    with pytest.raises(_lib.DiffuVolumeError):
        wgrad([x], g, 5)
    with pytest.raises(_lib.DiffuVolumeError):
        wgrad([x[:, :, :3]], g, 3)                                   # mismatched planes
    with pytest.raises(ValueError):
        conv2d_cat_weight_grad([x], g, 3, f16=True, elem="bf16")      # the two spellings must agree
    # the entry itself returns its error code for them, it launches nothing
    dw, ws = torch.zeros(8, 8, 5, 5, device="cuda"), torch.zeros(1 << 16, device="cuda")
    one, five = (ctypes.c_int * 1)(8), (ctypes.c_int * 5)(8, 8, 8, 8, 8)
    p1, p5 = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_void_p * 5)(*[x.data_ptr()] * 5)
    fn = getattr(lib, ENTRY)
    assert fn(p1, one, 1, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 4, 4, 8, 5, _lib.stream_ptr()) == -3
    assert fn(p5, five, 5, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 4, 4, 8, 3, _lib.stream_ptr()) == -2
    assert getattr(lib, SIZE)(one, 1, 1, 4, 4, 8, 5) == 0
    assert getattr(lib, SIZE)(five, 5, 1, 4, 4, 8, 3) == 0
    torch.cuda.synchronize()
    assert float(dw.abs().sum()) == 0.0


@pytest.mark.parametrize("n,offset", [(3, 0), (4099, 0), (1027, 1)])
def test_gate_kernels_match_torch_bfloat16_arithmetic(n, offset):
    """dv_gru_reset_mul_bf16 / dv_gru_blend_bf16 against torch's bfloat16 expressions R * H and (1 - Z) * H + Z * Q, bit for
    bit: lengths that are no multiple of 4 and a view misaligned by one float (the scalar body).  Operands are tanh /
    sigmoid of randn rounded to bf16, so every result is a normal number."""
    gen = torch.Generator().manual_seed(n + offset)
    mk = lambda f: rb16(f(torch.randn(n + offset, generator=gen))).cuda()[offset:]
    h, q, z, r = mk(torch.tanh), mk(torch.tanh), mk(torch.sigmoid), mk(torch.sigmoid)
    rh, hn = (torch.full((n + offset,), float("nan"), device="cuda")[offset:] for _ in range(2))
    train2d._gates("dv_gru_reset_mul_bf16", r, h, rh, n)
    train2d._gates("dv_gru_blend_bf16", z, q, h, hn, n)
    H, Q, Z, R = (t.bfloat16() for t in (h, q, z, r))
    assert torch.equal(rh, (R * H).float())
    assert torch.equal(hn, ((1 - Z) * H + Z * Q).float())
