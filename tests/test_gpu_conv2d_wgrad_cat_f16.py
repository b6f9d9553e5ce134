"""dv_conv2d_wgrad_cat_f16 (csrc/conv2d_wgrad_cat_f16.hip) and the fp16 gate kernels of mixed-precision training.

Exact contract: dW = sum r16(g) * r16(x) with fp32 accumulation, so the reference is the float64 weight gradient of
``x.half().double()`` and ``g.half().double()`` on the CPU and the only difference is the fp32 accumulation order (a
product of two fp16 values is exact in fp32).  Bar: the one tests/test_gpu_conv2d_wgrad_cat.py holds the fp32 kernel to,
per element  |dW - dW_f64| <= c * 2^-24 * sum |g x|  with  c = ceil(bricks / S) * TY * TX + S  (every product passes
through at most one rounding per position of its split and one per split; the order inside a matrix instruction is
covered by the same count), the brick here being 4 x 32 positions and S what the workspace query implies.  (That file has
no relative-L2 bar; the per-element one implies it.)"""
import ctypes

import pytest
import torch

from diffuvolume_amd import _lib, train2d
from diffuvolume_amd.train2d import conv2d_cat_weight_grad
from test_gpu_conv2d_wgrad_cat import rand, ref_wgrad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TY, TX = 4, 32                        # the kernel's output brick


def r16(t):
    return t.half().float()


def splits_of(chans, b, h, w, cout, k):
    arr = (ctypes.c_int * len(chans))(*chans)
    n = _lib.load().dv_conv2d_wgrad_cat_f16_workspace_floats(arr, len(chans), b, h, w, cout, k)
    assert n > 0 and n % (cout * sum(chans) * k * k) == 0 and n * 4 <= 48 << 20
    return n // (cout * sum(chans) * k * k)


def depth_c(chans, b, h, w, cout, k):
    nbricks = b * -(-h // TY) * -(-w // TX)
    s = splits_of(chans, b, h, w, cout, k)
    return -(-nbricks // s) * TY * TX + s


def check(sources, g, k, gpu_sources=None):
    gpu_sources = [t.cuda() for t in sources] if gpu_sources is None else gpu_sources
    dw = conv2d_cat_weight_grad(gpu_sources, g.cuda(), k, f16=True)
    assert dw.dtype == torch.float32
    dw = dw.cpu().double()
    x64, g64 = torch.cat([r16(t) for t in sources], dim=1).double(), r16(g).double()
    ref, mag = ref_wgrad(x64, g64, k), ref_wgrad(x64.abs(), g64.abs(), k)
    c = depth_c([t.shape[1] for t in sources], g.shape[0], g.shape[2], g.shape[3], g.shape[1], k)
    err = (dw - ref).abs()
    assert dw.shape == ref.shape
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"WGRAD16 {[t.shape[1] for t in sources]}->{g.shape[1]} k{k} {tuple(g.shape[2:])}: worst {worst:.2f} of c = {c}, "
          f"relative L2 {rel:.2e}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return dw


BLOCK_LAYERS = [  # (source channels, cout, k): the block's real layers
    ((128, 128, 128, 128), 128, 3),     # a ConvGRU over four sources
    ((64, 64), 127, 3),                 # encoder.conv
    ((162,), 64, 1),                    # encoder.convc1
    ((128,), 256, 3),                   # disp_head.conv1
    ((256,), 1, 3),                     # disp_head.conv2
    ((128,), 32, 3),                    # mask_feat_4
]
EDGES = [  # (source channels, cout, k, batch, h, w)
    ((8,), 8, 3, 1, 1, 1),                        # H = W = 1
    ((16, 8), 24, 3, 3, 2, 3),                    # B 3, 2 x 3
    ((5, 3), 7, 3, 2, 6, 9),                      # channel counts that are no multiples of 8
    ((33,), 17, 1, 2, 5, 7),                      # k = 1
    ((12,), 20, 3, 1, 3, 5),                      # 15 positions: below one K step of the matrix instruction
    ((40, 9), 66, 3, 1, 4, 32),                   # exactly one brick
    ((7, 64, 1, 30), 65, 3, 2, 9, 33),            # four sources; one row and one column past a brick
]


@pytest.mark.parametrize("h,w", [(20, 28), (13, 37)])
@pytest.mark.parametrize("chans,cout,k", BLOCK_LAYERS)
def test_update_block_layers(chans, cout, k, h, w):
    srcs = [rand(2, c, h, w, seed=11 * i + c + h) for i, c in enumerate(chans)]
    check(srcs, rand(2, cout, h, w, seed=cout + 3 * h + k), k)


@pytest.mark.parametrize("chans,cout,k,b,h,w", EDGES)
def test_edge_shapes(chans, cout, k, b, h, w):
    srcs = [rand(b, c, h, w, seed=17 * i + c + w) for i, c in enumerate(chans)]
    check(srcs, rand(b, cout, h, w, seed=cout + w), k)


def test_non_contiguous_channel_view():
    """A source handed over as a channel slice of a wider tensor: the wrapper makes it contiguous."""
    wide = rand(2, 40, 7, 19, seed=3)
    other = rand(2, 11, 7, 19, seed=4)
    g = rand(2, 13, 7, 19, seed=5)
    view = wide.cuda()[:, 3:27]
    assert not view.is_contiguous()
    check([wide[:, 3:27], other], g, 3, gpu_sources=[view, other.cuda()])


def test_two_launches_same_bits_dirty_workspace_and_every_element_written():
    chans, b, h, w, cout = (128, 64, 9), 2, 20, 44, 96
    srcs = [rand(b, c, h, w, seed=c).cuda() for c in chans]
    g = rand(b, cout, h, w, seed=2).cuda()
    a = conv2d_cat_weight_grad(srcs, g, 3, f16=True)
    assert torch.equal(a, conv2d_cat_weight_grad(srcs, g, 3, f16=True)) and torch.isfinite(a).all()
    lib = _lib.load()
    arr = (ctypes.c_int * 3)(*chans)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in srcs])
    n = lib.dv_conv2d_wgrad_cat_f16_workspace_floats(arr, 3, b, h, w, cout, 3)
    ws = torch.full((n,), float("nan"), device="cuda")                # stale contents must not leak into the result
    for _ in range(2):
        dw = torch.full((cout, sum(chans), 3, 3), float("nan"), device="cuda")
        _lib.check(lib.dv_conv2d_wgrad_cat_f16(ptrs, arr, 3, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, h, w, cout, 3,
                                               _lib.stream_ptr()), "dv_conv2d_wgrad_cat_f16")
        torch.cuda.synchronize()
        assert torch.equal(dw, a)


def test_overflow_of_the_gradient_stays_in_its_output_channel():
    """One g element beyond the fp16 range becomes Inf while it is staged: Inf / NaN in that output channel's rows of dW
    (what torch.amp.GradScaler skips a step on), every other row as without it."""
    srcs = [rand(2, 24, 12, 40, seed=5).cuda(), rand(2, 16, 12, 40, seed=6).cuda()]
    g = rand(2, 32, 12, 40, seed=7).cuda()
    clean = conv2d_cat_weight_grad(srcs, g, 3, f16=True)
    g[1, 5, 3, 7] = 1e6
    dw = conv2d_cat_weight_grad(srcs, g, 3, f16=True)
    assert torch.isfinite(clean).all()
    assert not torch.isfinite(dw[5]).all()
    keep = [c for c in range(32) if c != 5]
    assert torch.equal(dw[keep], clean[keep])


def test_refusals():
    lib = _lib.load()
    x, g = rand(1, 8, 4, 4, seed=1).cuda(), rand(1, 8, 4, 4, seed=2).cuda()
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x] * 5, g, 3, f16=True)
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x], g, 5, f16=True)
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x[:, :, :3]], g, 3, f16=True)        # mismatched planes
    # the entry itself returns its error code for them, it launches nothing
    dw, ws = torch.zeros(8, 8, 5, 5, device="cuda"), torch.zeros(1 << 16, device="cuda")
    one, five = (ctypes.c_int * 1)(8), (ctypes.c_int * 5)(8, 8, 8, 8, 8)
    p1, p5 = (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_void_p * 5)(*[x.data_ptr()] * 5)
    assert lib.dv_conv2d_wgrad_cat_f16(p1, one, 1, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 4, 4, 8, 5, _lib.stream_ptr()) != 0
    assert lib.dv_conv2d_wgrad_cat_f16(p5, five, 5, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 4, 4, 8, 3, _lib.stream_ptr()) != 0
    assert lib.dv_conv2d_wgrad_cat_f16_workspace_floats(one, 1, 1, 4, 4, 8, 5) == 0
    assert lib.dv_conv2d_wgrad_cat_f16_workspace_floats(five, 5, 1, 4, 4, 8, 3) == 0
    torch.cuda.synchronize()
    assert float(dw.abs().sum()) == 0.0


@pytest.mark.parametrize("n,offset", [(3, 0), (4099, 0), (1027, 1)])
def test_gate_kernels_match_torch_half_arithmetic(n, offset):
    """dv_gru_reset_mul_f16 / dv_gru_blend_f16 against torch's half arithmetic, bit for bit: lengths that are no multiple
    of 4 and a view misaligned by one float (the scalar body)."""
    gen = torch.Generator().manual_seed(n + offset)
    mk = lambda f: r16(f(torch.randn(n + offset, generator=gen))).cuda()[offset:]
    h, q, z, r = mk(torch.tanh), mk(torch.tanh), mk(torch.sigmoid), mk(torch.sigmoid)
    rh, hn = (torch.full((n + offset,), float("nan"), device="cuda")[offset:] for _ in range(2))
    train2d._gates("dv_gru_reset_mul_f16", r, h, rh, n)
    train2d._gates("dv_gru_blend_f16", z, q, h, hn, n)
    H, Q, Z, R = (t.half() for t in (h, q, z, r))
    assert torch.equal(rh, (R * H).float())
    assert torch.equal(hn, ((1 - Z) * H + Z * Q).float())
