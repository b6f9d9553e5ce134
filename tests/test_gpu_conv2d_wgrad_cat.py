"""dv_conv2d_wgrad_cat_f32 (csrc/conv2d_wgrad_cat.hip) against float64 ``torch.nn.grad.conv2d_weight`` of the materialised
concatenation, for every layer of IGEV's update block at the three scales of a 20 x 28 plane and for edge shapes.

Bar, per element: |dW_hip - dW_f64| <= c * 2^-24 * sum |g * x| over that element's sum.  The kernel adds each element's
products in one fp32 fma chain per K split -- the split's bricks, 2 x 32 output positions each, positions outside the
image included as exact zeros -- and then the S split partials one after the other, so a product passes through at most
    c = ceil(bricks / S) * 64 + S
roundings (the recursive-summation bound gamma_c, as in tests/test_gpu_conv2d_wgrad.py).  S is what the workspace query
implies: floats / (Cout * Cin * k * k).

The split plan counts the bricks of the WHOLE batch, so it is not batch-independent: a batch and its two halves are not
summed in the same order and equal bits are not promised (tested below: the split count moves with B, the halves' sum
holds the same bound)."""
import ctypes

import pytest
import torch

from diffuvolume_amd import _lib
from diffuvolume_amd.train2d import conv2d_cat_weight_grad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TY, TX = 2, 32                        # the kernel's output brick


def splits_of(chans, b, h, w, cout, k):
    arr = (ctypes.c_int * len(chans))(*chans)
    n = _lib.load().dv_conv2d_wgrad_cat_workspace_floats(arr, len(chans), b, h, w, cout, k)
    assert n > 0 and n % (cout * sum(chans) * k * k) == 0 and n * 4 <= 48 << 20
    return n // (cout * sum(chans) * k * k)


def depth_c(chans, b, h, w, cout, k):
    nbricks = b * -(-h // TY) * -(-w // TX)
    s = splits_of(chans, b, h, w, cout, k)
    return -(-nbricks // s) * TY * TX + s


def ref_wgrad(x, g, k):
    return torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], k, k), g, padding=(k - 1) // 2)


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def check(sources, g, k):
    dw = conv2d_cat_weight_grad([t.cuda() for t in sources], g.cuda(), k).cpu().double()
    x64, g64 = torch.cat(sources, dim=1).double(), g.double()
    ref, mag = ref_wgrad(x64, g64, k), ref_wgrad(x64.abs(), g64.abs(), k)
    c = depth_c([t.shape[1] for t in sources], g.shape[0], g.shape[2], g.shape[3], g.shape[1], k)
    err = (dw - ref).abs()
    assert dw.shape == ref.shape
    assert torch.all(err <= c * U * mag), (float((err / (mag * U).clamp_min(1e-300)).max()), c)
    return dw


PLANES = [(20, 28), (10, 14), (5, 7)]
BLOCK_LAYERS = [  # (source channels, cout, k): every 3x3 / 1x1 layer of BasicMultiUpdateBlock
    ((128, 128, 128), 128, 3),      # gru04 convz / convr / convq: [h | motion features | interp]
    ((128, 256), 128, 3),           # gru08 with its two x sources given as one
    ((128, 128), 128, 3),           # gru16
    ((162,), 64, 1),                # encoder.convc1
    ((64,), 64, 3),                 # encoder.convc2 / convd2
    ((64, 64), 127, 3),             # encoder.conv
    ((128,), 256, 3),               # disp_head.conv1
    ((256,), 1, 3),                 # disp_head.conv2
    ((128,), 32, 3),                # mask_feat_4
]
EDGES = [  # (source channels, cout, k, batch, h, w)
    ((32, 64, 16, 24), 48, 3, 2, 7, 45),          # four sources; H odd, W not a multiple of 32
    ((127, 1), 128, 3, 1, 9, 33),                 # sources that are no multiples of 8; one column past a brick
    ((5, 13, 3), 7, 1, 3, 13, 35),                # k = 1, odd everything
    ((1,), 1, 3, 1, 1, 1),                        # the smallest problem
    ((64, 64), 70, 3, 3, 3, 65),
]


@pytest.mark.parametrize("h,w", PLANES)
@pytest.mark.parametrize("chans,cout,k", BLOCK_LAYERS)
def test_update_block_layers(chans, cout, k, h, w):
    srcs = [rand(2, c, h, w, seed=11 * i + c + h) for i, c in enumerate(chans)]
    check(srcs, rand(2, cout, h, w, seed=cout + 3 * h + k), k)


@pytest.mark.parametrize("chans,cout,k,b,h,w", EDGES)
def test_edge_shapes(chans, cout, k, b, h, w):
    srcs = [rand(b, c, h, w, seed=17 * i + c + w) for i, c in enumerate(chans)]
    check(srcs, rand(b, cout, h, w, seed=cout + w), k)


def test_two_launches_same_bits_and_workspace_reuse():
    chans, b, h, w, cout = (128, 64, 8), 2, 20, 44, 96
    srcs = [rand(b, c, h, w, seed=c).cuda() for c in chans]
    g = rand(b, cout, h, w, seed=2).cuda()
    a = conv2d_cat_weight_grad(srcs, g, 3)
    assert torch.equal(a, conv2d_cat_weight_grad(srcs, g, 3))
    lib = _lib.load()
    arr = (ctypes.c_int * 3)(*chans)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in srcs])
    n = lib.dv_conv2d_wgrad_cat_workspace_floats(arr, 3, b, h, w, cout, 3)
    ws = torch.full((n,), float("nan"), device="cuda")                # stale contents must not leak into the result
    for _ in range(2):
        dw = torch.empty(cout, sum(chans), 3, 3, device="cuda")
        _lib.check(lib.dv_conv2d_wgrad_cat_f32(ptrs, arr, 3, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, h, w, cout, 3,
                                               _lib.stream_ptr()), "dv_conv2d_wgrad_cat_f32")
        torch.cuda.synchronize()
        assert torch.equal(dw, a)


def test_split_plan_depends_on_the_batch():
    """Not batch-independent (see the module docstring): the split count moves with B, and the two halves' gradients
    add up to the batch's within the bound of the three sums involved, not bit for bit."""
    assert splits_of((128, 128), 1, 5, 7, 128, 3) < splits_of((128, 128), 4, 5, 7, 128, 3)
    srcs = [rand(4, c, 10, 14, seed=c) for c in (128, 128)]
    g = rand(4, 128, 10, 14, seed=9)
    full = check(srcs, g, 3)
    halves = check([t[:2] for t in srcs], g[:2], 3) + check([t[2:] for t in srcs], g[2:], 3)
    mag = ref_wgrad(torch.cat(srcs, 1).double().abs(), g.double().abs(), 3)
    c = depth_c((128, 128), 4, 10, 14, 128, 3) + 2 * depth_c((128, 128), 2, 10, 14, 128, 3)
    assert torch.all((full - halves).abs() <= c * U * mag)


def test_nan_stays_in_its_source_channel():
    srcs = [rand(2, 24, 12, 40, seed=5), rand(2, 16, 12, 40, seed=6)]
    g = rand(2, 32, 12, 40, seed=7)
    srcs[1][1, 3, 3, 7] = float("nan")                                 # channel 27 of the concatenation
    dw = conv2d_cat_weight_grad([t.cuda() for t in srcs], g.cuda(), 3).cpu()
    nan = torch.isnan(dw)
    assert nan[:, 27].any() and not nan[:, :27].any() and not nan[:, 28:].any()


def test_refusals():
    x, g = rand(1, 8, 4, 4, seed=1).cuda(), rand(1, 8, 4, 4, seed=2).cuda()
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x] * 5, g, 3)
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x], g, 5)
    with pytest.raises(_lib.DiffuVolumeError):
        conv2d_cat_weight_grad([x.cpu()], g, 3)


@pytest.mark.parametrize("k,cout,b,h,w", [(7, 64, 2, 20, 28), (7, 64, 1, 5, 7), (7, 5, 3, 9, 33), (7, 3, 1, 2, 3)])
def test_single_input_channel_weight_gradient(k, cout, b, h, w):
    """dv_conv2d_1in_wgrad_f32 (convd1): each of the block's 256 threads adds ceil(BHW / 256) products in one chain, then
    an 8-level tree: c = ceil(BHW / 256) + 8.  Two launches give the same bits."""
    x, g = rand(b, 1, h, w, seed=k + h), rand(b, cout, h, w, seed=cout + w)
    lib = _lib.load()
    outs = []
    for _ in range(2):
        dw = torch.full((cout, 1, k, k), float("nan"), device="cuda")
        xc, gc = x.cuda(), g.cuda()
        _lib.check(lib.dv_conv2d_1in_wgrad_f32(xc.data_ptr(), gc.data_ptr(), dw.data_ptr(), b, h, w, cout, k,
                                               _lib.stream_ptr()), "dv_conv2d_1in_wgrad_f32")
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    ref = torch.nn.grad.conv2d_weight(x.double(), (cout, 1, k, k), g.double(), padding=k // 2)
    mag = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 1, k, k), g.double().abs(), padding=k // 2)
    c = -(-b * h * w // 256) + 8
    assert torch.all((outs[0].double() - ref).abs() <= c * U * mag)
