"""dv_conv3d_wgrad_f16_f32 (csrc/conv3d_wgrad_f16.hip): the weight gradient of the 3x3x3 stride-1 convolutions at train
precision "f16".

Exact contract: dW = sum r16(g) * r16(x) with fp32 accumulation and an unrounded float32 dW, so the reference is the
float64 weight gradient of ``x.half().double()`` and ``g.half().double()`` on the CPU and the only difference is the fp32
accumulation order.  Bar, per element (the one of tests/test_gpu_conv2d_wgrad_cat_f16.py):
    |dW - dW_f64| <= c * 2^-24 * sum |g x|,   c = ceil(bricks / S) * TZ * TY * TX + S
(every product passes through at most one rounding per position of its split and one per split; the order inside a matrix
instruction is covered by the same count), the brick being 2 x 2 x 32 positions and S what the workspace query implies.
(Measured: the worst ratio is at most 1.9 against c = 129 .. 284 on the shapes here, the relative L2 error at most 1.2e-7.)"""
import pytest
import torch
import torch.nn.functional as F

import arena as A
from diffuvolume_amd import _lib, train3d

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TZ, TY, TX = 2, 2, 32                 # the kernel's output brick


def r16(t):
    return t.half().float()


def rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ref_wgrad(x64, g64):
    """dW[co,ci,t] = sum_{b,o} g[b,co,o] x[b,ci,o+t-1]: a convolution of x (channels as batch) with g as its kernel."""
    return F.conv3d(x64.transpose(0, 1), g64.transpose(0, 1), padding=1).transpose(0, 1).contiguous()


def plan_of(b, cin, d, h, w, cout):
    n = _lib.load().dv_conv3d_wgrad_f16_workspace_floats(b, cin, d, h, w, cout)
    assert n > 0 and n % (cout * cin * 27) == 0 and n * 4 <= 48 << 20
    nbricks = b * -(-d // TZ) * -(-h // TY) * -(-w // TX)
    return nbricks, n // (cout * cin * 27)


def depth_c(b, cin, d, h, w, cout):
    nbricks, s = plan_of(b, cin, d, h, w, cout)
    return -(-nbricks // s) * TZ * TY * TX + s


def check(x, g):
    dw = train3d.conv3d_weight_grad_f16(x.cuda(), g.cuda())
    assert dw.dtype == torch.float32
    dw = dw.cpu().double()
    x64, g64 = r16(x).double(), r16(g).double()
    ref, mag = ref_wgrad(x64, g64), ref_wgrad(x64.abs(), g64.abs())
    assert dw.shape == ref.shape == (g.shape[1], x.shape[1], 3, 3, 3)
    c = depth_c(*x.shape, g.shape[1])
    err = (dw - ref).abs()
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"WGRAD3D16 {tuple(x.shape)} -> {g.shape[1]}: worst {worst:.2f} of c = {c}, relative L2 {rel:.2e}, "
          f"(bricks, splits) = {plan_of(*x.shape, g.shape[1])}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return dw


SHAPES = [  # (B, Cin, Cout, D, H, W)
    (2, 40, 32, 3, 5, 50),        # the real layers at tiny planes
    (1, 32, 32, 2, 4, 48),
    (1, 64, 32, 1, 1, 1),
    (2, 64, 64, 4, 6, 20),
    (1, 128, 128, 2, 3, 8),
    (1, 5, 7, 2, 3, 17),          # channel tails
    (1, 32, 33, 2, 2, 16),
    (2, 65, 5, 3, 3, 33),
    (1, 8, 8, 2, 2, 32),          # exactly one brick, one split
    (1, 8, 8, 2, 2, 64),          # two bricks
    (3, 128, 128, 4, 6, 33),      # 36 bricks in 28 splits: a ragged split range
]


@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_shapes(b, cin, cout, d, h, w):
    check(rand(b, cin, d, h, w, seed=cin + w), rand(b, cout, d, h, w, seed=cout + 3 * h))


def test_the_plans_the_shapes_are_there_for():
    assert plan_of(1, 8, 2, 2, 32, 8) == (1, 1)
    assert plan_of(1, 8, 2, 2, 64, 8) == (2, 2)
    nbricks, s = plan_of(3, 128, 4, 6, 33, 128)
    assert (nbricks, s) == (36, 28) and nbricks % s              # 32 wanted, 28 within the 48 MB workspace bound


def test_outputs_written_fully_and_nowhere_else_and_the_same_bits_on_every_launch():
    b, cin, d, h, w, cout = 2, 40, 3, 5, 50, 33
    x, g = rand(b, cin, d, h, w, seed=1).cuda(), rand(b, cout, d, h, w, seed=2).cuda()
    first = train3d.conv3d_weight_grad_f16(x, g)
    assert torch.isfinite(first).all()
    lib = _lib.load()
    n = lib.dv_conv3d_wgrad_f16_workspace_floats(b, cin, d, h, w, cout)
    for offset in (0, 1):
        dw = A.place(torch.empty(cout, cin, 3, 3, 3), offset, kind="out", device="cuda", name="dw")
        ws = A.place(torch.empty(n), offset, kind="out", device="cuda", name="workspace")   # stale contents: NaN
        for _ in range(2):
            _lib.check(lib.dv_conv3d_wgrad_f16_f32(x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, d, h, w,
                                                   cout, _lib.stream_ptr()), "dv_conv3d_wgrad_f16_f32")
            torch.cuda.synchronize()
            A.check_output(dw)
            A.check_output(ws)
            assert torch.equal(dw.view, first)


def test_overflow_of_the_gradient_stays_in_its_output_channel():
    x, g = rand(2, 24, 4, 6, 64, seed=5).cuda(), rand(2, 16, 4, 6, 64, seed=7).cuda()
    clean = train3d.conv3d_weight_grad_f16(x, g)
    g[1, 5, 2, 3, 7] = 1e6
    dw = train3d.conv3d_weight_grad_f16(x, g)
    assert torch.isfinite(clean).all() and not torch.isfinite(dw[5]).all()
    keep = [c for c in range(16) if c != 5]
    assert torch.equal(dw[keep], clean[keep])


def test_refusals():
    lib = _lib.load()
    assert lib.dv_conv3d_wgrad_f16_workspace_floats(0, 8, 2, 2, 8, 8) == 0
    assert lib.dv_conv3d_wgrad_f16_workspace_floats(1, 8, 2, -1, 8, 8) == 0
    assert lib.dv_conv3d_wgrad_f16_workspace_floats(1, 1024, 2, 2, 8, 1024) == 0      # one split beyond the 48 MB bound
    x = rand(1, 8, 2, 2, 8, seed=1).cuda()
    dw = A.place(torch.empty(8, 8, 3, 3, 3), kind="out", device="cuda", name="dw")
    ws = A.place(torch.empty(8 * 8 * 27), kind="out", device="cuda", name="workspace")
    s = _lib.stream_ptr()
    assert lib.dv_conv3d_wgrad_f16_f32(x.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 8, 0, 2, 8, 8, s) == -2
    assert lib.dv_conv3d_wgrad_f16_f32(x.data_ptr(), None, dw.data_ptr(), ws.data_ptr(), 1, 8, 2, 2, 8, 8, s) == -1
    torch.cuda.synchronize()
    A.check_untouched(dw)
    A.check_untouched(ws)
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.conv3d_weight_grad_f16(x, rand(1, 8, 2, 2, 9, seed=2).cuda())


def test_overflow_of_the_input_stays_in_its_input_channel():
    """One x beyond the fp16 range becomes Inf while it is staged: Inf / NaN in the entries of dW of that input channel
    (NaN also in taps whose exact sum does not hold the element, where it meets a staged 0 of g past the volume's edge --
    the departure from the exact sum that include/diffuvolume_hip_amp3d.h states), every other input channel as without
    it.  The volume is no multiple of the brick and the element sits next to its far edge."""
    x, g = rand(2, 24, 3, 5, 50, seed=8).cuda(), rand(2, 16, 3, 5, 50, seed=9).cuda()
    clean = train3d.conv3d_weight_grad_f16(x, g)
    x[1, 7, 2, 4, 49] = 1e6
    dw = train3d.conv3d_weight_grad_f16(x, g)
    assert torch.isfinite(clean).all() and not torch.isfinite(dw[:, 7]).all()
    keep = [c for c in range(24) if c != 7]
    assert torch.equal(dw[:, keep], clean[:, keep])
