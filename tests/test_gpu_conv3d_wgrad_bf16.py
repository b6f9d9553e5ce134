"""dv_conv3d_wgrad_bf16_f32 (csrc/conv3d_wgrad_bf16.hip, the bf16 instantiation of csrc/conv3d_wgrad_mp.h): the weight
gradient of the 3x3x3 stride-1 convolutions at train precision "bf16".  tests/test_gpu_conv3d_wgrad_f16.py restated with
``rb16 = t.bfloat16().float()``; its shape list is used as it is.

Exact contract: dW = sum rb16(g) * rb16(x) with fp32 accumulation and an unrounded float32 dW, so the reference is the
float64 weight gradient of ``x.bfloat16().double()`` and ``g.bfloat16().double()`` on the CPU and the only difference is the
fp32 accumulation order.  Bar, per element, the derived one of the fp16 test unchanged (same kernel body, same split plan):
    |dW - dW_f64| <= c * 2^-24 * sum |g x|,   c = ceil(bricks / S) * TZ * TY * TX + S
the brick being 2 x 2 x 32 positions and S what the workspace query implies.
(Measured: the worst ratio is at most 1.6 against c = 129 .. 284 on the shapes here, the relative L2 error at most 1.1e-7.)"""
import pytest
import torch

import arena as A
from diffuvolume_amd import _lib, train3d
from test_gpu_conv3d_wgrad_f16 import SHAPES, TX, TY, TZ, U, rand, ref_wgrad

pytestmark = pytest.mark.gpu


def rb16(t):
    return t.bfloat16().float()


def plan_of(b, cin, d, h, w, cout):
    lib = _lib.load()
    n = lib.dv_conv3d_wgrad_bf16_workspace_floats(b, cin, d, h, w, cout)
    assert n == lib.dv_conv3d_wgrad_f16_workspace_floats(b, cin, d, h, w, cout)      # the same workspace plan
    assert n > 0 and n % (cout * cin * 27) == 0 and n * 4 <= 48 << 20
    nbricks = b * -(-d // TZ) * -(-h // TY) * -(-w // TX)
    return nbricks, n // (cout * cin * 27)


def depth_c(b, cin, d, h, w, cout):
    nbricks, s = plan_of(b, cin, d, h, w, cout)
    return -(-nbricks // s) * TZ * TY * TX + s


def check(x, g, what=""):
    dw = train3d.conv3d_weight_grad_bf16(x.cuda(), g.cuda())
    assert dw.dtype == torch.float32
    dw = dw.cpu().double()
    x64, g64 = rb16(x).double(), rb16(g).double()
    ref, mag = ref_wgrad(x64, g64), ref_wgrad(x64.abs(), g64.abs())
    assert dw.shape == ref.shape == (g.shape[1], x.shape[1], 3, 3, 3)
    c = depth_c(*x.shape, g.shape[1])
    err = (dw - ref).abs()
    worst = float((err / (mag * U).clamp_min(1e-300)).max())
    rel = float((dw - ref).norm() / ref.norm().clamp_min(1e-300))
    print(f"WGRAD3DBF16 {what}{tuple(x.shape)} -> {g.shape[1]}: worst {worst:.2f} of c = {c}, relative L2 {rel:.2e}, "
          f"(bricks, splits) = {plan_of(*x.shape, g.shape[1])}")
    assert torch.all(err <= c * U * mag), (worst, c)
    return dw


@pytest.mark.parametrize("b,cin,cout,d,h,w", SHAPES)
def test_shapes(b, cin, cout, d, h, w):
    check(rand(b, cin, d, h, w, seed=cin + w), rand(b, cout, d, h, w, seed=cout + 3 * h))


def test_the_plans_the_shapes_are_there_for():
    assert (2, 65, 5, 3, 3, 33) in SHAPES                          # the Cin 65 tail
    assert plan_of(1, 8, 2, 2, 32, 8) == (1, 1)
    assert plan_of(1, 8, 2, 2, 64, 8) == (2, 2)
    nbricks, s = plan_of(3, 128, 4, 6, 33, 128)
    assert (nbricks, s) == (36, 28) and nbricks % s              # 32 wanted, 28 within the 48 MB workspace bound


def test_outputs_written_fully_and_nowhere_else_and_the_same_bits_on_every_launch():
    b, cin, d, h, w, cout = 2, 40, 3, 5, 50, 33
    x, g = rand(b, cin, d, h, w, seed=1).cuda(), rand(b, cout, d, h, w, seed=2).cuda()
    first = train3d.conv3d_weight_grad_bf16(x, g)
    assert torch.isfinite(first).all()
    assert not torch.equal(first, train3d.conv3d_weight_grad_f16(x, g))     # another rounding than the fp16 entry's
    lib = _lib.load()
    n = lib.dv_conv3d_wgrad_bf16_workspace_floats(b, cin, d, h, w, cout)
    for offset in (0, 1):
        dw = A.place(torch.empty(cout, cin, 3, 3, 3), offset, kind="out", device="cuda", name="dw")
        ws = A.place(torch.empty(n), offset, kind="out", device="cuda", name="workspace")   # stale contents: NaN
        for _ in range(2):
            _lib.check(lib.dv_conv3d_wgrad_bf16_f32(x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, d, h, w,
                                                    cout, _lib.stream_ptr()), "dv_conv3d_wgrad_bf16_f32")
            torch.cuda.synchronize()
            A.check_output(dw)
            A.check_output(ws)
            assert torch.equal(dw.view, first)


def test_a_batch_and_its_items_each_meet_the_bar_of_their_own_plan():
    """The split ranges run over the batch, so the bits of a batch are not those of its items; each item alone meets the
    bar of its own plan."""
    x, g = rand(2, 24, 3, 5, 50, seed=3), rand(2, 16, 3, 5, 50, seed=4)
    check(x, g, "batch ")
    for i in range(2):
        check(x[i:i + 1], g[i:i + 1], f"item {i} ")


def test_operands_beyond_the_fp16_range_stay_finite_at_bf16():
    """The point of the precision: x and g scaled so that entries pass 7e4.  Through the fp16 entry they are Inf and dW
    is not finite; through the bf16 entry every element is finite and within the bar."""
    x, g = rand(2, 24, 4, 6, 64, seed=5) * 3e4, rand(2, 16, 4, 6, 64, seed=7) * 3e4
    assert int((x.abs() > 7e4).sum()) > 10 and int((g.abs() > 7e4).sum()) > 10
    assert not torch.isfinite(train3d.conv3d_weight_grad_f16(x.cuda(), g.cuda())).all()
    assert torch.isfinite(check(x, g, "beyond fp16 ")).all()


def test_an_inf_of_the_gradient_stays_in_its_output_channel():
    """3.4e38 rounds to Inf while it is staged (1e6, which overflowed fp16, is an ordinary number here)."""
    x, g = rand(2, 24, 4, 6, 64, seed=5).cuda(), rand(2, 16, 4, 6, 64, seed=7).cuda()
    clean = train3d.conv3d_weight_grad_bf16(x, g)
    g[1, 5, 2, 3, 7] = 1e6
    assert torch.isfinite(train3d.conv3d_weight_grad_bf16(x, g)).all()
    g[1, 5, 2, 3, 7] = 3.4e38
    dw = train3d.conv3d_weight_grad_bf16(x, g)
    assert torch.isfinite(clean).all() and not torch.isfinite(dw[5]).all()
    keep = [c for c in range(16) if c != 5]
    assert torch.equal(dw[keep], clean[keep])


def test_refusals():
    lib = _lib.load()
    assert lib.dv_conv3d_wgrad_bf16_workspace_floats(0, 8, 2, 2, 8, 8) == 0
    assert lib.dv_conv3d_wgrad_bf16_workspace_floats(1, 8, 2, -1, 8, 8) == 0
    assert lib.dv_conv3d_wgrad_bf16_workspace_floats(1, 1024, 2, 2, 8, 1024) == 0     # one split beyond the 48 MB bound
    x = rand(1, 8, 2, 2, 8, seed=1).cuda()
    dw = A.place(torch.empty(8, 8, 3, 3, 3), kind="out", device="cuda", name="dw")
    ws = A.place(torch.empty(8 * 8 * 27), kind="out", device="cuda", name="workspace")
    s = _lib.stream_ptr()
    assert lib.dv_conv3d_wgrad_bf16_f32(x.data_ptr(), x.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1, 8, 0, 2, 8, 8, s) == -2
    assert lib.dv_conv3d_wgrad_bf16_f32(x.data_ptr(), None, dw.data_ptr(), ws.data_ptr(), 1, 8, 2, 2, 8, 8, s) == -1
    torch.cuda.synchronize()
    A.check_untouched(dw)
    A.check_untouched(ws)
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.conv3d_weight_grad_bf16(x, rand(1, 8, 2, 2, 9, seed=2).cuda())


def test_an_inf_of_the_input_stays_in_its_input_channel():
    """One x that rounds to Inf while it is staged: Inf / NaN in the entries of dW of that input channel (NaN also in taps
    whose exact sum does not hold the element, where it meets a staged 0 of g past the volume's edge -- the departure
    from the exact sum that include/diffuvolume_hip_amp3d_bf16.h states, as at fp16), every other input channel as
    without it.  The volume is no multiple of the brick and the element sits next to its far edge."""
    x, g = rand(2, 24, 3, 5, 50, seed=8).cuda(), rand(2, 16, 3, 5, 50, seed=9).cuda()
    clean = train3d.conv3d_weight_grad_bf16(x, g)
    x[1, 7, 2, 4, 49] = 3.4e38
    dw = train3d.conv3d_weight_grad_bf16(x, g)
    assert torch.isfinite(clean).all() and not torch.isfinite(dw[:, 7]).all()
    keep = [c for c in range(24) if c != 7]
    assert torch.equal(dw[:, keep], clean[:, keep])
