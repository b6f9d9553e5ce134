"""The fp16-autocast 2-D convolution of IGEV's update block (csrc/conv2d_f16.hip, `Conv2dF16Plan`) against a float64
emulation of the rounding contract: operands rounded to fp16, exact products and sums, the output and every epilogue op
rounded to fp16.

Bars.  The contract fixes the rounding points and leaves the arithmetic order free, so the kernel's fp32 accumulator may
land on the other side of a rounding boundary now and then.  Each element gets the forward error bound of that freedom:
the accumulator's own rounding (2^-20 * sum |x * w|, 16 fp32 ulps of the operand scale), then one fp16 ulp per rounding
point, carried through every later op by its derivative (sigmoid' <= 1/4, tanh' <= 1, the `mul` / blend factors).  A plain
convolution (+ bias + ReLU) is thus held to 1 fp16 ulp plus the accumulator term.  Every element must be inside its bound,
at most 2 % of the elements may differ from the emulation at all, and reruns and batch shards are bit-identical."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = {"none": S.ACT_NONE, "relu": S.ACT_RELU, "sigmoid": S.ACT_SIGMOID, "tanh": S.ACT_TANH}


def r16(t):
    """fp16 rounding (round to nearest even) of a float64 tensor, back as float64 (via fp32: the kernel's accumulator)."""
    return t.float().half().double()


def ulp16(t):
    """fp16 ulp of |t| (subnormal spacing 2^-24 below 2^-14)."""
    e = torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def emulate(parts, w, b, act, residual=None, mul=None, blend=None):
    """-> (the contract's result, the per-element bound on |kernel - result| the free accumulation order allows)"""
    x = r16(torch.cat([p.cpu().double() for p in parts], 1))
    wr = r16(w.cpu().double())
    y = F.conv2d(x, wr, None, padding=w.shape[-1] // 2)
    bound = F.conv2d(x.abs(), wr.abs(), None, padding=w.shape[-1] // 2)
    if b is not None:
        y = y + r16(b.cpu().double())[None, :, None, None]
        bound = bound + r16(b.cpu().double()).abs()[None, :, None, None]
    bound = bound * 2.0 ** -20
    y = r16(y)
    bound = bound + ulp16(y)
    if residual is not None:
        y = r16(y + residual.cpu().double())
        bound = bound + ulp16(y)
    if act == "relu":
        y = y.clamp(min=0)
    elif act == "sigmoid":
        s = torch.sigmoid(y)
        y = r16(s)
        bound = bound * (s * (1 - s)).clamp(min=0) + ulp16(y)
    elif act == "tanh":
        t = torch.tanh(y)
        y = r16(t)
        bound = bound * (1 - t * t).clamp(min=0) + ulp16(y)
    if mul is not None:
        y = r16(y * mul.cpu().double())
        bound = bound * mul.cpu().double().abs() + ulp16(y)
    if blend is not None:
        z, h = blend[0].cpu().double(), blend[1].cpu().double()
        a, c = r16(r16(1 - z) * h), r16(z * y)
        y = r16(a + c)
        bound = bound * z.abs() + ulp16(c) + ulp16(y)
    return y, bound


def check(out, emu):
    ref, bound = emu
    out = out.cpu().double()
    assert torch.equal(out, r16(out)), "the outputs must be fp16-exact values"
    excess = float(((out - ref).abs() - bound).max())
    differ = float((out != ref).double().mean())
    print(f"  differ {differ:.2e}, max |out - ref| - bound {excess:.2e}")
    assert excess <= 0 and differ <= 0.02, (excess, differ)
    return differ


def fp16_vals(t):
    return t.half().float()


def rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


SHAPES = [(1, 96, 312), (4, 96, 312), (1, 48, 156), (4, 24, 78), (2, 11, 70), (1, 5, 3)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("act", list(ACTS))
def test_plain_conv_bias_act(shape, k, act):
    b, h, w = shape
    g = _gen(301, f"{shape}{k}{act}")
    cin, cout = (162, 64) if k == 1 else (96, 128)
    x = rand(g, b, cin, h, w)
    wt, bias = rand(g, cout, cin, k, k, scale=(cin * k * k) ** -0.5), rand(g, cout, scale=0.1)
    plan = S.Conv2dF16Plan(wt.to(DEV), bias.to(DEV), act=ACTS[act])
    out = plan(x.to(DEV))
    check(out, emulate([x], wt, bias, act))
    assert torch.equal(plan(x.to(DEV)), out)                                  # rerun: same bits


@pytest.mark.parametrize("chans", [(128,), (127, 1), (128, 128, 128), (64, 64), (5, 27, 33, 63), (1, 31, 97, 2),
                                   (9,), (40, 1, 7)])
@pytest.mark.parametrize("k", [1, 3])
def test_virtual_concatenation_sources(chans, k):
    """1..4 sources with channel counts that are not multiples of the 32-channel chunk (127 + 1: the motion features)."""
    g = _gen(302, f"{chans}{k}")
    b, h, w = 2, 13, 70
    parts = [rand(g, b, c, h, w) for c in chans]
    cin, cout = sum(chans), 64
    wt, bias = rand(g, cout, cin, k, k, scale=(cin * k * k) ** -0.5), rand(g, cout, scale=0.1)
    plan = S.Conv2dF16Plan(wt.to(DEV), bias.to(DEV), act=S.ACT_RELU)
    check(plan([p.to(DEV) for p in parts]), emulate(parts, wt, bias, "relu"))


@pytest.mark.parametrize("cout", [1, 32, 127])
def test_narrow_outputs(cout):
    """disp_head.conv2 (1 channel), mask_feat_4 (32), the motion encoder's 127 (+1 zero) channels."""
    g = _gen(303, f"{cout}")
    x = rand(g, 2, 128, 24, 78)
    wt, bias = rand(g, cout, 128, 3, 3, scale=(128 * 9) ** -0.5), rand(g, cout, scale=0.1)
    plan = S.Conv2dF16Plan(wt.to(DEV), bias.to(DEV), act=S.ACT_NONE)
    check(plan(x.to(DEV)), emulate([x], wt, bias, "none"))


@pytest.mark.parametrize("shape", [(1, 96, 312), (4, 48, 156), (1, 24, 78), (4, 24, 78), (3, 7, 41)])
def test_gate_chains(shape):
    """The ConvGRU: z / r*h from the pair launch, then (1-z)*h + z*tanh(convq(.) + cq), fp16-valued h and context."""
    b, h, w = shape
    g = _gen(304, f"{shape}")
    cin = 384
    hx = [fp16_vals(rand(g, b, 128, h, w).tanh()), rand(g, b, 127, h, w), rand(g, b, 1, h, w) * 20,
          rand(g, b, 128, h, w)]
    hid = hx[0]
    cz, cr, cq = (fp16_vals(rand(g, b, 128, h, w, scale=0.5)) for _ in range(3))
    wz, wr, wq = (rand(g, 128, cin, 3, 3, scale=(cin * 9) ** -0.5) for _ in range(3))
    bz, br, bq = (rand(g, 128, scale=0.1) for _ in range(3))
    pair = S.Conv2dF16Plan(wz.to(DEV), bz.to(DEV), S.ACT_SIGMOID, pair=(wr.to(DEV), br.to(DEV)))
    d = [t.to(DEV) for t in hx]
    z, rh = pair(d, residual=(cz.to(DEV), cr.to(DEV)), mul=(None, hid.to(DEV)))
    z_ref = emulate(hx, wz, bz, "sigmoid", residual=cz)
    rh_ref = emulate(hx, wr, br, "sigmoid", residual=cr, mul=hid)
    check(z, z_ref)
    check(rh, rh_ref)
    # the candidate and the blend from the kernel's own z and r*h (rounding points, not the chain's first flips)
    q = S.Conv2dF16Plan(wq.to(DEV), bq.to(DEV), S.ACT_TANH)
    qx = [rh] + d[1:]
    hn = q(qx, residual=cq.to(DEV), blend=(z, hid.to(DEV)))
    check(hn, emulate([t.cpu() for t in qx], wq, bq, "tanh", residual=cq, blend=(z.cpu(), hid)))
    # batch 4 == four batch-1 shards, bit for bit (the launch shape choices look at one batch item)
    if b > 1:
        for i in range(b):
            zi, rhi = pair([t[i:i + 1] for t in d], residual=(cz[i:i + 1].to(DEV), cr[i:i + 1].to(DEV)),
                           mul=(None, hid[i:i + 1].to(DEV)))
            assert torch.equal(zi, z[i:i + 1]) and torch.equal(rhi, rh[i:i + 1])


def test_ksplit_small_launches(monkeypatch):
    """The 1/16- and 1/8-scale launches K-split (the factor depends on one batch item); both forms meet the bars."""
    lib = _lib.load()
    assert lib.dv_conv2d_f16_auto_kslices(256, 24, 78, 256, 3) > 1
    assert lib.dv_conv2d_f16_auto_kslices(384, 96, 312, 256, 3) == 1
    g = _gen(305, "ks")
    x = rand(g, 4, 256, 24, 78)
    wt, bias = rand(g, 128, 256, 3, 3, scale=(256 * 9) ** -0.5), rand(g, 128, scale=0.1)
    res = fp16_vals(rand(g, 4, 128, 24, 78))
    plan = S.Conv2dF16Plan(wt.to(DEV), bias.to(DEV), S.ACT_TANH)
    ref = emulate([x], wt, bias, "tanh", residual=res)
    split = plan(x.to(DEV), residual=res.to(DEV))
    check(split, ref)
    for i in range(4):
        assert torch.equal(plan(x[i:i + 1].to(DEV), residual=res[i:i + 1].to(DEV)), split[i:i + 1])
    monkeypatch.setattr(S.Conv2dF16Plan, "KSPLIT", False)
    check(plan(x.to(DEV), residual=res.to(DEV)), ref)


def test_abi_rejects_bad_arguments():
    lib = _lib.load()
    assert lib.dv_conv2d_f16_packed_bytes(384, 256, 3) == 12 * 9 * 16 * 512 * 2
    assert lib.dv_conv2d_f16_packed_bytes(384, 256, 5) == 0
    import ctypes
    ptrs = (ctypes.c_void_p * 1)(0)
    chans = (ctypes.c_int * 1)(8)
    assert lib.dv_conv2d_f16_cat(ptrs, chans, 1, 0, 0, 0, 0, 0, 0, 0, 1, 4, 4, 8, 3, 0, 0) == -1   # DV_ERR_NULL
