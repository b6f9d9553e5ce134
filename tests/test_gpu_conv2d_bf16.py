"""The bf16 2-D convolution of IGEV's update block at train precision "bf16" (csrc/conv2d_bf16.hip, the bf16 instantiation
of csrc/conv2d_mp.h; `Conv2dF16Plan(elem="bf16")`) and `dv_conv2d_1in_bf16`, against a float64 emulation of the rounding
contract: operands rounded to bfloat16, exact products and sums, the output and every epilogue op rounded to bfloat16.
The method is tests/test_gpu_conv2d_f16.py's with a bf16 ulp, 2^(e-7) with the floor 2^-126 (the contract claims nothing
about bf16 subnormals).

Bars.  The contract fixes the rounding points and leaves the arithmetic order free, so the kernel's fp32 accumulator may
land on the other side of a rounding boundary now and then.  Each element gets the forward error bound of that freedom:
the accumulator's own rounding (2^-20 * sum |x * w|), then one bf16 ulp per rounding point, carried through every later
op by its derivative (sigmoid' <= 1/4, tanh' <= 1, the `mul` / blend factors).  Every element must be inside its bound,
outputs are bf16-exact float32, reruns and batch shards are bit-identical, and at most 0.5 % of the elements may differ from
the emulation at all: a float32 CPU convolution of the same rounded operands differs from the float64 emulation in 1.4e-4
of the elements at [2,96,13,70] -> 128 k3, [2,162,13,70] -> 64 k1 and [1,384,24,78] -> 128 k3 (randn inputs, weights
scaled by fan-in^-1/2), so flips of that kind are rare and 0.5 % leaves room for the longer chains only."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = {"none": S.ACT_NONE, "relu": S.ACT_RELU, "sigmoid": S.ACT_SIGMOID, "tanh": S.ACT_TANH}
DIFFER = 0.005


def rb16(t):
    """bfloat16 rounding (round to nearest even) of a float64 tensor, back as float64 (via fp32: the kernel's accumulator)."""
    return t.float().bfloat16().double()


def ulpb16(t):
    """bf16 ulp of |t|: 2^(e - 7), floor 2^-126."""
    e = torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -119)))
    return torch.pow(2.0, e - 7)


def emulate(parts, w, b, act, residual=None, mul=None, blend=None):
    """-> (the contract's result, the per-element bound on |kernel - result| the free accumulation order allows)"""
    x = rb16(torch.cat([p.cpu().double() for p in parts], 1))
    wr = rb16(w.cpu().double())
    y = F.conv2d(x, wr, None, padding=w.shape[-1] // 2)
    bound = F.conv2d(x.abs(), wr.abs(), None, padding=w.shape[-1] // 2)
    if b is not None:
        y = y + rb16(b.cpu().double())[None, :, None, None]
        bound = bound + rb16(b.cpu().double()).abs()[None, :, None, None]
    bound = bound * 2.0 ** -20
    y = rb16(y)
    bound = bound + ulpb16(y)
    if residual is not None:
        y = rb16(y + residual.cpu().double())
        bound = bound + ulpb16(y)
    if act == "relu":
        y = y.clamp(min=0)
    elif act == "sigmoid":
        s = torch.sigmoid(y)
        y = rb16(s)
        bound = bound * (s * (1 - s)).clamp(min=0) + ulpb16(y)
    elif act == "tanh":
        t = torch.tanh(y)
        y = rb16(t)
        bound = bound * (1 - t * t).clamp(min=0) + ulpb16(y)
    if mul is not None:
        y = rb16(y * mul.cpu().double())
        bound = bound * mul.cpu().double().abs() + ulpb16(y)
    if blend is not None:
        z, h = blend[0].cpu().double(), blend[1].cpu().double()
        a, c = rb16(rb16(1 - z) * h), rb16(z * y)
        y = rb16(a + c)
        bound = bound * z.abs() + ulpb16(c) + ulpb16(y)
    return y, bound


def check(out, emu):
    ref, bound = emu
    assert out.dtype == torch.float32
    out = out.cpu().double()
    assert torch.equal(out, rb16(out)), "the outputs must be bf16-exact values"
    excess = float(((out - ref).abs() - bound).max())
    differ = float((out != ref).double().mean())
    print(f"  differ {differ:.2e}, max |out - ref| - bound {excess:.2e}")
    assert excess <= 0 and differ <= DIFFER, (excess, differ)
    return differ


def bf16_vals(t):
    return t.bfloat16().float()


def rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def plan_bf16(w, b, act, pair=None):
    return S.Conv2dF16Plan(w.to(DEV), None if b is None else b.to(DEV), act, pair=pair, elem="bf16")


@pytest.mark.parametrize("shape", [(2, 11, 70), (1, 5, 3), (4, 24, 78)])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("act", list(ACTS))
def test_plain_conv_bias_act(shape, k, act):
    b, h, w = shape
    g = _gen(401, f"{shape}{k}{act}")
    cin, cout = (162, 64) if k == 1 else (96, 128)
    x = rand(g, b, cin, h, w)
    wt, bias = rand(g, cout, cin, k, k, scale=(cin * k * k) ** -0.5), rand(g, cout, scale=0.1)
    plan = plan_bf16(wt, bias, ACTS[act])
    out = plan(x.to(DEV))
    check(out, emulate([x], wt, bias, act))
    assert torch.equal(plan(x.to(DEV)), out)                                  # rerun: same bits
    if b > 1:                                                                 # a shard has the batch's bits
        assert torch.equal(plan(x[1:2].to(DEV)), out[1:2])


def test_the_fp16_plan_is_another_kernel():
    """The default element type stays fp16: the same weights and input give other bits, each exact in its own format."""
    g = _gen(402, "elem")
    x, wt = rand(g, 1, 32, 5, 9), rand(g, 16, 32, 3, 3, scale=0.06)
    o16, ob = S.Conv2dF16Plan(wt.to(DEV), None)(x.to(DEV)), plan_bf16(wt, None, S.ACT_NONE)(x.to(DEV))
    assert S.Conv2dF16Plan(wt.to(DEV), None).elem == "f16"
    assert torch.equal(o16, o16.half().float()) and torch.equal(ob, bf16_vals(ob)) and not torch.equal(o16, ob)
    with pytest.raises(ValueError):
        S.Conv2dF16Plan(wt.to(DEV), None, elem="f32")


@pytest.mark.parametrize("chans", [(127, 1), (5, 27, 33, 63), (1, 31, 97, 2), (9,)])
@pytest.mark.parametrize("k", [1, 3])
def test_virtual_concatenation_sources(chans, k):
    """1..4 sources with channel counts that are not multiples of the 32-channel chunk (127 + 1: the motion features)."""
    g = _gen(403, f"{chans}{k}")
    b, h, w = 2, 13, 70
    parts = [rand(g, b, c, h, w) for c in chans]
    cin, cout = sum(chans), 64
    wt, bias = rand(g, cout, cin, k, k, scale=(cin * k * k) ** -0.5), rand(g, cout, scale=0.1)
    check(plan_bf16(wt, bias, S.ACT_RELU)([p.to(DEV) for p in parts]), emulate(parts, wt, bias, "relu"))


@pytest.mark.parametrize("cout", [1, 32, 127])
def test_narrow_outputs(cout):
    """disp_head.conv2 (1 channel), mask_feat_4 (32), the motion encoder's 127 channels."""
    g = _gen(404, f"{cout}")
    x = rand(g, 2, 128, 11, 70)
    wt, bias = rand(g, cout, 128, 3, 3, scale=(128 * 9) ** -0.5), rand(g, cout, scale=0.1)
    check(plan_bf16(wt, bias, S.ACT_NONE)(x.to(DEV)), emulate([x], wt, bias, "none"))


@pytest.mark.parametrize("shape", [(3, 7, 41), (1, 24, 78)])
def test_gate_chains(shape):
    """The ConvGRU: z / r*h from the pair launch, then (1-z)*h + z*tanh(convq(.) + cq), bf16-valued h and context."""
    b, h, w = shape
    g = _gen(405, f"{shape}")
    cin = 384
    hx = [bf16_vals(rand(g, b, 128, h, w).tanh()), rand(g, b, 127, h, w), rand(g, b, 1, h, w) * 20,
          rand(g, b, 128, h, w)]
    hid = hx[0]
    cz, cr, cq = (bf16_vals(rand(g, b, 128, h, w, scale=0.5)) for _ in range(3))
    wz, wr, wq = (rand(g, 128, cin, 3, 3, scale=(cin * 9) ** -0.5) for _ in range(3))
    bz, br, bq = (rand(g, 128, scale=0.1) for _ in range(3))
    pair = plan_bf16(wz, bz, S.ACT_SIGMOID, pair=(wr.to(DEV), br.to(DEV)))
    d = [t.to(DEV) for t in hx]
    z, rh = pair(d, residual=(cz.to(DEV), cr.to(DEV)), mul=(None, hid.to(DEV)))
    check(z, emulate(hx, wz, bz, "sigmoid", residual=cz))
    check(rh, emulate(hx, wr, br, "sigmoid", residual=cr, mul=hid))
    # the candidate and the blend from the kernel's own z and r*h (rounding points, not the chain's first flips)
    q = plan_bf16(wq, bq, S.ACT_TANH)
    qx = [rh] + d[1:]
    hn = q(qx, residual=cq.to(DEV), blend=(z, hid.to(DEV)))
    check(hn, emulate([t.cpu() for t in qx], wq, bq, "tanh", residual=cq, blend=(z.cpu(), hid)))
    if b > 1:                                       # batch 3 == three batch-1 shards, bit for bit
        for i in range(b):
            zi, rhi = pair([t[i:i + 1] for t in d], residual=(cz[i:i + 1].to(DEV), cr[i:i + 1].to(DEV)),
                           mul=(None, hid[i:i + 1].to(DEV)))
            assert torch.equal(zi, z[i:i + 1]) and torch.equal(rhi, rh[i:i + 1])


def test_ksplit_small_launches(monkeypatch):
    """The 1/16- and 1/8-scale launches K-split (the fp16 entry's choice serves both element types); both forms meet the
    bars."""
    assert _lib.load().dv_conv2d_f16_auto_kslices(256, 24, 78, 128, 3) > 1
    g = _gen(406, "ks")
    x = rand(g, 4, 256, 24, 78)
    wt, bias = rand(g, 128, 256, 3, 3, scale=(256 * 9) ** -0.5), rand(g, 128, scale=0.1)
    res = bf16_vals(rand(g, 4, 128, 24, 78))
    plan = plan_bf16(wt, bias, S.ACT_TANH)
    ref = emulate([x], wt, bias, "tanh", residual=res)
    split = plan(x.to(DEV), residual=res.to(DEV))
    check(split, ref)
    for i in (0, 3):
        assert torch.equal(plan(x[i:i + 1].to(DEV), residual=res[i:i + 1].to(DEV)), split[i:i + 1])
    monkeypatch.setattr(S.Conv2dF16Plan, "KSPLIT", False)
    check(plan(x.to(DEV), residual=res.to(DEV)), ref)


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_conv2d_1in_bf16(act):
    """The one-input-channel kernel with the other rounding function: the same emulation (operands and bias rounded, exact
    sums, the output rounded before the activation, a tanh result rounded again)."""
    g = _gen(407, act)
    b, h, w, cout = 2, 11, 70, 64
    x, wt, bias = rand(g, b, 1, h, w), rand(g, cout, 1, 3, 3, scale=1 / 3), rand(g, cout, scale=0.1)
    xd, wd, bd = x.to(DEV), wt.to(DEV), bias.to(DEV)
    out = torch.full((b, cout, h, w), float("nan"), device=DEV)
    _lib.launch("dv_conv2d_1in_bf16", xd.device, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), b, h, w, cout,
                3, ACTS[act])
    check(out, emulate([x], wt, bias, act))
