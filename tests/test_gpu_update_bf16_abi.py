"""The pointer, bounds and stream contract of the launching entries of the sixth ABI table
(include/diffuvolume_hip_amp2d_bf16.h, ``_lib.AMP2D_BF16_SIGNATURES``): the bf16 convolutions of IGEV's update block over a
virtual concatenation (single and pair launch, each with its K-split form), dv_conv2d_1in_bf16, the two bf16 gate entries
and dv_conv2d_wgrad_cat_bf16.  The method is tests/test_gpu_amp3d_bf16_abi.py's (the fifth table), whose gate helper is
used as it is.

Pointer and bounds (tests/arena.py): every float operand is a view into a guard-banded buffer at each ``data_ptr() % 16``
in {0, 4, 8, 12}; inputs sit between NaN, outputs -- scratch and workspace included -- are filled with a sentinel.  After
the call the guards are intact, every output element is written, no NaN leaked in, the result meets the bar of the entry's
own test and has the bits of the 16-byte aligned call.  Refused calls write nothing.  (The packed weight image is the
packer's output and keeps the 16-byte alignment the header asks for.)

Stream (tests/streams.py): the entry runs on a side stream that was seen to run independently of the null stream, behind
a gate kernel, with operands that only arrive behind the gate; the call must return while the gate still spins, and the
result must equal the default-stream run bit for bit."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import arena as A
import streams
from diffuvolume_amd import _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.plans import pack
from test_gpu_amp3d_abi import GATE_MS, gated
from test_gpu_conv2d_bf16 import bf16_vals, emulate
from test_gpu_conv2d_wgrad_cat import rand, ref_wgrad
from test_gpu_conv2d_wgrad_cat_bf16 import depth_c, rb16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
B, H, W = 2, 5, 11
CHANS = (40, 30)                                   # 70 channels: three 32-channel chunks, two K slices
KS = 2


def case_of(ins, outs, **more):
    return SimpleNamespace(**ins, ins=ins, outs=outs, **more)


def place(case, off, zeros=False):
    z = (lambda t: torch.zeros_like(t)) if zeros else (lambda t: t)
    ar = {n: A.place(z(t), off, "in", DEV, n) for n, t in case.ins.items()}
    ar.update({n: A.place(torch.empty(shape), off, "out", DEV, n) for n, shape in case.outs.items()})
    return ar


def host_arrays(ar, names, chans):
    return (ctypes.c_void_p * len(names))(*[ar[n].data_ptr() for n in names]), (ctypes.c_int * len(chans))(*chans)


def within(out, emu):
    ref, bound = emu
    out = out.double()
    assert torch.equal(out, rb16(out.float()).double()), "bf16-exact outputs"
    assert float(((out - ref).abs() - bound).max()) <= 0


def sweep(case, call, verdict, out):
    """The four placements: every one inside its bar and guards, all with the bits of the 16-byte aligned call."""
    aligned = None
    for off in range(4):
        ar = place(case, off)
        assert ar[out].data_ptr() % 16 == 4 * off
        assert call(case, ar, _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        y = verdict(case, ar)
        aligned = y if aligned is None else aligned
        assert torch.equal(y, aligned), f"offset {off}: other bits than the 16-byte aligned call"


# ------------------------------------------------------------------ dv_conv2d_bf16_cat / _cat_ksplit
def cat_case(ksplit):
    cout = 7
    ins = {"x0": rand(B, CHANS[0], H, W, seed=51), "x1": rand(B, CHANS[1], H, W, seed=52), "bias": rand(cout, seed=53) * 0.1,
           "res": bf16_vals(rand(B, cout, H, W, seed=54))}
    w = rand(cout, sum(CHANS), 3, 3, seed=55) * (sum(CHANS) * 9) ** -0.5
    outs = {"out": (B, cout, H, W)}
    if ksplit:
        outs["scratch"] = (KS * B * cout * H * W,)
    wpk = pack("dv_conv2d_f16_packed_bytes", "dv_conv2d_bf16_pack_weights", w.to(DEV), sum(CHANS), cout, 3, dtype=torch.uint8)
    return case_of(ins, outs, cout=cout, wpk=wpk, ksplit=ksplit,
                   emu=emulate([ins["x0"], ins["x1"]], w, ins["bias"], "tanh", residual=ins["res"]))


def cat_call(case, ar, stream, **o):
    names = o.get("names", ("x0", "x1"))
    ptrs, chans = host_arrays(ar, names, o.get("chans", CHANS))
    head = (o.get("ptrs", ptrs), chans, len(names), o.get("wpk", case.wpk.data_ptr()), ar["bias"].data_ptr(),
            ar["res"].data_ptr(), None, None, None, o.get("out", ar["out"].data_ptr()))
    tail = (o.get("b", B), H, o.get("w", W), case.cout, o.get("k", 3), o.get("act", S.ACT_TANH), stream)
    lib = _lib.load()
    if case.ksplit:
        return lib.dv_conv2d_bf16_cat_ksplit(*head, o.get("scratch", ar["scratch"].data_ptr()), o.get("ks", KS), *tail)
    return lib.dv_conv2d_bf16_cat(*head, *tail)


def cat_verdict(case, ar):
    for n in case.ins:
        A.check_guards(ar[n])
    for n in case.outs:
        A.check_output(ar[n])
    y = ar["out"].view.cpu()
    within(y, case.emu)
    return y


def test_conv2d_bf16_cat_abi_offset_views_bounds_and_refusals():
    """dv_conv2d_bf16_cat and dv_conv2d_bf16_cat_ksplit (scratch included), inside the forward test's bound."""
    for ksplit in (False, True):
        case = cat_case(ksplit)
        sweep(case, cat_call, cat_verdict, "out")
        ar = place(case, 1)
        s = _lib.stream_ptr()
        assert cat_call(case, ar, s, ptrs=None) == -1 and cat_call(case, ar, s, wpk=None) == -1
        assert cat_call(case, ar, s, out=None) == -1
        assert cat_call(case, ar, s, k=5) == -3 and cat_call(case, ar, s, act=7) == -3
        assert cat_call(case, ar, s, names=("x0", "x1", "x0", "x1", "x0"), chans=(8,) * 5) == -3      # five sources
        assert cat_call(case, ar, s, b=0) == -2 and cat_call(case, ar, s, w=-1) == -2
        assert cat_call(case, ar, s, chans=(40, 0)) == -2
        if ksplit:
            assert cat_call(case, ar, s, scratch=None) == -3 and cat_call(case, ar, s, ks=9) == -3
            assert cat_call(case, ar, s, ks=4) == -3                               # more slices than chunks
        torch.cuda.synchronize()
        for n in case.outs:
            A.check_untouched(ar[n])


# ------------------------------------------------------------------ dv_conv2d_bf16_cat_pair / _cat_pair_ksplit
C1, C2 = 7, 6


def pair_case(ksplit):
    ins = {"x0": rand(B, CHANS[0], H, W, seed=61), "x1": rand(B, CHANS[1], H, W, seed=62), "bias": rand(C1 + C2, seed=63) * 0.1,
           "res1": bf16_vals(rand(B, C1, H, W, seed=64)), "mul2": bf16_vals(rand(B, C2, H, W, seed=65).tanh())}
    w = rand(C1 + C2, sum(CHANS), 3, 3, seed=66) * (sum(CHANS) * 9) ** -0.5
    outs = {"out1": (B, C1, H, W), "out2": (B, C2, H, W)}
    if ksplit:
        outs["scratch"] = (KS * B * (C1 + C2) * H * W,)
    wpk = pack("dv_conv2d_f16_packed_bytes", "dv_conv2d_bf16_pack_weights", w.to(DEV), sum(CHANS), C1 + C2, 3, dtype=torch.uint8)
    xs = [ins["x0"], ins["x1"]]
    return case_of(ins, outs, wpk=wpk, ksplit=ksplit,
                   emu1=emulate(xs, w[:C1], ins["bias"][:C1], "sigmoid", residual=ins["res1"]),
                   emu2=emulate(xs, w[C1:], ins["bias"][C1:], "sigmoid", mul=ins["mul2"]))


def pair_call(case, ar, stream, **o):
    ptrs, chans = host_arrays(ar, ("x0", "x1"), CHANS)
    head = (ptrs, chans, o.get("n", 2), case.wpk.data_ptr(), ar["bias"].data_ptr(), ar["res1"].data_ptr(), None,
            o.get("out1", ar["out1"].data_ptr()), None, ar["mul2"].data_ptr(), o.get("out2", ar["out2"].data_ptr()))
    tail = (B, o.get("h", H), W, C1, o.get("c2", C2), o.get("act", S.ACT_SIGMOID), stream)
    lib = _lib.load()
    if case.ksplit:
        return lib.dv_conv2d_bf16_cat_pair_ksplit(*head, o.get("scratch", ar["scratch"].data_ptr()), o.get("ks", KS), *tail)
    return lib.dv_conv2d_bf16_cat_pair(*head, *tail)


def pair_verdict(case, ar):
    for n in case.ins:
        A.check_guards(ar[n])
    for n in case.outs:
        A.check_output(ar[n])
    y1, y2 = ar["out1"].view.cpu(), ar["out2"].view.cpu()
    within(y1, case.emu1)
    within(y2, case.emu2)
    return torch.cat([y1.flatten(), y2.flatten()])


def test_conv2d_bf16_pair_abi_offset_views_bounds_and_refusals():
    """dv_conv2d_bf16_cat_pair and dv_conv2d_bf16_cat_pair_ksplit: both heads written fully and nowhere else."""
    for ksplit in (False, True):
        case = pair_case(ksplit)
        sweep(case, pair_call, pair_verdict, "out1")
        ar = place(case, 2)
        s = _lib.stream_ptr()
        assert pair_call(case, ar, s, out1=None) == -1 and pair_call(case, ar, s, out2=None) == -1
        assert pair_call(case, ar, s, c2=0) == -2 and pair_call(case, ar, s, h=0) == -2
        assert pair_call(case, ar, s, n=5) == -3 and pair_call(case, ar, s, act=9) == -3
        if ksplit:
            assert pair_call(case, ar, s, ks=0) == -3 and pair_call(case, ar, s, scratch=None) == -3
        torch.cuda.synchronize()
        for n in case.outs:
            A.check_untouched(ar[n])


# ------------------------------------------------------------------ dv_conv2d_1in_bf16
def one_case():
    cout = 6
    ins = {"x": rand(B, 1, H, W, seed=71), "w": rand(cout, 1, 3, 3, seed=72) / 3, "bias": rand(cout, seed=73) * 0.1}
    return case_of(ins, {"out": (B, cout, H, W)}, cout=cout, emu=emulate([ins["x"]], ins["w"], ins["bias"], "relu"))


def one_call(case, ar, stream, **o):
    return _lib.load().dv_conv2d_1in_bf16(o.get("x", ar["x"].data_ptr()), ar["w"].data_ptr(), ar["bias"].data_ptr(),
                                          o.get("out", ar["out"].data_ptr()), o.get("b", B), H, W, o.get("cout", case.cout),
                                          o.get("k", 3), o.get("act", S.ACT_RELU), stream)


def one_verdict(case, ar):
    for n in case.ins:
        A.check_guards(ar[n])
    A.check_output(ar["out"])
    y = ar["out"].view.cpu()
    within(y, case.emu)
    return y


def test_conv2d_1in_bf16_abi_offset_views_bounds_and_refusals():
    case = one_case()
    sweep(case, one_call, one_verdict, "out")
    ar = place(case, 3)
    s = _lib.stream_ptr()
    assert one_call(case, ar, s, x=None) == -1 and one_call(case, ar, s, out=None) == -1
    assert one_call(case, ar, s, k=4) == -3 and one_call(case, ar, s, k=9) == -3 and one_call(case, ar, s, act=11) == -3
    assert one_call(case, ar, s, b=0) == -2 and one_call(case, ar, s, cout=0) == -2
    assert one_call(case, ar, s, cout=1 << 14) == -3                           # the weight set does not fit the LDS
    torch.cuda.synchronize()
    A.check_untouched(ar["out"])


# ------------------------------------------------------------------ dv_gru_reset_mul_bf16 / dv_gru_blend_bf16
N = 1027


def gate_case():
    mk = lambda f, seed: rb16(f(rand(N, seed=seed)))
    ins = {"z": mk(torch.sigmoid, 81), "r": mk(torch.sigmoid, 82), "q": mk(torch.tanh, 83), "h": mk(torch.tanh, 84)}
    Z, R, Q, Hh = (ins[n].bfloat16() for n in ("z", "r", "q", "h"))
    return case_of(ins, {"rh": (N,), "hn": (N,)}, rh_ref=(R * Hh).float(), hn_ref=((1 - Z) * Hh + Z * Q).float())


def gate_call(case, ar, stream, **o):
    lib, n = _lib.load(), o.get("n", N)
    rc = lib.dv_gru_reset_mul_bf16(o.get("r", ar["r"].data_ptr()), ar["h"].data_ptr(), o.get("rh", ar["rh"].data_ptr()), n, stream)
    return rc or lib.dv_gru_blend_bf16(ar["z"].data_ptr(), o.get("q", ar["q"].data_ptr()), ar["h"].data_ptr(),
                                       o.get("hn", ar["hn"].data_ptr()), n, stream)


def gate_verdict(case, ar):
    for n in case.ins:
        A.check_guards(ar[n])
    A.check_output(ar["rh"])
    A.check_output(ar["hn"])
    rh, hn = ar["rh"].view.cpu(), ar["hn"].view.cpu()
    assert torch.equal(rh, case.rh_ref) and torch.equal(hn, case.hn_ref)         # torch's bfloat16 arithmetic, bit for bit
    return torch.cat([rh, hn])


def test_gru_gates_bf16_abi_offset_views_bounds_and_refusals():
    """dv_gru_reset_mul_bf16 and dv_gru_blend_bf16: the float4 body (offset 0) and the scalar body (every other offset)."""
    case = gate_case()
    sweep(case, gate_call, gate_verdict, "rh")
    ar = place(case, 1)
    s = _lib.stream_ptr()
    lib = _lib.load()
    assert lib.dv_gru_reset_mul_bf16(None, ar["h"].data_ptr(), ar["rh"].data_ptr(), N, s) == -1
    assert lib.dv_gru_reset_mul_bf16(ar["r"].data_ptr(), ar["h"].data_ptr(), None, N, s) == -1
    assert lib.dv_gru_reset_mul_bf16(ar["r"].data_ptr(), ar["h"].data_ptr(), ar["rh"].data_ptr(), 0, s) == -2
    assert lib.dv_gru_blend_bf16(ar["z"].data_ptr(), None, ar["h"].data_ptr(), ar["hn"].data_ptr(), N, s) == -1
    assert lib.dv_gru_blend_bf16(ar["z"].data_ptr(), ar["q"].data_ptr(), ar["h"].data_ptr(), None, N, s) == -1
    assert lib.dv_gru_blend_bf16(ar["z"].data_ptr(), ar["q"].data_ptr(), ar["h"].data_ptr(), ar["hn"].data_ptr(), 0, s) == -2
    torch.cuda.synchronize()
    A.check_untouched(ar["rh"])
    A.check_untouched(ar["hn"])


# ------------------------------------------------------------------ dv_conv2d_wgrad_cat_bf16
WG = dict(chans=(5, 9), cout=7, b=2, h=5, w=35)


def wg_case():
    s = WG
    ins = {"x0": rand(s["b"], s["chans"][0], s["h"], s["w"], seed=91), "x1": rand(s["b"], s["chans"][1], s["h"], s["w"], seed=92),
           "g": rand(s["b"], s["cout"], s["h"], s["w"], seed=93)}
    x64, g64 = torch.cat([rb16(ins["x0"]), rb16(ins["x1"])], 1).double(), rb16(ins["g"]).double()
    arr = (ctypes.c_int * 2)(*s["chans"])
    n = _lib.load().dv_conv2d_wgrad_cat_bf16_workspace_floats(arr, 2, s["b"], s["h"], s["w"], s["cout"], 3)
    return case_of(ins, {"dw": (s["cout"], sum(s["chans"]), 3, 3), "ws": (n,)}, ref=ref_wgrad(x64, g64, 3),
                   mag=ref_wgrad(x64.abs(), g64.abs(), 3), c=depth_c(s["chans"], s["b"], s["h"], s["w"], s["cout"], 3))


def wg_call(case, ar, stream, **o):
    s = dict(WG, **{k: v for k, v in o.items() if k in WG})
    names = o.get("names", ("x0", "x1"))
    ptrs, chans = host_arrays(ar, names, s["chans"])
    return _lib.load().dv_conv2d_wgrad_cat_bf16(ptrs, chans, len(names), o.get("g", ar["g"].data_ptr()),
                                                o.get("dw", ar["dw"].data_ptr()), o.get("ws", ar["ws"].data_ptr()), s["b"],
                                                s["h"], s["w"], s["cout"], o.get("k", 3), stream)


def wg_verdict(case, ar):
    for n in case.ins:
        A.check_guards(ar[n])
    A.check_output(ar["dw"], case.ref)
    A.check_output(ar["ws"])
    dw = ar["dw"].view.cpu()
    assert torch.all((dw.double() - case.ref).abs() <= case.c * U * case.mag)
    return dw


def test_conv2d_wgrad_cat_bf16_abi_offset_views_bounds_and_refusals():
    """dv_conv2d_wgrad_cat_bf16: dw AND the workspace are written fully and nowhere else."""
    case = wg_case()
    sweep(case, wg_call, wg_verdict, "dw")
    ar = place(case, 3)
    s = _lib.stream_ptr()
    assert wg_call(case, ar, s, g=None) == -1 and wg_call(case, ar, s, dw=None) == -1 and wg_call(case, ar, s, ws=None) == -1
    assert wg_call(case, ar, s, k=5) == -3
    assert wg_call(case, ar, s, names=("x0", "x1", "x0", "x1", "x0"), chans=(8,) * 5) == -2          # five sources
    assert wg_call(case, ar, s, w=0) == -2 and wg_call(case, ar, s, cout=-3) == -2
    assert wg_call(case, ar, s, h=1 << 15, w=1 << 15) == -2                                          # H*W >= 2^30
    assert wg_call(case, ar, s, chans=(4096, 4096), cout=4096) == -2                                 # beyond the workspace bound
    torch.cuda.synchronize()
    A.check_untouched(ar["dw"])
    A.check_untouched(ar["ws"])


# ------------------------------------------------------------------ the stream contract
@pytest.fixture(scope="module")
def gate():
    cycles = streams.calibrate_gate(GATE_MS)
    return SimpleNamespace(cycles=cycles, side=streams.pick_streams(1, cycles)[0])


@pytest.mark.parametrize("ksplit", [False, True], ids=["cat", "cat_ksplit"])
def test_conv2d_bf16_cat_keeps_to_its_stream(ksplit, gate):
    """(the K-split form: both launches -- the second one on another stream would read a scratch of sentinels)"""
    case = cat_case(ksplit)
    true, got = gated(case, place, cat_call, cat_verdict, list(case.outs), gate)
    assert torch.equal(true, got)


@pytest.mark.parametrize("ksplit", [False, True], ids=["pair", "pair_ksplit"])
def test_conv2d_bf16_pair_keeps_to_its_stream(ksplit, gate):
    case = pair_case(ksplit)
    true, got = gated(case, place, pair_call, pair_verdict, list(case.outs), gate)
    assert torch.equal(true, got)


def test_conv2d_1in_bf16_keeps_to_its_stream(gate):
    true, got = gated(one_case(), place, one_call, one_verdict, ["out"], gate)
    assert torch.equal(true, got)


def test_gru_gates_bf16_keep_to_their_stream(gate):
    true, got = gated(gate_case(), place, gate_call, gate_verdict, ["rh", "hn"], gate)
    assert torch.equal(true, got)


def test_conv2d_wgrad_cat_bf16_keeps_to_its_stream(gate):
    true, got = gated(wg_case(), place, wg_call, wg_verdict, ["dw", "ws"], gate)
    assert torch.equal(true, got)
