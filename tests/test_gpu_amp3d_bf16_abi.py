"""The pointer, bounds and stream contract of the launching entries of the fifth ABI table
(include/diffuvolume_hip_amp3d_bf16.h, ``_lib.AMP3D_BF16_SIGNATURES``): dv_conv3d_k3s1_bf16_f32 and dv_conv3d_wgrad_bf16_f32.
The method, the shapes and the harness are those of tests/test_gpu_amp3d_abi.py (the fourth table), whose placement,
verdict and gate helpers are used as they are; only the entries called and the rounding of the reference differ.

Pointer and bounds (tests/arena.py): every operand is a view into a guard-banded buffer at each ``data_ptr() % 16`` in
{0, 4, 8, 12}; inputs sit between NaN, outputs are filled with a sentinel.  After the call the guards are intact, every
output element is written, no NaN leaked in, the result meets the bar of the entry's own test and has the bits of the
16-byte aligned call (the forward entry's scalar stores against its 16-byte stores).  Refused calls write nothing.

Stream (tests/streams.py): the entry runs on a side stream that was seen to run independently of the null stream, behind
a gate kernel, with operands that only arrive behind the gate; the call must return while the gate still spins, and the
result must equal the default-stream run bit for bit."""
from types import SimpleNamespace

import pytest
import torch

import arena as A
import streams
from diffuvolume_amd import _lib
from test_gpu_amp3d_abi import FWD, FWD_ODD, GATE_MS, WG, fwd_place, fwd_verdict, gated, wg_place, wg_verdict
from test_gpu_conv3d_bf16 import depth_c as fwd_c, rand, reference
from test_gpu_conv3d_wgrad_bf16 import depth_c as wgrad_c, rb16
from test_gpu_conv3d_wgrad_f16 import ref_wgrad

pytestmark = pytest.mark.gpu


def fwd_case(s, flip):
    x = rand(s["b"], s["cin"], s["d"], s["h"], s["w"], seed=31)
    w = rand(*((s["cin"], s["cout"]) if flip else (s["cout"], s["cin"])), 3, 3, 3, seed=32, scale=0.1)
    bias = None if flip else rand(s["cout"], seed=33)
    ref, mag = reference(x, w.flip(2, 3, 4).transpose(0, 1) if flip else w, bias)
    return SimpleNamespace(x=x, w=w, bias=bias, ref=ref, mag=mag, s=s, flip=flip, c=fwd_c(s["cin"], bias is not None))


def fwd_call(case, ar, stream, **over):
    s = dict(case.s, **over)
    bias = ar["bias"].data_ptr() if "bias" in ar else None
    return _lib.load().dv_conv3d_k3s1_bf16_f32(over.get("x", ar["x"].data_ptr()), ar["w"].data_ptr(), bias,
                                               ar["out"].data_ptr(), s["b"], s["cin"], s["d"], s["h"], s["w"], s["cout"],
                                               over.get("k", 3), int(case.flip), stream)


def wg_case(s):
    x = rand(s["b"], s["cin"], s["d"], s["h"], s["w"], seed=41)
    g = rand(s["b"], s["cout"], s["d"], s["h"], s["w"], seed=42)
    x64, g64 = rb16(x).double(), rb16(g).double()
    n = _lib.load().dv_conv3d_wgrad_bf16_workspace_floats(s["b"], s["cin"], s["d"], s["h"], s["w"], s["cout"])
    return SimpleNamespace(x=x, g=g, ref=ref_wgrad(x64, g64), mag=ref_wgrad(x64.abs(), g64.abs()), s=s, n=n,
                           c=wgrad_c(s["b"], s["cin"], s["d"], s["h"], s["w"], s["cout"]))


def wg_call(case, ar, stream, **over):
    s = dict(case.s, **over)
    return _lib.load().dv_conv3d_wgrad_bf16_f32(ar["x"].data_ptr(), over.get("g", ar["g"].data_ptr()), ar["dw"].data_ptr(),
                                                over.get("ws", ar["ws"].data_ptr()), s["b"], s["cin"], s["d"], s["h"],
                                                s["w"], s["cout"], stream)


def test_conv3d_bf16_abi_offset_views_bounds_and_refusals():
    """dv_conv3d_k3s1_bf16_f32, forward (with a bias) and input-gradient view."""
    for shape in (FWD, FWD_ODD):
        for flip in (False, True):
            case = fwd_case(shape, flip)
            aligned = None
            for off in range(4):
                ar = fwd_place(case, off)
                assert ar["out"].data_ptr() % 16 == 4 * off
                assert fwd_call(case, ar, _lib.stream_ptr()) == 0
                torch.cuda.synchronize()
                y = fwd_verdict(case, ar)
                aligned = y if aligned is None else aligned
                assert torch.equal(y, aligned), f"offset {off}: other bits than the 16-byte aligned call"
    case = fwd_case(FWD, False)
    ar = fwd_place(case, 1)
    s = _lib.stream_ptr()
    assert fwd_call(case, ar, s, cout=1) == -3                   # the single-channel heads keep their float32 kernel
    assert fwd_call(case, ar, s, k=1) == -3 and fwd_call(case, ar, s, k=5) == -3
    assert fwd_call(case, ar, s, x=None) == -1
    assert fwd_call(case, ar, s, d=0) == -2 and fwd_call(case, ar, s, cin=-1) == -2
    assert fwd_call(case, ar, s, d=1 << 15, h=1 << 15, w=1 << 15) == -2        # beyond 31-bit byte offsets
    torch.cuda.synchronize()
    A.check_untouched(ar["out"])


def test_conv3d_wgrad_bf16_abi_offset_views_bounds_and_refusals():
    """dv_conv3d_wgrad_bf16_f32: dw AND the workspace are written fully and nowhere else."""
    case = wg_case(WG)
    aligned = None
    for off in range(4):
        ar = wg_place(case, off)
        assert ar["dw"].data_ptr() % 16 == 4 * off
        assert wg_call(case, ar, _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        dw = wg_verdict(case, ar)
        aligned = dw if aligned is None else aligned
        assert torch.equal(dw, aligned), f"offset {off}: other bits than the 16-byte aligned call"
    ar = wg_place(case, 3)
    s = _lib.stream_ptr()
    assert wg_call(case, ar, s, g=None) == -1 and wg_call(case, ar, s, ws=None) == -1
    assert wg_call(case, ar, s, w=0) == -2 and wg_call(case, ar, s, cout=-3) == -2
    assert wg_call(case, ar, s, d=1 << 10, h=1 << 10, w=1 << 10) == -2         # D*H*W >= 2^30
    assert wg_call(case, ar, s, cin=1024, cout=1024) == -2                     # one split beyond the workspace bound
    torch.cuda.synchronize()
    A.check_untouched(ar["dw"])
    A.check_untouched(ar["ws"])


# ------------------------------------------------------------------ the stream contract
@pytest.fixture(scope="module")
def gate():
    cycles = streams.calibrate_gate(GATE_MS)
    return SimpleNamespace(cycles=cycles, side=streams.pick_streams(1, cycles)[0])


@pytest.mark.parametrize("flip", [False, True], ids=["forward", "input_gradient"])
def test_conv3d_bf16_keeps_to_its_stream(flip, gate):
    true, got = gated(fwd_case(FWD, flip), fwd_place, fwd_call, fwd_verdict, ["out"], gate)
    assert torch.equal(true, got)


def test_conv3d_wgrad_bf16_keeps_to_its_stream(gate):
    """Both launches of the entry (the partial sums and the sum of the splits): the second one on another stream would
    read a workspace of sentinels."""
    true, got = gated(wg_case(WG), wg_place, wg_call, wg_verdict, ["dw", "ws"], gate)
    assert torch.equal(true, got)
