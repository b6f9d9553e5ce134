"""The bottleneck window attention of ACVNet_DDIM's training route (diffuvolume_amd/train_attn.py, csrc/window_attn_bwd.hip) as
far as it can be checked without a GPU: the switch, the rows of the third ABI table with their decisions, the workspace
size, the refusals that happen before the device is touched, and the Python function's refusal of CPU tensors."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("dv_window_attn3d_bwd_workspace_floats", "dv_window_attn3d_bwd_f32")
ABI_TEST = "test_attn_bwd_abi_offset_views_bounds_and_refusals"


@pytest.fixture(scope="module")
def lib():
    from diffuvolume_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_switch_is_listed_documented_and_read_on_every_call(monkeypatch):
    from diffuvolume_amd import _env, train_attn
    default = _env.KNOBS["DV_TRAIN_ATTN"][0]
    assert default in {"hip", "torch"}
    assert "DV_TRAIN_ATTN" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_ATTN", raising=False)
    assert train_attn.route() == default
    monkeypatch.setenv("DV_TRAIN_ATTN", "")
    assert train_attn.route() == default
    for r in ("torch", "hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_ATTN", r)
        assert train_attn.route() == r                              # read on every call
    monkeypatch.setenv("DV_TRAIN_ATTN", "eager")
    with pytest.raises(ValueError):
        train_attn.route()
    monkeypatch.setenv("DV_TRAIN_ATTN", "torch")
    assert _env.overrides().get("DV_TRAIN_ATTN") == "torch"


def test_rows_of_the_third_table_and_their_decisions(lib):
    from diffuvolume_amd import _lib
    table = _lib.VOLUME_TRAIN_SIGNATURES
    assert set(ENTRIES) <= set(table)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES))
    res, args, why = table["dv_window_attn3d_bwd_workspace_floats"]
    assert res is ctypes.c_size_t and len(args) == 6 and why == _lib.SIZE_ONLY
    res, args, why = table["dv_window_attn3d_bwd_f32"]
    assert res is ctypes.c_int and len(args) == 18 and args[-1] is ctypes.c_void_p      # the stream comes last
    assert why == _lib.held_by(f"test_gpu_attn_train.py::{ABI_TEST}")
    text = (ROOT / "tests" / "test_gpu_attn_train.py").read_text()
    assert f"def {ABI_TEST}(" in text and "pytest.mark.gpu" in text
    assert "dv_window_attn3d_bwd_f32" in text
    raw = ctypes.CDLL(str(_lib.lib_path()))
    assert all(hasattr(raw, name) for name in ENTRIES)
    header = (ROOT / "include" / "diffuvolume_hip_volume_train.h").read_text()
    assert all(name + "(" in header for name in ENTRIES)
    assert "submodule.py:398-429" in header and "acv_ddim.py:56-93" in header            # reference lines


def expected_workspace(b, d, h, w):
    vol, windows = d * h * w, b * (d // 4) * -(-h // 4) * -(-w // 4)
    chunks = b * -(-vol // 32)                                                          # the GEMMs split 32-token chunks
    return (b * 128 * vol                                                               # Om, channel-major
            + b * 384 * vol                                                             # dQKV, channel-major
            + windows * 384                                                             # one bias partial per window
            + min(chunks, 64) * 384 * 128 + min(chunks, 128) * 128 * 128)               # the partials of dWqkv and dWp


def test_workspace_size(lib):
    ws = lib.dv_window_attn3d_bwd_workspace_floats
    for b, d, h, w in ((4, 12, 16, 32), (1, 4, 4, 4), (2, 4, 5, 7), (2, 8, 6, 20)):
        assert ws(b, 128, d, h, w, 16) == expected_workspace(b, d, h, w), (b, d, h, w)
    assert ws(1, 128, 4, 4, 4, 16) == 512 * 64 + 384 + 2 * (384 * 128 + 128 * 128)      # one window, two chunks, two splits
    assert ws(4, 128, 12, 16, 32, 16) == 4 * 512 * 6144 + 384 * 384 + 64 * 384 * 128 + 128 * 128 * 128
    for bad in ((0, 128, 4, 4, 4, 16), (1, 128, 0, 4, 4, 16), (1, 128, 4, 0, 4, 16), (1, 128, 4, 4, 0, 16),
                (1, 128, 4, 4, -4, 16), (-1, 128, 4, 4, 4, 16), (1, 128, 6, 4, 4, 16), (1, 128, 2, 4, 4, 16),
                (1, 64, 4, 4, 4, 16), (1, 0, 4, 4, 4, 16), (1, 128, 4, 4, 4, 8), (1, 128, 4, 4, 4, 0), (1, 256, 4, 4, 4, 32)):
        assert ws(*bad) == 0, bad


def test_refusals_happen_before_the_device(lib):
    """No GPU here: a call that reached a launch would return a positive hipError_t, not these codes."""
    one = ctypes.c_void_p(16)                                        # never dereferenced on the host; on a 16-byte line
    off = ctypes.c_void_p(20)
    f = lib.dv_window_attn3d_bwd_f32
    size = (2, 128, 4, 5, 7, 16)                                     # B, C, D, H, W, heads
    assert f(*[None] * 11, *size, None) == -1
    for i in range(5):                                               # x, qkv_w, qkv_b, proj_w, dout
        a = [one] * 11
        a[i] = None
        assert f(*a, *size, None) == -1, i
    assert f(*[one] * 5, *[None] * 5, one, *size, None) == -1       # no output wanted
    for i in (6, 7, 8):                                              # dqkv_w, dqkv_b, dproj_w without a workspace
        a = [one] * 5 + [None] * 6
        a[i] = one
        assert f(*a, *size, None) == -1, i
    for i in (0, 2, 3, 4):
        bad = list(size)
        bad[i] = 0
        assert f(*[one] * 11, *bad, None) == -2, i
        bad[i] = -size[i]
        assert f(*[one] * 11, *bad, None) == -2, i
    assert f(*[one] * 11, 2, 128, 6, 5, 7, 16, None) == -2           # D % 4 != 0
    assert f(*[one] * 11, 2, 64, 4, 5, 7, 16, None) == -3            # C != 128
    assert f(*[one] * 11, 2, 128, 4, 5, 7, 8, None) == -3            # heads != 16
    fwd = lib.dv_window_attn3d_f32
    align = fwd(one, off, one, one, one, one, *size, None)           # the forward's code for weights off a 16-byte line
    assert align < 0 and align not in (-1, -2, -3)
    assert f(one, off, *[one] * 9, *size, None) == align
    assert f(one, one, one, off, *[one] * 7, *size, None) == align
    assert b"NULL" in lib.dv_error_string(-1)


def test_function_is_exported_and_cpu_tensors_raise_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd import train_attn
    assert "window_attention_train" in dv.__all__ and dv.window_attention_train is train_attn.window_attention_train
    x = torch.zeros(1, 128, 4, 4, 4, requires_grad=True)
    wq, bq = torch.ones(384, 128, requires_grad=True), torch.zeros(384)
    wp, bp = torch.ones(128, 128, 1, 1, 1), torch.zeros(128, requires_grad=True)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_ATTN", route)
        with pytest.raises(dv.DiffuVolumeError):
            dv.window_attention_train(x, wq, bq, wp, bp)
        with pytest.raises(dv.DiffuVolumeError):
            dv.window_attention_train(x.detach(), wq.detach(), bq, wp, bp.detach(), heads=16)


def test_the_hourglass_calls_the_function():
    text = (ROOT / "diffuvolume_amd" / "acv_ddim.py").read_text()
    assert "window_attention_train(" in text and "torch.softmax(logits" not in text
