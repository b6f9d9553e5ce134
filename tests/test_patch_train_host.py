"""The patch stencils of ACVNet_DDIM's training route (diffuvolume_amd/train_patch.py, csrc/patch_volume_bwd.hip) as far as
they can be checked without a GPU: the switch, the rows of the third ABI table with their decisions, the workspace size,
the refusals that happen before the device is touched, and the Python function's refusal of CPU tensors."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("dv_patch_volume_bwd_workspace_floats", "dv_patch_volume_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    from diffuvolume_amd import _build, _lib
    _build.build()
    return _lib.load()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_switch_is_listed_documented_and_read_on_every_call(monkeypatch):
    from diffuvolume_amd import _env, train_patch
    default = _env.KNOBS["DV_TRAIN_PATCH"][0]
    assert default in {"hip", "torch"}
    assert "DV_TRAIN_PATCH" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_PATCH", raising=False)
    assert train_patch.route() == default
    monkeypatch.setenv("DV_TRAIN_PATCH", "")
    assert train_patch.route() == default
    for r in ("torch", "hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_PATCH", r)
        assert train_patch.route() == r                             # read on every call
    monkeypatch.setenv("DV_TRAIN_PATCH", "eager")
    with pytest.raises(ValueError):
        train_patch.route()
    monkeypatch.setenv("DV_TRAIN_PATCH", "torch")
    assert _env.overrides().get("DV_TRAIN_PATCH") == "torch"


def test_rows_of_the_third_table_and_their_decisions(lib):
    from diffuvolume_amd import _lib
    table = _lib.VOLUME_TRAIN_SIGNATURES
    assert set(ENTRIES) <= set(table)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES))
    res, args, why = table["dv_patch_volume_bwd_workspace_floats"]
    assert res is ctypes.c_size_t and len(args) == 5 and why == _lib.SIZE_ONLY
    res, args, why = table["dv_patch_volume_bwd_f32"]
    assert res is ctypes.c_int and len(args) == 18 and args[-1] is ctypes.c_void_p      # the stream comes last
    assert why == _lib.held_by("test_gpu_patch_train.py::test_patch_bwd_abi_offset_views_bounds_and_refusals")
    text = (ROOT / "tests" / "test_gpu_patch_train.py").read_text()
    assert "def test_patch_bwd_abi_offset_views_bounds_and_refusals(" in text and "pytest.mark.gpu" in text
    assert "dv_patch_volume_bwd_f32" in text
    raw = ctypes.CDLL(str(_lib.lib_path()))
    assert all(hasattr(raw, name) for name in ENTRIES)
    header = (ROOT / "include" / "diffuvolume_hip_volume_train.h").read_text()
    assert all(name + "(" in header for name in ENTRIES) and "acv_ddim.py:181-188" in header      # reference lines


def test_workspace_size(lib):
    ws = lib.dv_patch_volume_bwd_workspace_floats
    # one slot of 18 floats (dw1, dw2 of the block's group) per block: a block owns a 16 x 128 tile of one (b, g, d) plane
    assert ws(4, 40, 48, 64, 128) == 40 * (4 * 48 * 4 * 1) * 18
    assert ws(2, 40, 2, 33, 140) == 40 * (2 * 2 * 3 * 2) * 18
    assert ws(1, 40, 1, 2, 3) == 40 * 18
    assert ws(1, 3, 1, 16, 128) == 3 * 18 and ws(1, 3, 1, 17, 129) == 3 * 4 * 18
    for bad in ((0, 4, 1, 8, 8), (2, 0, 1, 8, 8), (2, 4, 0, 8, 8), (2, 4, 1, 0, 8), (2, 4, 1, 8, 0), (2, 4, 1, -8, 8)):
        assert ws(*bad) == 0, bad


def test_null_pointers_and_malformed_runs_are_refused_before_the_device(lib):
    """No GPU here: a call that reached a launch would return a positive hipError_t, not these codes."""
    one = ctypes.c_void_p(16)                                        # never dereferenced on the host
    f = lib.dv_patch_volume_bwd_f32
    size = (2, 4, 1, 5, 8)                                           # B, G, D, H, W
    runs = (2, ints(0, 1), ints(1, 3), ints(1, 3))
    assert f(*[None] * 8, *size, *runs, None) == -1
    for i in (0, 1, 2, 3):                                           # gwc, w1, w2, dout
        a = [one] * 8
        a[i] = None
        assert f(*a, *size, *runs, None) == -1, i
    assert f(one, one, one, one, None, None, None, one, *size, *runs, None) == -1       # no output wanted
    assert f(one, one, one, one, one, one, None, None, *size, *runs, None) == -1        # dw1 without a workspace
    assert f(one, one, one, one, one, None, one, None, *size, *runs, None) == -1        # dw2 without a workspace
    for i in (1, 2, 3):                                              # the three run arrays
        r = list(runs)
        r[i] = None
        assert f(*[one] * 8, *size, *r, None) == -1, i
    for bad in ((0, 4, 1, 5, 8), (2, 0, 1, 5, 8), (2, 4, 0, 5, 8), (2, 4, 1, 0, 8), (2, 4, 1, 5, 0), (2, 4, 1, 5, -8)):
        assert f(*[one] * 8, *bad, *runs, None) == -2, bad
    assert f(*[one] * 8, *size, 0, *runs[1:], None) == -2            # no run
    for g0, ng, dil in (((0, 2), (1, 3), (1, 3)),                    # a gap: the second run does not start where the first ends
                        ((0, 1), (1, 2), (1, 3)),                    # 3 groups of 4
                        ((0, 1), (1, 4), (1, 3)),                    # 5 groups of 4
                        ((1, 2), (1, 2), (1, 3)),                    # does not start at group 0
                        ((0, 1), (1, 0), (1, 3)),                    # an empty run
                        ((0, 1), (1, 3), (1, 4)),                    # dilation outside 1..3
                        ((0, 1), (1, 3), (0, 2))):
        assert f(*[one] * 8, *size, 2, ints(*g0), ints(*ng), ints(*dil), None) == -2, (g0, ng, dil)
    assert b"NULL" in lib.dv_error_string(-1)


def test_function_is_exported_and_cpu_tensors_raise_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd import train_patch
    assert "patch_volume_train" in dv.__all__ and dv.patch_volume_train is train_patch.patch_volume_train
    x = torch.zeros(1, 4, 1, 2, 4, requires_grad=True)
    w1, w2 = torch.ones(4, 9), torch.ones(4, 9, requires_grad=True)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_PATCH", route)
        with pytest.raises(dv.DiffuVolumeError):
            dv.patch_volume_train(x, w1, w2, [1, 2, 2, 3])
        with pytest.raises(dv.DiffuVolumeError):
            dv.patch_volume_train(x.detach(), w1, w2.detach(), (1, 1, 1, 1))


def test_runs_come_from_the_host_sequence():
    from diffuvolume_amd import train_patch
    n, g0, ng, dl, triples = train_patch._runs((1,) * 8 + (2,) * 16 + (3,) * 16)
    assert n == 3 and list(g0) == [0, 8, 24] and list(ng) == [8, 16, 16] and list(dl) == [1, 2, 3]
    assert triples == ((0, 8, 1), (8, 16, 2), (24, 16, 3))
    assert train_patch._runs((2, 1, 1, 3, 2))[4] == ((0, 1, 2), (1, 2, 1), (3, 1, 3), (4, 1, 2))
