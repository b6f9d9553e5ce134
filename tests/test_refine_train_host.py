"""The warp + correlation of PWCNet_ddim's refinement input in training (train_refine.py, csrc/warp_corr.hip), as far as it
can be checked without a GPU: the switch, the rows of the third ABI table (tests/test_volume_train_host.py applies to them
as it stands), the workspace size and the refusals that come before the device is touched."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("dv_warp_corr_f32", "dv_warp_corr_bwd_workspace_floats", "dv_warp_corr_bwd_f32")


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_switch_is_listed_documented_and_read_on_every_call(monkeypatch):
    from diffuvolume_amd import _env, train_refine
    default = _env.KNOBS["DV_TRAIN_REFINE"][0]
    assert default in ("hip", "torch")
    assert "DV_TRAIN_REFINE" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_REFINE", raising=False)
    assert train_refine.route() == default
    monkeypatch.setenv("DV_TRAIN_REFINE", "")
    assert train_refine.route() == default
    for value in ("torch", "hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_REFINE", value)
        assert train_refine.route() == value                      # read on every call
    monkeypatch.setenv("DV_TRAIN_REFINE", "cpu")
    with pytest.raises(ValueError):
        train_refine.route()


def test_cpu_tensors_raise_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    left = torch.zeros(1, 4, 2, 24, requires_grad=True)
    right, disp = torch.zeros(1, 4, 2, 24), torch.zeros(1, 1, 2, 24)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_REFINE", route)
        with pytest.raises(dv.DiffuVolumeError):
            dv.warp_corr_train(left, right, disp)
        with pytest.raises(dv.DiffuVolumeError):
            dv.warp_corr_train(left.detach(), right, disp.requires_grad_(True), maxshift=24)
    monkeypatch.setenv("DV_TRAIN_REFINE", "eager")
    with pytest.raises(ValueError):                               # the switch is read before the tensors are looked at
        dv.warp_corr_train(left, right, disp)


def test_the_three_entries_are_rows_of_the_third_table_and_exported(built):
    import diffuvolume_amd as dv
    from diffuvolume_amd import _lib
    assert "warp_corr_train" in dv.__all__ and callable(dv.warp_corr_train)
    raw = ctypes.CDLL(str(built))
    for name in NAMES:
        assert name in _lib.VOLUME_TRAIN_SIGNATURES, name
        assert hasattr(raw, name), name
    assert _lib.VOLUME_TRAIN_SIGNATURES[NAMES[1]][2] == _lib.SIZE_ONLY
    for name in (NAMES[0], NAMES[2]):
        assert _lib.VOLUME_TRAIN_SIGNATURES[name][2].endswith("test_gpu_refine_train.py::"
                                                               "test_warp_corr_abi_offset_views_bounds_and_refusals")


def test_workspace_size_and_refusals_before_the_device(built):
    from diffuvolume_amd import _lib
    lib = _lib.load()
    ws = lib.dv_warp_corr_bwd_workspace_floats
    assert ws(4, 32, 256, 512) == 4 * 32 * 256 * 512              # m * dF: one feature map of floats
    assert ws(1, 1, 3, 24) == 72
    for bad in ((0, 32, 256, 512), (4, 0, 256, 512), (4, 32, -1, 512), (4, 32, 256, 0)):
        assert ws(*bad) == 0
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(16)                                     # never dereferenced: a NULL operand is refused first
    dims = (1, 4, 2, 24, 24)
    assert lib.dv_warp_corr_f32(null, null, null, null, null, *dims, None) == -1
    for i in range(5):
        a = [one] * 5
        a[i] = null
        assert lib.dv_warp_corr_f32(*a, *dims, None) == -1, i
        a = [one] * 9
        a[i] = null
        assert lib.dv_warp_corr_bwd_f32(*a, *dims, None) == -1, i
    assert lib.dv_warp_corr_bwd_f32(*([one] * 5), null, null, null, one, *dims, None) == -1      # no output wanted
    assert lib.dv_warp_corr_bwd_f32(*([one] * 5), one, one, one, null, *dims, None) == -1        # dright without workspace
    # shapes and what the kernels do not implement are refused before the device is touched, too
    assert lib.dv_warp_corr_f32(*([one] * 5), 1, 4, 0, 24, 24, None) == -2
    assert lib.dv_warp_corr_f32(*([one] * 5), 1, 33, 2, 24, 24, None) == -3
    assert lib.dv_warp_corr_f32(*([one] * 5), 1, 4, 2, 23, 24, None) == -3
    assert lib.dv_warp_corr_f32(*([one] * 5), 1, 4, 2, 24, 23, None) == -3
    assert lib.dv_warp_corr_f32(*([one] * 5), 65536, 4, 2, 24, 24, None) == -2
    assert lib.dv_warp_corr_bwd_f32(*([one] * 9), 1, 4, 65536, 24, 24, None) == -2
    assert lib.dv_warp_corr_bwd_f32(*([one] * 9), 1, 33, 2, 24, 24, None) == -3
    assert b"NULL" in lib.dv_error_string(-1)
