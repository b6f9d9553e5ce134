"""The fused BatchNorm3d + skip + activation of the training routes (diffuvolume_amd/train_norm.py, csrc/bn3d_act.hip) as far
as it can be checked without a GPU: the switch, the rows of the third ABI table with their decisions, the workspace size,
the refusals that happen before the device is touched, and the Python function's refusal of CPU tensors."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("dv_bn3d_train_workspace_floats", "dv_bn3d_stats_f32", "dv_bn3d_apply_act_f32", "dv_bn3d_act_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    from diffuvolume_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_switch_is_listed_documented_and_read_on_every_call(monkeypatch):
    from diffuvolume_amd import _env, train_norm
    default = _env.KNOBS["DV_TRAIN_NORM"][0]
    assert default in {"hip", "torch"}
    assert "DV_TRAIN_NORM" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_NORM", raising=False)
    assert train_norm.route() == default
    monkeypatch.setenv("DV_TRAIN_NORM", "")
    assert train_norm.route() == default
    for r in ("torch", "hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NORM", r)
        assert train_norm.route() == r                              # read on every call
    monkeypatch.setenv("DV_TRAIN_NORM", "eager")
    with pytest.raises(ValueError):
        train_norm.route()
    monkeypatch.setenv("DV_TRAIN_NORM", "torch")
    assert _env.overrides().get("DV_TRAIN_NORM") == "torch"


def test_rows_of_the_third_table_and_their_decisions():
    from diffuvolume_amd import _lib
    table = _lib.VOLUME_TRAIN_SIGNATURES
    assert set(ENTRIES) <= set(table)
    assert not set(ENTRIES) & (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES))
    res, args, why = table["dv_bn3d_train_workspace_floats"]
    assert res is ctypes.c_size_t and len(args) == 3 and why == _lib.SIZE_ONLY
    held = _lib.held_by("test_gpu_norm_train.py::test_bn3d_abi_offset_views_bounds_and_refusals")
    for name, nargs in (("dv_bn3d_stats_f32", 12), ("dv_bn3d_apply_act_f32", 12), ("dv_bn3d_act_bwd_f32", 17)):
        res, args, why = table[name]
        assert res is ctypes.c_int and len(args) == nargs and why == held, name
        assert args[-1] is ctypes.c_void_p, name                    # the stream comes last
    text = (ROOT / "tests" / "test_gpu_norm_train.py").read_text()
    assert "def test_bn3d_abi_offset_views_bounds_and_refusals(" in text and "pytest.mark.gpu" in text
    assert all(name in text for name in ENTRIES[1:])


def test_workspace_size(lib):
    ws = lib.dv_bn3d_train_workspace_floats
    # one block per chunk of 8192 floats of a (b,c) slab leaves one partial of at most 3 floats (count, mean, M2); behind
    # the partials, 2 floats per channel for the two means pass 2 of the backward subtracts
    assert ws(2, 4, 16 * 32 * 64) == 4 * (3 * (2 * 4) + 2)
    assert ws(2, 3, 5) == 3 * (3 * 2 + 2)
    assert ws(1, 32, 8193) == 32 * (3 * 2 + 2)
    assert ws(4, 32, 48 * 64 * 128) == 32 * (3 * (4 * 48) + 2)
    for bad in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (-1, 4, 8), (2, 4, -8)):
        assert ws(*bad) == 0, bad


def test_null_pointers_and_bad_sizes_are_refused_before_the_device(lib):
    """No GPU here: a call that reached a launch would return a positive hipError_t, not these codes."""
    one = ctypes.c_void_p(16)                                        # never dereferenced on the host
    assert lib.dv_bn3d_stats_f32(None, None, None, None, None, None, 2, 3, 5, 0.1, 1e-5, None) == -1
    assert lib.dv_bn3d_apply_act_f32(None, None, None, None, None, None, None, 2, 3, 5, 1, None) == -1
    assert lib.dv_bn3d_act_bwd_f32(*([None] * 12), 2, 3, 5, 1, None) == -1
    for i in (0, 1, 2, 5):                                           # x, mean, invstd, workspace
        a = [one] * 6
        a[i] = None
        assert lib.dv_bn3d_stats_f32(*a, 2, 3, 5, 0.1, 1e-5, None) == -1, i
    assert lib.dv_bn3d_stats_f32(one, one, one, one, None, one, 2, 3, 5, 0.1, 1e-5, None) == -1     # one buffer only
    for i in (0, 2, 3, 4, 5, 6):                                     # all but skip
        a = [one] * 7
        a[i] = None
        assert lib.dv_bn3d_apply_act_f32(*a, 2, 3, 5, 1, None) == -1, i
    for i in (0, 1, 3, 4, 5, 6, 11):                                 # all inputs but skip, and the workspace
        a = [one] * 12
        a[i] = None
        assert lib.dv_bn3d_act_bwd_f32(*a, 2, 3, 5, 1, None) == -1, i
    a = [one] * 7 + [None] * 4 + [one]
    assert lib.dv_bn3d_act_bwd_f32(*a, 2, 3, 5, 1, None) == -1      # no output wanted
    a = [one, one, None] + [one] * 9
    assert lib.dv_bn3d_act_bwd_f32(*a, 2, 3, 5, 1, None) == -1      # dskip without skip
    for bad in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (2, 3, -5)):
        assert lib.dv_bn3d_stats_f32(*[one] * 6, *bad, 0.1, 1e-5, None) == -2, bad
        assert lib.dv_bn3d_apply_act_f32(*[one] * 7, *bad, 1, None) == -2, bad
        assert lib.dv_bn3d_act_bwd_f32(*[one] * 12, *bad, 1, None) == -2, bad
    assert lib.dv_bn3d_stats_f32(*[one] * 6, 1, 3, 1, 0.1, 1e-5, None) == -3          # B*S == 1: no variance
    assert lib.dv_bn3d_act_bwd_f32(*[one] * 12, 1, 3, 1, 1, None) == -3
    for act in (-1, 3, 4, 5, 6):                                     # only NONE, RELU and MISH
        assert lib.dv_bn3d_apply_act_f32(*[one] * 7, 2, 3, 5, act, None) == -3, act
        assert lib.dv_bn3d_act_bwd_f32(*[one] * 12, 2, 3, 5, act, None) == -3, act
    assert b"NULL" in lib.dv_error_string(-1)


def test_function_is_exported_and_cpu_tensors_raise_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd import train_norm
    assert "batch_norm_act_train" in dv.__all__ and dv.batch_norm_act_train is train_norm.batch_norm_act_train
    x = torch.zeros(2, 3, 1, 2, 4, requires_grad=True)
    w, b, rm, rv = torch.ones(3), torch.zeros(3), torch.zeros(3), torch.ones(3)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NORM", route)
        for act in ("none", "relu", "mish"):
            with pytest.raises(dv.DiffuVolumeError):
                dv.batch_norm_act_train(x, w, b, rm, rv, act=act)
        with pytest.raises(dv.DiffuVolumeError):
            dv.batch_norm_act_train(x, w, b, None, None, act="relu", skip=torch.zeros_like(x))
        with pytest.raises(ValueError):
            dv.batch_norm_act_train(x, w, b, rm, rv, act="gelu")
    assert torch.equal(rm, torch.zeros(3)) and torch.equal(rv, torch.ones(3))


def test_bn_act_keeps_the_statement_outside_the_kernels_case(monkeypatch):
    """An eval-mode module, a module without running statistics or momentum, and a tensor that is not 5-D never reach the
    train function: the module's forward and the PyTorch statement, on either route (so CPU tensors work there)."""
    import torch
    import torch.nn.functional as F
    from diffuvolume_amd.train_norm import bn_act
    gen = torch.Generator().manual_seed(3)
    x, skip = torch.randn(2, 3, 2, 3, 4, generator=gen), torch.randn(2, 3, 2, 3, 4, generator=gen)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NORM", route)
        for make in (lambda: torch.nn.BatchNorm3d(3).eval(), lambda: torch.nn.BatchNorm3d(3, momentum=None),
                     lambda: torch.nn.BatchNorm3d(3, track_running_stats=False)):
            bn, twin = make(), make()
            assert torch.equal(bn_act(bn, x, "relu", skip=skip), F.relu(twin(x) + skip))
            y = twin(x)
            assert torch.equal(bn_act(bn, x, "mish"), y * torch.tanh(F.softplus(y)))
            assert torch.equal(bn_act(bn, x, "none"), twin(x))
            if bn.num_batches_tracked is not None:
                assert int(bn.num_batches_tracked) == int(twin.num_batches_tracked)
        bn2, twin2 = torch.nn.BatchNorm2d(3), torch.nn.BatchNorm2d(3)
        assert torch.equal(bn_act(bn2, x[:, :, 0], "relu"), F.relu(twin2(x[:, :, 0])))
        assert int(bn2.num_batches_tracked) == 1
