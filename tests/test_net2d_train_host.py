"""The HIP training route of the 2-D networks (diffuvolume_amd/train_net2d.py, csrc/resize_bwd.hip) as far as it can be
checked without a GPU: the switch, the row of the third ABI table, the refusals of the new entry before the device is
touched, the Python function's refusal of CPU tensors, which convolutions get a packed plan, and that a BatchNorm outside
the kernel's case keeps the PyTorch statement."""
import ctypes
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ENTRY = "dv_resize_bilinear_ac_bwd_f32"


@pytest.fixture(scope="module")
def lib():
    from diffuvolume_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_switch_is_listed_documented_and_read_on_every_call(monkeypatch):
    from diffuvolume_amd import _env, train_net2d
    default, where, what = _env.KNOBS["DV_TRAIN_NET2D"]
    assert default in {"hip", "torch"} and "train_net2d.route()" in where and "hip =" in what and "torch =" in what
    assert "DV_TRAIN_NET2D" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_NET2D", raising=False)
    assert train_net2d.route() == default
    monkeypatch.setenv("DV_TRAIN_NET2D", "")
    assert train_net2d.route() == default
    for r in ("torch", "hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NET2D", r)
        assert train_net2d.route() == r                             # read on every call
    for bad in ("eager", "miopen", "HIP"):
        monkeypatch.setenv("DV_TRAIN_NET2D", bad)
        with pytest.raises(ValueError):
            train_net2d.route()
    monkeypatch.setenv("DV_TRAIN_NET2D", "hip")
    assert _env.overrides().get("DV_TRAIN_NET2D") == "hip"
    # read only through _env.route: no module of the package names the variable next to `environ`
    for f in (ROOT / "diffuvolume_amd").glob("*.py"):
        if f.name != "_env.py":
            assert "environ" not in f.read_text() or "DV_TRAIN_NET2D" not in f.read_text(), f.name


def test_row_of_the_third_table_and_its_decision():
    from diffuvolume_amd import _lib
    res, args, why = _lib.VOLUME_TRAIN_SIGNATURES[ENTRY]
    assert res is ctypes.c_int and len(args) == 8 and args[-1] is ctypes.c_void_p
    assert why == _lib.held_by("test_gpu_resize_bwd.py::test_resize_bwd_abi_offset_views_bounds_and_refusals")
    assert ENTRY not in _lib.SIGNATURES and ENTRY not in _lib.TRAIN_SIGNATURES
    assert ENTRY not in (ROOT / "include" / "diffuvolume_hip.h").read_text()
    assert ENTRY in (ROOT / "include" / "diffuvolume_hip_volume_train.h").read_text()
    text = (ROOT / "tests" / "test_gpu_resize_bwd.py").read_text()
    assert "def test_resize_bwd_abi_offset_views_bounds_and_refusals(" in text and "pytest.mark.gpu" in text


def test_null_pointers_and_bad_sizes_are_refused_before_the_device(lib):
    """No GPU here: a call that reached a launch would return a positive hipError_t, not this code."""
    one = ctypes.c_void_p(16)                                       # never dereferenced on the host
    fn = lib.dv_resize_bilinear_ac_bwd_f32
    assert fn(None, None, 1, 1, 1, 1, 1, None) == -1
    assert fn(None, one, 2, 3, 5, 7, 9, None) == -1
    assert fn(one, None, 2, 3, 5, 7, 9, None) == -1
    for i in range(5):
        for bad in (0, -3):
            dims = [2, 3, 5, 7, 9]
            dims[i] = bad
            assert fn(one, one, *dims, None) == -1, dims
    assert fn(one, one, 2 ** 31 - 1, 64, 128, 256, 512, None) == -2        # more blocks than a grid takes
    assert b"NULL" in lib.dv_error_string(-1)


def test_function_is_exported_and_cpu_tensors_raise_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd import train_net2d
    assert "resize_bilinear_train" in dv.__all__ and dv.resize_bilinear_train is train_net2d.resize_bilinear_train
    x = torch.zeros(1, 2, 3, 5, requires_grad=True)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NET2D", route)
        with pytest.raises(dv.DiffuVolumeError):
            dv.resize_bilinear_train(x, (7, 9))
        with pytest.raises(TypeError):
            dv.resize_bilinear_train([1.0], (7, 9))


def test_feature_cnns_raise_on_cpu_tensors_on_both_routes(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd import acv_ddim, pwcnet_ddim
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NET2D", route)
        for fe in (acv_ddim.FeatureExtraction(), pwcnet_ddim.FeatureExtraction(True, 12)):
            with pytest.raises(dv.DiffuVolumeError):
                fe.train()(torch.zeros(1, 3, 32, 64))


def test_which_convolutions_get_a_packed_plan():
    """Stride 1, dilation 1, 3x3 / 1x1 from more than 4 channels: a TrainConvPlan.  The image convolution, the dilated
    layer4, the stride-2 3x3 and the stride-2 1x1 layers: train2d.conv2d_any."""
    from torch import nn
    from diffuvolume_amd import ACVNet_DDIM, acv_ddim, pwcnet_ddim, train_net2d
    for fe, convs, other in ((acv_ddim.FeatureExtraction(), 55, 9), (pwcnet_ddim.FeatureExtraction(True, 12), 94, 15)):
        all_convs = [m for m in fe.modules() if isinstance(m, nn.Conv2d)]
        planned = train_net2d._convs(fe, None)
        assert len(all_convs) == convs and len(all_convs) - len(planned) == other
        for m in all_convs:
            if not train_net2d._planned(m):
                assert m.in_channels == 3 or m.stride == (2, 2) or m.dilation == (2, 2), m
    model = ACVNet_DDIM(192)
    head = train_net2d._convs(model, ("concatconv.",))
    assert [(m.in_channels, m.out_channels, m.kernel_size[0]) for m in head] == [(320, 128, 3), (128, 32, 1)]


def test_bn_act2d_keeps_the_statement_outside_the_kernels_case():
    """An eval-mode module, a module without running statistics, momentum or affine parameters never reaches the train
    function: the module's forward and the PyTorch statement (so CPU tensors work there)."""
    import torch
    import torch.nn.functional as F
    from diffuvolume_amd.train_net2d import bn_act2d
    gen = torch.Generator().manual_seed(3)
    x, skip = torch.randn(2, 3, 4, 5, generator=gen), torch.randn(2, 3, 4, 5, generator=gen)
    for make in (lambda: torch.nn.BatchNorm2d(3).eval(), lambda: torch.nn.BatchNorm2d(3, momentum=None),
                 lambda: torch.nn.BatchNorm2d(3, track_running_stats=False), lambda: torch.nn.BatchNorm2d(3, affine=False)):
        bn, twin = make(), make()
        assert torch.equal(bn_act2d(bn, x, "none", skip=skip), twin(x) + skip)
        assert torch.equal(bn_act2d(bn, x, "relu"), F.relu(twin(x)))
        y = twin(x)
        assert torch.equal(bn_act2d(bn, x, "mish"), y * torch.tanh(F.softplus(y)))
        if bn.num_batches_tracked is not None:
            assert int(bn.num_batches_tracked) == int(twin.num_batches_tracked)
    with pytest.raises(ValueError):
        bn_act2d(torch.nn.BatchNorm2d(3).eval(), x, "gelu")


def test_bn_act_of_the_3d_stacks_sends_4d_tensors_to_the_statement(monkeypatch):
    """`train_norm.bn_act` is the 3-D stacks' call site and stays as it is: a BatchNorm2d on a 4-D tensor is the module's
    forward there on either route.  The 2-D networks go through `train_net2d.bn_act2d`."""
    import torch
    import torch.nn.functional as F
    from diffuvolume_amd.train_norm import bn_act
    x = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(4))
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NORM", route)
        bn, twin = torch.nn.BatchNorm2d(3), torch.nn.BatchNorm2d(3)
        assert torch.equal(bn_act(bn, x, "relu"), F.relu(twin(x)))          # CPU tensors: the train function would raise
        assert int(bn.num_batches_tracked) == 1
