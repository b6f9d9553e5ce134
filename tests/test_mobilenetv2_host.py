"""Host-side checks of the in-tree MobileNetV2 backbone (diffuvolume_amd/mobilenetv2.py), its routes in igev_layers and
the three `dv_dwconv3x3_*` rows of the C ABI, as far as they can be checked without a GPU.

timm is not a dependency: the layout of ``timm.create_model('mobilenetv2_100', features_only=True)`` is written out below
a second time, by hand, and the module's state_dict has to match it key by key and shape by shape."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from diffuvolume_amd import DiffuVolumeError, _lib, train2d
from diffuvolume_amd.igev_front2d import Feature
from diffuvolume_amd.igev_layers import ACT_RELU6, HIP, TORCH, TRAIN, hip_dwconv2d, hip_sequential, train_sequential
from diffuvolume_amd.mobilenetv2 import (DepthwiseSeparableConv, InvertedResidual, MobileNetV2Features, depthwise_separable,
                                         inverted_residual)
from diffuvolume_amd.synth import StubMobileNetV2, synth_state_dict

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"dv_dwconv3x3_f32": 13, "dv_dwconv3x3_bwd_workspace_floats": 5, "dv_dwconv3x3_bwd_f32": 12}


def bn_keys(prefix, c):
    return [(f"{prefix}.weight", (c,)), (f"{prefix}.bias", (c,)), (f"{prefix}.running_mean", (c,)),
            (f"{prefix}.running_var", (c,)), (f"{prefix}.num_batches_tracked", ())]


def expected_layout():
    """The ordered (key, shape) list of mobilenetv2_100's feature extractor."""
    keys = [("conv_stem.weight", (32, 3, 3, 3))] + bn_keys("bn1", 32)
    keys += [("blocks.0.0.conv_dw.weight", (32, 1, 3, 3))] + bn_keys("blocks.0.0.bn1", 32)
    keys += [("blocks.0.0.conv_pw.weight", (16, 32, 1, 1))] + bn_keys("blocks.0.0.bn2", 16)
    cin = 16
    for s, (n, cout) in enumerate([(2, 24), (3, 32), (4, 64), (3, 96), (3, 160), (1, 320)], start=1):
        for i in range(n):
            p, mid = f"blocks.{s}.{i}", 6 * cin
            keys += [(f"{p}.conv_pw.weight", (mid, cin, 1, 1))] + bn_keys(f"{p}.bn1", mid)
            keys += [(f"{p}.conv_dw.weight", (mid, 1, 3, 3))] + bn_keys(f"{p}.bn2", mid)
            keys += [(f"{p}.conv_pwl.weight", (cout, mid, 1, 1))] + bn_keys(f"{p}.bn3", cout)
            cin = cout
    return keys


def test_state_dict_is_timms_layout_key_by_key():
    sd = MobileNetV2Features().state_dict()
    got = [(k, tuple(v.shape)) for k, v in sd.items()]
    assert got == expected_layout()
    assert len(got) == 306
    assert tuple(sd["blocks.0.0.conv_dw.weight"].shape) == (32, 1, 3, 3)
    assert tuple(sd["blocks.1.0.conv_pw.weight"].shape) == (96, 16, 1, 1)
    assert tuple(sd["blocks.3.3.conv_pwl.weight"].shape) == (64, 384, 1, 1)
    assert tuple(sd["blocks.6.0.conv_pwl.weight"].shape) == (320, 960, 1, 1)


def test_strides_skips_and_norm_settings():
    m = MobileNetV2Features()
    assert [len(s) for s in m.blocks] == [1, 2, 3, 4, 3, 3, 1]
    assert [s[0].conv_dw.stride[0] for s in m.blocks] == [1, 2, 2, 2, 1, 2, 1]
    for s in m.blocks:
        assert all(b.conv_dw.stride == (1, 1) for b in list(s)[1:])
        assert [b.has_skip for b in s] == [False] + [True] * (len(s) - 1)
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d):
            assert mod.bias is None
        if isinstance(mod, nn.BatchNorm2d):
            assert mod.eps == 1e-5 and mod.momentum == 0.1
    outs = m.eval()(torch.zeros(1, 3, 32, 64))
    assert [tuple(o.shape[1:]) for o in outs] == [(16, 16, 32), (24, 8, 16), (32, 4, 8), (96, 2, 4), (320, 1, 2)]


def test_reference_checkpoint_keys_under_feature_round_trip():
    f = Feature(MobileNetV2Features())
    sd = f.state_dict()
    for k in ("conv_stem.weight", "bn1.running_mean", "block0.0.0.conv_dw.weight", "block1.0.1.conv_pwl.weight",
              "block3.0.3.bn1.num_batches_tracked", "block3.1.0.conv_pw.weight", "block3.1.2.bn3.running_var",
              "block4.0.2.conv_dw.weight", "deconv32_16.conv1.conv.weight"):
        assert k in sd, k
    assert tuple(sd["block3.1.0.conv_pw.weight"].shape) == (384, 64, 1, 1)
    assert not any(k.startswith(("blocks.", "block5.")) for k in sd)           # the 320-channel stage is not part of Feature
    new = synth_state_dict(sd, seed=11)
    g = Feature(MobileNetV2Features())
    g.load_state_dict(new, strict=True)
    back = g.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], new[k]) for k in sd)


class ForeignGrouped(nn.Module):
    """A backbone of another library: grouped nn.Conv2d in plain stages."""

    def __init__(self):
        super().__init__()
        stub = StubMobileNetV2()
        self.conv_stem, self.bn1, self.act1, self.blocks = stub.conv_stem, stub.bn1, stub.act1, stub.blocks
        self.blocks[1] = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1, groups=16, bias=False), nn.BatchNorm2d(16), nn.ReLU6(),
                                       nn.Conv2d(16, 24, 3, 2, 1, bias=False))


def test_backbone_on_hip_decision():
    assert Feature(MobileNetV2Features())._backbone_on_hip() is True
    assert Feature(StubMobileNetV2())._backbone_on_hip() is True
    assert Feature(ForeignGrouped())._backbone_on_hip() is False
    odd = MobileNetV2Features()
    odd.blocks[2][1].conv_dw = nn.Conv2d(192, 192, 5, 1, 2, groups=192, bias=False)      # not the geometry the kernel takes
    assert Feature(odd)._backbone_on_hip() is False


def bn_eval(bn, x):
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


@pytest.mark.parametrize("stride,cin,cout", [(1, 8, 8), (2, 8, 8), (1, 8, 12)])
def test_inverted_residual_forward_is_the_hand_written_expression(stride, cin, cout):
    m = InvertedResidual(cin, cout, stride)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=5))
    m.eval()
    x = torch.randn(2, cin, 7, 9, generator=torch.Generator().manual_seed(1)) * 3
    y = F.relu6(bn_eval(m.bn1, F.conv2d(x, m.conv_pw.weight)))
    y = F.relu6(bn_eval(m.bn2, F.conv2d(y, m.conv_dw.weight, None, stride, 1, 1, 6 * cin)))
    y = bn_eval(m.bn3, F.conv2d(y, m.conv_pwl.weight))
    ref = x + y if (stride == 1 and cin == cout) else y
    assert m.has_skip == (stride == 1 and cin == cout)
    with torch.no_grad():
        assert torch.equal(m(x), ref)
        assert torch.equal(inverted_residual(TORCH, m, x), ref)          # the layer function on the TORCH route: the same bits


def test_depthwise_separable_forward_is_the_hand_written_expression():
    m = DepthwiseSeparableConv(32, 16)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=6))
    m.eval()
    x = torch.randn(2, 32, 6, 10, generator=torch.Generator().manual_seed(2)) * 3
    y = F.relu6(bn_eval(m.bn1, F.conv2d(x, m.conv_dw.weight, None, 1, 1, 1, 32)))
    ref = bn_eval(m.bn2, F.conv2d(y, m.conv_pw.weight))
    with torch.no_grad():
        assert not m.has_skip and torch.equal(m(x), ref)
        assert torch.equal(depthwise_separable(TORCH, m, x), ref)


def test_cpu_tensors_raise_on_the_hip_and_train_functions(monkeypatch):
    conv, bn = nn.Conv2d(4, 4, 3, 1, 1, groups=4, bias=False), nn.BatchNorm2d(4).eval()
    x = torch.zeros(1, 4, 5, 6)
    with pytest.raises(DiffuVolumeError):
        hip_dwconv2d(conv, x, bn, ACT_RELU6)
    with pytest.raises(DiffuVolumeError):
        HIP.dwconv(conv, x, bn, ACT_RELU6)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_CONV2D", route)
        with pytest.raises(DiffuVolumeError):
            train2d.dwconv2d(x, conv.weight, 1)
        with pytest.raises(DiffuVolumeError):
            TRAIN.dwconv(conv, x, bn, ACT_RELU6)
    monkeypatch.delenv("DV_TRAIN_CONV2D")
    block = InvertedResidual(4, 4).eval()
    for walker in (hip_sequential, train_sequential):
        with pytest.raises(DiffuVolumeError):
            walker(nn.Sequential(block), x)


def test_plain_grouped_convolutions_stay_refused():
    """Depthwise layers reach the new kernels through the two block classes only."""
    conv = nn.Conv2d(4, 4, 3, 1, 1, groups=4, bias=False)
    with pytest.raises(DiffuVolumeError, match="no training route"):
        train2d.conv2d_any(conv, torch.zeros(1, 4, 5, 6))
    assert Feature(ForeignGrouped())._backbone_on_hip() is False


@pytest.mark.parametrize("walker,route", [(hip_sequential, "HIP"), (train_sequential, "training")])
def test_walkers_still_refuse_maxpool_with_their_message(walker, route):
    seq = nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.ReLU(), nn.Sequential(InvertedResidual(4, 4), nn.MaxPool2d(2)))
    with pytest.raises(DiffuVolumeError) as e:
        walker(seq, torch.zeros(1, 3, 8, 16))
    assert f"the 2-D front has no {route} route for MaxPool2d" in str(e.value)


def test_the_three_entries_are_rows_of_the_third_table_only():
    header = (ROOT / "include" / "diffuvolume_hip_volume_train.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {n: len(p.split(",")) for n, p in re.findall(r"\b(dv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    for name, nparams in ENTRIES.items():
        assert name in _lib.VOLUME_TRAIN_SIGNATURES, name
        assert decl[name] == nparams == len(_lib.VOLUME_TRAIN_SIGNATURES[name][1]), name
        assert name not in _lib.SIGNATURES and name not in _lib.TRAIN_SIGNATURES
        for other in ("diffuvolume_hip.h", "diffuvolume_hip_train.h"):
            assert name not in (ROOT / "include" / other).read_text(), (name, other)
    assert _lib.VOLUME_TRAIN_SIGNATURES["dv_dwconv3x3_bwd_workspace_floats"][2] == _lib.SIZE_ONLY
    for name in ("dv_dwconv3x3_f32", "dv_dwconv3x3_bwd_f32"):
        assert _lib.VOLUME_TRAIN_SIGNATURES[name][2] == _lib.held_by(
            "test_gpu_dwconv.py::test_dwconv_abi_offset_views_bounds_and_refusals")


def test_library_refuses_before_touching_the_device():
    from diffuvolume_amd import _build
    _build.build()
    lib = _lib.load()
    assert lib.dv_dwconv3x3_f32(None, None, None, None, None, 1, 1, 1, 1, 1, 0, 0.0, None) == -1
    assert lib.dv_dwconv3x3_bwd_f32(None, None, None, None, None, None, 1, 1, 1, 1, 1, None) == -1
    ws = lib.dv_dwconv3x3_bwd_workspace_floats
    assert ws(2, 5, 8, 10, 1) == 9 * 2 * 5 and ws(2, 5, 8, 10, 2) == 9 * 2 * 5          # one wave tile per plane
    assert ws(1, 1, 33, 300, 1) == 9 * 3 * 2                                 # two tiles of 256 columns, three bands of 16 rows
    assert ws(0, 5, 8, 10, 1) == 0 and ws(2, 5, 8, -1, 1) == 0 and ws(2, 5, 8, 10, 3) == 0
