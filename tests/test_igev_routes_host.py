"""Host-side checks of IGEV's route layer (diffuvolume_amd/igev_layers.py): the split modules hand out the objects
`igev_stereo_ddim` always did, both walkers refuse the same members with the same messages before anything is launched,
and the shared layer functions on the TORCH route are the plain module-by-module PyTorch expression, bit for bit."""
import importlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd import igev_stereo_ddim as M
from diffuvolume_amd.igev_layers import TORCH, conv2x, residual_block

HOMES = {"igev_layers": ("hip_conv2d", "instance_norm_act", "hip_sequential", "train_sequential", "BasicConv", "BasicConv_IN",
                         "Conv2x", "Conv2x_IN", "ResidualBlock", "freeze_bn", "HIP", "TORCH", "TRAIN"),
         "igev_front2d": ("Feature", "MultiBasicEncoder", "IGEVFront2d"),
         "igev_volume": ("FeatureAtt", "hourglass", "IGEVCostVolume", "_run"),
         "igev_upsample": ("context_upsample", "ContextUpsampleFn", "IGEVUpsampler"),
         "igev_loop": ("DynamicHead180", "round_gru_inputs_f16", "IGEVDiffusionLoop")}


@pytest.mark.parametrize("home", sorted(HOMES))
def test_reexports_are_the_same_objects(home):
    mod = importlib.import_module(f"diffuvolume_amd.{home}")
    for name in HOMES[home]:
        assert getattr(M, name) is getattr(mod, name), name
    assert M.IGEVStereo_ddim.__module__ == "diffuvolume_amd.igev_stereo_ddim"


@pytest.mark.parametrize("walker", ["hip_sequential", "train_sequential"])
@pytest.mark.parametrize("tail, message", [
    ([nn.InstanceNorm2d(4, affine=True)], "InstanceNorm2d on the HIP front: affine=False, no running statistics"),
    ([nn.InstanceNorm2d(4, track_running_stats=True)], "InstanceNorm2d on the HIP front: affine=False, no running statistics"),
    ([nn.BatchNorm2d(4), nn.LeakyReLU(0.2)], "LeakyReLU on the HIP front: negative_slope 0.01"),
    ([nn.ReLU(), nn.MaxPool2d(2)], "the 2-D front has no {route} route for MaxPool2d")])
def test_both_walkers_refuse_the_same_members_before_any_launch(walker, tail, message):
    """On the CPU: the invalid member comes after a valid convolution, so a walker that launched before it had parsed the
    whole list would fail on the CPU tensor (another message) first."""
    seq = nn.Sequential(nn.Conv2d(3, 4, 3, padding=1), nn.ReLU(), nn.Sequential(nn.Conv2d(4, 4, 3, padding=1), *tail))
    with pytest.raises(DiffuVolumeError) as e:
        getattr(M, walker)(seq, torch.zeros(1, 3, 8, 16))
    assert message.format(route={"hip_sequential": "HIP", "train_sequential": "training"}[walker]) in str(e.value)


def test_residual_block_on_the_torch_route_is_the_plain_expression():
    torch.manual_seed(3)
    m = M.ResidualBlock(6, 10, "batch", stride=2).eval()
    x = torch.randn(1, 6, 8, 16, requires_grad=True)
    y = F.relu(m.norm1(m.conv1(x)))
    y = F.relu(m.norm2(m.conv2(y)))
    ref = F.relu(m.norm3(m.downsample[0](x)) + y)
    for out in (residual_block(TORCH, m, x), m(x)):                   # the module's own forward picks TORCH for this input
        assert out.requires_grad and torch.equal(out, ref)
    (g,), (g_ref,) = torch.autograd.grad(m(x).square().sum(), x), torch.autograd.grad(ref.square().sum(), x)
    assert torch.equal(g, g_ref)


@pytest.mark.parametrize("deconv", [True, False])
def test_conv2x_in_on_the_torch_route_is_the_plain_expression(deconv):
    torch.manual_seed(4)
    m = M.Conv2x_IN(6, 4, deconv=deconv)
    x = torch.randn(1, 6, 8, 16, requires_grad=True)
    rem = torch.randn(1, 4, 16, 32) if deconv else torch.randn(1, 4, 4, 8)
    y = F.leaky_relu(m.conv1.IN(m.conv1.conv(x)), 0.01)
    ref = F.leaky_relu(m.conv2.IN(m.conv2.conv(torch.cat((y, rem), 1))), 0.01)
    for out in (conv2x(TORCH, m, x, rem), m(x, rem)):
        assert out.requires_grad and torch.equal(out, ref)
    # a skip tensor of another size: the stride-2 output is resized to it (nearest) before the concatenation
    odd = torch.randn(1, 4, 5, 9)
    y = F.interpolate(y, size=(5, 9), mode="nearest")
    ref = F.leaky_relu(m.conv2.IN(m.conv2.conv(torch.cat((y, odd), 1))), 0.01)
    assert torch.equal(conv2x(TORCH, m, x, odd), ref)
