"""MobileNetV2 (width 1.0) as IGEV's feature pyramid takes it from timm (KITTI15/core/extractor.py:327-361:
``timm.create_model('mobilenetv2_100', pretrained=True, features_only=True)``), written out here so that the real
backbone can be built, loaded from a reference checkpoint and run on the HIP kernels without timm.

`MobileNetV2Features` has the attributes `Feature(backbone)` takes -- ``conv_stem``, ``bn1``, ``act1`` and ``blocks``, an
nn.Sequential of seven nn.Sequential stages -- under timm's names, so ``feature.block3.1.0.conv_pw.weight`` and the like
load with ``strict=True``:

  stem      conv_stem Conv2d(3, 32, 3, 2, 1), bn1, act1 ReLU6
  stage 0   one DepthwiseSeparableConv 32 -> 16: conv_dw 3x3 stride 1, bn1, ReLU6, conv_pw 1x1, bn2 (no skip: 32 != 16)
  stage 1-6 InvertedResidual blocks, expansion 6:   blocks  out  stride of the first
                                                      2     24      2
                                                      3     32      2
                                                      4     64      2
                                                      3     96      1
                                                      3    160      2
                                                      1    320      1
            each: conv_pw 1x1 (in -> 6 in), bn1, ReLU6, conv_dw 3x3 at the block's stride, bn2, ReLU6, conv_pwl 1x1
            (6 in -> out), bn3, and the skip x + y when in == out and the stride is 1
All convolutions are bias-free; BatchNorm2d has eps 1e-5 and momentum 0.1; 306 state_dict entries in all.

The block classes' ``forward`` is the plain PyTorch expression.  `depthwise_separable` / `inverted_residual` are the same
blocks as functions of a route of igev_layers (registered in its ``_LAYERS``), which is how `Feature` runs them: on HIP the
1x1 layers run on ``Conv2dPlan`` (the skip as its ``residual``) and the 3x3 layers on ``dv_dwconv3x3_f32`` with the
BatchNorm folded and the ReLU6 inside the launch; on TRAIN every convolution is an autograd function on the HIP kernels
(``train2d.conv2d_any`` / ``train2d.dwconv2d``)."""
from __future__ import annotations

from torch import nn

from . import _lib
from .igev_layers import _LAYERS, ACT_NONE, ACT_RELU6, depthwise_stride

# (blocks, output channels, stride of the first block) of stages 1..6
STAGES = ((2, 24, 2), (3, 32, 2), (4, 64, 2), (3, 96, 1), (3, 160, 2), (1, 320, 1))
EXPANSION = 6
FEATURE_STAGES = (0, 1, 2, 4, 6)          # the stages whose outputs are the 1/2 .. 1/32 feature maps


def depthwise_separable(route, m, x):
    y = route.dwconv(m.conv_dw, x, m.bn1, ACT_RELU6)
    return route.conv(m.conv_pw, y, m.bn2, ACT_NONE, residual=x if m.has_skip else None)


def inverted_residual(route, m, x):
    y = route.conv(m.conv_pw, x, m.bn1, ACT_RELU6)
    y = route.dwconv(m.conv_dw, y, m.bn2, ACT_RELU6)
    return route.conv(m.conv_pwl, y, m.bn3, ACT_NONE, residual=x if m.has_skip else None)


class DepthwiseSeparableConv(nn.Module):
    """timm's block of the same name as mobilenetv2_100 builds it: depthwise 3x3 + BN + ReLU6, 1x1 + BN."""

    def __init__(self, in_chs, out_chs, stride=1):
        super().__init__()
        self.has_skip = stride == 1 and in_chs == out_chs
        self.conv_dw = nn.Conv2d(in_chs, in_chs, 3, stride, 1, groups=in_chs, bias=False)
        self.bn1 = nn.BatchNorm2d(in_chs)
        self.act1 = nn.ReLU6()
        self.conv_pw = nn.Conv2d(in_chs, out_chs, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        y = self.act1(self.bn1(self.conv_dw(x)))
        y = self.bn2(self.conv_pw(y))
        return x + y if self.has_skip else y


class InvertedResidual(nn.Module):
    """timm's block of the same name as mobilenetv2_100 builds it: 1x1 expand + BN + ReLU6, depthwise 3x3 + BN + ReLU6,
    1x1 project + BN, skip when the shapes allow."""

    def __init__(self, in_chs, out_chs, stride=1, exp_ratio=EXPANSION):
        super().__init__()
        mid = in_chs * exp_ratio
        self.has_skip = stride == 1 and in_chs == out_chs
        self.conv_pw = nn.Conv2d(in_chs, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.act1 = nn.ReLU6()
        self.conv_dw = nn.Conv2d(mid, mid, 3, stride, 1, groups=mid, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.act2 = nn.ReLU6()
        self.conv_pwl = nn.Conv2d(mid, out_chs, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_chs)

    def forward(self, x):
        y = self.act1(self.bn1(self.conv_pw(x)))
        y = self.act2(self.bn2(self.conv_dw(y)))
        y = self.bn3(self.conv_pwl(y))
        return x + y if self.has_skip else y


def _pointwise(conv) -> bool:
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None)


def block_on_hip(m) -> bool:
    """Whether ``m`` is one of the two block classes in the geometry the HIP routes take (what the constructors above
    build; a block whose layers were swapped for something else is not)."""
    if isinstance(m, DepthwiseSeparableConv):
        convs, norms = (m.conv_pw,), (m.bn1, m.bn2)
    elif isinstance(m, InvertedResidual):
        convs, norms = (m.conv_pw, m.conv_pwl), (m.bn1, m.bn2, m.bn3)
    else:
        return False
    try:
        depthwise_stride(m.conv_dw)
    except _lib.DiffuVolumeError:
        return False
    return all(_pointwise(c) for c in convs) and all(isinstance(n, nn.BatchNorm2d) for n in norms)


class MobileNetV2Features(nn.Module):
    """The module ``timm.create_model('mobilenetv2_100', features_only=True)`` returns, as far as `Feature` and a
    checkpoint see it: ``conv_stem``, ``bn1``, ``act1``, ``blocks``.  ``forward`` returns the five feature maps (1/2, 1/4,
    1/8, 1/16, 1/32 with 16, 24, 32, 96, 320 channels) as the plain PyTorch expression; `Feature` does not call it."""

    def __init__(self):
        super().__init__()
        self.conv_stem = nn.Conv2d(3, 32, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(32)
        self.act1 = nn.ReLU6()
        stages, cin = [nn.Sequential(DepthwiseSeparableConv(32, 16, 1))], 16
        for n, cout, stride in STAGES:
            stages.append(nn.Sequential(*[InvertedResidual(cin if i == 0 else cout, cout, stride if i == 0 else 1)
                                          for i in range(n)]))
            cin = cout
        self.blocks = nn.Sequential(*stages)

    def forward(self, x):
        x, outs = self.act1(self.bn1(self.conv_stem(x))), []
        for i, stage in enumerate(self.blocks):
            x = stage(x)
            if i in FEATURE_STAGES:
                outs.append(x)
        return outs


_LAYERS[DepthwiseSeparableConv] = depthwise_separable
_LAYERS[InvertedResidual] = inverted_residual
