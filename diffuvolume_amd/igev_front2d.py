"""IGEV's 2-D front: everything IGEVStereo_ddim.forward computes before the cost volume and the GRU loop
(KITTI15/core/igev_stereo_ddim.py:364-377 feature pyramid, stems, matching features; :395-398 context encoder and the
GRU's context terms), once per pair.  The pyramid (core/extractor.py:327-361), the context encoder (:190-295) and the
front are each one walk over a route of igev_layers: inference passes HIP, training TRAIN."""
from __future__ import annotations

from functools import partial, reduce
from typing import Optional

import torch
from torch import nn

from .igev_layers import (ACT_RELU, HIP, TORCH, TRAIN, BasicConv_IN, Conv2x_IN, ResidualBlock, _own_route,
                          _refuse_autocast, _require_cuda, _stem, _train_mode, _wants_autograd, basic_conv_in, conv2x,
                          freeze_bn, walk)
from .mobilenetv2 import block_on_hip
from .submodule import PlanCache


def context_encoder(route, m, x, dual_inp=False, num_layers=3):
    """MultiBasicEncoder.forward (core/extractor.py:258-295); an encoder of another class is called as is."""
    if not isinstance(m, MultiBasicEncoder):
        return m(x, num_layers=num_layers)
    x = walk(route, [m.layer1, m.layer2, m.layer3], route.conv(m.conv1, x, m.norm1, ACT_RELU))
    tail = ()
    if dual_inp:
        tail, x = (x,), x[:(x.shape[0] // 2)]
    outs = ([walk(route, f, x) for f in m.outputs04],)
    if num_layers >= 2:
        y = walk(route, m.layer4, x)
        outs += ([walk(route, f, y) for f in m.outputs08],)
    if num_layers >= 3:
        z = walk(route, m.layer5, y)
        outs += ([walk(route, f, z) for f in m.outputs16],)
    return outs + tail


class MultiBasicEncoder(nn.Module):
    """core/extractor.py:190-295: the context encoder (`cnet`)."""

    def __init__(self, output_dim=((128, 128, 128),), norm_fn="batch", dropout=0.0, downsample=3):
        super().__init__()
        self.norm_fn, self.downsample = norm_fn, downsample
        self.norm1 = nn.BatchNorm2d(64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=1 + (downsample > 2), padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 64
        self.layer1 = self._make_layer(64, stride=1)
        self.layer2 = self._make_layer(96, stride=1 + (downsample > 1))
        self.layer3 = self._make_layer(128, stride=1 + (downsample > 0))
        self.layer4 = self._make_layer(128, stride=2)
        self.layer5 = self._make_layer(128, stride=2)
        self.outputs04 = nn.ModuleList([nn.Sequential(ResidualBlock(128, 128, norm_fn, 1), nn.Conv2d(128, d[2], 3, padding=1))
                                        for d in output_dim])
        self.outputs08 = nn.ModuleList([nn.Sequential(ResidualBlock(128, 128, norm_fn, 1), nn.Conv2d(128, d[1], 3, padding=1))
                                        for d in output_dim])
        self.outputs16 = nn.ModuleList([nn.Conv2d(128, d[0], 3, padding=1) for d in output_dim])
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        layers = (ResidualBlock(self.in_planes, dim, self.norm_fn, stride=stride), ResidualBlock(dim, dim, self.norm_fn, 1))
        self.in_planes = dim
        return nn.Sequential(*layers)

    def forward(self, x, dual_inp=False, num_layers=3):
        return context_encoder(_own_route(x), self, x, dual_inp, num_layers)


def feature_pyramid(route, m, x):
    """Feature.forward (core/extractor.py:337-361); a feature module of another class is called as is."""
    if not isinstance(m, Feature):
        return m(x)
    # a backbone made of plain [Conv2d, BatchNorm2d, ReLU / ReLU6] stages (synth.StubMobileNetV2) or of the in-tree
    # MobileNetV2 blocks (mobilenetv2.MobileNetV2Features) is walked on the route; anything else (a timm object: its own
    # depth-wise / squeeze-excite block classes) is the injected module's own business
    stage = partial(walk, route) if m._backbone_on_hip() else (lambda mods, t: reduce(lambda v, f: f(v), mods, t))
    x2 = stage(m.block0, stage([m.conv_stem, m.bn1, m.act1], x))
    x4 = stage(m.block1, x2)
    x8 = stage(m.block2, x4)
    x16 = stage(m.block3, x8)
    x32 = stage(m.block4, x16)
    if route is HIP and _wants_autograd(x32):          # an injected backbone's outputs may ask for gradients where the image
        route = TORCH                                  # did not
    x16 = conv2x(route, m.deconv32_16, x32, x16)
    x8 = conv2x(route, m.deconv16_8, x16, x8)
    x4 = basic_conv_in(route, m.conv4, conv2x(route, m.deconv8_4, x8, x4))
    return [x4, x8, x16, x32]


class Feature(nn.Module):
    """core/extractor.py:327-361.  The reference takes its stem and blocks from
    ``timm.create_model('mobilenetv2_100', pretrained=True, features_only=True)``; neither timm nor the weights
    exist offline, so the backbone object is injected: anything with ``conv_stem``, ``bn1``, ``act1`` and ``blocks``
    (7 stages with 16/24/32/64/96/160/320 output channels) -- ``mobilenetv2.MobileNetV2Features`` (the real backbone
    under timm's names, on the HIP kernels), ``synth.StubMobileNetV2`` or a timm MobileNetV2 (which runs as it is)."""

    def __init__(self, backbone):
        super().__init__()
        chans = [16, 24, 32, 96, 160]
        cut = [1, 2, 3, 5, 6]
        self.conv_stem, self.bn1, self.act1 = backbone.conv_stem, backbone.bn1, backbone.act1
        blocks = list(backbone.blocks)
        self.block0 = nn.Sequential(*blocks[0:cut[0]])
        self.block1 = nn.Sequential(*blocks[cut[0]:cut[1]])
        self.block2 = nn.Sequential(*blocks[cut[1]:cut[2]])
        self.block3 = nn.Sequential(*blocks[cut[2]:cut[3]])
        self.block4 = nn.Sequential(*blocks[cut[3]:cut[4]])
        self.deconv32_16 = Conv2x_IN(chans[4], chans[3], deconv=True, concat=True)
        self.deconv16_8 = Conv2x_IN(chans[3] * 2, chans[2], deconv=True, concat=True)
        self.deconv8_4 = Conv2x_IN(chans[2] * 2, chans[1], deconv=True, concat=True)
        self.conv4 = BasicConv_IN(chans[1] * 2, chans[1] * 2, kernel_size=3, stride=1, padding=1)

    def _backbone_on_hip(self) -> bool:
        def plain(m):
            if isinstance(m, nn.Sequential):
                return all(plain(c) for c in m)
            if isinstance(m, nn.Conv2d):
                k = m.kernel_size[0]
                return (m.groups == 1 and m.dilation == (1, 1) and m.kernel_size == (k, k) and k in (1, 3)
                        and m.padding == (k // 2, k // 2) and m.stride[0] in (1, 2) and m.stride[0] == m.stride[1])
            return isinstance(m, (nn.BatchNorm2d, nn.ReLU, nn.ReLU6, nn.Identity)) or block_on_hip(m)
        return all(plain(m) for m in (self.conv_stem, self.bn1, self.act1, self.block0, self.block1, self.block2,
                                      self.block3, self.block4))

    def forward(self, x):
        return feature_pyramid(_own_route(x), self, x)


def _front2d(route, m, image1, image2, n_gru_layers):
    """:364-377 + :395-398 on the modules of ``m`` (an IGEVFront2d or the IGEVStereo_ddim itself) ->
    (features_left, stem_2x, match_left, match_right, net_list, inp_list).  ``route``: HIP, the inference kernels, or
    TRAIN (train mode with autograd recording)."""
    if route is TRAIN:
        _require_cuda(("image1", image1), ("image2", image2))
        _refuse_autocast("the 2-D front")
        image1, image2 = image1.float(), image2.float()
        feature, cnet = partial(feature_pyramid, TRAIN, m.feature), partial(context_encoder, TRAIN, m.cnet)
        feat_conv = partial(basic_conv_in, TRAIN, m.conv)
    else:                                # the three modules' own forwards: HIP, or TORCH for an input that asks for gradients
        feature, cnet, feat_conv = m.feature, m.cnet, m.conv
    image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
    features_left, features_right = feature(image1), feature(image2)
    stem_2x = walk(route, m.stem_2, image1)
    stem_4x = walk(route, m.stem_4, stem_2x)
    stem_4y = walk(route, m.stem_4, walk(route, m.stem_2, image2))
    features_left[0] = torch.cat((features_left[0], stem_4x), 1)
    features_right[0] = torch.cat((features_right[0], stem_4y), 1)
    match_left = route.conv(m.desc, feat_conv(features_left[0])).contiguous()
    match_right = route.conv(m.desc, feat_conv(features_right[0])).contiguous()
    cnet_list = cnet(image1, num_layers=n_gru_layers)
    net_list = [torch.tanh(x[0]) for x in cnet_list]
    inp_list = [torch.relu(x[1]) for x in cnet_list]
    inp_list = [list(route.conv(conv, i).split(split_size=conv.out_channels // 3, dim=1))
                for i, conv in zip(inp_list, m.context_zqr_convs)]
    inp_list = [[t.contiguous() for t in trio] for trio in inp_list]
    return features_left, stem_2x, match_left, match_right, net_list, inp_list


class IGEVFront2d(PlanCache, nn.Module):
    """The 2-D front's modules of IGEVStereo_ddim (:180-194 `feature`, `stem_2`, `stem_4`, `conv`, `desc`; :163-170 `cnet`,
    `context_zqr_convs`) under the reference's attribute names, and the parts of its forward that use them (:364-377,
    :395-398).  ``forward(image1, image2)`` (images in 0..255) returns ``(features_left, stem_2x, match_left, match_right,
    net_list, inp_list)``.  In eval mode (or under no_grad) it runs the inference kernels, the bits of
    IGEVStereo_ddim's own front; in train mode with autograd recording every layer is differentiable on the HIP kernels
    (the TRAIN route of igev_layers).  ``feature``: ``Feature(backbone)``, as for IGEVStereo_ddim."""

    def __init__(self, args, feature: nn.Module, cnet: Optional[nn.Module] = None):
        super().__init__()
        self.args = args
        hidden = list(args.hidden_dims)
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hidden, hidden], norm_fn="batch",
                                                                    downsample=args.n_downsample)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hidden[i], hidden[i] * 3, 3, padding=1)
                                                for i in range(args.n_gru_layers)])
        self.feature = feature
        self.stem_2, self.stem_4 = _stem(3, 32), _stem(32, 48)
        self.conv = BasicConv_IN(96, 96, kernel_size=3, padding=1, stride=1)
        self.desc = nn.Conv2d(96, 96, kernel_size=1, padding=0, stride=1)

    def _build_plans(self, slot):
        return {}                   # the front's inference plans live per layer (`hip_conv2d`), training builds them per call

    freeze_bn = freeze_bn

    def forward(self, image1, image2):
        return _front2d(TRAIN if _train_mode(self) else HIP, self, image1, image2, self.args.n_gru_layers)
