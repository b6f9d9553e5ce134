"""IGEV's once-per-pair cost-volume front (KITTI15/core/igev_stereo_ddim.py:377-386):
gwc volume (8 groups) -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier -> softmax -> regression.
Module and parameter names are the reference's, so its checkpoints load unchanged
(`corr_stem.conv.weight`, `cost_agg.feature_att_16.feat_att.1.bias`, ...)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, train2d, train3d
from .igev_layers import BasicConv, _require_cuda, _train_mode, hip_sequential
from .submodule import (ACT_NONE, Conv3dPlan, PlanCache, _gwc_volume_autograd, build_gwc_volume, feature_gate,
                        softmax_regress)


class FeatureAtt(nn.Module):
    """core/submodule.py:226-239: image-feature guided channel gate of a cost volume."""

    def __init__(self, cv_chan, feat_chan):
        super().__init__()
        self.feat_att = nn.Sequential(BasicConv(feat_chan, feat_chan // 2, kernel_size=1, stride=1, padding=0),
                                      nn.Conv2d(feat_chan // 2, cv_chan, 1))

    def forward(self, cv, feat, inplace=False):
        if _train_mode(self):                   # out of place: the gate's backward reads the ungated volume
            logit = train2d.conv2d_module(self.feat_att[1], self.feat_att[0].train_forward(feat))
            return train3d.feature_gate_train(cv, logit)
        return feature_gate(cv, hip_sequential(self.feat_att, feat), inplace=inplace)


def _seq_plans(seq):
    return [m.plan() for m in seq]


def _run(plans, x):
    for p in plans:
        x = p(x)
    return x


def _run_train(seq, x):
    for m in seq:
        x = m.train_forward(x)
    return x


class hourglass(PlanCache, nn.Module):
    """igev_stereo_ddim.py:24-91 (`hourglass(8)`, runs once per pair on the gated gwc volume)."""

    def __init__(self, in_channels):
        super().__init__()
        c = in_channels
        k3 = dict(is_3d=True, bn=True, relu=True, kernel_size=3, padding=1, dilation=1)
        self.conv1 = nn.Sequential(BasicConv(c, c * 2, stride=2, **k3), BasicConv(c * 2, c * 2, stride=1, **k3))
        self.conv2 = nn.Sequential(BasicConv(c * 2, c * 4, stride=2, **k3), BasicConv(c * 4, c * 4, stride=1, **k3))
        self.conv3 = nn.Sequential(BasicConv(c * 4, c * 6, stride=2, **k3), BasicConv(c * 6, c * 6, stride=1, **k3))
        up = dict(deconv=True, is_3d=True, kernel_size=(4, 4, 4), padding=(1, 1, 1), stride=(2, 2, 2))
        self.conv3_up = BasicConv(c * 6, c * 4, bn=True, relu=True, **up)
        self.conv2_up = BasicConv(c * 4, c * 2, bn=True, relu=True, **up)
        self.conv1_up = BasicConv(c * 2, 8, bn=False, relu=False, **up)

        def agg(cin, cout):
            return nn.Sequential(BasicConv(cin, cout, is_3d=True, kernel_size=1, padding=0, stride=1),
                                 BasicConv(cout, cout, is_3d=True, kernel_size=3, padding=1, stride=1),
                                 BasicConv(cout, cout, is_3d=True, kernel_size=3, padding=1, stride=1))

        self.agg_0 = agg(c * 8, c * 4)
        self.agg_1 = agg(c * 4, c * 2)
        self.feature_att_8 = FeatureAtt(c * 2, 64)
        self.feature_att_16 = FeatureAtt(c * 4, 192)
        self.feature_att_32 = FeatureAtt(c * 6, 160)
        self.feature_att_up_16 = FeatureAtt(c * 4, 192)
        self.feature_att_up_8 = FeatureAtt(c * 2, 64)

    def _build_plans(self, slot):
        p = {n: _seq_plans(getattr(self, n)) for n in ("conv1", "conv2", "conv3", "agg_0", "agg_1")}
        for n in ("conv3_up", "conv2_up", "conv1_up"):
            p[n] = getattr(self, n).plan()
        return p

    def _train_forward(self, x, features):
        conv1 = self.feature_att_8(_run_train(self.conv1, x), features[1])
        conv2 = self.feature_att_16(_run_train(self.conv2, conv1), features[2])
        conv3 = self.feature_att_32(_run_train(self.conv3, conv2), features[3])
        conv2 = _run_train(self.agg_0, torch.cat((self.conv3_up.train_forward(conv3), conv2), dim=1))
        conv2 = self.feature_att_up_16(conv2, features[2])
        conv1 = _run_train(self.agg_1, torch.cat((self.conv2_up.train_forward(conv2), conv1), dim=1))
        conv1 = self.feature_att_up_8(conv1, features[1])
        return self.conv1_up.train_forward(conv1)

    def forward(self, x, features):
        if _train_mode(self):
            return self._train_forward(x, features)
        p = self.plans()
        conv1 = self.feature_att_8(_run(p["conv1"], x), features[1], inplace=True)
        conv2 = self.feature_att_16(_run(p["conv2"], conv1), features[2], inplace=True)
        conv3 = self.feature_att_32(_run(p["conv3"], conv2), features[3], inplace=True)
        conv2 = _run(p["agg_0"], torch.cat((p["conv3_up"](conv3), conv2), dim=1))
        conv2 = self.feature_att_up_16(conv2, features[2], inplace=True)
        conv1 = _run(p["agg_1"], torch.cat((p["conv2_up"](conv2), conv1), dim=1))
        conv1 = self.feature_att_up_8(conv1, features[1], inplace=True)
        return p["conv1_up"](conv1)


def _cost_volume_plans(m):
    return m.corr_stem.plan(), Conv3dPlan(m.classifier.weight, None, stride=1, act=ACT_NONE)


def _cost_volume(m, match_left, match_right, features_left, max_disp):
    """IGEVStereo_ddim :378-386 on the modules of ``m`` (an IGEVCostVolume or the IGEVStereo_ddim itself): gwc (8 groups)
    -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier -> softmax + regression."""
    if _train_mode(m):
        return _cost_volume_train(m, match_left, match_right, features_left, max_disp)
    m.refresh_plans()
    stem, classifier = m.plans()
    gwc = stem(build_gwc_volume(match_left, match_right, max_disp // 4, 8))
    gwc = m.corr_feature_att(gwc, features_left[0], inplace=True)
    geo = m.cost_agg(gwc, features_left)
    return geo, softmax_regress(classifier(geo)).unsqueeze(1)          # F.softmax + disparity_regression :382-383


def _cost_volume_train(m, match_left, match_right, features_left, max_disp):
    """The same front for training (train mode with autograd recording): every convolution and gate an autograd function
    on the HIP kernels, BatchNorm / LeakyReLU / softmax / regression PyTorch, the gwc volume its differentiable expression
    (whether or not the features ask for gradients, so that a frozen backbone gives the same bits).  It stays on the
    statement and not on train_volume.build_gwc_volume_train: with the eval kernel's forward (8.97e-8 relative L2 from the
    statement's, rounding) and the HIP convolutions, the recorded step `even` of tests/test_gpu_igev_volume_train.py lands
    2.5e-3 from the float64 gradients against a bar of 1.2e-5, and within the bar on the statement."""
    _require_cuda(("match_left", match_left), ("match_right", match_right),
                  *((f"features_left[{i}]", f) for i, f in enumerate(features_left)))
    if match_left.dim() != 4 or match_left.shape != match_right.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(match_left.shape)} vs {tuple(match_right.shape)}")
    d, (h, w) = max_disp // 4, match_left.shape[2:]
    if d % 8 or h % 8 or w % 8:
        raise _lib.DiffuVolumeError(f"training the cost-volume front needs d, h, w of the 1/4-resolution volume to be "
                                    f"multiples of 8 (three stride-2 levels whose skips are concatenated), got {d} x {h} x {w}")
    gwc = _gwc_volume_autograd(match_left, match_right, d, 8)
    gwc = m.corr_feature_att(m.corr_stem.train_forward(gwc), features_left[0])
    geo = m.cost_agg(gwc, features_left)
    prob = F.softmax(train3d.conv3d_module(m.classifier, geo).squeeze(1), dim=1)            # :382
    disp_values = torch.arange(0, d, dtype=prob.dtype, device=prob.device).view(1, d, 1, 1)
    return geo, torch.sum(prob * disp_values, 1, keepdim=True)                               # disparity_regression :383


class IGEVCostVolume(PlanCache, nn.Module):
    """The volume-side modules of IGEVStereo_ddim (:196-199) and the part of its forward that uses them
    (:377-386).  ``forward(match_left, match_right, features_left)`` returns the geometry encoding volume
    [B,8,D/4,h,w] (what Combined_Geo_Encoding_Volume filters at every GRU iteration) and `init_disp`
    [B,1,h,w]."""

    def __init__(self, max_disp: int = 192):
        super().__init__()
        self.max_disp = max_disp
        self.corr_stem = BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1)
        self.corr_feature_att = FeatureAtt(8, 96)
        self.cost_agg = hourglass(8)
        self.classifier = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

    def _build_plans(self, slot):
        return _cost_volume_plans(self)

    def forward(self, match_left, match_right, features_left):
        return _cost_volume(self, match_left, match_right, features_left, self.max_disp)
