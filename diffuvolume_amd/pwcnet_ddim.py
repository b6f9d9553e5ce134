"""PCWNet + DiffuVolume (KITTI12 flavour) behind the reference's module API.

Drop-in for ``PWCNet_ddim`` of KITTI12/models/pwcnet_ddim.py:335-758 (eval path): same
constructor, ``forward(left, right, used, disp, mask) -> ([disp_finetune], [pred3_volume])``,
``model_predictions`` and ``ddim_sample``; same parameter / buffer names (reference
``state_dict`` loads with ``strict=True``).

HIP (libdiffuvolume_hip.so): the four group-wise-correlation and concat volumes (KITTI12
zero-fill flavour), dres0/dres1, ``hourglassup`` and, per DDIM step, the volume filter, the three
Mish hourglasses, ``classif3``, the align_corners=True trilinear/softmax/regression tail with the
uncertainty taken about the *refined* disparity, the two-hot re-encoding and the DDIM update.
Also HIP: the per-step 2-D refinement network ``refinenet3`` (dilated 3x3 convbn +
Mish, BasicBlocks, 1x1 downsamples) on the 2-D implicit-GEMM kernel (csrc/conv2d.hip).
The multi-scale 2-D feature CNN runs on the same 2-D kernel; PyTorch keeps the bilinear feature upsampling and the
concatenations.
Differences from the ACV flavour: x_T = randn, 3 steps, fill = cumulative
q_sample(asd), thresholds dif<1 & unc<1, ensemble [0.9,0,0,0.1], Mish activations.
Training (``model.train()``, the reference's :643-735 branch): ``forward`` returns
``[pred0, combine, pred1, pred2, pred3, disp_finetune]`` with the 3-D convolutions on ``train3d.py``, the BatchNorm3d +
Mish behind them on ``train_norm.py``, the 2-D convolutions of ``refinenet3`` on ``train2d.py`` and the rest (feature
CNN, BatchNorm2d and its Mish, the resize of ``finetune_feature``; ``dispupsample`` in float64) on PyTorch autograd -- with
``DV_TRAIN_NET2D=hip`` the feature CNN, BatchNorm2d + Mish and the resize run on ``train_net2d.py``; on CPU tensors it raises.
The containers (convbn, BasicBlock, the hourglass, ``Mish``), their prepared plans and the walk that runs a Sequential in
training are ``net_blocks.py``'s, shared with the ACV flavour; the training filter is ``ddim.train_filter``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, ddim, net_blocks, train2d, train3d, train_net2d
from .acv_ddim import ProbVolumeHandle
from .head import DynamicHead
from .net_blocks import (BasicBlockPlan, Mish, PairPlan, cb2, cb3, deconv_plan, head2d, init_weights, plan_cb2, plan_cb3,
                         plan_seq2d, run_plans, stack, walk)
from .plans import settle_build
from .train_tail import regress_head
from .train_refine import warp_corr_train
from .train_norm import act_statement
from .submodule import (ACT_MISH, ACT_NONE, Conv2dPlan, Conv3dPlan, PlanCache, _dev_f32, build_concat_volume,
                        build_gwc_volume, check_split_overflow, refine_inputs,
                        upsample_softmax_regress)


class FeatureExtraction(PlanCache, nn.Module):
    """Multi-scale 2-D feature CNN (pwcnet_ddim.py:12-128): gw1..gw4 at 1/4..1/32, concat features,
    refinement feature.  On the GPU (eval) every convolution runs on the 2-D HIP kernel."""

    STACKS = ("layer1", "layer2", "layer3", "layer4", "layer5", "layer7", "layer9")

    def __init__(self, concat_feature=False, concat_feature_channel=12):
        super().__init__()
        self.concat_feature = concat_feature
        self.firstconv = nn.Sequential(cb2(3, 32, 3, 2, 1, 1), Mish(), cb2(32, 32, 3, 1, 1, 1), Mish(),
                                       cb2(32, 32, 3, 1, 1, 1), Mish())
        self.layer1 = stack(32, 32, 3, 1, 1, 1, "mish")
        self.layer2 = stack(32, 64, 16, 2, 1, 1, "mish")
        self.layer3 = stack(64, 128, 3, 1, 1, 1, "mish")
        self.layer4 = stack(128, 128, 3, 1, 1, 2, "mish")
        self.layer5 = stack(128, 192, 3, 2, 1, 1, "mish")
        self.layer7 = stack(192, 256, 3, 2, 1, 1, "mish")
        self.layer9 = stack(256, 512, 3, 2, 1, 1, "mish")
        self.gw2 = head2d(192, 320, 320)
        self.gw3 = head2d(256, 320, 320)
        self.gw4 = head2d(512, 320, 320)
        self.layer11 = head2d(320, 320, 320)
        self.layer_refine = nn.Sequential(cb2(320, 128, 3, 1, 1, 1), Mish(), cb2(128, 32, 1, 1, 0, 1), Mish())
        if concat_feature:
            self.lastconv = head2d(320, 128, concat_feature_channel)
            self.concat2 = head2d(192, 128, concat_feature_channel)
            self.concat3 = head2d(256, 128, concat_feature_channel)
            self.concat4 = head2d(512, 128, concat_feature_channel)

    # ---- HIP plans (csrc/conv2d.hip: BN / Mish / residual fused), rebuilt when the parameters change ----
    def _build_plans(self, slot):
        if slot == train_net2d.SLOT:
            return train_net2d.build_plans(self)
        heads = ("gw2", "gw3", "gw4", "layer11") + (("lastconv", "concat2", "concat3", "concat4") if self.concat_feature else ())
        with torch.no_grad():
            p = {"firstconv": plan_seq2d(self.firstconv)}
            for n in self.STACKS:
                p[n] = [BasicBlockPlan(b) for b in getattr(self, n)]
            for n in heads + ("layer_refine",):
                p[n] = plan_seq2d(getattr(self, n))
        return p

    def _graph(self, x, stack, head):
        """The network, once for its three routes: ``stack(name, x)`` runs a layer of BasicBlocks, ``head(name, x)`` a
        plain Sequential (firstconv, the gw / concat heads, layer_refine)."""
        x = stack("layer1", head("firstconv", x))
        l2 = stack("layer2", x)
        l3 = stack("layer3", l2)
        l4 = stack("layer4", l3)
        l5 = stack("layer5", l4)
        l6 = stack("layer7", l5)
        l7 = stack("layer9", l6)
        fc = torch.cat((l2, l3, l4), dim=1)
        out = {"gw1": head("layer11", fc), "gw2": head("gw2", l5), "gw3": head("gw3", l6), "gw4": head("gw4", l7)}
        if self.concat_feature:
            out.update(concat_feature1=head("lastconv", fc), finetune_feature=head("layer_refine", fc),
                       concat_feature2=head("concat2", l5), concat_feature3=head("concat3", l6),
                       concat_feature4=head("concat4", l7))
        return out

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.DiffuVolumeError(f"input is on {x.device}: the feature CNN runs on the MI355X (no CPU fallback)")
        if self.training and train_net2d.route() == "hip":
            n = train_net2d.Net2d(self)                     # training on the HIP route of `train_net2d`
            return self._graph(x, lambda k, t: n.stack(getattr(self, k), t), lambda k, t: n.seq(getattr(self, k), t))
        if self.training or (torch.is_grad_enabled() and x.requires_grad):
            return self._forward_modules(x)
        p = self.prepare(check_weights=True)
        plan = lambda k, t: run_plans(p[k], t)
        with torch.no_grad():
            return self._graph(x, plan, plan)

    def _forward_modules(self, x):
        """The graph on the plain nn.Modules (training / autograd on the GPU; reference for the tests)."""
        module = lambda k, t: getattr(self, k)(t)
        return self._graph(x, module, module)


class RefineNet(nn.Module):
    """refinenet_version3 (pwcnet_ddim.py:251-306): dilated 2-D residual stack -> disparity residual."""

    def __init__(self, in_channels):
        super().__init__()
        self.conv1 = nn.Sequential(cb2(in_channels, 128, 3, 1, 1, 1), Mish())
        self.conv2 = nn.Sequential(cb2(128, 128, 3, 1, 1, 1), Mish())
        self.conv3 = nn.Sequential(cb2(128, 128, 3, 1, 2, 2), Mish())
        self.conv4 = nn.Sequential(cb2(128, 128, 3, 1, 4, 4), Mish())
        self.conv5 = stack(128, 96, 1, 1, 1, 8, "mish")
        self.conv6 = stack(96, 64, 1, 1, 1, 16, "mish")
        self.conv7 = stack(64, 32, 1, 1, 1, 1, "mish")
        self.conv8 = nn.Conv2d(32, 1, 3, 1, 1, bias=False)

    def forward(self, x, disp):
        for m in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5, self.conv6, self.conv7, self.conv8):
            x = m(x)
        return disp + x

    def train_forward(self, x, disp):
        """pwcnet_ddim.py:292-306 in training: every convolution on `train2d`; with DV_TRAIN_NET2D=hip a BatchNorm2d runs
        on `train_net2d.bn_act2d` with the Mish or the block's skip behind it."""
        n = train_net2d.Net2d(conv2d=train2d.conv2d_module)
        for m in (self.conv1, self.conv2, self.conv3, self.conv4):
            x = n.seq(m, x)
        for m in (self.conv5, self.conv6, self.conv7):
            x = n.stack(m, x)
        return disp + n.seq(self.conv8, x)


class HourglassUp(nn.Module):
    """Parameters of hourglassup (pwcnet_ddim.py:131-205): fuses the 1/8, 1/16, 1/32 volumes."""

    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv3d(c, 2 * c, 3, 2, 1, bias=False)
        self.conv2 = nn.Sequential(cb3(2 * c, 2 * c, 3, 1, 1), Mish())
        self.conv3 = nn.Conv3d(2 * c, 4 * c, 3, 2, 1, bias=False)
        self.conv4 = nn.Sequential(cb3(4 * c, 4 * c, 3, 1, 1), Mish())
        self.conv5 = nn.Conv3d(4 * c, 4 * c, 3, 2, 1, bias=False)
        self.conv6 = nn.Sequential(cb3(4 * c, 4 * c, 3, 1, 1), Mish())
        self.conv7 = nn.Sequential(nn.ConvTranspose3d(4 * c, 4 * c, 3, padding=1, output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(4 * c))
        self.conv8 = nn.Sequential(nn.ConvTranspose3d(4 * c, 2 * c, 3, padding=1, output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(2 * c))
        self.conv9 = nn.Sequential(nn.ConvTranspose3d(2 * c, c, 3, padding=1, output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(c))
        self.combine1 = nn.Sequential(cb3(4 * c, 2 * c, 3, 1, 1), Mish())
        self.combine2 = nn.Sequential(cb3(6 * c, 4 * c, 3, 1, 1), Mish())
        self.combine3 = nn.Sequential(cb3(6 * c, 4 * c, 3, 1, 1), Mish())
        self.redir1 = cb3(c, c, 1, 1, 0)
        self.redir2 = cb3(2 * c, 2 * c, 1, 1, 0)
        self.redir3 = cb3(4 * c, 4 * c, 1, 1, 0)

    def forward(self, x, f4, f5, f6):
        """Training path (pwcnet_ddim.py:181-205); eval runs ``_HourglassUpPlan``."""
        c2 = walk(self.conv2, walk(self.combine1, torch.cat((walk(self.conv1, x), f4), dim=1)))
        c4 = walk(self.conv4, walk(self.combine2, torch.cat((walk(self.conv3, c2), f5), dim=1)))
        c6 = walk(self.conv6, walk(self.combine3, torch.cat((walk(self.conv5, c4), f6), dim=1)))
        c7 = walk(self.conv7, c6, "mish", skip=walk(self.redir3, c4))
        c8 = walk(self.conv8, c7, "mish", skip=walk(self.redir2, c2))
        return walk(self.conv9, c8, "mish", skip=walk(self.redir1, x))


class Hourglass(net_blocks.Hourglass):
    """Parameters of the Mish hourglass (pwcnet_ddim.py:208-248): no bottleneck attention."""

    def __init__(self, c):
        super().__init__(c, "mish")


# ---- prepared hot-path layers ---------------------------------------------------------------------
class _HourglassPlan(net_blocks.HourglassPlan):
    """With the members of a step's first hourglass, whose input is filtered (``in_scale``)."""

    def __init__(self, hg: Hourglass):
        super().__init__(hg, filtered=True)


class _HourglassUpPlan:
    def __init__(self, m: HourglassUp):
        self.conv1 = Conv3dPlan(m.conv1.weight, None, stride=2, act=ACT_NONE)
        self.conv3 = Conv3dPlan(m.conv3.weight, None, stride=2, act=ACT_NONE)
        self.conv5 = Conv3dPlan(m.conv5.weight, None, stride=2, act=ACT_NONE)
        self.conv2 = plan_cb3(m.conv2[0], 1, ACT_MISH)
        self.conv4 = plan_cb3(m.conv4[0], 1, ACT_MISH)
        self.conv6 = plan_cb3(m.conv6[0], 1, ACT_MISH)
        self.combine1 = plan_cb3(m.combine1[0], 1, ACT_MISH)
        self.combine2 = plan_cb3(m.combine2[0], 1, ACT_MISH)
        self.combine3 = plan_cb3(m.combine3[0], 1, ACT_MISH)
        self.conv7 = deconv_plan(m.conv7, ACT_MISH, m.redir3)
        self.conv8 = deconv_plan(m.conv8, ACT_MISH, m.redir2)
        self.conv9 = deconv_plan(m.conv9, ACT_MISH, m.redir1)

    def __call__(self, x, f4, f5, f6):
        c1 = self.combine1(torch.cat((self.conv1(x), f4), dim=1))
        c2 = self.conv2(c1)
        c3 = self.combine2(torch.cat((self.conv3(c2), f5), dim=1))
        c4 = self.conv4(c3)
        c5 = self.combine3(torch.cat((self.conv5(c4), f6), dim=1))
        c6 = self.conv6(c5)
        c7 = self.conv7(c6, skip=c4)
        c8 = self.conv8(c7, skip=c2)
        return self.conv9(c8, skip=x)


def space_to_batch2(x: torch.Tensor) -> torch.Tensor:
    """[N,C,h,w] -> [4N,C,h/2,w/2]: sub-image (y & 1, x & 1) of item n becomes item 4n + 2(y & 1) + (x & 1) (HIP)."""
    n, c, h, w = x.shape
    out = torch.empty((4 * n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    _lib.launch("dv_space_to_batch2_f32", x.device, x.data_ptr(), out.data_ptr(), n, c, h, w)
    return out


def batch_to_space(x: torch.Tensor, levels: int) -> torch.Tensor:
    """The inverse of ``levels`` applications of `space_to_batch2` at once (HIP)."""
    n, c, h, w = x.shape
    b = n >> (2 * levels)
    out = torch.empty((b, c, h << levels, w << levels), dtype=torch.float32, device=x.device)
    _lib.launch("dv_batch_to_space_f32", x.device, x.data_ptr(), out.data_ptr(), b, c, h << levels, w << levels, levels)
    return out


class _RefinePlan:
    """refinenet_version3.forward (pwcnet_ddim.py:292-306) on the 2-D implicit-GEMM kernel."""

    # Round 5: the dilated layers run in the sub-image domain (csrc/refine_inputs.hip, `space_to_batch2`): a layer whose
    # dilation is twice that of the tensor's current de-interleave gets one more de-interleave by 2 in front and is then a
    # plain dense convolution -- loads and stores of whole cache lines instead of 4-byte accesses at a 4 d-byte stride
    # (conv2d_wino issued 0.34 of the matrix pipe at d = 8 and 0.56 at d = 1), and the d = 16 block, too far apart for the
    # dilated Winograd kernel, becomes a Winograd layer as well.  Pointwise members of a block (1x1 down-sampling,
    # BatchNorm, Mish, the skip add) do not care.  Same arithmetic per output as the dilated kernel (which is the
    # dilation-1 kernel on a sub-image).  `sub_image_domain = False` keeps every layer on the image as it lies.
    sub_image_domain = True

    def __init__(self, m: RefineNet):
        self.mods = [getattr(m, n)[0] for n in ("conv1", "conv2", "conv3", "conv4")]        # convbn of the four head layers
        self.mods += [b for n in ("conv5", "conv6", "conv7") for b in getattr(m, n)]        # BasicBlocks
        self.dils = [mod[0].dilation[0] if isinstance(mod, nn.Sequential) else mod.conv2[0].dilation[0] for mod in self.mods]
        self._cache = {}
        self.conv8 = Conv2dPlan(m.conv8.weight, None, dilation=1, act=ACT_NONE)
        self.chain_ok = all(d & (d - 1) == 0 for d in self.dils)       # powers of two

    def plan(self, i, dil):
        """Layer i with `dil` of its dilation left to the kernel (the rest is in the tensor's de-interleave level)."""
        if (i, dil) not in self._cache:
            mod = self.mods[i]
            plan = plan_cb2(mod, ACT_MISH, dil) if isinstance(mod, nn.Sequential) else BasicBlockPlan(mod, dil)
            settle_build(self.conv8.wpacked.device)    # built on first use, after PlanCache.plans() returned: same guarantee
            self._cache[(i, dil)] = plan
        return self._cache[(i, dil)]

    PAD_LIMIT = 1.15

    @staticmethod
    def max_level(h, w):
        """How often an h x w plane may be de-interleaved before the 16 x 16 tiles of the Winograd kernel pad the sub-planes
        by more than 15 % (384 x 1248: three times -- 48 x 156; a fourth gives 24 x 78 planes computed as 32 x 80 -- measured with
        PAD_LIMIT = 1.4: 120.9 against 118.1 ms per batch of 4, the d = 16 block no faster dense than strided)."""
        lvl = 0
        while h % 2 == 0 and w % 2 == 0:
            h, w = h // 2, w // 2
            if (-(-h // 16) * 16) * (-(-w // 16) * 16) > _RefinePlan.PAD_LIMIT * h * w:
                break
            lvl += 1
        return lvl

    def __call__(self, x, disp):
        h, w = x.shape[-2], x.shape[-1]
        lmax = self.max_level(h, w)
        if not (self.sub_image_domain and self.chain_ok and lmax > 0 and max(self.dils) > 1):
            for i, d in enumerate(self.dils):
                x = self.plan(i, d)(x)
            return self.conv8(x, residual=disp)      # disp + conv8(conv7)
        want = [min(d.bit_length() - 1, lmax) for d in self.dils]      # de-interleave level every layer runs at
        level = 0                                    # x is de-interleaved `level` times: [B * 4^level, C, h >> level, w >> level]
        for i, d in enumerate(self.dils):
            if want[i] < level:                      # back on the image (the dilation-1 tail of the stack)
                x = batch_to_space(x, level)
                level = 0
            while level < want[i]:
                x = space_to_batch2(x)
                level += 1
            plan = self.plan(i, d >> level)
            # a plain convolution in front of a level step stores its result de-interleaved itself
            # (`dv_conv2d_wino_s2b_f32`): no separate pass over the tensor
            nxt = want[i + 1] if i + 1 < len(self.dils) else 0
            fuse = (nxt == level + 1 and isinstance(plan, Conv2dPlan) and plan.wino_packed is not None and plan.dilation == 1
                    and x.shape[-2] % 2 == 0 and x.shape[-1] % 2 == 0)
            if fuse:
                x = plan(x, group=4 ** level, s2b_out=True)
                level += 1
            else:
                x = plan(x, group=4 ** level) if isinstance(plan, Conv2dPlan) else plan(x, 4 ** level)
        if level:
            x = batch_to_space(x, level)
        return self.conv8(x, residual=disp)          # disp + conv8(conv7)


class _Plans:
    def __init__(self, m: "PWCNet_ddim"):
        self.dres0 = PairPlan(m.dres0)
        self.dres1 = PairPlan(m.dres1)
        self.combine1 = _HourglassUpPlan(m.combine1)
        self.dres2, self.dres3, self.dres4 = (_HourglassPlan(h) for h in (m.dres2, m.dres3, m.dres4))
        self.classif3 = PairPlan(m.classif3)
        self.refinenet3 = _RefinePlan(m.refinenet3)
        conv, bn = m.dispupsample[0][0], m.dispupsample[0][1]          # 1x1 conv (1 -> 32) + BN folded to a*d + b
        g = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
        self.du_a = (conv.weight.detach().float().reshape(-1) * g).contiguous()
        self.du_b = (bn.bias.detach().float() - bn.running_mean.detach().float() * g).contiguous()
        # the origin network has no schedule
        self.ddim = ddim.Tables(m.alphas_cumprod) if hasattr(m, "alphas_cumprod") else None


def groupwise_corr_pm(ref: torch.Tensor, tgt: torch.Tensor, maxdisp: int) -> torch.Tensor:
    """build_corrleation_volume(ref, tgt, maxdisp, 1) squeezed (KITTI12/models/submodule.py:121-135):
    mean over channels of ref(x) * tgt(x - i) for i >= 0; for i < 0 the reference's slices pair the first
    |i| columns of ref with the last |i| columns of tgt -- kept literally.  [B, 2*maxdisp+1, H, W]."""
    b, c, h, w = ref.shape
    out = ref.new_zeros(b, 2 * maxdisp + 1, h, w)
    for i in range(-maxdisp, maxdisp + 1):
        if i > 0:
            out[:, i + maxdisp, :, i:] = (ref[..., i:] * tgt[..., :-i]).mean(dim=1)
        elif i < 0:   # as written in the reference: `[:-i]` (first |i| columns) against `[i:]` (last |i| columns)
            out[:, i + maxdisp, :, :-i] = (ref[..., :-i] * tgt[..., i:]).mean(dim=1)
        else:
            out[:, maxdisp] = (ref * tgt).mean(dim=1)
    return out


def warp(x: torch.Tensor, disp: torch.Tensor) -> torch.Tensor:
    """warp (KITTI12/models/submodule.py:137-175) as written there: the grid is normalised by W-1 / H-1 but sampled
    with grid_sample's default align_corners=False (bilinear, zero padding); the mask is the grid_sample of ones set to
    0 below 0.999 and to 1 elsewhere (it carries no gradient, every entry is overwritten).  The gradient reaches
    ``disp`` through the sampling grid."""
    b, c, h, w = x.shape
    xx = torch.arange(0, w, device=x.device).view(1, 1, 1, w).expand(b, 1, h, w).to(x.dtype)
    yy = torch.arange(0, h, device=x.device).view(1, 1, h, 1).expand(b, 1, h, w).to(x.dtype)
    gx = 2.0 * (xx - disp) / max(w - 1, 1) - 1.0
    gy = 2.0 * yy / max(h - 1, 1) - 1.0
    grid = torch.cat((gx, gy), 1).permute(0, 2, 3, 1)
    out = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    with torch.no_grad():
        ones = torch.ones((b, 1, h, w), dtype=x.dtype, device=x.device)       # equal in every channel
        mask = (F.grid_sample(ones, grid, mode="bilinear", padding_mode="zeros", align_corners=False) >= 0.999).to(x.dtype)
    return out * mask


class _PWCCommon(PlanCache):
    """What the origin network (`PWCNet`, pwcnet.py:310-507) and `PWCNet_ddim` share: the plan cache, the fused
    multi-scale volume and the 2-D refinement of a regressed disparity."""

    def _build_plans(self, slot) -> _Plans:
        dev = self.dres0[0][0].weight.device
        if dev.type != "cuda":
            raise _lib.DiffuVolumeError("PWCNet_ddim hot path needs the model on the MI355X; no CPU fallback")
        with torch.no_grad(), torch.cuda.device(dev):
            return _Plans(self)

    def _volumes(self, fl, fr):
        """pwcnet_ddim.py:608-627: the four group-wise-correlation (+ concat) volumes at 1/4 .. 1/32."""
        vols = []
        for i, div in enumerate((4, 8, 16, 32), start=1):
            v = build_gwc_volume(fl[f"gw{i}"], fr[f"gw{i}"], self.maxdisp // div, self.num_groups)
            if self.use_concat_volume:
                cv = build_concat_volume(fl[f"concat_feature{i}"], fr[f"concat_feature{i}"], self.maxdisp // div,
                                         zero_left=True)
                v = torch.cat((v, cv), 1)
            vols.append(v)
        return vols

    @torch.no_grad()
    def fused_volume(self, fl, fr):
        """pwcnet_ddim.py:608-641: four gwc(+concat) volumes -> dres0/dres1 -> hourglassup -> `combine`."""
        p = self.prepare()
        vols = self._volumes(fl, fr)
        cost0 = p.dres0(vols[0])
        cost0 = p.dres1(cost0, residual_self=True)
        return p.combine1(cost0, vols[1], vols[2], vols[3])

    def _init_backbone(self, use_concat_volume: bool, time_embedding: bool):
        """Sub-modules under the reference's attribute names, in its construction order (pwcnet.py:318-362,
        pwcnet_ddim.py:389-431), and its weight initialisation (:364-381 / :433-447)."""
        self.concat_channels = 12 if use_concat_volume else 0
        self.feature_extraction = FeatureExtraction(use_concat_volume, 12)
        cin = self.num_groups + 2 * self.concat_channels
        self.dres0 = nn.Sequential(cb3(cin, 32, 3, 1, 1), Mish(), cb3(32, 32, 3, 1, 1), Mish())
        self.dres1 = nn.Sequential(cb3(32, 32, 3, 1, 1), Mish(), cb3(32, 32, 3, 1, 1))
        self.combine1 = HourglassUp(32)
        if time_embedding:
            self.time_embedding = DynamicHead(d_model=48)
        self.dres2, self.dres3, self.dres4 = Hourglass(32), Hourglass(32), Hourglass(32)
        for i in range(5):
            setattr(self, f"classif{i}", nn.Sequential(cb3(32, 32, 3, 1, 1), Mish(), nn.Conv3d(32, 1, 3, 1, 1, bias=False)))
        self.refinenet3 = RefineNet(146)
        self.dispupsample = nn.Sequential(cb2(1, 32, 1, 1, 0, 1), Mish())
        init_weights(self)

    @staticmethod
    def refine_features(features_left, features_right, size):
        """pwcnet_ddim.py:487-492 / pwcnet.py:481-486: both `finetune_feature` maps resized to full resolution
        (bilinear, align_corners=True).  They do not depend on the DDIM step: `ddim_sample` resizes them once per
        call instead of once per step."""
        hh, ww = size
        fl = F.interpolate(features_left["finetune_feature"], [hh, ww], mode="bilinear", align_corners=True)
        fr = F.interpolate(features_right["finetune_feature"], [hh, ww], mode="bilinear", align_corners=True)
        return fl, fr

    def _refine(self, pred3, features_left, features_right, resized=None):
        """pwcnet_ddim.py:486-502: warp the right refinement feature by pred3, +-24 correlation, concat
        (one HIP kernel), refinenet3 (2-D implicit-GEMM kernel) -> disp_finetune [B,H,W].  ``resized``: the two
        full-resolution feature maps of `refine_features` when the caller already has them."""
        p3 = pred3.unsqueeze(1)
        fl, fr = resized if resized is not None else self.refine_features(features_left, features_right, pred3.shape[-2:])
        plans = self.prepare()
        comb = refine_inputs(fl, fr, p3, plans.du_a, plans.du_b, 24)      # warp, +-24 correlation, concat
        return plans.refinenet3(comb, p3.contiguous()).squeeze(1)


class PWCNet(_PWCCommon, nn.Module):
    """The origin PCWNet of KITTI12/models/pwcnet.py:310-507 (`gwcnet-g` / `gwcnet-gc` in the registry,
    models/__init__.py:5-9) -- the network whose output is the `used` disparity of KITTI12/test.py:86-92 -- on the
    same kernels as `PWCNet_ddim`: eval ``forward(left, right) -> ([disp_finetune], [pred3])`` (:483-507).  Same
    parameter names and shapes as the reference class (no time embedding, no schedule buffers)."""

    def __init__(self, maxdisp: int, use_concat_volume: bool = False):
        super().__init__()
        if maxdisp != 192:
            raise ValueError("PWCNet is defined for maxdisp == 192 here (the volume pyramid divides it by 4..32)")
        self.maxdisp, self.use_concat_volume, self.num_groups = maxdisp, use_concat_volume, 40
        self._init_backbone(use_concat_volume, time_embedding=False)

    def forward(self, left, right):
        if self.training:
            raise NotImplementedError("the MI355X DiffuVolume path is inference-only (model.eval())")
        with torch.no_grad():
            p = self.prepare(check_weights=True)
            fl = self.feature_extraction(left)
            fr = self.feature_extraction(right)
            combine = self.fused_volume(fl, fr)
            cost3 = p.classif3(p.dres4(p.dres3(p.dres2(combine))))            # pwcnet.py:421-424, :469
            pred3, _ = upsample_softmax_regress(cost3, want_uncertainty=False, align_corners=True)
            disp_finetune = self._refine(pred3, fl, fr)
        return [disp_finetune], [pred3]


def PWCNet_G(d):
    return PWCNet(d, use_concat_volume=False)


def PWCNet_GC(d):
    return PWCNet(d, use_concat_volume=True)


class PWCNet_ddim(train3d.TrainPrecision, _PWCCommon, nn.Module):
    def __init__(self, maxdisp: int, use_concat_volume: bool = True, sampling_timesteps: int = 3,
                 ensemble_cof: Optional[Sequence[float]] = None):
        super().__init__()
        if maxdisp != 192:
            raise ValueError("PWCNet_ddim is defined for maxdisp == 192 (hard-coded 48 / 192 in the reference)")
        self.maxdisp, self.use_concat_volume, self.num_groups = maxdisp, use_concat_volume, 40
        self.scale, self.num_timesteps, self.sampling_timesteps = 1.0, 1000, sampling_timesteps
        self.ddim_sampling_eta, self.renewal, self.use_ensemble = 1.0, True, True
        if ensemble_cof is None:
            if sampling_timesteps != 3:
                raise ValueError("give ensemble_cof (S+1 weights) when sampling_timesteps != 3")
            ensemble_cof = (0.9, 0.0, 0.0, 0.1)                       # pwcnet_ddim.py:599
        if len(ensemble_cof) != sampling_timesteps + 1:
            raise ValueError("ensemble_cof needs sampling_timesteps + 1 entries")
        self.ensemble_cof = tuple(float(c) for c in ensemble_cof)
        self.dif_threshold, self.unc_threshold = 1.0, 1.0            # :571-572 (the last step's <2 mask is unused)

        ddim.register_schedule(self, self.num_timesteps)
        self._init_backbone(use_concat_volume, time_embedding=True)

    # ---- pieces ---------------------------------------------------------------------------------------
    def _loop_plan(self):
        return ddim.loop_plan(self, self.prepare().ddim, self.dres0[0][0].weight.device)

    def _time_pairs(self):
        return ddim.time_pairs(self.num_timesteps, self.sampling_timesteps)

    def _filter(self, x_t, t, shift=None):
        return ddim.noise_prepare(self.time_embedding, x_t, t, shift)

    def _aggregate(self, volume, n01f):
        """pwcnet_ddim.py:472-477: (volume * filter) -> dres2 -> dres3 -> dres4 -> classif3."""
        p = self.prepare()
        return p.classif3(p.dres4(p.dres3(p.dres2(volume, in_scale=n01f))))

    def _uncertainty_about(self, cost, disp):
        """sum_k |disp - k| * softmax(upsampled cost)_k with ``disp`` = the refined disparity (:548-552)."""
        cost = cost[:, 0] if cost.dim() == 5 else cost
        b, d, h, w = cost.shape
        unc = torch.empty_like(disp)
        _lib.timed_launch("upsample_softmax_uncertainty", 0.0, 4.0 * (cost.numel() + 2 * disp.numel()),
                          "dv_upsample_softmax_uncertainty_f32", cost.device, cost.data_ptr(), disp.data_ptr(), unc.data_ptr(),
                          b, d, h, w, 1)
        return unc

    def _step_coef(self, time, time_next, cof):
        return ddim.step_coef(self.prepare().ddim, time, time_next, cof, eta=self.ddim_sampling_eta,
                              dif_thr=self.dif_threshold, unc_thr=self.unc_threshold,
                              clamp_max=float(self.maxdisp - 1), ens_dif_thr=0.0)

    def _predict(self, volume, img, t, features_left, features_right, shift=None, resized=None):
        n01, n01f = self._filter(img, t, shift)
        cost = self._aggregate(volume, n01f)
        pred3, _ = upsample_softmax_regress(cost, want_uncertainty=False, align_corners=True)
        disp = self._refine(pred3, features_left, features_right, resized).contiguous()
        unc = self._uncertainty_about(cost, disp)
        return n01, cost, disp, unc

    # ---- reference API ---------------------------------------------------------------------------------
    @torch.no_grad()
    def model_predictions(self, volume, noise, t, features_left, features_right):
        """pwcnet_ddim.py:466-528 -> (pred_noise fp64, x_start fp32, disp_finetune [B,H,W], ProbVolumeHandle)."""
        volume = _dev_f32(volume, "volume")
        b, _, d, h, w = volume.shape
        with torch.cuda.device(volume.device):
            n01, cost, disp, unc = self._predict(volume, noise, t, features_left, features_right)
            coef = self._step_coef(int(t.reshape(-1)[0]), -1, 0.0)
            mask = torch.zeros((b, h, w), dtype=torch.float32, device=volume.device)
            x_start, _, pred_noise = ddim.ddim_update(disp, disp, n01, None, None, mask, None, coef, unc=unc,
                                                      want_pred_noise=True)
        return pred_noise, x_start, disp, ProbVolumeHandle(cost, unc, self.maxdisp, align_corners=True)

    @torch.no_grad()
    def ddim_sample(self, volume, used, asd, features_left, features_right, noise: Optional[ddim.NoiseFn] = None,
                    generator: Optional[torch.Generator] = None, trace=None):
        """pwcnet_ddim.py:530-602.  Random draws in reference order: 'x_T' (torch.randn, :541), then per
        non-final step 'eps' (randn_like(img), :585) and 'q' (randn_like(asd) inside q_sample, :590)."""
        volume = _dev_f32(volume, "volume")
        used = ddim.check_loop_args(volume, _dev_f32(used, "used"), asd, self.maxdisp, what="fused volume")
        b, _, d, h, w = volume.shape
        dev = volume.device
        p = self.prepare(check_weights=True)
        draw = ddim.make_draw(noise, generator, dev)
        with torch.cuda.device(dev):
            img = draw("x_T", (b, 48, h, w), torch.float32)
            asd = asd.to(dev)
            final = [used]
            mask = torch.zeros((b, h, w), dtype=torch.float32, device=dev)
            ens = used * self.ensemble_cof[0]
            handle = None
            # step-invariant: the two refinement feature maps at full resolution (the reference resizes them inside
            # every model_predictions call, :487-492)
            resized = self.refine_features(features_left, features_right, (4 * h, 4 * w))
            for i, st in enumerate(self._loop_plan()):
                time, time_next = st.time, st.time_next
                eps = fill = None
                if time_next >= 0:
                    eps = draw("eps", tuple(img.shape), img.dtype)
                    # asd = q_sample(asd, t): float64 from the first step on (float64 schedule buffers)
                    asd = p.ddim.q_fill(time, asd, draw("q", tuple(asd.shape), asd.dtype))
                    fill = asd.contiguous()
                if trace is not None:
                    trace(i, {"when": "in", "img": img, "mask": mask.clone(), "eps": eps, "fill": fill})
                # (the last step's mask is never read again: the reference only builds the unused mask_final there)
                disp, unc, x_start, x_next, cost = self.ddim_step(i, volume, used, img, mask, ens, eps, fill,
                                                                  features_left, features_right, want_cost=True,
                                                                  resized=resized)
                if trace is not None:
                    trace(i, {"when": "out", "disp": disp, "unc": unc, "x_start": x_start, "x_next": x_next,
                              "mask": mask.clone()})
                handle = ProbVolumeHandle(cost, unc, self.maxdisp, align_corners=True)
                final.append(disp)
                img = x_start if time_next < 0 else x_next
        if getattr(p.dres0.b, "split", False):
            check_split_overflow(dev)
        if self.use_ensemble:
            return ens, handle
        return final[-1], handle

    @torch.no_grad()
    def ddim_step(self, i, volume, used, img, mask, ens=None, eps=None, fill=None, features_left=None,
                  features_right=None, want_cost=False, resized=None):
        """Iteration ``i`` of the loop of pwcnet_ddim.py:545-598 from explicit state (``img`` entering the step,
        ``mask`` updated in place, ``eps`` = randn_like(img), ``fill`` = the q_sample'd origin encoding).
        Returns (disp_finetune [B,4h,4w], uncertainty, x_start fp32, x_next fp64 | None[, cost])."""
        st = self._loop_plan()[i]
        n01, cost, disp, unc = self._predict(volume, img, None, features_left, features_right,
                                             shift=st.shift_rows(volume.shape[0]), resized=resized)
        x_start, x_next, _ = ddim.ddim_update(disp, used, n01, eps, fill, mask, ens, st.coef, unc=unc)
        return (disp, unc, x_start, x_next, cost) if want_cost else (disp, unc, x_start, x_next)

    @torch.no_grad()
    def encode_disparity(self, disp):
        return ddim.encode_two_hot(_dev_f32(disp, "disp"), 48)

    def train_forward(self, left, right, disp):
        """The reference's training branch (pwcnet_ddim.py:604-735) -> [pred0, combine, pred1, pred2, pred3,
        disp_finetune], each [B,H,W].  ``disp``: the quarter-resolution disparity [B,1,H/4,W/4] (KITTI12/main.py:148-150).
        Draws ``t = torch.randint(0, T, (1,))`` and then q_sample's ``torch.randn_like`` (in that order).
        Runs at ``self.train_precision`` ("f32", "f16" or "bf16"; ``set_train_precision``, which takes ``torch.bfloat16``
        for the last): every ``train3d`` call below sees it for the length of this call, on this thread only."""
        with self._train_scope():
            return self._train_forward(left, right, disp)

    def _train_forward(self, left, right, disp):
        if not left.is_cuda:
            raise NotImplementedError("training runs on the MI355X only (model.cuda()); no CPU path")
        hh, ww = left.shape[-2], left.shape[-1]
        if hh % 32 or ww % 32:
            raise _lib.DiffuVolumeError(f"PWCNet_ddim training needs H and W divisible by 32, got {hh}x{ww}: the stride-2 "
                                        "input gradient of the 3-D stack needs even dims at 1/4, 1/8 and 1/16")
        fl = self.feature_extraction(left)
        fr = self.feature_extraction(right)
        vols = self._volumes(fl, fr)
        cost0 = walk(self.dres0, vols[0])
        cost0 = walk(self.dres1, cost0) + cost0
        combine = self.combine1(cost0, vols[1], vols[2], vols[3])

        # two-hot disp_volume_final (:644-659), then t, then q_sample's noise
        x_start = self.encode_disparity(disp.detach().float())
        noisy = ddim.train_filter(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, self.time_embedding,
                                  self.scale, self.num_timesteps, x_start)

        out1 = self.dres2(combine * noisy)
        out2 = self.dres3(out1)
        out3 = self.dres4(out2)
        size = [self.maxdisp, hh, ww]

        # the fused tail with its HIP backward (train_tail.py; DV_TRAIN_TAIL)
        pred0 = regress_head(walk(self.classif0, cost0), size, align_corners=True)
        pred1 = regress_head(walk(self.classif1, out1), size, align_corners=True)
        pred2 = regress_head(walk(self.classif2, out2), size, align_corners=True)
        pred3 = regress_head(walk(self.classif3, out3), size, align_corners=True).unsqueeze(1)
        pred_combine = regress_head(walk(self.classif4, combine), size, align_corners=True)

        # refinement (:711-728)
        # (:487-492 on the route of train_net2d: DV_TRAIN_NET2D=hip resizes on the HIP kernel with the atomics-free backward)
        rl = train_net2d.resize_bilinear_train(fl["finetune_feature"], (hh, ww))
        rr = train_net2d.resize_bilinear_train(fr["finetune_feature"], (hh, ww))
        # left - warp(right, pred3) and their +-24 correlation with the HIP backward (train_refine.py; DV_TRAIN_REFINE)
        diff, corr = warp_corr_train(rl, rr, pred3, 24)
        refine_in = torch.cat((diff, rl, self._dispupsample_train(pred3), pred3, corr), dim=1)
        disp_finetune = self.refinenet3.train_forward(refine_in, pred3).squeeze(1)
        return [pred0, pred_combine, pred1, pred2, pred3.squeeze(1), disp_finetune]

    def _dispupsample_train(self, pred3):
        """`dispupsample` (1x1 conv 1 -> 32, BatchNorm2d, Mish; pwcnet_ddim.py:722) in training, evaluated in float64.

        With a single input channel the BatchNorm in train mode makes the output independent of the scale of each weight
        (BN(w * d) = BN(d) * sign(w) up to the eps term), so the weight's gradient -- sum over all pixels of the output
        gradient times d, behind the BatchNorm backward -- cancels to almost nothing: in float32 it is rounding noise of
        the size of the result (the reference's own float32 gradient is 2e-3 from float64, and PyTorch's float32
        reductions make it differ from run to run).  In float64 the cancellation leaves the true value; the layer has 32
        channels and costs little.  Output, gradients and BatchNorm statistics are stored back in float32."""
        conv, bn = self.dispupsample[0][0], self.dispupsample[0][1]
        # a 1x1 conv of one channel is a per-channel scale; BatchNorm2d in train mode as nn.BatchNorm2d computes it
        # (biased variance to normalise, unbiased into running_var), written out elementwise: no float64 conv / BN path
        x = pred3.double() * conv.weight.double().view(1, -1, 1, 1)
        mean = x.mean(dim=(0, 2, 3), keepdim=True)
        var = (x - mean).square().mean(dim=(0, 2, 3), keepdim=True)
        y = (x - mean) / torch.sqrt(var + bn.eps) * bn.weight.double().view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
        with torch.no_grad():                      # what nn.BatchNorm2d.forward does to its buffers in train mode
            bn.num_batches_tracked.add_(1)
            factor = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            n = x.numel() // x.shape[1]
            bn.running_mean.mul_(1 - factor).add_((factor * mean.reshape(-1)).float())
            bn.running_var.mul_(1 - factor).add_((factor * var.reshape(-1) * n / max(n - 1, 1)).float())
        return act_statement(y, "mish").float()

    def forward(self, left, right, used, disp, mask=None):
        if self.training:
            return self.train_forward(left, right, disp)
        with torch.no_grad():
            self.prepare(check_weights=True)
            fl = self.feature_extraction(left)
            fr = self.feature_extraction(right)
            combine = self.fused_volume(fl, fr)
            x_T = self.encode_disparity(disp)
            disp_finetune, handle = self.ddim_sample(combine, used, x_T, fl, fr)
        return [disp_finetune], [handle]
