"""IGEV's convex-upsampling head (KITTI15/core/igev_stereo_ddim.py:203-211 `upsample_disp`, once per GRU iteration in
the train loop :441-457; :390-393 + :462 for `init_disp`; `context_upsample` core/submodule.py:241-253), shared by
IGEVStereo_ddim and IGEVUpsampler."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, train2d
from .igev_layers import (TRAIN, BasicConv_IN, Conv2x, Conv2x_IN, _bn_tuple, _refuse_autocast, _require_cuda, _train_mode,
                          basic_conv_in, conv2x)
from .submodule import ACT_LEAKY, ACT_NONE, Conv2dPlan, Deconv2dK4S2Plan, PlanCache, _dev_f32, weight_key


def _context_upsample_shapes(disp_low, up_weights):
    b, c, h, w = disp_low.shape
    if c != 1 or tuple(up_weights.shape) != (b, 9, 4 * h, 4 * w):
        raise RuntimeError(f"context_upsample: disp_low [B,1,h,w] and up_weights [B,9,4h,4w], got "
                           f"{tuple(disp_low.shape)} and {tuple(up_weights.shape)}")
    return b, h, w


def _context_upsample_launch(disp_low, up_weights, scale, apply_softmax):
    b, h, w = _context_upsample_shapes(disp_low, up_weights)
    out = torch.empty((b, 4 * h, 4 * w), dtype=torch.float32, device=disp_low.device)
    _lib.launch("dv_context_upsample_f32", disp_low.device, disp_low.data_ptr(), up_weights.data_ptr(), out.data_ptr(), b, h, w,
                float(scale), int(bool(apply_softmax)))
    return out


class ContextUpsampleFn(torch.autograd.Function):
    """context_upsample with both gradients on ``dv_context_upsample_bwd_f32``: the forward is the inference launch (its
    bits); the backward recomputes the softmax from the saved logits -- no probabilities, no unfolded or x4-repeated
    disparity are kept -- and gathers, so two runs give the same bits."""

    @staticmethod
    def forward(ctx, disp_low, up_weights, scale, apply_softmax):
        disp_low, up_weights = disp_low.contiguous(), up_weights.contiguous()
        ctx.save_for_backward(disp_low, up_weights)
        ctx.scale, ctx.apply_softmax = scale, apply_softmax
        return _context_upsample_launch(disp_low, up_weights, scale, apply_softmax)

    @staticmethod
    def backward(ctx, g):
        disp_low, up_weights = ctx.saved_tensors
        b, _, h, w = disp_low.shape
        g = g.contiguous()
        need_d, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_d or need_w):
            return None, None, None, None
        d_w = torch.empty_like(up_weights) if need_w else None
        d_d = torch.empty_like(disp_low) if need_d else None
        sums = torch.empty((b, 9, h, w), dtype=torch.float32, device=g.device) if need_d else None
        _lib.launch("dv_context_upsample_bwd_f32", g.device, disp_low.data_ptr(), up_weights.data_ptr(), g.data_ptr(),
                    _lib.ptr(d_w), _lib.ptr(d_d), _lib.ptr(sums), b, h, w, float(ctx.scale), int(ctx.apply_softmax))
        return d_d, d_w, None, None


def context_upsample(disp_low: torch.Tensor, up_weights: torch.Tensor, scale: float = 1.0,
                     apply_softmax: bool = False) -> torch.Tensor:
    """core/submodule.py:241-253: disp_low [B,1,h,w], up_weights [B,9,4h,4w] -> [B,4h,4w].  ``apply_softmax`` /
    ``scale`` fold the ``F.softmax(spx_pred, 1)`` and ``disp*4.`` of the call site into the same pass.  Differentiable
    when autograd records and an input asks for gradients (``ContextUpsampleFn``; the reference's torch expression under
    DV_TRAIN_CONV2D=torch); otherwise the inference launch."""
    if torch.is_grad_enabled() and (disp_low.requires_grad or up_weights.requires_grad):
        _lib.check_f32(disp_low, "disp_low")
        _lib.check_f32(up_weights, "up_weights")
        b, h, w = _context_upsample_shapes(disp_low, up_weights)
        if train2d.route() == "torch":
            weights = F.softmax(up_weights, 1) if apply_softmax else up_weights
            unfold = F.unfold(disp_low * scale, 3, 1, 1).reshape(b, -1, h, w)
            unfold = F.interpolate(unfold, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
            return (unfold * weights).sum(1)
        return ContextUpsampleFn.apply(disp_low, up_weights, float(scale), bool(apply_softmax))
    disp_low, up_weights = _dev_f32(disp_low, "disp_low"), _dev_f32(up_weights, "up_weights")
    return _context_upsample_launch(disp_low, up_weights, scale, apply_softmax)


def _spx_plans(m):
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    bn = lambda c: _bn_tuple(c.bn if c.use_bn else None)
    act = lambda c: ACT_LEAKY if c.relu else ACT_NONE
    return (Deconv2dK4S2Plan(c1.conv.weight, bn(c1), act=act(c1), eps=c1.bn.eps),
            Conv2dPlan(c2.conv.weight, bn(c2), act=act(c2), eps=c2.bn.eps),
            Deconv2dK4S2Plan(head.weight, None, bias=head.bias))


def _spx_train_key(m):
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    return weight_key((c1.conv.weight, c2.conv.weight, head.weight, head.bias))


def _spx_train_plans(m):
    """(key, plans) of the three layers for the training route: forward plans without BatchNorm / activation and the
    packed weights of the input gradients.  The key covers the three layers' weights only: in train mode BatchNorm
    rewrites its running statistics on every call, which the module-wide key of ``refresh_plans`` would take for a change."""
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    return _spx_train_key(m), (train2d.TrainDeconvPlan(c1.conv.weight), train2d.TrainConvPlan(c2.conv, ACT_NONE),
                               train2d.TrainDeconvPlan(head.weight, head.bias))


def _upsample_disp(m, disp, mask_feat_4, stem_2x, slot, train_slot):
    if _train_mode(m):
        return _upsample_disp_train(m, disp, mask_feat_4, stem_2x, train_slot)
    if mask_feat_4.is_cuda and m.spx_2_gru.concat:
        up, mix, head = m.plans(slot)
        x = up(mask_feat_4)
        if x.shape != stem_2x.shape:
            x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
        spx_pred = head(mix([x, stem_2x]))              # torch.cat((x, rem), 1) is never materialised
    else:
        spx_pred = m.spx_gru(m.spx_2_gru(mask_feat_4, stem_2x))
    return context_upsample(disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


def _upsample_disp_train(m, disp, mask_feat_4, stem_2x, train_slot):
    """`upsample_disp` for training (train mode with autograd recording): both transposed convolutions and the 3x3 over
    the un-materialised [x | stem_2x] concatenation autograd functions on the HIP kernels (train2d), BatchNorm on batch
    statistics and LeakyReLU in PyTorch, softmax + convex upsampling one differentiable HIP pass."""
    _require_cuda(("disp", disp), ("mask_feat_4", mask_feat_4), ("stem_2x", stem_2x))
    _refuse_autocast("the convex-upsampling head")
    c = m.spx_2_gru
    if not c.concat:
        raise _lib.DiffuVolumeError("the training route of upsample_disp needs spx_2_gru built with concat=True")

    def plan(i):
        def get():                                   # only called on the HIP route; rebuilt when a weight was written
            if m.plans(train_slot)[0] != _spx_train_key(m):
                m.drop_slot(train_slot)
            return m.plans(train_slot)[1][i]
        return get
    x = c.conv1.train_forward(mask_feat_4, plan(0))
    if x.shape != stem_2x.shape:
        x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
    x = train2d.conv_cat(plan(1), c.conv2.conv, ACT_NONE, [x, stem_2x])
    if c.conv2.use_bn:
        x = c.conv2.bn(x)
    if c.conv2.relu:
        x = F.leaky_relu(x, 0.01)
    spx_pred = train2d.conv_transpose2d_module(m.spx_gru[0], x, plan(2))
    return context_upsample(disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


def _spx_init_train(m, features_left0, stem_2x):
    """The spx_4 / spx_2 / spx logits (:390-392) on the training route, on the modules of ``m`` (an IGEVUpsampler or the
    IGEVStereo_ddim itself).  These heads train on PyTorch's InstanceNorm (``torch_norm``), not on the front's HIP pass."""
    s4 = m.spx_4
    x = s4[3](s4[2](train2d.conv2d_module(s4[1], basic_conv_in(TRAIN, s4[0], features_left0, torch_norm=True))))
    return train2d.conv_transpose2d_module(m.spx[0], conv2x(TRAIN, m.spx_2, x, stem_2x, torch_norm=True))


class IGEVUpsampler(PlanCache, nn.Module):
    """The upsampling-side modules of IGEVStereo_ddim (:110-112 `spx_2_gru` / `spx_gru`, :104-108 `spx_4` / `spx_2` /
    `spx`) under the reference's attribute names, and the parts of its forward that use them.
    ``forward(disp, mask_feat_4, stem_2x)`` is `upsample_disp` (:203-211) -> [B,1,4h,4w]; ``init_forward(features_left0,
    stem_2x, init_disp)`` is :390-393 + :462 -> [B,1,4h,4w].  In eval mode (or under no_grad) ``forward`` runs the fused
    inference plans; in train mode with autograd recording it is differentiable on the HIP kernels (see
    ``_upsample_disp_train``).  `spx_4` / `spx_2` / `spx` run once per pair: the modules' own forwards in eval mode, in train
    mode their convolutions as the same autograd functions (plans built per call, InstanceNorm / activations PyTorch)
    and their softmax + convex upsampling of `init_disp` the same differentiable HIP pass."""

    def __init__(self):
        super().__init__()
        self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.spx_2 = Conv2x_IN(24, 32, True)
        self.spx_4 = nn.Sequential(BasicConv_IN(96, 24, kernel_size=3, stride=1, padding=1),
                                   nn.Conv2d(24, 24, 3, 1, 1, bias=False), nn.InstanceNorm2d(24), nn.ReLU())
        self.spx_2_gru = Conv2x(32, 32, True)
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))

    def _build_plans(self, slot):
        return _spx_train_plans(self) if slot == "train" else _spx_plans(self)

    def forward(self, disp, mask_feat_4, stem_2x):
        if not _train_mode(self):
            for c in (self.spx_2_gru.conv1, self.spx_2_gru.conv2):
                if c.use_bn and c.bn.training:
                    raise _lib.DiffuVolumeError("BatchNorm2d in training mode under no_grad: the inference plans fold "
                                                "running statistics (model.eval())")
            _dev_f32(mask_feat_4, "mask_feat_4")
            self.refresh_plans()
        return _upsample_disp(self, disp, mask_feat_4, stem_2x, None, "train")

    def init_forward(self, features_left0, stem_2x, init_disp):
        if _train_mode(self):
            _require_cuda(("features_left[0]", features_left0), ("stem_2x", stem_2x), ("init_disp", init_disp))
            _refuse_autocast("the convex-upsampling head")
            # (the modules' own forwards take the inference kernels for inputs that ask for no gradient, which would leave
            # these weights without one under a frozen backbone; and MIOpen's backward-weights of these layers does not
            # return the same bits twice, so the convolutions go through train2d like the per-iteration ones)
            spx_pred = _spx_init_train(self, features_left0, stem_2x)
        else:
            spx_pred = self.spx(self.spx_2(self.spx_4(features_left0), stem_2x))
        return context_upsample(init_disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)
