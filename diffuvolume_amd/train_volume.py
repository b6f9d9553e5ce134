"""Differentiable cost-volume builders on the HIP kernels (the volumes ACVNet_DDIM and PWCNet_ddim train through; IGEV's
training front keeps the PyTorch statement, see igev_volume._cost_volume_train).

``build_gwc_volume_train`` and ``build_concat_volume_train`` are ``build_gwc_volume`` / ``build_concat_volume``
(submodule.py:209-238, :180-191; KITTI12 :86-97 with ``zero_left``) as ``torch.autograd.Function``s:
  * forward: the eval launch -- ``dv_gwc_volume_f32``; ``dv_concat_volume_f32``, or ``dv_concat_prob_volume_f32`` when a
    ``scale`` [B,D,H,W] multiplies the volume -- so a training forward has the bits of the eval forward;
  * backward: ``dv_gwc_volume_bwd_f32`` / ``dv_concat_volume_bwd_f32`` (csrc/volume_bwd.hip): only the feature maps and
    the scale are saved (the PyTorch statement keeps strided views of a padded copy, products and the ``cat``), the
    gradient of the volume is read once, and every element of a gradient is written once in a fixed order: no atomics,
    the same bits on every launch and for every batch split.
There is no double backward.  ``DV_TRAIN_VOLUME=torch`` routes both to the PyTorch statements of submodule.py instead
(A/B runs, tests).  CPU tensors raise, as everywhere on the hot path."""
from __future__ import annotations

import functools

import torch
from torch.autograd.function import once_differentiable

from . import _env, _lib

route = functools.partial(_env.route, "DV_TRAIN_VOLUME")


def _check_pair(ref, tgt):
    _lib.check_f32(ref, "refimg_fea")
    _lib.check_f32(tgt, "targetimg_fea")
    if ref.dim() != 4 or ref.shape != tgt.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(ref.shape)} vs {tuple(tgt.shape)}")


def gwc_volume_grad(ref, tgt, dvol, num_groups, want_ref=True, want_tgt=True):
    """(dref, dtgt) [B,C,H,W] from the features and the volume's gradient [B,G,D,H,W]; None for a side not wanted."""
    ref, tgt, dvol = ref.contiguous(), tgt.contiguous(), dvol.contiguous()
    b, c, h, w = ref.shape
    dref = torch.empty_like(ref) if want_ref else None
    dtgt = torch.empty_like(tgt) if want_tgt else None
    if dvol.numel() == 0:
        return (None if dref is None else dref.zero_()), (None if dtgt is None else dtgt.zero_())
    _lib.launch("dv_gwc_volume_bwd_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), dvol.data_ptr(), _lib.ptr(dref),
                _lib.ptr(dtgt), b, c, h, w, dvol.shape[2], num_groups)
    return dref, dtgt


def concat_volume_grad(ref, tgt, scale, dvol, zero_left=False, want_ref=True, want_tgt=True, want_scale=False):
    """(dref, dtgt, dscale) from the features, the scale [B,D,H,W] (or None) and the volume's gradient [B,2C,D,H,W]."""
    ref, tgt, dvol = ref.contiguous(), tgt.contiguous(), dvol.contiguous()
    scale = None if scale is None else scale.contiguous()
    b, c, h, w = ref.shape
    d = dvol.shape[2]
    dref = torch.empty_like(ref) if want_ref else None
    dtgt = torch.empty_like(tgt) if want_tgt else None
    ds = torch.empty_like(scale) if want_scale else None
    if dvol.numel() == 0:
        return tuple(None if t is None else t.zero_() for t in (dref, dtgt, ds))
    ws = _lib.workspace("dv_concat_volume_bwd_workspace_floats", ref.device, b, c, h, w, d) if want_scale else None
    _lib.launch("dv_concat_volume_bwd_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), _lib.ptr(scale), dvol.data_ptr(),
                _lib.ptr(dref), _lib.ptr(dtgt), _lib.ptr(ds), _lib.ptr(ws), b, c, h, w, d, int(bool(zero_left)))
    return dref, dtgt, ds


class GwcVolumeFn(torch.autograd.Function):
    """ref, tgt [B,C,H,W] -> [B,G,D,H,W]; saves ref and tgt."""

    @staticmethod
    def forward(ctx, ref, tgt, maxdisp, num_groups):
        ref, tgt = ref.contiguous(), tgt.contiguous()
        b, c, h, w = ref.shape
        out = torch.empty((b, num_groups, maxdisp, h, w), dtype=torch.float32, device=ref.device)
        if out.numel():
            _lib.launch("dv_gwc_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), out.data_ptr(), b, c, h, w, maxdisp,
                        num_groups)
        ctx.save_for_backward(ref, tgt)
        ctx.num_groups = num_groups
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ref, tgt = ctx.saved_tensors
        want_ref, want_tgt = ctx.needs_input_grad[:2]
        if not (want_ref or want_tgt):
            return None, None, None, None
        _lib.check_f32(g, "grad_volume")
        dref, dtgt = gwc_volume_grad(ref, tgt, g, ctx.num_groups, want_ref, want_tgt)
        return dref, dtgt, None, None


class ConcatVolumeFn(torch.autograd.Function):
    """ref, tgt [B,C,H,W] (, scale [B,D,H,W]) -> [B,2C,D,H,W]; saves ref, tgt and the scale."""

    @staticmethod
    def forward(ctx, ref, tgt, scale, maxdisp, zero_left):
        ref, tgt = ref.contiguous(), tgt.contiguous()
        scale = None if scale is None else scale.contiguous()
        b, c, h, w = ref.shape
        out = torch.empty((b, 2 * c, maxdisp, h, w), dtype=torch.float32, device=ref.device)
        if out.numel() and scale is None:
            _lib.launch("dv_concat_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), out.data_ptr(), b, c, h, w,
                        maxdisp, int(zero_left))
        elif out.numel():
            _lib.launch("dv_concat_prob_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), scale.data_ptr(),
                        out.data_ptr(), b, c, h, w, maxdisp)
        if scale is None:
            ctx.save_for_backward(ref, tgt)
        else:
            ctx.save_for_backward(ref, tgt, scale)
        ctx.zero_left = zero_left
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ref, tgt, *rest = ctx.saved_tensors
        scale = rest[0] if rest else None
        want_ref, want_tgt, want_scale = ctx.needs_input_grad[:3]
        want_scale = want_scale and scale is not None
        if not (want_ref or want_tgt or want_scale):
            return None, None, None, None, None
        _lib.check_f32(g, "grad_volume")
        dref, dtgt, ds = concat_volume_grad(ref, tgt, scale, g, ctx.zero_left, want_ref, want_tgt, want_scale)
        return dref, dtgt, ds, None, None


def build_gwc_volume_train(ref: torch.Tensor, tgt: torch.Tensor, maxdisp: int, num_groups: int) -> torch.Tensor:
    """[B,C,H,W] x2 -> [B,num_groups,maxdisp,H,W], differentiable with respect to both feature maps."""
    r = route()
    _check_pair(ref, tgt)
    assert ref.shape[1] % num_groups == 0          # submodule.py:211
    if r == "torch":
        from .submodule import _gwc_volume_autograd
        return _gwc_volume_autograd(ref, tgt, maxdisp, num_groups)
    return GwcVolumeFn.apply(ref, tgt, int(maxdisp), int(num_groups))


def build_concat_volume_train(ref: torch.Tensor, tgt: torch.Tensor, maxdisp: int, zero_left: bool = False,
                              scale: torch.Tensor = None) -> torch.Tensor:
    """[B,C,H,W] x2 -> [B,2C,maxdisp,H,W], times ``scale`` [B,maxdisp,H,W] over the channels if given; differentiable
    with respect to the feature maps and the scale.  ``scale`` and ``zero_left`` do not go together."""
    r = route()
    _check_pair(ref, tgt)
    zero_left = bool(zero_left)
    if scale is not None:
        _lib.check_f32(scale, "scale")
        b, _, h, w = ref.shape
        if tuple(scale.shape) != (b, maxdisp, h, w):
            raise RuntimeError(f"scale must be {(b, maxdisp, h, w)}, got {tuple(scale.shape)}")
        if zero_left:
            raise RuntimeError("scale and zero_left do not go together (no model builds that volume)")
    if r == "torch":
        from .submodule import _concat_volume_autograd
        vol = _concat_volume_autograd(ref, tgt, maxdisp, zero_left)
        return vol if scale is None else scale.unsqueeze(1) * vol
    return ConcatVolumeFn.apply(ref, tgt, scale, int(maxdisp), zero_left)
