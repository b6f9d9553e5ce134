"""The differentiable part of PWCNet_ddim's refinement input on HIP kernels (csrc/warp_corr.hip).

``warp_corr_train(left, right, disp)`` is the pair of statements of the reference's training branch
(KITTI12/models/pwcnet_ddim.py:719-725)

    rr_warp = warp(right, disp);  diff = left - rr_warp;  corr = build_corrleation_volume(left, rr_warp, 24, 1)

as one ``torch.autograd.Function``:
  * forward: ``dv_warp_corr_f32`` -- the eval kernel of csrc/refine_inputs.hip without the channels that need no gradient
    path of their own, so ``diff`` and ``corr`` have the bits of ``submodule.refine_inputs``;
  * backward: ``dv_warp_corr_bwd_f32`` -- only ``left``, ``right`` and ``disp`` are saved (the warped map is recomputed),
    and every element of every gradient is written once in a fixed order: no atomics (grid_sample's backward scatters with
    them), the same bits on every launch and for every batch split.
There is no double backward.  ``DV_TRAIN_REFINE=torch`` routes the function to the PyTorch statements (``warp`` +
``groupwise_corr_pm`` of pwcnet_ddim.py) instead (A/B runs, tests).  CPU tensors raise, as everywhere on the hot path."""
from __future__ import annotations

import functools

import torch
from torch.autograd.function import once_differentiable

from . import _env, _lib

MAXSHIFT, CMAX = 24, 32               # what csrc/warp_corr.hip implements (as csrc/refine_inputs.hip)

route = functools.partial(_env.route, "DV_TRAIN_REFINE")


def warp_corr_grad(left, right, disp, g_diff, g_corr, maxshift=MAXSHIFT, want_left=True, want_right=True, want_disp=True):
    """(dleft, dright [B,C,H,W], ddisp [B,1,H,W]) from the inputs and the gradients of diff / corr; None where not wanted."""
    left, right, disp = left.contiguous(), right.contiguous(), disp.contiguous()
    g_diff, g_corr = g_diff.contiguous(), g_corr.contiguous()
    b, c, h, w = left.shape
    dleft = torch.empty_like(left) if want_left else None
    dright = torch.empty_like(right) if want_right else None
    ddisp = torch.empty_like(disp) if want_disp else None
    if left.numel() == 0:
        return tuple(None if t is None else t.zero_() for t in (dleft, dright, ddisp))
    ws = _lib.workspace("dv_warp_corr_bwd_workspace_floats", left.device, b, c, h, w) if want_right else None
    _lib.launch("dv_warp_corr_bwd_f32", left.device, left.data_ptr(), right.data_ptr(), disp.data_ptr(), g_diff.data_ptr(),
                g_corr.data_ptr(), _lib.ptr(dleft), _lib.ptr(dright), _lib.ptr(ddisp), _lib.ptr(ws), b, c, h, w,
                int(maxshift))
    return dleft, dright, ddisp


class WarpCorrFn(torch.autograd.Function):
    """left, right [B,C,H,W], disp [B,1,H,W] -> (diff [B,C,H,W], corr [B,2*maxshift+1,H,W]); saves the three inputs."""

    @staticmethod
    def forward(ctx, left, right, disp, maxshift):
        left, right, disp = left.contiguous(), right.contiguous(), disp.contiguous()
        b, c, h, w = left.shape
        diff = torch.empty_like(left)
        corr = torch.empty((b, 2 * maxshift + 1, h, w), dtype=torch.float32, device=left.device)
        if left.numel():
            _lib.launch("dv_warp_corr_f32", left.device, left.data_ptr(), right.data_ptr(), disp.data_ptr(), diff.data_ptr(),
                        corr.data_ptr(), b, c, h, w, maxshift)
        else:
            corr.zero_()
        ctx.save_for_backward(left, right, disp)
        ctx.maxshift = maxshift
        return diff, corr

    @staticmethod
    @once_differentiable
    def backward(ctx, g_diff, g_corr):
        left, right, disp = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if not any(want):
            return None, None, None, None
        _lib.check_f32(g_diff, "grad_diff")
        _lib.check_f32(g_corr, "grad_corr")
        dleft, dright, ddisp = warp_corr_grad(left, right, disp, g_diff, g_corr, ctx.maxshift, *want)
        return dleft, dright, ddisp, None


def warp_corr_train(left: torch.Tensor, right: torch.Tensor, disp: torch.Tensor, maxshift: int = MAXSHIFT):
    """left, right [B,C,H,W], disp [B,1,H,W] -> (left - warp(right, disp) [B,C,H,W], their +-maxshift correlation
    [B,2*maxshift+1,H,W]), differentiable with respect to all three inputs."""
    r = route()
    _lib.check_f32(left, "left")
    _lib.check_f32(right, "right")
    _lib.check_f32(disp, "disp")
    if left.dim() != 4 or left.shape != right.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(left.shape)} vs {tuple(right.shape)}")
    b, c, h, w = left.shape
    if tuple(disp.shape) != (b, 1, h, w):
        raise RuntimeError(f"disp must be {(b, 1, h, w)}, got {tuple(disp.shape)}")
    if r == "torch":
        from .pwcnet_ddim import groupwise_corr_pm, warp
        warped = warp(right, disp)
        return left - warped, groupwise_corr_pm(left, warped, maxshift)
    if left.numel() and (c > CMAX or maxshift != MAXSHIFT or w < MAXSHIFT):
        raise _lib.DiffuVolumeError(f"warp_corr_train on HIP takes C <= {CMAX}, maxshift == {MAXSHIFT} and W >= {MAXSHIFT}; "
                                    f"got C = {c}, maxshift = {maxshift}, W = {w} (DV_TRAIN_REFINE=torch runs the "
                                    "PyTorch statements)")
    return WarpCorrFn.apply(left, right, disp, int(maxshift))
