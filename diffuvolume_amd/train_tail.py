"""Differentiable regression tail on the HIP kernels (the heads of ACVNet_DDIM and PWCNet_ddim in training).

``upsample_softmax_regress_train(cost, align_corners=False)`` is ``F.interpolate(cost, [4D,4h,4w], mode="trilinear")`` +
``F.softmax(dim=1)`` + ``disparity_regression`` (acv_ddim.py:457-480, pwcnet_ddim.py:682-710) as one
``torch.autograd.Function``:
  * forward: ``dv_upsample_softmax_regress_f32`` without the uncertainty output -- the bits of the eval path;
  * backward: ``dv_upsample_softmax_regress_bwd_f32`` (csrc/regress_bwd.hip): the softmax is recomputed from the cost, so
    only ``cost`` [B,D,h,w] and ``disp`` [B,4h,4w] are saved -- the torch expression keeps a [B,4D,4h,4w] softmax per head
    until backward -- and every element of the gradient is written once in a fixed order: no atomics, the same bits on
    every launch and for every batch split (PyTorch's trilinear backward adds with atomics).
There is no double backward.  ``DV_TRAIN_TAIL=torch`` routes the function to the torch expression instead (A/B runs,
tests).  CPU tensors raise, as everywhere on the hot path."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _env, _lib

route = functools.partial(_env.route, "DV_TRAIN_TAIL")


def torch_tail(cost: torch.Tensor, size, align_corners: bool = False) -> torch.Tensor:
    """The reference's expression: cost [B,1,D,h,w] -> disp [B,size[1],size[2]] over size[0] bins."""
    kw = {"align_corners": True} if align_corners else {}
    up = torch.squeeze(F.interpolate(cost, list(size), mode="trilinear", **kw), 1)
    k = torch.arange(0, size[0], dtype=up.dtype, device=up.device).view(1, size[0], 1, 1)
    return torch.sum(F.softmax(up, dim=1) * k, 1, keepdim=False)


def regress_tail_grad(cost: torch.Tensor, disp: torch.Tensor, grad_disp: torch.Tensor,
                      align_corners: bool = False) -> torch.Tensor:
    """dcost [B,D,h,w] from cost [B,D,h,w], the forward's disp [B,4h,4w] and its gradient."""
    cost, disp, grad_disp = cost.contiguous(), disp.contiguous(), grad_disp.contiguous()
    b, d, h, w = cost.shape
    dcost = torch.empty_like(cost)
    ws = _lib.workspace("dv_upsample_softmax_regress_bwd_workspace_floats", cost.device, b, d, h, w)
    _lib.launch("dv_upsample_softmax_regress_bwd_f32", cost.device, cost.data_ptr(), disp.data_ptr(), grad_disp.data_ptr(),
                dcost.data_ptr(), _lib.ptr(ws), b, d, h, w, int(bool(align_corners)))
    return dcost


class UpsampleSoftmaxRegressFn(torch.autograd.Function):
    """cost [B,D,h,w] -> disp [B,4h,4w]; saves cost and disp."""

    @staticmethod
    def forward(ctx, cost, align_corners):
        _lib.check_f32(cost, "cost")
        cost = cost.contiguous()
        b, d, h, w = cost.shape
        disp = torch.empty((b, 4 * h, 4 * w), dtype=torch.float32, device=cost.device)
        if disp.numel():
            _lib.launch("dv_upsample_softmax_regress_f32", cost.device, cost.data_ptr(), disp.data_ptr(), None, b, d, h, w,
                        int(align_corners))
        ctx.save_for_backward(cost, disp)
        ctx.align_corners = align_corners
        return disp

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cost, disp = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        _lib.check_f32(g, "grad_disp")
        if not cost.numel():
            return torch.zeros_like(cost), None
        return regress_tail_grad(cost, disp, g, ctx.align_corners), None


def upsample_softmax_regress_train(cost: torch.Tensor, align_corners: bool = False) -> torch.Tensor:
    """cost [B,1,D,h,w] (or [B,D,h,w]) -> disp [B,4h,4w], differentiable with respect to cost."""
    r = route()
    _lib.check_f32(cost, "cost")
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise RuntimeError("cost must have one channel")
        cost = cost[:, 0]
    if cost.dim() != 4:
        raise RuntimeError(f"cost must be [B,1,D,h,w] or [B,D,h,w], got {tuple(cost.shape)}")
    align_corners = bool(align_corners)
    if r == "torch":
        d, h, w = cost.shape[1:]
        return torch_tail(cost.unsqueeze(1), (4 * d, 4 * h, 4 * w), align_corners)
    return UpsampleSoftmaxRegressFn.apply(cost, align_corners)


def regress_head(cost: torch.Tensor, size, align_corners: bool = False) -> torch.Tensor:
    """A training head of the two models: ``size`` = [maxdisp, H, W] is four times the cost's [D, h, w] there, which is what
    the fused kernels compute; any other target size is the reference's torch expression."""
    if tuple(size) == tuple(4 * n for n in cost.shape[-3:]):
        return upsample_softmax_regress_train(cost, align_corners)
    return torch_tail(cost, size, align_corners)
