"""BatchNorm3d (batch statistics) + skip + activation of the ACV and PCW 3-D stacks in training on HIP kernels
(csrc/bn3d_act.hip).

``batch_norm_act_train(x, weight, bias, running_mean, running_var, momentum=, eps=, act=, skip=)`` is the statement the
aggregation stacks apply to every convolution output in training,

    y = act(F.batch_norm(x, running_mean, running_var, weight, bias, training=True, momentum, eps) + skip)

with ``act`` ``"none"``, ``"relu"`` or ``"mish"`` (``x * tanh(softplus(x))``), as one ``torch.autograd.Function``:
  * forward: ``dv_bn3d_stats_f32`` (per-block shifted partials, merged per channel in a fixed order in double; updates the
    running buffers in place) and ``dv_bn3d_apply_act_f32`` (the Mish of the eval epilogues, ``dv_act``);
  * backward: ``dv_bn3d_act_bwd_f32`` -- ``z`` is recomputed from ``x``, ``skip`` and the statistics, so only ``x``,
    ``skip``, ``mean``, ``invstd`` and the parameters are saved: not the normalised tensor, ``softplus``, ``tanh`` or the
    sum.  Every reduction is partials + a fixed-order combine, without atomics: the same bits on every launch.
There is no double backward.  ``DV_TRAIN_NORM=torch`` routes the function to the PyTorch statement (A/B runs, tests).
CPU tensors raise, as everywhere on the hot path.

``bn_act(bn, x, act, skip=None)`` is the call site's form: it takes the ``nn.BatchNorm3d`` module, bumps
``num_batches_tracked`` and keeps the PyTorch statement for whatever lies outside the kernel's case.  Its body,
``bn_act_rank``, also serves ``train_net2d.bn_act2d`` (rank 4), and ``act_statement(y, act, skip=None)`` is the one PyTorch
spelling of ``act(y + skip)`` for the whole package (``net_blocks.walk`` ends every Sequential with it)."""
from __future__ import annotations

import functools
from typing import Optional

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _env, _lib

ACTS = {"none": 0, "relu": 1, "mish": 2}            # DV_ACT_NONE / DV_ACT_RELU / DV_ACT_MISH


route = functools.partial(_env.route, "DV_TRAIN_NORM")


def act_statement(y: torch.Tensor, act: str, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(y + skip) in PyTorch: ``"relu"``, ``"mish"`` (x * tanh(softplus(x)), KITTI12/models/submodule.py:11-18) or
    ``"none"``."""
    if skip is not None:
        y = y + skip
    if act == "relu":
        return F.relu(y)
    if act == "mish":
        return y * torch.tanh(F.softplus(y))
    if act != "none":
        raise ValueError(f"act must be one of {sorted(ACTS)}, got {act!r}")
    return y


def _bcs(x: torch.Tensor):
    b, c = x.shape[:2]
    return b, c, x.numel() // (b * c)


class BatchNormActFn(torch.autograd.Function):
    """x [B,C,...], weight, bias [C] (+ running buffers, skip) -> act(bn(x) + skip); saves x, skip, mean, invstd and the
    parameters."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, skip, momentum, eps, act):
        x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
        skip = None if skip is None else skip.contiguous()
        b, c, s = _bcs(x)
        mean = torch.empty(c, dtype=torch.float32, device=x.device)
        invstd = torch.empty_like(mean)
        y = torch.empty_like(x)
        ws = _lib.workspace("dv_bn3d_train_workspace_floats", x.device, b, c, s)
        _lib.launch("dv_bn3d_stats_f32", x.device, x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _lib.ptr(running_mean),
                    _lib.ptr(running_var), _lib.ptr(ws), b, c, s, float(momentum), float(eps))
        _lib.launch("dv_bn3d_apply_act_f32", x.device, x.data_ptr(), _lib.ptr(skip), mean.data_ptr(), invstd.data_ptr(),
                    weight.data_ptr(), bias.data_ptr(), y.data_ptr(), b, c, s, act)
        ctx.save_for_backward(x, skip, mean, invstd, weight, bias)
        ctx.act = act
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, skip, mean, invstd, weight, bias = ctx.saved_tensors
        want_x, want_w, want_b, _, _, want_s = ctx.needs_input_grad[:6]
        want_s = want_s and skip is not None
        none = (None,) * 9
        if not (want_x or want_w or want_b or want_s):
            return none
        _lib.check_f32(dy, "grad_output")
        dy = dy.contiguous()
        b, c, s = _bcs(x)
        dx = torch.empty_like(x) if want_x else None
        dskip = torch.empty_like(x) if want_s else None
        dgamma = torch.empty_like(mean) if want_w else None
        dbeta = torch.empty_like(mean) if want_b else None
        ws = _lib.workspace("dv_bn3d_train_workspace_floats", x.device, b, c, s)
        _lib.launch("dv_bn3d_act_bwd_f32", x.device, dy.data_ptr(), x.data_ptr(), _lib.ptr(skip), mean.data_ptr(),
                    invstd.data_ptr(), weight.data_ptr(), bias.data_ptr(), _lib.ptr(dx), _lib.ptr(dskip), _lib.ptr(dgamma),
                    _lib.ptr(dbeta), _lib.ptr(ws), b, c, s, ctx.act)
        return dx, dgamma, dbeta, None, None, dskip, None, None, None


def batch_norm_act_train(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                         running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor], *,
                         momentum: float = 0.1, eps: float = 1e-5, act: str = "none",
                         skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(batch_norm(x) + skip) with batch statistics for x [B,C,...], differentiable in x, skip, weight and bias; the
    running buffers (both or neither) are updated in place, also under ``torch.no_grad()``.  Returns a fresh tensor."""
    r = route()
    if act not in ACTS:
        raise ValueError(f"act must be one of {sorted(ACTS)}, got {act!r}")
    named = dict(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var, skip=skip)
    if (running_mean is None) != (running_var is None):
        raise RuntimeError("running_mean and running_var go together")
    for name, t in named.items():
        if t is not None or name in ("x", "weight", "bias"):
            _lib.check_f32(t, name)
    if x.dim() < 2:
        raise RuntimeError(f"x must be [B,C,...], got {tuple(x.shape)}")
    c = x.shape[1]
    for name in ("weight", "bias", "running_mean", "running_var"):
        if named[name] is not None and tuple(named[name].shape) != (c,):
            raise RuntimeError(f"{name} must be {(c,)}, got {tuple(named[name].shape)}")
    if skip is not None and skip.shape != x.shape:
        raise RuntimeError(f"skip must be {tuple(x.shape)}, got {tuple(skip.shape)}")
    if x.numel() <= c:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if r == "torch":
        # the PyTorch statement as the call sites ran it before the kernels
        return act_statement(F.batch_norm(x, running_mean, running_var, weight, bias, True, momentum, eps), act, skip)
    for name in ("running_mean", "running_var"):
        if named[name] is not None and not named[name].is_contiguous():
            raise RuntimeError(f"{name} must be contiguous (it is updated in place)")
    return BatchNormActFn.apply(x, weight, bias, running_mean, running_var, skip, float(momentum), float(eps), ACTS[act])


def bn_act_rank(rank: int, bn: torch.nn.Module, x: torch.Tensor, act: str, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(bn(x) + skip) for a BatchNorm module of a training graph.  Inside the kernel's case -- module in training mode
    with running statistics, a momentum and affine parameters, x a contiguous float32 tensor of ``rank`` dimensions -- this
    is ``batch_norm_act_train`` (on the route of DV_TRAIN_NORM) after the module's own ``num_batches_tracked`` bump;
    outside it, the module's forward and the PyTorch statement on either route."""
    inside = (bn.training and bn.track_running_stats and bn.momentum is not None and bn.weight is not None
              and bn.bias is not None and bn.running_mean is not None and x.dim() == rank and x.dtype == torch.float32
              and x.is_contiguous() and (skip is None or (skip.dtype == torch.float32 and skip.is_contiguous())))
    if not inside:
        return act_statement(bn(x), act, skip)
    y = batch_norm_act_train(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, momentum=bn.momentum, eps=bn.eps,
                             act=act, skip=skip)
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return y


def bn_act(bn: torch.nn.Module, x: torch.Tensor, act: str, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 3-D stacks' call site: an nn.BatchNorm3d on [B,C,D,H,W] (a 4-D tensor goes to the module's forward)."""
    return bn_act_rank(5, bn, x, act, skip)
