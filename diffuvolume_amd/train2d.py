"""Differentiable 2-D convolutions on the HIP kernels (training of PWCNet_ddim's refinement network ``refinenet3``).

``conv2d(x, w, bias=None, dilation=1)`` (k in {1, 3}, stride 1, padding = dilation for k = 3, dilation 1..16) is a
``torch.autograd.Function`` whose three products all run on libdiffuvolume_hip.so:
  * forward: the inference kernels through ``Conv2dPlan`` (no BN folding, no activation; Winograd routing applies);
  * input gradient: the same forward kernels on the output gradient, with the weights repacked on every call
        3x3, dilation d   conv of g with w.flip(2,3).transpose(0,1), dilation d
        1x1               conv of g with w^T
    The kernels pad channel counts internally (to 32 output and 8 input channels), so conv1's input gradient
    (128 -> 146 channels) needs no padding here.  A single-channel output gradient (conv8's, 1 -> 32 channels, 3x3,
    dilation 1) runs on ``dv_conv2d_1in_f32``, the direct kernel for single-channel inputs;
  * weight gradient: ``dv_conv2d_wgrad_f32`` (csrc/conv2d_wgrad.hip); bias gradient ``g.sum((0, 2, 3))``.
BatchNorm and Mish stay PyTorch.  ``DV_TRAIN_CONV2D=torch`` routes the function to ``F.conv2d`` instead (A/B runs,
tests).  CPU tensors raise, as everywhere on the hot path.  Only ``refinenet3`` uses this route; every other 2-D
convolution of the training graphs keeps PyTorch autograd."""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib
from .submodule import ACT_NONE, Conv2dPlan
from .train3d import _check


def route() -> str:
    """'hip' (default) or 'torch' (DV_TRAIN_CONV2D)."""
    r = os.environ.get("DV_TRAIN_CONV2D", "hip") or "hip"
    if r not in ("hip", "torch"):
        raise ValueError(f"DV_TRAIN_CONV2D must be 'hip' or 'torch', got {r!r}")
    return r


def conv2d_weight_grad(x: torch.Tensor, g: torch.Tensor, k: int, dilation: int, cout: int) -> torch.Tensor:
    """dW [Cout,Cin,k,k] of a stride-1 convolution (padding = dilation for k = 3) with input ``x`` and output
    gradient ``g``."""
    x, g = x.contiguous(), g.contiguous()
    b, cin, h, w = x.shape
    lib = _lib.load()
    n = lib.dv_conv2d_wgrad_workspace_floats(b, cin, h, w, cout, k, dilation)
    if n == 0:
        raise _lib.DiffuVolumeError(f"dv_conv2d_wgrad_f32 does not take k={k} dilation={dilation}")
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.dv_conv2d_wgrad_f32(x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, h, w,
                                           cout, k, dilation, _lib.stream_ptr()), "dv_conv2d_wgrad_f32")
    return dw


def _input_grad(g: torch.Tensor, w: torch.Tensor, dilation: int) -> torch.Tensor:
    k = w.shape[2]
    wt = (w.transpose(0, 1) if k == 1 else w.flip(2, 3).transpose(0, 1)).contiguous()      # [Cin, Cout, k, k]
    if g.shape[1] == 1 and k == 3 and dilation == 1:
        b, _, h, wd = g.shape
        dx = torch.empty((b, wt.shape[0], h, wd), dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().dv_conv2d_1in_f32(g.data_ptr(), wt.data_ptr(), 0, dx.data_ptr(), b, h, wd,
                                                     wt.shape[0], 3, ACT_NONE, _lib.stream_ptr()), "dv_conv2d_1in_f32")
        return dx
    return Conv2dPlan(wt, None, dilation=dilation, act=ACT_NONE)(g)


class Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        _check(x, "x")
        _check(weight, "weight")
        k = weight.shape[2]
        if tuple(weight.shape[2:]) != (k, k) or k not in (1, 3) or not 1 <= dilation <= 16:
            raise _lib.DiffuVolumeError(f"unsupported Conv2d: kernel {tuple(weight.shape[2:])}, dilation {dilation}")
        dilation = dilation if k == 3 else 1
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        b = None if bias is None else bias.detach()
        return Conv2dPlan(weight.detach().contiguous(), None, dilation=dilation, act=ACT_NONE, bias=b)(x)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        d, k = ctx.dilation, w.shape[2]
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(g, w.detach(), d)
        if ctx.needs_input_grad[1]:
            dw = conv2d_weight_grad(x, g, k, d, w.shape[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3))
        return dx, dw, db, None


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, dilation: int = 1) -> torch.Tensor:
    k = weight.shape[2]
    if route() == "torch":
        return F.conv2d(x, weight, bias, padding=dilation if k == 3 else 0, dilation=dilation if k == 3 else 1)
    return Conv2dFn.apply(x, weight, bias, dilation)


def conv2d_module(m: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """An nn.Conv2d of refinenet3 (stride 1, padding equal to its dilation; 1x1: no padding) on the differentiable HIP
    route."""
    k, d = m.kernel_size[0], m.dilation[0]
    if m.stride != (1, 1) or m.kernel_size != (k, k) or m.padding != ((d, d) if k == 3 else (0, 0)) or m.groups != 1:
        raise _lib.DiffuVolumeError(f"conv2d_module: stride 1 and padding = dilation only, got {m}")
    return conv2d(x, m.weight, m.bias, dilation=d)
