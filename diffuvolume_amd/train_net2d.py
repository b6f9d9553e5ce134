"""The 2-D networks in front of the ACV and PCW 3-D stages in training on HIP kernels: the feature CNNs, ACV's
``concatconv``, the BatchNorm2d layers of PCW's ``refinenet3`` and the bilinear resize of PCW's refinement feature.

``DV_TRAIN_NET2D`` (``route()``) decides: ``torch`` keeps the ``nn.Module`` calls (MIOpen convolutions and BatchNorm,
ATen's atomic backward of ``F.interpolate``), ``hip`` runs

  * ``resize_bilinear_train(x, size)`` -- ``F.interpolate(x, size, mode="bilinear", align_corners=True)`` as one
    ``torch.autograd.Function``: forward ``dv_resize_bilinear_ac_f32`` (the inference kernel), backward
    ``dv_resize_bilinear_ac_bwd_f32`` (csrc/resize_bwd.hip), a gather that writes every element once in a fixed order;
  * ``Net2d(owner)`` -- the Conv2d + BatchNorm2d + activation (+ skip) statement of the BasicBlocks and heads.  A
    convolution is picked by its geometry: stride 1, dilation 1, 3x3 (padding 1) or 1x1 with more than 4 input channels
    runs on ``train2d.TrainConvPlan`` / ``ConvCatFn`` with one source (weight gradient on ``dv_conv2d_wgrad_cat_f32``, input
    gradient one forward launch with flipped weights packed once); everything else -- the 3 -> 32 image convolution (no
    input gradient), dilation 2, 3x3 stride 2, 1x1 stride 2 -- goes through ``train2d.conv2d_any``.  The packed plans live
    in the ``"net2d"`` slot of the owning ``PlanCache`` module under a key of the convolution weights alone (BatchNorm
    rewrites its buffers on every call): packed once per optimizer step, shared by the left and the right image.
    A BatchNorm2d in training mode with running statistics and affine parameters is ``train_norm.batch_norm_act_train``
    (``relu`` / ``mish`` / ``none``, the BasicBlock's residual as ``skip``; csrc/bn3d_act.hip takes [B,C,S] for any S)
    behind the module's own ``num_batches_tracked`` bump; any other BatchNorm keeps the PyTorch statement.  Which leaf of
    a Sequential rides in which statement is decided by ``net_blocks.walk``; ``bn_act2d`` shares its body with
    ``train_norm.bn_act`` (``bn_act_rank``) and the PyTorch statement is ``train_norm.act_statement``.

All reductions behind these are partials combined in a fixed order: the same bits on every launch.  CPU tensors raise,
as everywhere on the hot path."""
from __future__ import annotations

import functools
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _env, _lib, train2d
from .submodule import ACT_NONE, weight_key
from .net_blocks import walk
from .train_norm import bn_act_rank

SLOT = "net2d"

route = functools.partial(_env.route, "DV_TRAIN_NET2D")


# ---- bilinear resize, align_corners=True ------------------------------------------------------------------------------

class ResizeBilinearFn(torch.autograd.Function):
    """x [B,C,h,w] -> [B,C,H,W]; nothing is saved but the input's size."""

    @staticmethod
    def forward(ctx, x, hh, ww):
        x = x.contiguous()
        b, c, h, w = x.shape
        y = torch.empty((b, c, hh, ww), dtype=torch.float32, device=x.device)
        _lib.launch("dv_resize_bilinear_ac_f32", x.device, x.data_ptr(), y.data_ptr(), b * c, h, w, hh, ww)
        ctx.in_size = (h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        _lib.check_f32(dy, "grad_output")
        dy = dy.contiguous()
        b, c, hh, ww = dy.shape
        h, w = ctx.in_size
        dx = torch.empty((b, c, h, w), dtype=torch.float32, device=dy.device)
        _lib.launch("dv_resize_bilinear_ac_bwd_f32", dy.device, dy.data_ptr(), dx.data_ptr(), b * c, h, w, hh, ww)
        return dx, None, None


def resize_bilinear_train(x: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(x, size, mode="bilinear", align_corners=True) for x [B,C,h,w], differentiable in x."""
    r = route()
    _lib.check_f32(x, "x")
    if x.dim() != 4:
        raise RuntimeError(f"x must be [B,C,h,w], got {tuple(x.shape)}")
    hh, ww = (int(s) for s in size)
    if hh <= 0 or ww <= 0 or x.numel() == 0:
        raise RuntimeError(f"resize_bilinear_train: input {tuple(x.shape)} -> ({hh}, {ww})")
    if r == "torch":
        return F.interpolate(x, [hh, ww], mode="bilinear", align_corners=True)
    return ResizeBilinearFn.apply(x, hh, ww)


# ---- Conv2d + BatchNorm2d + activation (+ skip) -------------------------------------------------------------------------

def _planned(m: nn.Module) -> bool:
    """The geometry that runs on TrainConvPlan / ConvCatFn."""
    if not isinstance(m, nn.Conv2d) or isinstance(m, nn.ConvTranspose2d):
        return False
    k = m.kernel_size[0]
    return (m.kernel_size == (k, k) and k in (1, 3) and m.stride == (1, 1) and m.dilation == (1, 1) and m.groups == 1
            and m.padding == ((k - 1) // 2,) * 2 and m.padding_mode == "zeros" and m.in_channels > 4)


def _convs(owner: nn.Module, prefixes):
    return [m for name, m in owner.named_modules()
            if _planned(m) and (prefixes is None or name.startswith(tuple(prefixes)))]


def _key(convs) -> tuple:
    return weight_key(t for m in convs for t in (m.weight, m.bias) if t is not None)


def build_plans(owner: nn.Module, prefixes=None):
    """(key, plans) of the ``"net2d"`` slot of ``owner`` (called from its ``_build_plans``): one TrainConvPlan per planned
    convolution below ``owner`` (below the attribute names ``prefixes`` when given), in ``named_modules`` order."""
    convs = _convs(owner, prefixes)
    with torch.no_grad():
        return _key(convs), [train2d.TrainConvPlan(m, ACT_NONE) for m in convs]


def bn_act2d(bn: nn.Module, x: torch.Tensor, act: str, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(bn(x) + skip) for a BatchNorm2d of a training graph on the HIP route: ``train_norm.bn_act_rank`` for 4-D tensors
    -- inside the kernel's case ``batch_norm_act_train`` after the module's own ``num_batches_tracked`` bump; outside it
    the module's forward and the PyTorch statement."""
    return bn_act_rank(4, bn, x, act, skip)


class Net2d:
    """The 2-D statements of a training graph for one call: convolutions, Sequentials and BasicBlocks.

    ``Net2d(owner[, prefixes])`` is the HIP route below one ``owner`` (a ``PlanCache`` module whose
    ``_build_plans("net2d")`` is ``build_plans``): it resolves the slot once -- rebuilt when a convolution weight was
    written or swapped -- and sends every BatchNorm2d to ``bn_act2d``.  ``Net2d(conv2d=fn)`` has no packed plans (PCW's
    refinenet3): every Conv2d runs on ``fn``, a BatchNorm2d on ``bn_act2d`` only where ``route()`` is ``hip`` and on its own
    forward otherwise."""

    def __init__(self, owner: Optional[nn.Module] = None, prefixes=None, conv2d=None):
        if (owner is None) == (conv2d is None):
            raise ValueError("Net2d takes an owner with packed plans or a conv2d function")
        self.conv2d, self.plan = conv2d, {}
        self.bn2d = bn_act2d if owner is not None or route() == "hip" else None
        if owner is None:
            return
        convs = _convs(owner, prefixes)
        key = _key(convs)
        if owner.plans(SLOT)[0] != key:
            owner.drop_slot(SLOT)           # (a DataParallel replica gets the plans parked for its source's weights back)
        plans = owner.plans(SLOT)[1]
        if len(plans) != len(convs):
            raise _lib.DiffuVolumeError(f"{type(owner).__name__}: {len(plans)} packed plans for {len(convs)} convolutions")
        self.plan = {id(m): p for m, p in zip(convs, plans)}

    def conv(self, m: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
        if self.conv2d is not None:
            return self.conv2d(m, x)
        _lib.check_f32(x, "x")
        p = self.plan.get(id(m))
        if p is None:
            return train2d.conv2d_any(m, x)
        return train2d.ConvCatFn.apply(p, m.weight, m.bias, x)

    def seq(self, mod: nn.Module, x: torch.Tensor, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``mod(x) + skip`` for a (nested) Sequential of Conv2d, BatchNorm2d, ReLU and Mish (``net_blocks.walk``): a
        BatchNorm2d takes the activation behind it, or -- when it ends the walk -- the skip, into its kernel."""
        return walk(mod, x, "none", skip, conv2d=self.conv, bn2d=self.bn2d)

    def block(self, blk: nn.Module, x: torch.Tensor) -> torch.Tensor:
        """A BasicBlock: conv2(conv1(x)) + (x, or downsample(x))."""
        skip = x if blk.downsample is None else self.seq(blk.downsample, x)
        return self.seq(blk.conv2, self.seq(blk.conv1, x), skip=skip)

    def stack(self, layer: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        for blk in layer:
            x = self.block(blk, x)
        return x
