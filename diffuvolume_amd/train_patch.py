"""The patch stencils of ACVNet_DDIM's attention branch in training on HIP kernels (csrc/patch_volume.hip forward,
csrc/patch_volume_bwd.hip backward).

``patch_volume_train(gwc, w1, w2, dilation)`` is the statement the attention branch applies to the group-wise correlation
volume (SceneFlow/models/acv_ddim.py:377-381),

    gwc   = patch(gwc)                                         Conv3d(G, G, (1,3,3), groups=G, padding (0,1,1))
    patch = cat(patch_l1(gwc[:, :8]), patch_l2(gwc[:, 8:24]), patch_l3(gwc[:, 24:40]))       dilation 1 / 2 / 3

with the stencils given as ``w1``, ``w2`` [G,9] and the dilation of each group as a host sequence, as one
``torch.autograd.Function``:
  * forward: ``dv_patch_volume_runs_f32``, the eval path's fused pass (the bits of ``submodule.patch_volume``);
  * backward: ``dv_patch_volume_bwd_f32`` -- one pass that reads ``gwc`` and the gradient once, recomputes the first
    stencil's output on chip and writes the input gradient once; the weight gradients are per-block partials merged in a
    fixed order in double.  Only ``gwc``, ``w1`` and ``w2`` are saved: not the intermediate volume, the slice copies or
    the concatenation.  No atomics: the same bits on every launch.  A gradient that is not needed is not computed.
There is no double backward.  ``DV_TRAIN_PATCH=torch`` routes the function to the PyTorch statement (A/B runs, tests).
CPU tensors raise, as everywhere on the hot path."""
from __future__ import annotations

import ctypes
import functools
from typing import Sequence

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _env, _lib


route = functools.partial(_env.route, "DV_TRAIN_PATCH")


@functools.lru_cache(maxsize=16)
def _runs(dilation: tuple):
    """Runs of consecutive groups with one dilation, as the launchers take them: (n, g0[], ng[], dil[]) and the plain
    (g0, ng, dil) triples.  Host arithmetic on a host sequence: no device read."""
    r = []
    for i, v in enumerate(dilation):
        if r and r[-1][2] == v:
            r[-1][1] += 1
        else:
            r.append([i, 1, v])
    arr = lambda k: (ctypes.c_int * len(r))(*[x[k] for x in r])
    return len(r), arr(0), arr(1), arr(2), tuple(tuple(x) for x in r)


@functools.lru_cache(maxsize=16)
def _dilation_table(dilation: tuple, device: torch.device) -> torch.Tensor:
    """The per-group table the forward's element-wise kernel reads (W % 4 != 0 or unaligned tensors)."""
    return torch.tensor(dilation, dtype=torch.int32, device=device)


def _statement(gwc, w1, w2, dilation):
    """The PyTorch statement: the depth-wise convolution of all groups, then one per run of the slices, and their cat."""
    g = gwc.shape[1]
    mid = F.conv3d(gwc, w1.reshape(g, 1, 1, 3, 3), None, 1, (0, 1, 1), 1, g)
    outs = [F.conv3d(mid[:, g0:g0 + ng], w2[g0:g0 + ng].reshape(ng, 1, 1, 3, 3), None, 1, (0, dl, dl), dl, ng)
            for g0, ng, dl in _runs(dilation)[4]]
    return torch.cat(outs, dim=1)


class PatchVolumeFn(torch.autograd.Function):
    """gwc [B,G,D,H,W], w1, w2 [G,9] -> the two stencils applied in one pass; saves its three inputs only."""

    @staticmethod
    def forward(ctx, gwc, w1, w2, dilation):
        gwc, w1, w2 = gwc.contiguous(), w1.contiguous(), w2.contiguous()
        b, g, d, h, w = gwc.shape
        n, g0, ng, dl, _ = _runs(dilation)
        out = torch.empty_like(gwc)
        table = _dilation_table(dilation, gwc.device)
        _lib.launch("dv_patch_volume_runs_f32", gwc.device, gwc.data_ptr(), w1.data_ptr(), w2.data_ptr(), table.data_ptr(),
                    out.data_ptr(), b, g, d, h, w, n, g0, ng, dl)
        ctx.save_for_backward(gwc, w1, w2)
        ctx.dilation = dilation
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        gwc, w1, w2 = ctx.saved_tensors
        want_x, want_w1, want_w2 = ctx.needs_input_grad[:3]
        if not (want_x or want_w1 or want_w2):
            return None, None, None, None
        _lib.check_f32(dout, "grad_output")
        dout = dout.contiguous()
        b, g, d, h, w = gwc.shape
        n, g0, ng, dl, _ = _runs(ctx.dilation)
        dgwc = torch.empty_like(gwc) if want_x else None
        dw1 = torch.empty_like(w1) if want_w1 else None
        dw2 = torch.empty_like(w2) if want_w2 else None
        ws = None
        if want_w1 or want_w2:
            ws = _lib.workspace("dv_patch_volume_bwd_workspace_floats", gwc.device, b, g, d, h, w)
        _lib.launch("dv_patch_volume_bwd_f32", gwc.device, gwc.data_ptr(), w1.data_ptr(), w2.data_ptr(), dout.data_ptr(),
                    _lib.ptr(dgwc), _lib.ptr(dw1), _lib.ptr(dw2), _lib.ptr(ws), b, g, d, h, w, n, g0, ng, dl)
        return dgwc, dw1, dw2, None


def patch_volume_train(gwc: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, dilation: Sequence[int]) -> torch.Tensor:
    """`patch` followed by `patch_l1/l2/l3` for gwc [B,G,D,H,W] with the stencils w1, w2 [G,9] and ``dilation`` a host
    sequence of G ints in 1..3, differentiable in gwc, w1 and w2.  Returns a fresh tensor."""
    r = route()
    for name, t in (("gwc", gwc), ("w1", w1), ("w2", w2)):
        _lib.check_f32(t, name)
    if gwc.dim() != 5:
        raise RuntimeError(f"gwc must be [B,G,D,H,W], got {tuple(gwc.shape)}")
    g = gwc.shape[1]
    if tuple(w1.shape) != (g, 9) or tuple(w2.shape) != (g, 9):
        raise RuntimeError(f"w1 and w2 must be {(g, 9)}, got {tuple(w1.shape)} and {tuple(w2.shape)}")
    dilation = tuple(int(v) for v in dilation)
    if len(dilation) != g or not all(1 <= v <= 3 for v in dilation):
        raise ValueError(f"dilation must be {g} ints in 1..3, got {dilation}")
    if gwc.numel() == 0:
        raise RuntimeError(f"gwc is empty: {tuple(gwc.shape)}")
    if r == "torch":
        return _statement(gwc, w1, w2, dilation)
    return PatchVolumeFn.apply(gwc, w1, w2, dilation)
