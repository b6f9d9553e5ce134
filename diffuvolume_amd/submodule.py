"""L1 ops of the DiffuVolume hot path behind the reference's function signatures.

Same names, argument meaning and error behaviour as SceneFlow/models/submodule.py
(``build_gwc_volume`` :228-238, ``build_concat_volume`` :180-191,
``disparity_regression`` :173-177) and their KITTI12 / KITTI15 twins; the work is
done by the HIP kernels of libdiffuvolume_hip.so on the current stream.  The three
builders / the regression are differentiable in the reference (they are used in training):
when autograd is recording and an input requires grad, the two volume builders dispatch to the
autograd functions of train_volume.py (eval kernel forward, HIP backward) for CUDA float32
tensors and to a differentiable PyTorch statement of the same function otherwise;
everything else is inference only and runs on the MI355X or raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib, train_volume
# the plans and what goes with them live in plans.py; every name that was importable from here still is, as the same object
from .plans import (ACT_LEAKY, ACT_MISH, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, AttentionConcatVolume,  # noqa: F401
                    Conv2dF16Plan, Conv2dPairPlan, Conv2dPlan, Conv3dPlan, Deconv2dK4S2Plan, Deconv3dPlan, PlanCache,
                    PointwiseExpandPlan, Rank1FilterPlan, _OVERFLOW_FLAGS, _dev_f32, _fold_bn, check_split_overflow,
                    default_conv_precision, set_default_conv_precision, split_overflow_flag, volume_factors, weight_key)

__all__ = ["build_gwc_volume", "build_concat_volume", "build_concat_attention_volume", "AttentionConcatVolume",
           "volume_factors",
           "disparity_regression", "upsample_softmax_regress", "Conv3dPlan", "Conv2dPlan", "Conv2dF16Plan", "Deconv3dPlan",
           "window_attention", "feature_gate", "softmax_regress", "refine_inputs", "patch_volume", "ACT_NONE", "ACT_RELU", "ACT_MISH", "ACT_LEAKY", "ACT_SIGMOID", "ACT_TANH"]


def _wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _on_hip_f32(*tensors) -> bool:
    """CUDA float32 tensors: what the autograd functions of train_volume.py take (their forward is the eval launch)."""
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _shift_bank(t: torch.Tensor, maxdisp: int) -> torch.Tensor:
    """[B,C,H,W] -> [B,C,D,H,W] with bank[..., d, y, x] = t[..., y, x - d] (0 where x < d): every disparity shift
    of the target features as one strided view of a left-padded copy (differentiable)."""
    w = t.shape[-1]
    win = torch.nn.functional.pad(t, (maxdisp - 1, 0)).unfold(3, w, 1)      # [B,C,H,D,W], window k starts at D-1-d
    return win.flip(3).permute(0, 1, 3, 2, 4)


def _valid_wedge(maxdisp: int, w: int, device) -> torch.Tensor:
    """[D,1,W] bool: x >= d (the reference leaves `new_zeros` where the shifted target has no pixel)."""
    return (torch.arange(w, device=device).view(1, 1, w) >= torch.arange(maxdisp, device=device).view(maxdisp, 1, 1))


def _gwc_volume_autograd(ref, tgt, maxdisp, num_groups):
    """Differentiable statement of build_gwc_volume (submodule.py:209-238) for training / autograd callers:
    products against the shift bank, mean over the channels of a group, exact zeros in the x < d wedge."""
    b, c, h, w = ref.shape
    cpg = c // num_groups
    valid = _valid_wedge(maxdisp, w, ref.device)
    step = max(1, (64 << 20) // max(1, b * cpg * maxdisp * h * w))           # groups per slab (<= ~256 MB of products)
    slabs = []
    for g0 in range(0, num_groups, step):
        g1 = min(num_groups, g0 + step)
        r = ref[:, g0 * cpg:g1 * cpg]
        prod = r.unsqueeze(2) * _shift_bank(tgt[:, g0 * cpg:g1 * cpg], maxdisp)
        slabs.append(prod.reshape(b, g1 - g0, cpg, maxdisp, h, w).mean(dim=2))
    vol = torch.cat(slabs, dim=1)
    return torch.where(valid, vol, torch.zeros((), dtype=vol.dtype, device=vol.device)).contiguous()


def _concat_volume_autograd(ref, tgt, maxdisp, zero_left):
    """Differentiable statement of build_concat_volume (submodule.py:180-191; KITTI12 :86-97 with zero_left)."""
    b, c, h, w = ref.shape
    left = ref.unsqueeze(2).expand(b, c, maxdisp, h, w)
    if zero_left:
        left = torch.where(_valid_wedge(maxdisp, w, ref.device), left, torch.zeros((), dtype=ref.dtype, device=ref.device))
    return torch.cat((left, _shift_bank(tgt, maxdisp)), dim=1).contiguous()


def build_gwc_volume(refimg_fea: torch.Tensor, targetimg_fea: torch.Tensor, maxdisp: int,
                     num_groups: int) -> torch.Tensor:
    """[B,C,H,W] x2 -> [B,num_groups,maxdisp,H,W] (submodule.py:228-238)."""
    if _wants_grad(refimg_fea, targetimg_fea):
        if refimg_fea.dim() != 4 or refimg_fea.shape != targetimg_fea.shape:
            raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(refimg_fea.shape)} vs {tuple(targetimg_fea.shape)}")
        assert refimg_fea.shape[1] % num_groups == 0          # submodule.py:211
        if _on_hip_f32(refimg_fea, targetimg_fea):             # eval kernel + HIP backward (DV_TRAIN_VOLUME)
            return train_volume.build_gwc_volume_train(refimg_fea, targetimg_fea, maxdisp, num_groups)
        return _gwc_volume_autograd(refimg_fea, targetimg_fea, maxdisp, num_groups)
    ref = _dev_f32(refimg_fea, "refimg_fea")
    tgt = _dev_f32(targetimg_fea, "targetimg_fea")
    if ref.dim() != 4 or ref.shape != tgt.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(ref.shape)} vs {tuple(tgt.shape)}")
    b, c, h, w = ref.shape
    assert c % num_groups == 0          # submodule.py:211
    out = torch.empty((b, num_groups, maxdisp, h, w), dtype=torch.float32, device=ref.device)
    if out.numel() == 0:                # empty batch / empty image: the reference returns the empty volume
        return out
    _lib.timed_launch("gwc_volume", 2.0 * out.numel() * (c // num_groups), 4.0 * (2 * ref.numel() + out.numel()),
                      "dv_gwc_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), out.data_ptr(), b, c, h, w, maxdisp, num_groups)
    return out


def build_concat_volume(refimg_fea: torch.Tensor, targetimg_fea: torch.Tensor, maxdisp: int,
                        zero_left: bool = False) -> torch.Tensor:
    """[B,C,H,W] x2 -> [B,2C,maxdisp,H,W] (submodule.py:180-191).  ``zero_left=True``
    is the KITTI12 flavour (KITTI12/models/submodule.py:86-97)."""
    if _wants_grad(refimg_fea, targetimg_fea):
        if refimg_fea.dim() != 4 or refimg_fea.shape != targetimg_fea.shape:
            raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(refimg_fea.shape)} vs {tuple(targetimg_fea.shape)}")
        if _on_hip_f32(refimg_fea, targetimg_fea):             # eval kernel + HIP backward (DV_TRAIN_VOLUME)
            return train_volume.build_concat_volume_train(refimg_fea, targetimg_fea, maxdisp, bool(zero_left))
        return _concat_volume_autograd(refimg_fea, targetimg_fea, maxdisp, bool(zero_left))
    ref = _dev_f32(refimg_fea, "refimg_fea")
    tgt = _dev_f32(targetimg_fea, "targetimg_fea")
    if ref.dim() != 4 or ref.shape != tgt.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(ref.shape)} vs {tuple(tgt.shape)}")
    b, c, h, w = ref.shape
    out = torch.empty((b, 2 * c, maxdisp, h, w), dtype=torch.float32, device=ref.device)
    if out.numel() == 0:
        return out
    _lib.launch("dv_concat_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), out.data_ptr(), b, c, h, w, maxdisp,
                int(bool(zero_left)))
    return out



def _attention_factors(refimg_fea, targetimg_fea, att_weights, maxdisp):
    ref = _dev_f32(refimg_fea, "refimg_fea")
    tgt = _dev_f32(targetimg_fea, "targetimg_fea")
    att = _dev_f32(att_weights, "att_weights")
    b, c, h, w = ref.shape
    if ref.shape != tgt.shape or tuple(att.shape) != (b, 1, maxdisp, h, w):
        raise RuntimeError("shape mismatch between features and attention weights")
    p_att = torch.empty((b, maxdisp, h, w), dtype=torch.float32, device=ref.device)
    if p_att.numel() == 0:              # empty batch / image: the reference's product is the empty volume
        return ref, tgt, att, p_att
    _lib.launch("dv_softmax_d_f32", ref.device, att.data_ptr(), p_att.data_ptr(), b, maxdisp, h * w)
    return ref, tgt, att, p_att


def build_concat_attention_volume(refimg_fea: torch.Tensor, targetimg_fea: torch.Tensor,
                                  att_weights: torch.Tensor, maxdisp: int, lazy: bool = False):
    """``F.softmax(att_weights, dim=2) * build_concat_volume(...)`` in one pass
    (acv_ddim.py:388-390).  att_weights [B,1,maxdisp,H,W] are logits.

    ``lazy=False`` (default): the [B,2C,maxdisp,H,W] tensor, with private copies of its factors riding along so that
    ``ACVNet_DDIM`` can run its first aggregation layer on them; the ride-along is void the moment the tensor is
    edited in place (``Rank1FilterPlan.applies`` compares ``_version``).  ``lazy=True``: an ``AttentionConcatVolume``
    -- the factors only, nothing of the volume written -- which ``ACVNet_DDIM.ddim_sample / model_predictions`` accept
    in the tensor's place (what ``ACVNet_DDIM.forward`` passes itself)."""
    ref, tgt, att, p_att = _attention_factors(refimg_fea, targetimg_fea, att_weights, maxdisp)
    b, c, h, w = ref.shape
    # private copies (2 x 31 MB at batch 8): `ref` / `tgt` may BE the caller's tensors (`contiguous()` of a contiguous
    # tensor is the tensor itself), and the rank-1 tables are built from them later, on the first DDIM step
    handle = AttentionConcatVolume(p_att, ref.clone(), tgt.clone())
    if lazy:
        return handle
    out = torch.empty((b, 2 * c, maxdisp, h, w), dtype=torch.float32, device=ref.device)
    if out.numel() == 0:
        return out
    _lib.timed_launch("concat_attn_volume", 2.0 * out.numel(), 4.0 * (2 * ref.numel() + att.numel() + out.numel()),
                      "dv_concat_attn_volume_f32", ref.device, ref.data_ptr(), tgt.data_ptr(), att.data_ptr(), out.data_ptr(),
                      b, c, h, w, maxdisp)
    out._dv_factors = handle
    out._dv_factors_version = out._version
    return out



def disparity_regression(x: torch.Tensor, maxdisp: int, keepdim: bool = False) -> torch.Tensor:
    """[B,D,H,W] probabilities -> sum_d d*p_d (submodule.py:173-177; keepdim=True is the
    KITTI15 flavour, core/submodule.py:219-223)."""
    assert len(x.shape) == 4            # submodule.py:174
    if _wants_grad(x):                  # training: the differentiable statement (sum_d d * p_d)
        if x.shape[1] != maxdisp:
            raise RuntimeError(f"The size of tensor a ({x.shape[1]}) must match the size of tensor b ({maxdisp}) "
                               "at non-singleton dimension 1")
        k = torch.arange(0, maxdisp, dtype=x.dtype, device=x.device).view(1, maxdisp, 1, 1)
        return torch.sum(x * k, 1, keepdim=keepdim)
    x = _dev_f32(x, "x")
    b, d, h, w = x.shape
    if d != maxdisp:
        raise RuntimeError(f"The size of tensor a ({d}) must match the size of tensor b ({maxdisp}) "
                           "at non-singleton dimension 1")
    out = torch.empty((b, h, w), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out.unsqueeze(1) if keepdim else out
    _lib.launch("dv_disparity_regression_f32", x.device, x.data_ptr(), out.data_ptr(), b, d, h, w)
    return out.unsqueeze(1) if keepdim else out


def upsample_softmax_regress(cost: torch.Tensor, want_uncertainty: bool = True,
                             align_corners: bool = False, out_disp: Optional[torch.Tensor] = None
                             ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """cost [B,1,D,h,w] (or [B,D,h,w]) -> (disp [B,4h,4w], uncertainty | None): trilinear x4,
    softmax over 4D bins, soft-argmax and sum_k |disp-k| p_k (acv_ddim.py:267-270, :325-329)."""
    cost = _dev_f32(cost, "cost")
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise RuntimeError("cost must have one channel")
        cost = cost[:, 0]
    b, d, h, w = cost.shape
    if out_disp is None:
        disp = torch.empty((b, 4 * h, 4 * w), dtype=torch.float32, device=cost.device)
    else:                                   # e.g. a slice of the per-step stack of ddim_sample
        disp = out_disp
        if tuple(disp.shape) != (b, 4 * h, 4 * w) or disp.dtype != torch.float32 or not disp.is_contiguous() \
                or disp.device != cost.device:
            raise RuntimeError("out_disp must be a contiguous float32 [B,4h,4w] tensor on the cost's device")
    unc = torch.empty_like(disp) if want_uncertainty else None
    _lib.timed_launch("upsample_softmax_regress", 0.0, 4.0 * (cost.numel() + 2 * disp.numel()),
                      "dv_upsample_softmax_regress_f32", cost.device, cost.data_ptr(), disp.data_ptr(), _lib.ptr(unc), b, d, h, w,
                      int(bool(align_corners)))
    return disp, unc


def softmax_regress(cost: torch.Tensor) -> torch.Tensor:
    """`disparity_regression(F.softmax(cost, 1), D)` without upsampling (igev_stereo_ddim.py:382-383):
    cost [B,1,D,H,W] or [B,D,H,W] -> [B,H,W]."""
    cost = _dev_f32(cost, "cost")
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise RuntimeError("cost must have one channel")
        cost = cost[:, 0]
    b, d, h, w = cost.shape
    disp = torch.empty((b, h, w), dtype=torch.float32, device=cost.device)
    _lib.timed_launch("softmax_regress", 0.0, 4.0 * (cost.numel() + disp.numel()), "dv_softmax_regress_f32", cost.device,
                      cost.data_ptr(), disp.data_ptr(), b, d, h, w)
    return disp


def feature_gate(cv: torch.Tensor, logit: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """`torch.sigmoid(feat_att) * cv` of FeatureAtt.forward (KITTI15/core/submodule.py:234-239); logit is the
    2-D branch's output [B,C,H,W] before the sigmoid, cv the volume [B,C,D,H,W]."""
    cv = _dev_f32(cv, "cv")
    logit = _dev_f32(logit, "logit")
    b, c, d, h, w = cv.shape
    if tuple(logit.shape) != (b, c, h, w):
        raise RuntimeError(f"gate logits {tuple(logit.shape)} do not match volume {tuple(cv.shape)}")
    out = cv if inplace else torch.empty_like(cv)
    _lib.timed_launch("feature_gate", float(cv.numel()), 8.0 * cv.numel(), "dv_feature_gate_f32", cv.device,
                      cv.data_ptr(), logit.data_ptr(), out.data_ptr(), b, c, d, h, w)
    return out


def refine_inputs(left: torch.Tensor, right: torch.Tensor, disp: torch.Tensor, du_a: torch.Tensor,
                  du_b: torch.Tensor, maxshift: int = 24) -> torch.Tensor:
    """cat(left - warp(right, disp), left, Mish(du_a*disp + du_b), disp, corr(left, warp(right, disp), +-24)):
    the refinement network's input (KITTI12/models/pwcnet_ddim.py:486-502) in one kernel.
    left/right [B,C,H,W], disp [B,1,H,W] or [B,H,W] -> [B, 3C+1+49, H, W]."""
    left, right = _dev_f32(left, "left"), _dev_f32(right, "right")
    disp = _dev_f32(disp, "disp")
    b, c, h, w = left.shape
    if tuple(right.shape) != (b, c, h, w) or disp.numel() != b * h * w:
        raise RuntimeError("left / right / disp shapes do not match")
    du_a, du_b = _dev_f32(du_a, "du_a"), _dev_f32(du_b, "du_b")
    out = torch.empty((b, 3 * c + 1 + 2 * maxshift + 1, h, w), dtype=torch.float32, device=left.device)
    _lib.timed_launch("refine_inputs", 2.0 * b * h * w * c * (2 * maxshift + 1), 4.0 * (2 * left.numel() + out.numel()),
                      "dv_refine_inputs_f32", left.device, left.data_ptr(), right.data_ptr(), disp.data_ptr(), du_a.data_ptr(),
                      du_b.data_ptr(), out.data_ptr(), b, c, h, w, maxshift)
    return out


def patch_volume(gwc: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, dilation: torch.Tensor) -> torch.Tensor:
    """`patch` followed by `patch_l1/l2/l3` (acv_ddim.py:377-381): two per-channel (1,3,3) stencils in one pass.
    gwc [B,G,D,H,W]; w1, w2 [G,9] float32; dilation [G] int32 (1..3).  The dilation table is turned into runs of
    consecutive groups on the host ONCE per tensor object (cached on it: a device tensor costs one synchronising read
    the first time) so that the launcher can pick the dilation-specialised 16-byte kernels."""
    gwc = _dev_f32(gwc, "gwc")
    b, g, d, h, w = gwc.shape
    w1, w2 = _dev_f32(w1, "w1"), _dev_f32(w2, "w2")
    if tuple(w1.shape) != (g, 9) or tuple(w2.shape) != (g, 9) or dilation.numel() != g or dilation.dtype != torch.int32:
        raise RuntimeError("w1 / w2 must be [G,9] and dilation [G] int32")
    runs = getattr(dilation, "_dv_runs", None)
    key = (dilation.data_ptr(), dilation._version)       # (a `.data` swap keeps _version: the pointer is part of the key)
    if runs is None or runs[0] != key:
        vals, r = dilation.detach().cpu().tolist(), []
        for i, v in enumerate(vals):
            if r and r[-1][2] == v:
                r[-1][1] += 1
            else:
                r.append([i, 1, v])
        arr = lambda k: (ctypes.c_int * len(r))(*[x[k] for x in r])
        runs = (key, len(r), arr(0), arr(1), arr(2), all(1 <= x[2] <= 3 for x in r))
        dilation._dv_runs = runs
    out = torch.empty_like(gwc)
    dil_dev = dilation.contiguous()
    name, tail = ("dv_patch_volume_runs_f32", runs[1:5]) if runs[5] else ("dv_patch_volume_f32", ())
    _lib.timed_launch("patch_volume", 36.0 * gwc.numel(), 8.0 * gwc.numel(), name, gwc.device, gwc.data_ptr(), w1.data_ptr(),
                      w2.data_ptr(), dil_dev.data_ptr(), out.data_ptr(), b, g, d, h, w, *tail)
    return out


def window_attention(x: torch.Tensor, qkv_w: torch.Tensor, qkv_b: torch.Tensor, proj_w: torch.Tensor,
                     proj_b: torch.Tensor, heads: int = 16) -> torch.Tensor:
    """attention_block.forward (submodule.py:398-429) on [B,C,D,H,W]."""
    x = _dev_f32(x, "x")
    b, c, d, h, w = x.shape
    qkv_w = _dev_f32(qkv_w.detach(), "qkv_w")
    qkv_b = _dev_f32(qkv_b.detach(), "qkv_b")
    proj_w = _dev_f32(proj_w.detach().reshape(c, c), "proj_w")
    proj_b = _dev_f32(proj_b.detach(), "proj_b")
    out = torch.empty_like(x)
    flops = float(b * d * h * w) * (2.0 * c * 3 * c + 2.0 * c * c + 4.0 * 64 * c)
    _lib.timed_launch("window_attn3d", flops, 8.0 * x.numel(), "dv_window_attn3d_f32", x.device, x.data_ptr(), qkv_w.data_ptr(),
                      qkv_b.data_ptr(), proj_w.data_ptr(), proj_b.data_ptr(), out.data_ptr(), b, c, d, h, w, heads, issued=flops)
    return out
