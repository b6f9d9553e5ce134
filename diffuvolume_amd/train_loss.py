"""The masked training losses on HIP kernels (csrc/masked_loss.hip).

``masked_loss_train(preds, gt, mask, weights, kind)`` is the expression every training script of the three models ends in,

    sum(w * fn(est[mask], gt[mask], reduction="mean") for est, w in zip(preds, weights))      fn = smooth-L1 or L1

as one ``torch.autograd.Function``:
  * forward: ``dv_masked_loss_fwd_f32`` -- one grid-stride launch reads ``gt`` and the mask once for all K predictions and
    leaves per-block partial sums in double, a one-block launch merges them in a fixed order; the loss stays on the device
    (no ``nonzero``, so no host synchronisation, no index tensor, no gathered copies);
  * backward: ``dv_masked_loss_bwd_f32`` -- one launch writes every element of every gradient once, zero at unselected
    pixels by selection; the incoming gradient is read from device memory (a GradScaler's scaled loss works unchanged).
Only the predictions, ``gt``, the mask and ``stats`` (K + 6 doubles per launch) are saved.  No atomics: loss and gradients
repeat bit for bit.  There is no double backward.  More than ``MAX_K`` predictions run as several launches of each kind
whose float32 losses are added in order.

``sequence_loss_train`` is KITTI15/train_stereo.py:33-62 on the same kernels with the ``valid >= 0.5 & |gt| < max_disp``
selection formed inside them; its metrics and the "selected gt is infinite" flag come back in ONE device-to-host copy.

``loss._weighted`` and ``loss.sequence_loss`` come here when ``DV_TRAIN_LOSS=hip`` and `fusable` / `sequence_fusable`
accept the arguments; everything else (CPU tensors, float64, broadcasting shapes, a ``gt`` that requires a gradient) is the
torch expression of loss.py, unchanged."""
from __future__ import annotations

import ctypes
import functools
from typing import Sequence

import torch
from torch.autograd.function import once_differentiable

from . import _env, _lib

MAX_K = 24                                  # DV_MASKED_LOSS_MAX_K: predictions per launch
MAX_BLOCKS, THREADS, PER_THREAD = 1024, 256, 4
GRID_ELEMENTS = MAX_BLOCKS * THREADS * PER_THREAD     # elements one sweep of the capped grid covers; beyond it blocks loop
EXTRA = 6                                   # count, sum |d|, #<1, #<3, #<5, flag behind the K sums of `stats`
L1, SMOOTH_L1 = 0, 1                        # DV_LOSS_*
MASK_U8, MASK_VALID_F32 = 0, 1              # DV_MASK_*
KINDS = {"l1": L1, "smooth_l1": SMOOTH_L1}

route = functools.partial(_env.route, "DV_TRAIN_LOSS")


def _chunks(k: int):
    return [(lo, min(lo + MAX_K, k)) for lo in range(0, k, MAX_K)]


def _host_arrays(preds, weights, kinds):
    k = len(preds)
    return ((ctypes.c_void_p * k)(*[_lib.ptr(p) for p in preds]), (ctypes.c_double * k)(*[float(w) for w in weights]),
            (ctypes.c_int * k)(*[int(c) for c in kinds]))


def masked_loss_forward(preds, gt, mask, mode, max_disp, weights, kinds, metric_pred=-1):
    """(loss 0-dim float32, stats [launches, MAX_K + 6] float64) on the device; row c of ``stats`` holds, for the c-th group
    of at most MAX_K predictions, its K sums, the count, the four metric sums (of prediction ``metric_pred`` when it is in
    that group) and the infinity flag in its first K + 6 entries.  Contiguous float32 tensors of one element count."""
    n, dev = gt.numel(), gt.device
    groups = _chunks(len(preds))
    stats = torch.zeros((len(groups), MAX_K + EXTRA), dtype=torch.float64, device=dev)
    losses = torch.empty(len(groups), dtype=torch.float32, device=dev)
    for c, (lo, hi) in enumerate(groups):
        k = hi - lo
        pa, wa, ka = _host_arrays(preds[lo:hi], weights[lo:hi], kinds[lo:hi])
        ws = _lib.workspace("dv_masked_loss_workspace_floats", dev, k, n)
        mp = metric_pred - lo if lo <= metric_pred < hi else -1
        _lib.launch("dv_masked_loss_fwd_f32", dev, pa, wa, ka, gt.data_ptr(), mask.data_ptr(), mode, float(max_disp), k, n,
                    mp, ws.data_ptr(), stats[c].data_ptr(), losses[c:].data_ptr())
    return (losses[0] if len(groups) == 1 else losses.sum()), stats


def masked_loss_backward(preds, gt, mask, mode, max_disp, weights, kinds, stats, gout, want):
    """The gradients of the predictions ``want`` names (None elsewhere) from the forward's ``stats`` and the incoming
    gradient ``gout`` (a float32 tensor of one element on the device)."""
    n, dev = gt.numel(), gt.device
    grads = [torch.empty_like(p) if w else None for p, w in zip(preds, want)]
    for c, (lo, hi) in enumerate(_chunks(len(preds))):
        if not any(want[lo:hi]):
            continue
        pa, wa, ka = _host_arrays(preds[lo:hi], weights[lo:hi], kinds[lo:hi])
        ga = (ctypes.c_void_p * (hi - lo))(*[_lib.ptr(g) for g in grads[lo:hi]])
        _lib.launch("dv_masked_loss_bwd_f32", dev, pa, wa, ka, gt.data_ptr(), mask.data_ptr(), mode, float(max_disp),
                    stats[c].data_ptr(), gout.data_ptr(), ga, hi - lo, n)
    return grads


class MaskedLossFn(torch.autograd.Function):
    """(gt, mask, (mode, max_disp, weights, kinds, metric_pred), *preds) -> (loss, stats); saves preds, gt, mask, stats."""

    @staticmethod
    def forward(ctx, gt, mask, cfg, *preds):
        mode, max_disp, weights, kinds, metric_pred = cfg
        loss, stats = masked_loss_forward(preds, gt, mask, mode, max_disp, weights, kinds, metric_pred)
        ctx.save_for_backward(gt, mask, stats, *preds)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_stats):
        gt, mask, stats, *preds = ctx.saved_tensors
        mode, max_disp, weights, kinds, _ = ctx.cfg
        want = ctx.needs_input_grad[3:]
        if not any(want):
            return (None,) * (3 + len(preds))
        _lib.check_f32(g_loss, "grad_loss")
        gout = g_loss.reshape(1).contiguous()
        grads = masked_loss_backward(preds, gt, mask, mode, max_disp, weights, kinds, stats, gout, want)
        return (None, None, None, *grads)


def _kinds(kind, k: int):
    names = [kind] * k if isinstance(kind, str) else list(kind)[:k]
    if len(names) != k or any(s not in KINDS for s in names):
        raise ValueError(f"kind must be 'l1' or 'smooth_l1' (one, or one per prediction), got {kind!r}")
    return [KINDS[s] for s in names]


def _byte_mask(mask: torch.Tensor) -> torch.Tensor:
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _check(preds, gt, mask_like):
    _lib.check_f32(gt, "gt")
    for i, p in enumerate(preds):
        _lib.check_f32(p, f"preds[{i}]")
        if p.numel() != gt.numel() or p.device != gt.device:
            raise RuntimeError(f"preds[{i}] has {p.numel()} elements on {p.device}, gt {gt.numel()} on {gt.device}")
    if not isinstance(mask_like, torch.Tensor):
        raise TypeError("mask must be a tensor")
    if mask_like.device != gt.device or mask_like.numel() != gt.numel():
        raise RuntimeError(f"the mask has {mask_like.numel()} elements on {mask_like.device}, gt {gt.numel()} on {gt.device}")
    if gt.requires_grad:
        raise RuntimeError("gt requires a gradient: the fused loss has none for it (DV_TRAIN_LOSS=torch has)")
    if gt.numel() == 0:
        raise RuntimeError("empty tensors")


def masked_loss_train(preds: Sequence[torch.Tensor], gt: torch.Tensor, mask: torch.Tensor, weights: Sequence[float],
                      kind="smooth_l1") -> torch.Tensor:
    """sum_k weights[k] * mean over the pixels ``mask`` selects of smooth-L1 (``kind`` 'smooth_l1', beta 1) or L1 ('l1') of
    preds[k] - gt, as a 0-dim float32 tensor on the device, differentiable with respect to the predictions.  ``preds`` and
    ``gt``: float32 on the GPU with one element count; ``mask``: bool or uint8 of that count (non-zero selects).  K is the
    shorter of ``preds`` and ``weights``.  An empty selection gives NaN and zero gradients.  Always the HIP kernels."""
    preds, weights = list(preds), [float(w) for w in weights]
    k = min(len(preds), len(weights))
    if k == 0:
        raise ValueError("masked_loss_train needs at least one prediction and one weight")
    preds, weights = preds[:k], weights[:k]
    _check(preds, gt, mask)
    cfg = (MASK_U8, 0.0, tuple(weights), tuple(_kinds(kind, k)), -1)
    loss, _ = MaskedLossFn.apply(gt.contiguous(), _byte_mask(mask), cfg, *[p.contiguous() for p in preds])
    return loss


def sequence_metrics(stats: torch.Tensor, k: int) -> dict:
    """`stats` of a forward over ``k`` predictions whose metric prediction is the last one -> sequence_loss's metrics as
    Python floats, with ONE device-to-host copy; AssertionError from that copy when the forward saw a selected gt that is
    infinite (the reference's ``assert not torch.isinf(disp_gt[valid]).any()``)."""
    last = stats.cpu()[-1].tolist()
    kl = k - (stats.shape[0] - 1) * MAX_K
    count, (epe, c1, c3, c5), inf = last[kl], last[kl + 1:kl + 5], last[kl + 5] != 0
    assert not inf, "a selected pixel of disp_gt is infinite"
    nan = float("nan")
    return {"epe": epe / count if count else nan, "1px": c1 / count if count else nan,
            "3px": c3 / count if count else nan, "5px": c5 / count if count else nan}


def sequence_loss_train(disp_preds, disp_init_pred, disp_gt, valid, loss_gamma: float = 0.9, max_disp: float = 192):
    """KITTI15/train_stereo.py:33-62 -> (loss, metrics): smooth-L1 of the initial disparity with weight 1 plus L1 of the n
    predictions with weights gamma ** (n - i - 1), gamma = loss_gamma ** (15 / (n - 1)) (1 for n == 1), over the pixels with
    ``valid >= 0.5`` and ``|gt| < max_disp``; metrics epe / 1px / 3px / 5px of the last prediction as Python floats.
    ``valid``: float32 [B,H,W]; the others float32 [B,1,H,W].  The reference's assert that no selected gt is infinite is
    `sequence_metrics`'s, on the flag the forward leaves in ``stats`` (under this selection an infinite gt is never selected,
    here as in the reference: inf < max_disp is false; a byte mask can select one)."""
    n = len(disp_preds)
    assert n >= 1
    preds = [disp_init_pred, *disp_preds]
    _check(preds, disp_gt, valid)
    _lib.check_f32(valid, "valid")
    gamma = loss_gamma ** (15 / (n - 1)) if n > 1 else 1.0
    weights = (1.0, *[gamma ** (n - i - 1) for i in range(n)])
    cfg = (MASK_VALID_F32, float(max_disp), weights, (SMOOTH_L1, *[L1] * n), n)
    loss, stats = MaskedLossFn.apply(disp_gt.contiguous(), valid.contiguous(), cfg, *[p.contiguous() for p in preds])
    return loss, sequence_metrics(stats, n + 1)


def _gpu_f32(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def fusable(preds, gt, mask) -> bool:
    """Whether `loss._weighted` may hand these arguments to `masked_loss_train`: every prediction and gt float32 on one GPU
    in ONE shape (no broadcasting), a bool / uint8 mask of that shape there too, gt without a gradient, at least one
    prediction and one element."""
    if not preds or not _gpu_f32(gt) or gt.requires_grad or gt.numel() == 0:
        return False
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        return False
    if mask.device != gt.device or mask.shape != gt.shape:
        return False
    return all(_gpu_f32(p) and p.device == gt.device and p.shape == gt.shape for p in preds)


def sequence_fusable(disp_preds, disp_init_pred, disp_gt, valid) -> bool:
    """The same for `loss.sequence_loss`: one-channel [B,1,H,W] float32 tensors on one GPU and a float32 ``valid`` [B,H,W]."""
    if not _gpu_f32(disp_gt) or disp_gt.requires_grad or disp_gt.dim() != 4 or disp_gt.shape[1] != 1 or disp_gt.numel() == 0:
        return False
    if not _gpu_f32(valid) or valid.device != disp_gt.device or valid.requires_grad:
        return False
    if tuple(valid.shape) != (disp_gt.shape[0], *disp_gt.shape[2:]):
        return False
    return all(_gpu_f32(p) and p.device == disp_gt.device and p.shape == disp_gt.shape
               for p in (disp_init_pred, *disp_preds))
