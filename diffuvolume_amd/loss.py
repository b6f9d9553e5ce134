"""Training losses of the SceneFlow models (SceneFlow/models/loss.py) and of the KITTI12 model (KITTI12/models/loss.py,
``model_loss_kitti12``), importable from the package so that the reference's ``main.py`` scripts can take them from here:
a weighted sum of smooth-L1 (L1 for the test loss) terms over the pixels selected by ``mask``, one weight per prediction
(``zip`` stops at the shorter of the two lists), and IGEV's ``sequence_loss`` (KITTI15/train_stereo.py:33-62).

The expressions below are the reference's, and they are what runs for CPU tensors, float64, shapes that broadcast, a ground
truth that requires a gradient, and under ``DV_TRAIN_LOSS=torch``.  Under ``DV_TRAIN_LOSS=hip`` float32 tensors on the GPU in
one common shape go to the fused forward and backward of ``train_loss`` (csrc/masked_loss.hip) instead: no ``nonzero`` and
host synchronisation per prediction, no index tensors kept for the backward, loss and gradients that repeat bit for bit.
The knob's default and the measurements behind it are in DESIGN.md, "The losses in training"."""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn.functional as F

from . import train_loss

_KIND = {F.smooth_l1_loss: "smooth_l1", F.l1_loss: "l1"}


def _weighted(disp_ests: Sequence[torch.Tensor], disp_gt: torch.Tensor, mask: torch.Tensor, weights, fn):
    if train_loss.route() == "hip":
        ests = [est for est, _ in zip(disp_ests, weights)]
        if train_loss.fusable(ests, disp_gt, mask):
            return train_loss.masked_loss_train(ests, disp_gt, mask, weights, _KIND[fn])
    return sum(w * fn(est[mask], disp_gt[mask], reduction="mean") for est, w in zip(disp_ests, weights))


def model_loss_train_attn_only(disp_ests, disp_gt, mask):
    return _weighted(disp_ests, disp_gt, mask, [1.0], F.smooth_l1_loss)


def model_loss_train_freeze_attn(disp_ests, disp_gt, mask):
    return _weighted(disp_ests, disp_gt, mask, [0.5, 0.7, 1.0], F.smooth_l1_loss)


def model_loss_train(disp_ests, disp_gt, mask):
    return _weighted(disp_ests, disp_gt, mask, [0.5, 0.5, 0.7, 1.0], F.smooth_l1_loss)


def model_loss_test(disp_ests, disp_gt, mask):
    return _weighted(disp_ests, disp_gt, mask, [1.0], F.l1_loss)


def model_loss_kitti12(disp_ests, disp_gt, mask):
    """KITTI12/models/loss.py ``model_loss``: the six predictions of PWCNet_ddim's training branch."""
    return _weighted(disp_ests, disp_gt, mask, [0.5, 0.5, 0.5, 0.7, 1.0, 1.3], F.smooth_l1_loss)


def sequence_loss(disp_preds, disp_init_pred, disp_gt, valid, loss_gamma: float = 0.9, max_disp: int = 192):
    """KITTI15/train_stereo.py:33-62: smooth-L1 of the initial disparity plus the exponentially weighted L1 of every GRU
    iteration's prediction over the valid pixels -> (loss, metrics).  ``disp_preds``: the list `forward_train` returns,
    ``disp_gt`` [B,1,H,W], ``valid`` [B,H,W].  (A single prediction gets weight 1: the reference divides by zero there.)"""
    n = len(disp_preds)
    assert n >= 1
    if train_loss.route() == "hip" and train_loss.sequence_fusable(disp_preds, disp_init_pred, disp_gt, valid):
        return train_loss.sequence_loss_train(disp_preds, disp_init_pred, disp_gt, valid, loss_gamma, max_disp)
    mag = torch.sum(disp_gt ** 2, dim=1).sqrt()
    valid = ((valid >= 0.5) & (mag < max_disp)).unsqueeze(1)
    assert valid.shape == disp_gt.shape, [valid.shape, disp_gt.shape]
    assert not torch.isinf(disp_gt[valid]).any()
    loss = 1.0 * F.smooth_l1_loss(disp_init_pred[valid], disp_gt[valid], reduction="mean")
    gamma = loss_gamma ** (15 / (n - 1)) if n > 1 else 1.0
    for i, pred in enumerate(disp_preds):
        i_loss = (pred - disp_gt).abs()
        assert i_loss.shape == valid.shape, [i_loss.shape, valid.shape, disp_gt.shape, pred.shape]
        loss = loss + gamma ** (n - i - 1) * i_loss[valid].mean()
    epe = torch.sum((disp_preds[-1] - disp_gt) ** 2, dim=1).sqrt().view(-1)[valid.view(-1)]
    metrics = {"epe": epe.mean().item(), "1px": (epe < 1).float().mean().item(), "3px": (epe < 3).float().mean().item(),
               "5px": (epe < 5).float().mean().item()}
    return loss, metrics
