"""Training losses of the SceneFlow models (SceneFlow/models/loss.py) and of the KITTI12 model (KITTI12/models/loss.py,
``model_loss_kitti12``), importable from the package so that the reference's ``main.py`` scripts can take them from here:
a weighted sum of smooth-L1 (L1 for the test loss) terms over the pixels selected by ``mask``, one weight per prediction
(``zip`` stops at the shorter of the two lists)."""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn.functional as F


def _weighted(disp_ests: Sequence[torch.Tensor], disp_gt: torch.Tensor, mask: torch.Tensor, weights, fn):
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
