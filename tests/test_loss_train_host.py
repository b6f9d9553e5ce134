"""What can be checked of the fused training losses without a GPU: the DV_TRAIN_LOSS switch, the routing of loss.py (CPU
tensors see the torch expression's bits on both values of the switch), the fixture tests/golden/loss_train.npz against the
package's CPU expression, the seeded inputs, and the rows of the third ABI table."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import _env, _lib, loss as L, synth, train_loss
import diffuvolume_amd as dv

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("dv_masked_loss_workspace_floats", "dv_masked_loss_fwd_f32", "dv_masked_loss_bwd_f32")
WEIGHTS = {"model_loss_train": ([0.5, 0.5, 0.7, 1.0], F.smooth_l1_loss),
           "model_loss_train_freeze_attn": ([0.5, 0.7, 1.0], F.smooth_l1_loss),
           "model_loss_train_attn_only": ([1.0], F.smooth_l1_loss), "model_loss_test": ([1.0], F.l1_loss),
           "model_loss_kitti12": ([0.5, 0.5, 0.5, 0.7, 1.0, 1.3], F.smooth_l1_loss)}


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "loss_train.npz") as z:
        return {k: z[k] for k in z.files}


def plain(preds, gt, mask, weights, fn):
    return sum(w * fn(est[mask], gt[mask], reduction="mean") for est, w in zip(preds, weights))


def plain_sequence(disp_preds, disp_init_pred, disp_gt, valid, loss_gamma=0.9, max_disp=192):
    """KITTI15/train_stereo.py:33-62 as loss.py has always stated it."""
    n = len(disp_preds)
    mag = torch.sum(disp_gt ** 2, dim=1).sqrt()
    valid = ((valid >= 0.5) & (mag < max_disp)).unsqueeze(1)
    loss = 1.0 * F.smooth_l1_loss(disp_init_pred[valid], disp_gt[valid], reduction="mean")
    gamma = loss_gamma ** (15 / (n - 1)) if n > 1 else 1.0
    for i, pred in enumerate(disp_preds):
        loss = loss + gamma ** (n - i - 1) * (pred - disp_gt).abs()[valid].mean()
    epe = torch.sum((disp_preds[-1] - disp_gt) ** 2, dim=1).sqrt().view(-1)[valid.view(-1)]
    return loss, {"epe": epe.mean().item(), "1px": (epe < 1).float().mean().item(),
                  "3px": (epe < 3).float().mean().item(), "5px": (epe < 5).float().mean().item()}


def test_switch_is_listed_documented_and_refuses_bad_values(monkeypatch):
    assert _env.KNOBS["DV_TRAIN_LOSS"][0] in ("hip", "torch")
    assert "DV_TRAIN_LOSS" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_LOSS", raising=False)
    assert train_loss.route() == _env.KNOBS["DV_TRAIN_LOSS"][0]
    for value in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_LOSS", value)
        assert train_loss.route() == value                           # read on every call
    monkeypatch.setenv("DV_TRAIN_LOSS", "cpu")
    with pytest.raises(ValueError):
        train_loss.route()
    preds, gt, mask = synth.loss_train_inputs(**synth.LOSS_TRAIN_CASE)
    with pytest.raises(ValueError):
        L.model_loss_train(preds, gt, mask)
    assert dv.masked_loss_train is train_loss.masked_loss_train and "masked_loss_train" in dv.__all__
    assert train_loss.MAX_K >= 24


@pytest.mark.parametrize("route", ["hip", "torch"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_calls_are_the_plain_expression_bit_for_bit(route, dtype, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_LOSS", route)
    preds, gt, mask = synth.loss_train_inputs(**synth.LOSS_TRAIN_CASE, dtype=dtype)
    for name, (weights, fn) in WEIGHTS.items():
        a = [p.clone().requires_grad_(True) for p in preds]
        b = [p.clone().requires_grad_(True) for p in preds]
        got, want = getattr(L, name)(a, gt, mask), plain(b, gt, mask, weights, fn)
        assert got.dtype == dtype and torch.equal(got, want), name
        got.backward()
        want.backward()
        for x, y in zip(a, b):
            assert (x.grad is None and y.grad is None) or torch.equal(x.grad, y.grad), name
    sp, init, sgt, valid = synth.igev_sequence_loss_inputs(synth.IGEV_TRAIN_STEP_CASE["seed"], dtype=dtype)
    got, gm = L.sequence_loss(sp, init, sgt, valid, max_disp=192)
    want, wm = plain_sequence(sp, init, sgt, valid, max_disp=192)
    assert torch.equal(got, want) and gm == wm
    # broadcasting shapes stay with the torch expression too: a [H,W] mask row against [B,H,W] is not what it takes, a
    # [B,H,W] mask on [B,H,W] predictions with a gt that requires a gradient is
    g = gt.clone().requires_grad_(True)
    L.model_loss_test(preds, g, mask).backward()
    assert g.grad is not None


def test_fixture_matches_the_package_expression(gold):
    c = synth.LOSS_TRAIN_CASE
    assert int(gold["seed"]) == c["seed"] and tuple(int(v) for v in gold["shape"]) == (c["b"], c["h"], c["w"])
    assert [str(n) for n in gold["names"]] == list(WEIGHTS) and int(gold["k"]) == c["k"] == 6
    for tag, dt, tol in (("f32", torch.float32, 1e-6), ("f64", torch.float64, 1e-12)):
        preds, gt, mask = synth.loss_train_inputs(**c, dtype=dt)
        for name, (weights, _) in WEIGHTS.items():
            leaves = [p.clone().requires_grad_(True) for p in preds]
            loss = getattr(L, name)(leaves, gt, mask)
            loss.backward()
            ref = float(gold[f"{name}_loss_{tag}"])
            assert abs(float(loss.detach()) - ref) <= tol * abs(ref), (name, tag, float(loss.detach()), ref)
            grads = gold[f"{name}_grad_{tag}"]
            assert grads.shape == (len(weights), c["b"], c["h"], c["w"]) and grads.dtype == np.dtype(tag.replace("f", "float"))
            for i in range(len(weights)):
                want = torch.from_numpy(grads[i])
                err = float((leaves[i].grad - want).double().norm() / want.double().norm())
                assert err <= tol, (name, tag, i, err)
            assert all(p.grad is None for p in leaves[len(weights):])
    assert (GOLDEN / "loss_train.npz").stat().st_size < 512 * 1024


def test_seeded_inputs_exercise_every_branch():
    preds, gt, mask = synth.loss_train_inputs(**synth.LOSS_TRAIN_CASE)
    assert bool(mask.any()) and bool((~mask).any())
    assert bool((gt[~mask] == 0).any()) and bool((gt[~mask] > 192).any())
    exact = 0
    for p in preds:
        a = (p - gt)[mask].abs()
        assert bool((a < 1).any()) and bool((a > 1).any())
        for thr in (1.0, 3.0, 5.0):
            assert float((a - thr).abs().min()) > 1e-4, thr
        exact += int((a == 0).sum())
    assert exact >= 1
    sp, init, sgt, valid = synth.igev_sequence_loss_inputs(synth.IGEV_TRAIN_STEP_CASE["seed"])
    sel = ((valid >= 0.5) & (sgt[:, 0] < 192)).unsqueeze(1)
    for p in (*sp, init):
        a = (p - sgt)[sel].abs()
        for thr in (1.0, 3.0, 5.0):
            assert float((a - thr).abs().min()) > 1e-4, thr


def test_entries_are_rows_of_the_third_table_only():
    header = (ROOT / "include" / "diffuvolume_hip_volume_train.h").read_text()
    source = (ROOT / "diffuvolume_amd" / "csrc" / "masked_loss.hip").read_text()
    here = Path(__file__).resolve().parent
    for name in ENTRIES:
        assert name in _lib.VOLUME_TRAIN_SIGNATURES and name not in _lib.SIGNATURES and name not in _lib.TRAIN_SIGNATURES
        assert name not in (ROOT / "include" / "diffuvolume_hip.h").read_text()
        assert re.search(rf"\b{name}\(", header) and re.search(rf'extern "C" \w+ {name}\(', source), name
    assert _lib.VOLUME_TRAIN_SIGNATURES[ENTRIES[0]][2] == _lib.SIZE_ONLY
    for name in ENTRIES[1:]:
        why = _lib.VOLUME_TRAIN_SIGNATURES[name][2]
        assert why == _lib.held_by("test_gpu_loss_train.py::test_masked_loss_abi_offset_views_bounds_and_refusals")
        text = (here / "test_gpu_loss_train.py").read_text()
        assert "def test_masked_loss_abi_offset_views_bounds_and_refusals(" in text and name in text
    assert f"#define DV_MASKED_LOSS_MAX_K {train_loss.MAX_K}" in header
    assert f"#define DV_MASKED_LOSS_MAX_BLOCKS {train_loss.MAX_BLOCKS}" in header
    assert "atomic" not in re.sub(r"//[^\n]*", "", source) and "getenv" not in source
