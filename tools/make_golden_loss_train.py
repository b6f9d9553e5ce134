"""Golden vectors for the masked training losses (tests/golden/loss_train.npz), from the imported reference's own functions:
SceneFlow/models/loss.py (model_loss_train, model_loss_train_freeze_attn, model_loss_train_attn_only, model_loss_test) and
KITTI12/models/loss.py (model_loss), each on ``synth.loss_train_inputs(**synth.LOSS_TRAIN_CASE)`` in float32 and in float64,
with backward().

Stored (seeds and results, no weights):
  seed, shape [B,H,W], k, names
  {name}_loss_f32 / _f64          the loss
  {name}_grad_f32 / _f64          the gradients of the predictions the function reads, stacked [K_name, B, H, W]
``sequence_loss`` has its record already: seq_loss_* / seq_metrics_* of igev_train_step.npz.

The seeded inputs are checked first: selected and unselected pixels, |d| on both sides of 1 for every prediction, an exact
d == 0 at a selected pixel, and no |d| within 1e-4 of 1, 3 or 5 (no count and no branch hangs on a rounding).  A second run
writes identical arrays.

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loss_train.py"""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import LOSS_TRAIN_CASE, loss_train_inputs  # noqa: E402
from oracle.make_golden import REF, _load_file  # noqa: E402

OUT = REPO / "tests" / "golden" / "loss_train.npz"
# name in the fixture (the package's name) -> (reference module, its function)
FUNCTIONS = {"model_loss_train": ("sf", "model_loss_train"),
             "model_loss_train_freeze_attn": ("sf", "model_loss_train_freeze_attn"),
             "model_loss_train_attn_only": ("sf", "model_loss_train_attn_only"),
             "model_loss_test": ("sf", "model_loss_test"),
             "model_loss_kitti12": ("k12", "model_loss")}


def check_inputs(preds, gt, mask):
    assert bool(mask.any()) and bool((~mask).any())
    exact = 0
    for p in preds:
        a = (p - gt)[mask].abs()
        assert bool((a < 1).any()) and bool((a > 1).any())
        for thr in (1.0, 3.0, 5.0):
            assert float((a - thr).abs().min()) > 1e-4, thr
        exact += int((a == 0).sum())
    assert exact >= 1


def run(fn, dtype):
    preds, gt, mask = loss_train_inputs(**LOSS_TRAIN_CASE, dtype=dtype)
    check_inputs(preds, gt, mask)
    preds = [p.requires_grad_(True) for p in preds]
    loss = fn(preds, gt, mask)
    assert loss.dtype == dtype
    loss.backward()
    return loss.detach(), torch.stack([p.grad for p in preds if p.grad is not None])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    mods = {"sf": _load_file(REF / "SceneFlow/models/loss.py", "ref_sf_loss"),
            "k12": _load_file(REF / "KITTI12/models/loss.py", "ref_k12_loss")}
    c = LOSS_TRAIN_CASE
    arrays = dict(seed=c["seed"], shape=np.array([c["b"], c["h"], c["w"]]), k=c["k"], names=np.array(list(FUNCTIONS)))
    for name, (mod, attr) in FUNCTIONS.items():
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            loss, grads = run(getattr(mods[mod], attr), dt)
            arrays[f"{name}_loss_{tag}"] = loss.numpy()
            arrays[f"{name}_grad_{tag}"] = grads.numpy()
        print(f"{name}: loss {float(arrays[f'{name}_loss_f64']):.9f}, {arrays[f'{name}_grad_f64'].shape[0]} gradients")
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
