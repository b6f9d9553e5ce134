"""Golden vectors for an unrolled TRAINING loop of IGEV's recurrent update block (tests/golden/update_train_loop.npz),
from the imported reference ``BasicMultiUpdateBlock`` (KITTI15/core/update.py:104-142; args corr_levels 2, corr_radius 4,
n_gru_layers 3, n_downsample 2, hidden 128 x 3).

The reference block gets the synthetic weights ``synth_state_dict(WEIGHT_SEED)`` and runs, in float32 and in float64,
the loop of ``synth.update_train_loop`` (the reference's own, igev_stereo_ddim.py:441-457, with a loss shaped like
sequence_loss at 1/4 resolution) on the seeded inputs of ``synth.update_train_inputs``.  Two cases:
  even     B 2, 16 x 32, T = 6
  ragged   B 2, 20 x 28, T = 4   (10 x 14 and 5 x 7 below it: pool2x, interp and every tile edge off the grid)

Stored per case (prefix ``<case>_``; seeds, never weights), float32 and float64:
  disp{i} / mask{i}      the disparity and mask features of iteration i at sampled positions (pix_idx / mask_idx)
  loss
  grad_norm, grad_val    per parameter (order in grad_names) the gradient's L2 norm and SAMPLES entries (grad_idx)
  leaf_norm, leaf_val    the same for the net / inp leaves (order in leaf_names, positions in leaf_idx)
  ref_err                the reference float32's relative L2 error against float64 per full tensor:
                         rows [weights, biases, leaves, outputs] = the worst of that kind
The file is written only if the reference's float32 gradients are within GATE = 1e-4 relative L2 of its float64 ones
for every parameter and leaf (otherwise choose another seed).  The loops are short on purpose: with random weights the
disparity moves tens of pixels per iteration and a ReLU or |.| that flips between float32 and float64 moves a gradient
visibly (20 x 28 with T = 6 was measured at 2e-3).

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_update_train.py"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import (UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, _gen, synth_state_dict,  # noqa: E402
                                   update_train_inputs, update_train_loop)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "update_train_loop.npz"
WEIGHT_SEED = 7
CASES = {"even": dict(seed=31, b=2, h=16, w=32, iters=6), "ragged": dict(seed=32, b=2, h=20, w=28, iters=4)}
SAMPLES, PIX = 32, 256
GATE = 1e-4


def import_reference():
    """KITTI15/core/update.py needs only an opt_einsum stub (oracle/make_golden_igev.py)."""
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    from core.update import BasicMultiUpdateBlock
    return BasicMultiUpdateBlock


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(WEIGHT_SEED, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def run(Block, sd, case, dtype):
    block = Block(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=list(UPDATE_TRAIN_HIDDEN))
    block.load_state_dict(sd, strict=True)
    block = block.to(dtype).train()
    x = update_train_inputs(dtype=dtype, **case)
    loss, disps, masks, _ = update_train_loop(block, x)
    loss.backward()
    leaves = {f"net{i}": t for i, t in enumerate(x["net"])}
    leaves.update({f"inp{i}{j}": t for i, lv in enumerate(x["inp"]) for j, t in enumerate(lv)})
    return block, loss, disps, masks, leaves


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Block = import_reference()
    from diffuvolume_amd.update import BasicMultiUpdateBlock as Ours
    template = Ours(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN).state_dict()
    sd = synth_state_dict(template, seed=WEIGHT_SEED)
    arrays = dict(weight_seed=WEIGHT_SEED, gate=GATE, cases=np.array(list(CASES)))
    for cname, case in CASES.items():
        m32, l32, d32, k32, f32 = run(Block, sd, case, torch.float32)
        m64, l64, d64, k64, f64 = run(Block, sd, case, torch.float64)
        p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
        names = list(p32)
        err = {"weights": 0.0, "biases": 0.0, "leaves": 0.0, "outputs": 0.0}
        for n in names:
            assert p32[n].grad is not None, n
            r = rel(p32[n].grad, p64[n].grad)
            kind = "biases" if n.endswith("bias") else "weights"
            err[kind] = max(err[kind], r)
            if r > GATE:
                raise SystemExit(f"{cname}: {n}: fp32 gradient {r:.2e} from fp64 (> {GATE}): choose another seed")
        for n in f32:
            r = rel(f32[n].grad, f64[n].grad)
            err["leaves"] = max(err["leaves"], r)
            if r > GATE:
                raise SystemExit(f"{cname}: leaf {n}: fp32 gradient {r:.2e} from fp64 (> {GATE}): choose another seed")
        for a, b in zip(d32 + k32 + [l32], d64 + k64 + [l64]):
            err["outputs"] = max(err["outputs"], rel(a.detach(), b.detach()))
        print(f"{cname}: gate ok, reference fp32 against fp64, worst per kind: " +
              ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        pre = cname + "_"
        grad_idx = np.stack([sample_index(f"{cname}:g:{n}", p32[n].numel(), SAMPLES) for n in names])
        leaf_names = list(f32)
        leaf_idx = np.stack([sample_index(f"{cname}:l:{n}", f32[n].numel(), SAMPLES) for n in leaf_names])
        pix = sample_index(f"{cname}:pix", d32[0].numel(), PIX)
        mpix = sample_index(f"{cname}:mask", k32[0].numel(), PIX)
        arrays.update({pre + "seed": case["seed"], pre + "shape": np.array([case["b"], case["h"], case["w"], case["iters"]]),
                       pre + "grad_names": np.array(names), pre + "grad_idx": grad_idx, pre + "leaf_names": np.array(leaf_names),
                       pre + "leaf_idx": leaf_idx, pre + "pix_idx": pix, pre + "mask_idx": mpix,
                       pre + "ref_err": np.array([err[k] for k in ("weights", "biases", "leaves", "outputs")])})
        for tag, (params, leaves, loss, disps, masks) in (("f32", (p32, f32, l32, d32, k32)), ("f64", (p64, f64, l64, d64, k64))):
            arrays[f"{pre}loss_{tag}"] = loss.detach().numpy()
            arrays[f"{pre}grad_norm_{tag}"] = np.array([float(params[n].grad.double().norm()) for n in names])
            arrays[f"{pre}grad_val_{tag}"] = np.stack([params[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(names, grad_idx)])
            arrays[f"{pre}leaf_norm_{tag}"] = np.array([float(leaves[n].grad.double().norm()) for n in leaf_names])
            arrays[f"{pre}leaf_val_{tag}"] = np.stack([leaves[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(leaf_names, leaf_idx)])
            for i, (d, k) in enumerate(zip(disps, masks)):
                arrays[f"{pre}disp{i}_{tag}"] = d.detach().reshape(-1)[torch.from_numpy(pix)].numpy()
                arrays[f"{pre}mask{i}_{tag}"] = k.detach().reshape(-1)[torch.from_numpy(mpix)].numpy()
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
