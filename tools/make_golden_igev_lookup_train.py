"""Golden vectors for one TRAINING step of IGEV's geometry lookup (tests/golden/igev_lookup_train.npz), from the imported
reference class ``core.geometry_ddim.Combined_Geo_Encoding_Volume`` (KITTI15/core/geometry_ddim.py:6-80).

The reference class runs, in float32 and in float64, ``synth.igev_lookup_train_step`` (one volume, T lookups with their
own detached disparity and noise, loss sum_t mean(out_t * cot_t)) + backward on the seeded inputs of
``synth.igev_lookup_train_inputs``.  Two cases (``synth.IGEV_LOOKUP_TRAIN_CASES``):
  even   B 2, C 8, D 48, 8 x 24, T 3
  odd    B 1, C 8, D 48, 5 x 7,  T 2   odd planes and an odd W2: the last correlation entry has no pooled partner

Stored per case (prefix ``<case>_``; seeds, never tensors), float32 and float64:
  loss
  grad_norm, grad_val    per leaf (order of synth.IGEV_LOOKUP_LEAVES: fmap1, fmap2, geo) the L2 norm and SAMPLES entries
                         of its gradient (positions grad_idx)
  ref_err                the reference float32's relative L2 error against float64 over the full gradient, per kind
                         [df1, df2, dgeo]
The file is written only if every reference float32 gradient is within GATE = 1e-4 relative L2 of its float64 one.
(The reference ends its lookup with ``.float()``, :69, so the float64 run rounds the cotangent / numel to float32 once on
the way back: a relative 3e-8 per element, inside every ref_err below.)

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_igev_lookup_train.py"""
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import (IGEV_LOOKUP_LEAVES, IGEV_LOOKUP_TRAIN_CASES, _gen, igev_lookup_train_inputs,  # noqa: E402
                                   igev_lookup_train_leaves, igev_lookup_train_step)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "igev_lookup_train.npz"
SAMPLES = 512
GATE = 1e-4
KINDS = ("df1", "df2", "dgeo")          # the gradients of IGEV_LOOKUP_LEAVES, in that order


def import_reference():
    """The timm and opt_einsum stubs of oracle/make_golden_igev_volume.py."""
    warnings.filterwarnings("ignore")
    sys.modules.setdefault("timm", types.ModuleType("timm"))
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    from core.geometry_ddim import Combined_Geo_Encoding_Volume
    return Combined_Geo_Encoding_Volume


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(0, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def run(Volume, case, dtype):
    x = igev_lookup_train_inputs(dtype=dtype, **case)
    loss, _ = igev_lookup_train_step(Volume, x)
    loss.backward()
    return loss.detach(), {n: t.grad for n, t in igev_lookup_train_leaves(x).items()}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Volume = import_reference()
    arrays = dict(gate=GATE, cases=np.array(list(IGEV_LOOKUP_TRAIN_CASES)), kinds=np.array(KINDS),
                  leaves=np.array(IGEV_LOOKUP_LEAVES))
    for cname, case in IGEV_LOOKUP_TRAIN_CASES.items():
        l32, g32 = run(Volume, case, torch.float32)
        l64, g64 = run(Volume, case, torch.float64)
        err = []
        for n in IGEV_LOOKUP_LEAVES:
            assert g32[n] is not None and g64[n] is not None and g64[n].dtype == torch.float64
            r = rel(g32[n], g64[n])
            if not r <= GATE:
                raise SystemExit(f"{cname}: {n}: fp32 gradient {r:.2e} from fp64 (> {GATE})")
            err.append(r)
        print(f"{cname}: gate ok, reference fp32 against fp64: " + ", ".join(f"{k} {v:.2e}" for k, v in zip(KINDS, err)))
        pre = cname + "_"
        idx = np.stack([sample_index(f"{cname}:{n}", g32[n].numel(), SAMPLES) for n in IGEV_LOOKUP_LEAVES])
        arrays.update({pre + "seed": case["seed"],
                       pre + "shape": np.array([case[k] for k in ("b", "c", "d", "h", "w", "iters")]),
                       pre + "grad_idx": idx, pre + "ref_err": np.array(err)})
        for tag, loss, grads in (("f32", l32, g32), ("f64", l64, g64)):
            arrays[f"{pre}loss_{tag}"] = loss.numpy()
            arrays[f"{pre}grad_norm_{tag}"] = np.array([float(grads[n].double().norm()) for n in IGEV_LOOKUP_LEAVES])
            arrays[f"{pre}grad_val_{tag}"] = np.stack([grads[n].reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(IGEV_LOOKUP_LEAVES, idx)])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
