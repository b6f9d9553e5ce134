"""Golden vectors for one TRAINING step of IGEV's once-per-pair cost-volume front (tests/golden/igev_volume_train.npz),
from the imported reference modules (KITTI15/core/igev_stereo_ddim.py `hourglass` :24-91; core/submodule.py BasicConv /
FeatureAtt / build_gwc_volume / disparity_regression) wired as IGEVStereo_ddim.forward :377-386 does, under the
reference's attribute names (the full class needs timm's pretrained backbone).

The reference modules get the synthetic weights ``synth_state_dict(template, seed=91, logit_gain=1.0)``, are put in
train mode and run, in float32 and in float64, forward + ``synth.igev_volume_train_loss`` + backward on the seeded inputs
of ``synth.igev_volume_train_inputs``.  Two cases (``synth.IGEV_VOLUME_TRAIN_CASES``):
  even   B 2, 16 x 32, max_disp 64  (D 16)   every level a whole tile multiple
  tall   B 2,  8 x 24, max_disp 192 (D 48)   full disparity depth; widths 24 -> 12 -> 6 -> 3: the deepest transposed layer
                                             sees 1 x 3 planes and odd W

Stored per case (prefix ``<case>_``; seeds, never weights), float32 and float64:
  loss, geo / init (the outputs at sampled positions geo_idx / init_idx)
  grad_norm, grad_val    per parameter with a gradient (order in grad_names) the L2 norm and SAMPLES entries (grad_idx)
  none_names             the parameters the step leaves without a gradient (cost_agg.conv1_up.bn.*: built, never called)
  leaf_norm, leaf_val    the same for the six leaves (synth.IGEV_VOLUME_LEAVES, positions leaf_idx)
  bn                     every BatchNorm running_mean / running_var after the step, concatenated in bn_names order
  ref_err                the reference float32's relative L2 error against float64 per full tensor:
                         [weights, biases, leaves, outputs] = the worst of that kind (outputs: loss, geo, init_disp, bn)
The file is written only if every reference float32 gradient is within GATE = 1e-4 relative L2 of its float64 one.
(``logit_gain=60``, the eval fixture's setting, fails that gate at 2e-4: the sharp softmax amplifies float32 rounding.)

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_igev_volume_train.py"""
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import (IGEV_VOLUME_TRAIN_CASES, IGEV_VOLUME_TRAIN_WEIGHT_SEED, _gen,  # noqa: E402
                                   igev_volume_train_inputs, igev_volume_train_leaves, igev_volume_train_loss,
                                   synth_state_dict)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "igev_volume_train.npz"
SAMPLES, PIX = 32, 256
GATE = 1e-4


def import_reference():
    """The timm and opt_einsum stubs of oracle/make_golden_igev_volume.py."""
    warnings.filterwarnings("ignore")
    sys.modules.setdefault("timm", types.ModuleType("timm"))
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    import core.igev_stereo_ddim as R
    from core.submodule import BasicConv, FeatureAtt, build_gwc_volume, disparity_regression

    class VolumeSide(nn.Module):
        """igev_stereo_ddim.py:196-199 and the part of forward that uses them (:377-386)."""

        def __init__(self):
            super().__init__()
            self.corr_stem = BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1)
            self.corr_feature_att = FeatureAtt(8, 96)
            self.cost_agg = R.hourglass(8)
            self.classifier = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

        def forward(self, match_left, match_right, features_left, max_disp):
            gwc_volume = build_gwc_volume(match_left, match_right, max_disp // 4, 8)
            gwc_volume = self.corr_stem(gwc_volume)
            gwc_volume = self.corr_feature_att(gwc_volume, features_left[0])
            geo_encoding_volume = self.cost_agg(gwc_volume, features_left)
            prob = F.softmax(self.classifier(geo_encoding_volume).squeeze(1), dim=1)
            return geo_encoding_volume, disparity_regression(prob, max_disp // 4)

    return VolumeSide


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(IGEV_VOLUME_TRAIN_WEIGHT_SEED, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def bn_names(model):
    return [k for k in model.state_dict() if k.endswith("running_mean") or k.endswith("running_var")]


def run(Model, sd, case, dtype):
    model = Model()
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    x = igev_volume_train_inputs(dtype=dtype, **case)
    geo, init = model(x["match_left"], x["match_right"], x["features"], case["max_disp"])
    loss = igev_volume_train_loss(geo, init, x)
    loss.backward()
    return model, loss, geo, init, igev_volume_train_leaves(x)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Model = import_reference()
    from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume
    sd = synth_state_dict(IGEVCostVolume(64).state_dict(), seed=IGEV_VOLUME_TRAIN_WEIGHT_SEED, logit_gain=1.0)
    arrays = dict(weight_seed=IGEV_VOLUME_TRAIN_WEIGHT_SEED, logit_gain=1.0, gate=GATE,
                  cases=np.array(list(IGEV_VOLUME_TRAIN_CASES)))
    for cname, case in IGEV_VOLUME_TRAIN_CASES.items():
        m32, l32, g32, i32, f32 = run(Model, sd, case, torch.float32)
        m64, l64, g64, i64, f64 = run(Model, sd, case, torch.float64)
        p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
        names = [n for n in p32 if p32[n].grad is not None]
        none_names = [n for n in p32 if p32[n].grad is None]
        assert none_names == [n for n in p64 if p64[n].grad is None]
        assert all(n.startswith("cost_agg.conv1_up.bn.") for n in none_names), none_names
        err = {"weights": 0.0, "biases": 0.0, "leaves": 0.0, "outputs": 0.0}
        for n in names:
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
        bnn = bn_names(m32)
        s32, s64 = m32.state_dict(), m64.state_dict()
        for a, b in [(l32, l64), (g32, g64), (i32, i64)] + [(s32[k], s64[k]) for k in bnn]:
            err["outputs"] = max(err["outputs"], rel(a.detach(), b.detach()))
        print(f"{cname}: gate ok, reference fp32 against fp64, worst per kind: " +
              ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        pre = cname + "_"
        grad_idx = np.stack([sample_index(f"{cname}:g:{n}", p32[n].numel(), SAMPLES) for n in names])
        leaf_names = list(f32)
        leaf_idx = np.stack([sample_index(f"{cname}:l:{n}", f32[n].numel(), SAMPLES) for n in leaf_names])
        geo_idx = sample_index(f"{cname}:geo", g32.numel(), PIX)
        init_idx = sample_index(f"{cname}:init", i32.numel(), PIX)
        arrays.update({pre + "seed": case["seed"],
                       pre + "shape": np.array([case["b"], case["h"], case["w"], case["max_disp"]]),
                       pre + "geo_shape": np.array(g32.shape), pre + "init_shape": np.array(i32.shape),
                       pre + "grad_names": np.array(names), pre + "none_names": np.array(none_names),
                       pre + "grad_idx": grad_idx, pre + "leaf_names": np.array(leaf_names), pre + "leaf_idx": leaf_idx,
                       pre + "geo_idx": geo_idx, pre + "init_idx": init_idx, pre + "bn_names": np.array(bnn),
                       pre + "ref_err": np.array([err[k] for k in ("weights", "biases", "leaves", "outputs")])})
        for tag, (params, leaves, loss, geo, init, sdict) in (("f32", (p32, f32, l32, g32, i32, s32)),
                                                             ("f64", (p64, f64, l64, g64, i64, s64))):
            arrays[f"{pre}loss_{tag}"] = loss.detach().numpy()
            arrays[f"{pre}geo_{tag}"] = geo.detach().reshape(-1)[torch.from_numpy(geo_idx)].numpy()
            arrays[f"{pre}init_{tag}"] = init.detach().reshape(-1)[torch.from_numpy(init_idx)].numpy()
            arrays[f"{pre}grad_norm_{tag}"] = np.array([float(params[n].grad.double().norm()) for n in names])
            arrays[f"{pre}grad_val_{tag}"] = np.stack([params[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(names, grad_idx)])
            arrays[f"{pre}leaf_norm_{tag}"] = np.array([float(leaves[n].grad.double().norm()) for n in leaf_names])
            arrays[f"{pre}leaf_val_{tag}"] = np.stack([leaves[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(leaf_names, leaf_idx)])
            arrays[f"{pre}bn_{tag}"] = torch.cat([sdict[k].reshape(-1) for k in bnn]).numpy()
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
