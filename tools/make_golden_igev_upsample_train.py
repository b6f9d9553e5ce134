"""Golden vectors for one TRAINING step of IGEV's convex-upsampling head (tests/golden/igev_upsample_train.npz), from the
imported reference modules (KITTI15/core/submodule.py Conv2x / Conv2x_IN / BasicConv_IN / context_upsample) built under
the reference's attribute names (KITTI15/core/igev_stereo_ddim.py:104-112) and wired as its forward does: `upsample_disp`
:203-211 once per GRU iteration (:456-457), the spx_4 / spx_2 / spx logits :390-393 and the upsampled initial disparity
:462.  (The full class needs timm's pretrained backbone.)

The reference modules get the synthetic weights ``synth.igev_upsample_state_dict(template, seed=93, logit_gain)``, are put
in train mode and run, in float32 and in float64, ``synth.igev_upsample_train_step`` (forward over T iterations + a loss
shaped like sequence_loss at full resolution) + backward on the seeded inputs of ``synth.igev_upsample_train_inputs``.
Two cases (``synth.IGEV_UPSAMPLE_TRAIN_CASES``):
  even   B 2, 8 x 16, T 3
  odd    B 1, 5 x 7,  T 2   odd planes: every cell row and column meets a border within two cells

Stored per case (prefix ``<case>_``; seeds, never weights), float32 and float64:
  loss, init / up<i> (the outputs at sampled positions init_idx / up_idx)
  grad_norm, grad_val    per parameter (order in grad_names) the L2 norm and SAMPLES entries (grad_idx)
  leaf_norm, leaf_val    the same for the leaves (synth.igev_upsample_train_leaves, positions leaf_idx)
  bn                     every BatchNorm running_mean / running_var after the T calls, concatenated in bn_names order
  ref_err                the reference float32's relative L2 error against float64 per full tensor:
                         [weights, biases, leaves, outputs] = the worst of that kind (outputs: loss, init, up<i>, bn)
The file is written only if every reference float32 gradient is within GATE = 1e-4 relative L2 of its float64 one;
``logit_gain`` (stored) scales the two 9-logit heads and is lowered from 1 only if the 9-way softmax fails that gate.

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_igev_upsample_train.py"""
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
from diffuvolume_amd.synth import (IGEV_UPSAMPLE_TRAIN_CASES, IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED, _gen,  # noqa: E402
                                   igev_upsample_state_dict, igev_upsample_train_inputs, igev_upsample_train_leaves,
                                   igev_upsample_train_step)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "igev_upsample_train.npz"
SAMPLES, PIX = 32, 256
GATE = 1e-4
LOGIT_GAIN = 1.0
KINDS = ("weights", "biases", "leaves", "outputs")


def import_reference():
    """The timm and opt_einsum stubs of oracle/make_golden_igev_volume.py."""
    warnings.filterwarnings("ignore")
    sys.modules.setdefault("timm", types.ModuleType("timm"))
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    from core.submodule import BasicConv_IN, Conv2x, Conv2x_IN, context_upsample

    class UpsampleSide(nn.Module):
        """igev_stereo_ddim.py:104-112 and the parts of forward that use them (:203-211, :390-393, :462)."""

        def __init__(self):
            super().__init__()
            self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
            self.spx_2 = Conv2x_IN(24, 32, True)
            self.spx_4 = nn.Sequential(BasicConv_IN(96, 24, kernel_size=3, stride=1, padding=1),
                                       nn.Conv2d(24, 24, 3, 1, 1, bias=False), nn.InstanceNorm2d(24), nn.ReLU())
            self.spx_2_gru = Conv2x(32, 32, True)
            self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))

        def forward(self, disp, mask_feat_4, stem_2x):
            xspx = self.spx_2_gru(mask_feat_4, stem_2x)
            spx_pred = self.spx_gru(xspx)
            spx_pred = F.softmax(spx_pred, 1)
            return context_upsample(disp * 4., spx_pred).unsqueeze(1)

        def init_forward(self, features_left0, stem_2x, init_disp):
            xspx = self.spx_4(features_left0)
            xspx = self.spx_2(xspx, stem_2x)
            spx_pred = self.spx(xspx)
            spx_pred = F.softmax(spx_pred, 1)
            return context_upsample(init_disp * 4., spx_pred).unsqueeze(1)      # (:462's .float() undoes autocast only)

    return UpsampleSide


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def bn_names(model):
    return [k for k in model.state_dict() if k.endswith("running_mean") or k.endswith("running_var")]


def run(Model, sd, case, dtype):
    model = Model()
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    x = igev_upsample_train_inputs(dtype=dtype, **case)
    loss, init_up, ups = igev_upsample_train_step(model, x)
    loss.backward()
    return model, loss, init_up, ups, igev_upsample_train_leaves(x)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Model = import_reference()
    from diffuvolume_amd.igev_stereo_ddim import IGEVUpsampler
    sd = igev_upsample_state_dict(IGEVUpsampler().state_dict(), IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED, LOGIT_GAIN)
    arrays = dict(weight_seed=IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED, logit_gain=LOGIT_GAIN, gate=GATE,
                  cases=np.array(list(IGEV_UPSAMPLE_TRAIN_CASES)))
    for cname, case in IGEV_UPSAMPLE_TRAIN_CASES.items():
        m32, l32, i32, u32, f32 = run(Model, sd, case, torch.float32)
        m64, l64, i64, u64, f64 = run(Model, sd, case, torch.float64)
        p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
        names = list(p32)
        assert all(p32[n].grad is not None and p64[n].grad is not None for n in names)
        err = dict.fromkeys(KINDS, 0.0)
        for n in names:
            r = rel(p32[n].grad, p64[n].grad)
            kind = "biases" if n.endswith("bias") else "weights"
            err[kind] = max(err[kind], r)
            if r > GATE:
                raise SystemExit(f"{cname}: {n}: fp32 gradient {r:.2e} from fp64 (> {GATE}): lower LOGIT_GAIN")
        for n in f32:
            r = rel(f32[n].grad, f64[n].grad)
            err["leaves"] = max(err["leaves"], r)
            if r > GATE:
                raise SystemExit(f"{cname}: leaf {n}: fp32 gradient {r:.2e} from fp64 (> {GATE}): lower LOGIT_GAIN")
        bnn = bn_names(m32)
        s32, s64 = m32.state_dict(), m64.state_dict()
        for a, b in [(l32, l64), (i32, i64)] + list(zip(u32, u64)) + [(s32[k], s64[k]) for k in bnn]:
            err["outputs"] = max(err["outputs"], rel(a.detach(), b.detach()))
        print(f"{cname}: gate ok, reference fp32 against fp64, worst per kind: " +
              ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        pre = cname + "_"
        grad_idx = np.stack([sample_index(f"{cname}:g:{n}", p32[n].numel(), SAMPLES) for n in names])
        leaf_names = list(f32)
        leaf_idx = np.stack([sample_index(f"{cname}:l:{n}", f32[n].numel(), SAMPLES) for n in leaf_names])
        up_idx = sample_index(f"{cname}:up", i32.numel(), PIX)
        arrays.update({pre + "seed": case["seed"],
                       pre + "shape": np.array([case["b"], case["h"], case["w"], case["iters"]]),
                       pre + "up_shape": np.array(i32.shape), pre + "grad_names": np.array(names),
                       pre + "grad_idx": grad_idx, pre + "leaf_names": np.array(leaf_names), pre + "leaf_idx": leaf_idx,
                       pre + "up_idx": up_idx, pre + "bn_names": np.array(bnn),
                       pre + "ref_err": np.array([err[k] for k in KINDS])})
        for tag, (params, leaves, loss, init, ups, sdict) in (("f32", (p32, f32, l32, i32, u32, s32)),
                                                             ("f64", (p64, f64, l64, i64, u64, s64))):
            idx = torch.from_numpy(up_idx)
            arrays[f"{pre}loss_{tag}"] = loss.detach().numpy()
            arrays[f"{pre}init_{tag}"] = init.detach().reshape(-1)[idx].numpy()
            arrays[f"{pre}up_{tag}"] = np.stack([u.detach().reshape(-1)[idx].numpy() for u in ups])
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
