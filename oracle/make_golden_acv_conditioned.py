"""Golden vectors for the CONDITIONED SceneFlow network (oracle/calibrate.py): the synthetic ACVNet_DDIM weights (seed 1,
classifier gain 1) with the BatchNorm buffers of the DDIM-loop layers set to the statistics of the fixture's own input
(pooled over the five steps of the oracle's own trajectory,
oracle/calibrate.py: pooled_loop_statistics).  On this network two correct fp32 evaluations agree within the contract's
bar on every pixel, so tests/test_gpu_acv_conditioned.py asserts the RAW bar -- |d disp| <= 1e-3 px on 99.9 % of the
pixels, |d EPE| < 1e-4 -- against the reference's own outputs.

  acv_conditioned_16x32.npz      B = 1, quarter-resolution volume 16 x 32: the F(2x2x2,3x3x3) kernel on the 64- and
                                 128-channel layers of both hourglasses with tile shape 0 (16 x 4)
  acv_conditioned_24x32_b2.npz   B = 2, volume 24 x 32: the 128-channel layers at 6 x 8 take tile shape 1 (8 x 8) and
                                 the bottleneck [12, 6, 8] is padded in H only (the reference's mask quirk,
                                 SceneFlow/models/submodule.py:414-416)

Each holds the BN statistics (never the weights), the seeds of the input (synth_hot_inputs) and of the noise tape, x_T,
`used`, and the outputs of the IMPORTED REFERENCE (SceneFlow/models/acv_ddim.py): model_predictions at t = 999
(:254-296) and the per-step stack and ensemble of ddim_sample (:299-370) under a NoiseTape.  A fixture is written only
if the network is well conditioned on it (float64 gate: the reference's step-1 disparity and every step of the fp32
oracle's trajectory within 1e-3 px of the float64 oracle on every pixel, no renewal decision flipped).

  layer_attention_padh.npz       the reference's attention_block with only H padded, B = 2, two depth windows

Build container only:  PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_acv_conditioned.py"""
import os
import sys
import warnings
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import NoiseTape, synth_state_dict  # noqa: E402
from oracle import acv_oracle as O  # noqa: E402
from oracle import calibrate as C  # noqa: E402
from oracle.make_golden import REF, rnd, save  # noqa: E402
from oracle.make_golden_acv_calibrated import GAIN, LOOP_PREFIXES  # noqa: E402

warnings.filterwarnings("ignore")
BAR_PX = 1e-3
# name: (batch, h, w, input seed, tape seed)
FIXTURES = {"acv_conditioned_16x32": (1, 16, 32, 110, 81), "acv_conditioned_24x32_b2": (2, 24, 32, 111, 82)}


def import_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self                  # hard-coded .cuda() in the reference
    sys.path.insert(0, str(REF / "SceneFlow"))
    cwd = os.getcwd()
    os.chdir(REF / "SceneFlow")
    from models import __models__ as REF_MODELS
    from models.submodule import attention_block
    os.chdir(cwd)
    return REF_MODELS, attention_block


@torch.no_grad()
def reference_sample(ref, vol, used, x_T, tape_seed):
    """ref.ddim_sample(vol, used, x_T) with its draws from NoiseTape(tape_seed), as oracle/make_golden.py feeds them:
    the odd torch.randn_like calls are the update's eps (:354), the even ones q_sample's noise (:359, only the shape
    of its output is used), torch.rand_like is the renewal fill (:360)."""
    tape, calls = NoiseTape(tape_seed), {"n": 0}
    real_randn_like, real_rand_like = torch.randn_like, torch.rand_like

    def fake_randn_like(x, *a, **k):
        calls["n"] += 1
        return tape("eps", tuple(x.shape), x.dtype) if calls["n"] % 2 == 1 else torch.zeros_like(x)

    torch.randn_like = fake_randn_like
    torch.rand_like = lambda x, *a, **k: tape("fill", tuple(x.shape), x.dtype)
    try:
        return ref.ddim_sample(vol, used, x_T)
    finally:
        torch.randn_like, torch.rand_like = real_randn_like, real_rand_like


def fixture(name, REF_MODELS):
    from diffuvolume_amd.acv_ddim import ACVNet_DDIM
    b, h, w, seed, tape_seed = FIXTURES[name]
    sd = synth_state_dict(ACVNet_DDIM(192, False, False).state_dict(), seed=C.ACV_WEIGHT_SEED, logit_gain=GAIN)
    x = C.conditioned_acv_inputs(b, h, w, seed)
    vol, used = x["vol"], x["used"]
    x_T = O.ACVDiffusionOracle(sd).encode_x_T(x["dq"])
    t = torch.full((b,), 999, dtype=torch.long)
    stats = C.pooled_loop_statistics(sd, vol, used, x_T, tape_seed, LOOP_PREFIXES)
    sd.update(stats)
    keys, vals, lens = C.pack(stats)
    ref = REF_MODELS["acvnet_ddim"](192, False, False).eval()
    ref.load_state_dict(sd, strict=True)
    with torch.no_grad():
        pn, xs, disp, pv = ref.model_predictions(vol, x_T, t)
        kk = torch.arange(0, 192, dtype=disp.dtype).view(1, -1, 1, 1)
        unc = torch.sum(torch.abs(disp.unsqueeze(1) - kk) * pv, dim=1)
    final, stack = reference_sample(ref, vol, used, x_T, tape_seed)
    # conditioning gate: the float64 oracle
    gate = C.acv_float64_gate(sd, vol, used, x_T, tape_seed)
    e_ref = float((disp.double() - gate["disp64"]).abs().max())
    keep = ((disp - used).abs() < 1) & (unc < 3)
    print(f"  {name}: disp {float(disp.min()):.1f}..{float(disp.max()):.1f} px, unc mean {float(unc.mean()):.1f} px, "
          f"renewed at step 1 {float(keep.float().mean()):.1%}")
    print(f"    gate: reference step 1 vs float64 max {e_ref:.2e} px; fp32 oracle vs float64 per step max "
          f"{[f'{m:.2e}' for m in gate['max_px']]} px, final {gate['final_max_px']:.2e} px; renewal flips {gate['flips']}")
    if not (e_ref <= BAR_PX and max(gate["max_px"]) <= BAR_PX and gate["flips"] == 0):
        raise SystemExit(f"{name}: the network is not well conditioned on this input; nothing written")
    save(name, batch=b, h=h, w=w, seed=seed, tape_seed=tape_seed, gain=GAIN, bn_keys=keys, bn_vals=vals, bn_lens=lens,
         x_T=x_T, t=t, used=used, pred_noise=pn, x_start=xs, disp=disp, unc=unc, final=final, stack=stack)


def attention_padh(attention_block):
    """The reference's attention_block with only H padded (6 -> 8; W = 8): under its mask quirk the padded tokens take
    part in the attention.  B = 2 and D = 8 (two depth windows).  Weights as in layer_attention_* of make_golden.py."""
    from diffuvolume_amd.acv_ddim import _WindowAttention
    at = attention_block(channels_3d=128, num_heads=16, block=(4, 4, 4)).eval()
    at.load_state_dict(synth_state_dict(_WindowAttention(128, 16).state_dict(), seed=23))
    x = rnd(23, "xatpadh", 2, 128, 8, 6, 8)
    with torch.no_grad():
        save("layer_attention_padh", x=x, y=at(x), seed=23)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    REF_MODELS, attention_block = import_reference()
    for name in FIXTURES:
        fixture(name, REF_MODELS)
    attention_padh(attention_block)
    print("done")


if __name__ == "__main__":
    main()
