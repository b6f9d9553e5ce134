"""Golden vectors for one TRAINING step of PWCNet_ddim (tests/golden/pcw_train_step.npz), from the imported reference
(KITTI12/models/pwcnet_ddim.py:604-735, KITTI12/models/loss.py:model_loss, KITTI12/main.py:140-170).

The reference network gets the synthetic weights ``synth_state_dict(seed)`` and runs in train mode, in float32 and in
float64, on B = 2 images of 64 x 128 (the 1/32 volume is 6 x 2 x 4, every stride-2 input of the 3-D stack has even
dims, and the full-resolution plane of refinenet3 is wide enough for its dilation-16 block) with a seeded ground truth
of which some pixels lie outside (0, 192).  ``disp_net`` is formed from that ground truth exactly as main.py:148-150
forms it.  The two random draws are fixed: ``torch.randint`` (the timestep, :660) returns T_STEP and
``torch.randn_like`` (q_sample's noise) is the 'q' draw of NoiseTape(TAPE).  Then model_loss and backward().

Stored (seeds, never weights):
  pred{i}_f32 / pred{i}_f64   the six predictions at PIX sampled pixels (positions in pix_idx), loss_f32 / loss_f64
  grad_norm_f32 / _f64        per parameter (order in grad_names) the gradient's L2 norm
  grad_val_f32 / _f64         per parameter SAMPLES entries at seeded flat positions (grad_idx), rows in grad_names order
  none_grad_names             parameters whose gradient is None after backward (time_embedding: `torch.tensor(noisy)`)
  bn_val_f32 / _f64, bn_idx   running_mean / running_var after the step, sampled the same way (rows in bn_names order)
The file is written only if the reference's float32 gradients are within GATE relative L2 of its float64 ones for every
parameter (otherwise choose another seed); a second run writes identical arrays.  GATE is 1e-2, the ACV fixture's gate
(tools/make_golden_acv_train.py): in train mode every BatchNorm normalises by its batch statistics and the gradients that
pass through the ~100 of them lose digits to cancellation.  The tests hold the HIP route to twice the reference float32's
own error, per kind of tensor, so the gate only keeps a badly conditioned seed out.

The float64 run sets float64 as the default dtype around the forward: the reference's warp() samples a mask of
``torch.ones`` (default dtype) on the disparity's grid, and grid_sample needs both in one dtype.  So the time MLP runs in
float64 there as well; its output is rounded to float32 by ``torch.tensor(noisy, dtype=torch.float32)`` and carries no
gradient.

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_pcw_train.py"""
import os
import sys
import warnings
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import NoiseTape, _gen, synth_state_dict, synth_stereo_batch  # noqa: E402
from oracle.make_golden import REF  # noqa: E402

warnings.filterwarnings("ignore")
OUT = REPO / "tests" / "golden" / "pcw_train_step.npz"
WEIGHT_SEED, INPUT_SEED, TAPE, T_STEP = 5, 140, 93, 611
B, H, W = 2, 64, 128
SAMPLES, PIX = 32, 1024
GATE = 1e-2


def inputs():
    """Images, a ground truth with invalid pixels, and disp_net formed from it as KITTI12/main.py:148-150 does."""
    x = synth_stereo_batch(B, H, W, seed=INPUT_SEED)
    gt = x["gt"].clone()
    bad = torch.rand(B, H, W, generator=_gen(INPUT_SEED, "train_gt_invalid"))
    gt[bad < 0.05] = 0.0                       # no ground truth
    gt[bad > 0.97] = 200.0                     # beyond maxdisp
    disp_net = torch.clamp(gt, 0, 192 - 1).unsqueeze(1)
    disp_net = F.interpolate(disp_net, size=(H // 4, W // 4), mode="bilinear") / 4
    return x["left"], x["right"], disp_net, gt


def sample_index(seed_key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(WEIGHT_SEED, seed_key)).numpy().astype(np.int64)


def import_reference():
    """The recipe of oracle/make_golden_pcw_conditioned.py: .cuda() and get_device() patched for the CPU."""
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.get_device = lambda self: self.device                 # KITTI12 warp() (submodule.py:146)
    sys.path.insert(0, str(REF / "KITTI12"))
    cwd = os.getcwd()
    os.chdir(REF / "KITTI12")
    from models import __models__ as REF_MODELS
    import models.loss as loss_mod
    os.chdir(cwd)
    return REF_MODELS, loss_mod


def run(REF_MODELS, loss_mod, sd, dtype):
    """One training step of the reference in ``dtype`` -> (model, predictions, loss)."""
    model = REF_MODELS["pwc_ddimgc"](192)
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()             # (the time MLP too: under the float64 default its sinusoid is float64)
    for name, buf in model.named_buffers():     # the schedule stays float64 (as in the float32 model)
        if name in sd and sd[name].dtype == torch.float64:
            buf.data = sd[name].clone()
    left, right, disp_net, gt = inputs()
    mask = (gt < 192) & (gt > 0)
    tape = NoiseTape(TAPE)
    real_randint, real_randn_like = torch.randint, torch.randn_like
    torch.randint = lambda low, high, size, *a, **k: torch.full(size, T_STEP, dtype=torch.long)
    torch.randn_like = lambda x, *a, **k: tape("q", tuple(x.shape), x.dtype)
    default = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        outs = model(left.to(dtype), right.to(dtype), None, disp_net.float(), None)
    finally:
        torch.randint, torch.randn_like = real_randint, real_randn_like
        torch.set_default_dtype(default)
    loss = loss_mod.model_loss(outs, gt.to(dtype), mask)
    loss.backward()
    return model, outs, loss


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    REF_MODELS, loss_mod = import_reference()
    from diffuvolume_amd.pwcnet_ddim import PWCNet_ddim
    sd = synth_state_dict(PWCNet_ddim(192).state_dict(), seed=WEIGHT_SEED)
    m32, outs32, loss32 = run(REF_MODELS, loss_mod, sd, torch.float32)
    m64, outs64, loss64 = run(REF_MODELS, loss_mod, sd, torch.float64)

    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
    names = [n for n in p32 if p32[n].grad is not None]
    none_names = [n for n in p32 if p32[n].grad is None]
    worst = 0.0
    for n in names:
        a, b = p32[n].grad.double(), p64[n].grad
        rel = float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())
        worst = max(worst, rel)
        if rel > GATE:
            raise SystemExit(f"{n}: fp32 gradient {rel:.2e} from fp64 (> {GATE}): choose another seed")
    print(f"gate ok: worst relative L2 gradient error of the reference fp32 {worst:.2e}")

    grad_idx = np.stack([sample_index("g:" + n, p32[n].numel(), SAMPLES) for n in names])
    arrays = dict(weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED, tape_seed=TAPE, t_step=T_STEP, shape=np.array([B, H, W]),
                  grad_names=np.array(names), none_grad_names=np.array(none_names), grad_idx=grad_idx,
                  loss_f32=loss32.detach().numpy(), loss_f64=loss64.detach().numpy())
    for tag, params in (("f32", p32), ("f64", p64)):
        arrays[f"grad_norm_{tag}"] = np.array([float(params[n].grad.double().norm()) for n in names])
        arrays[f"grad_val_{tag}"] = np.stack([params[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                              for n, i in zip(names, grad_idx)])
    pix = sample_index("pix", B * H * W, PIX)
    arrays["pix_idx"] = pix
    for i in range(6):
        arrays[f"pred{i}_f32"] = outs32[i].detach().reshape(-1)[torch.from_numpy(pix)].numpy()
        arrays[f"pred{i}_f64"] = outs64[i].detach().reshape(-1)[torch.from_numpy(pix)].numpy()
    b32, b64 = dict(m32.named_buffers()), dict(m64.named_buffers())
    bn = [n for n in b32 if n.endswith(("running_mean", "running_var"))]
    bn_idx = np.stack([sample_index("b:" + n, b32[n].numel(), SAMPLES) for n in bn])
    arrays.update(bn_names=np.array(bn), bn_idx=bn_idx,
                  bn_val_f32=np.stack([b32[n].reshape(-1)[torch.from_numpy(i)].numpy() for n, i in zip(bn, bn_idx)]),
                  bn_val_f64=np.stack([b64[n].reshape(-1)[torch.from_numpy(i)].numpy() for n, i in zip(bn, bn_idx)]))
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB, {len(names)} gradients, {len(bn)} BN statistics, "
          f"loss {float(loss64):.6f}")


if __name__ == "__main__":
    main()
