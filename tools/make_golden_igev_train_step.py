"""Golden vectors for one whole TRAINING step of IGEVStereo_ddim (tests/golden/igev_train_step.npz): the reference
class's own `forward` in train mode (KITTI15/core/igev_stereo_ddim.py:361-463) and the reference's `sequence_loss`
(KITTI15/train_stereo.py:33-62), as train_stereo.py:160-163 calls them.

What it takes to run the reference's train branch here:
  * `timm.create_model` stubbed to synth.StubMobileNetV2 and `Tensor.cuda` to the identity, as in
    oracle/make_golden_igev_model.py;
  * the branch crashes as committed: :404 builds `coords` as [b,h,w,1], core/geometry_ddim.py:36-37 reads it as
    [batch,_,h1,w1] and reshapes `noisy` to b*w rows, which :56 cannot broadcast.  A subclass of the reference's
    Combined_Geo_Encoding_Volume whose __call__ passes ``coords.reshape(disp.shape)`` (the same element order, [B,1,h,w]) is
    bound to the module global that :401 reads;
  * `torch.randint` / `torch.randn_like` patched to the fixed ``t`` and ``noise`` of synth.igev_train_step_inputs;
  * `train_stereo` imported with stubs for the modules that are not installed (tensorboard, evaluate_stereo,
    core.stereo_datasets);
  * the float64 run: `time_embedding` kept in float32, `flow_gt` passed as float32 and `Tensor.float` neutralised during the
    call (the casts the reference hard-codes at :402 and :407).
One case (``synth.IGEV_TRAIN_STEP_CASE``): B 2, 64 x 128, 3 iterations, after `freeze_bn()`, weights
``synth_state_dict(template, seed=IGEV_TRAIN_WEIGHT_SEED)``.

Stored (seeds, samples and norms, never weights), float32 and float64:
  loss, init / preds       the outputs at sampled positions (out_idx)
  grad_norm / grad_val     per parameter with a gradient (order in grad_names) the L2 norm and SAMPLES entries (grad_idx)
  no_grad_names            the parameters that get no gradient
  ref_err                  the reference float32's relative L2 error against float64 per full tensor:
                           [weights, biases, outputs] = the worst of that kind
  ref_err_each             the same per parameter (grad_names order)
  seq_loss / seq_metrics   the reference's sequence_loss alone on synth.igev_sequence_loss_inputs (loss; epe, 1px, 3px, 5px)
No gate: whole-model float32 gradients are not well conditioned (L1 signs, ReLU kinks, the sampler's floor); the recorded
error is the yardstick.

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_igev_train_step.py"""
import contextlib
import io
import os
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import (IGEV_TRAIN_ARGS, IGEV_TRAIN_STEP_CASE, IGEV_TRAIN_WEIGHT_SEED, StubMobileNetV2, _gen,  # noqa: E402
                                   igev_sequence_loss_inputs, igev_train_step_inputs, synth_state_dict)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "igev_train_step.npz"
SAMPLES, PIX = 32, 256
KINDS = ("weights", "biases", "outputs")


def import_reference():
    warnings.filterwarnings("ignore")
    torch.Tensor.cuda = lambda self, *a, **k: self
    timm = types.ModuleType("timm")
    timm.create_model = lambda *a, **k: StubMobileNetV2()
    sys.modules["timm"] = timm
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    import core
    import core.igev_stereo_ddim as R

    class Geo(R.Combined_Geo_Encoding_Volume):
        def __call__(self, disp, coords, noisy):
            return super().__call__(disp, coords.reshape(disp.shape), noisy)

    R.Combined_Geo_Encoding_Volume = Geo
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.modules.setdefault("evaluate_stereo", types.ModuleType("evaluate_stereo"))
    ds = types.ModuleType("core.stereo_datasets")
    sys.modules.setdefault("core.stereo_datasets", ds)
    core.stereo_datasets = ds
    visible = os.environ.get("CUDA_VISIBLE_DEVICES")
    import train_stereo                       # (sets CUDA_VISIBLE_DEVICES on import)
    if visible is None:
        os.environ.pop("CUDA_VISIBLE_DEVICES", None)
    else:
        os.environ["CUDA_VISIBLE_DEVICES"] = visible
    return R, train_stereo.sequence_loss


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(IGEV_TRAIN_WEIGHT_SEED, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def run(R, sequence_loss, sd, dtype):
    with contextlib.redirect_stdout(io.StringIO()):
        model = R.IGEVStereo_ddim(types.SimpleNamespace(**IGEV_TRAIN_ARGS))
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    model.freeze_bn()
    x = igev_train_step_inputs(dtype=dtype, **IGEV_TRAIN_STEP_CASE)
    real = torch.randn_like, torch.randint, torch.Tensor.float
    torch.randn_like = lambda t, *a, **k: x["noise"].to(t.dtype)
    torch.randint = lambda *a, **k: x["t"].clone()
    flow_gt = x["flow_gt"]
    if dtype == torch.float64:
        model.time_embedding.float()
        flow_gt = flow_gt.float()
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        init, preds = model(x["image1"], x["image2"], x["flow_full"], flow_gt, iters=x["iters"])
        loss, _ = sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=IGEV_TRAIN_ARGS["max_disp"])
    finally:
        torch.randn_like, torch.randint, torch.Tensor.float = real
    assert init.dtype == dtype and loss.dtype == dtype, (init.dtype, loss.dtype)
    loss.backward()
    return dict(model.named_parameters()), loss.detach(), init.detach(), [p.detach() for p in preds]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R, sequence_loss = import_reference()
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    template = IGEVStereo_ddim(types.SimpleNamespace(**IGEV_TRAIN_ARGS), feature=Feature(StubMobileNetV2())).state_dict()
    sd = synth_state_dict(template, seed=IGEV_TRAIN_WEIGHT_SEED)
    p32, l32, i32, u32 = run(R, sequence_loss, sd, torch.float32)
    p64, l64, i64, u64 = run(R, sequence_loss, sd, torch.float64)
    no_grad = [n for n in p32 if p32[n].grad is None]
    assert no_grad == [n for n in p64 if p64[n].grad is None]
    names = [n for n in p32 if p32[n].grad is not None]
    err = dict.fromkeys(KINDS, 0.0)
    each = []
    for n in names:
        r = rel(p32[n].grad, p64[n].grad)
        each.append(r)
        kind = "biases" if n.endswith("bias") else "weights"
        err[kind] = max(err[kind], r)
    for a, b in [(l32, l64), (i32, i64)] + list(zip(u32, u64)):
        err["outputs"] = max(err["outputs"], rel(a, b))
    order = np.argsort(each)[::-1][:5]
    print(f"loss {float(l64):.6f} (fp32 {rel(l32, l64):.2e} off); reference fp32 against fp64, worst per kind: " +
          ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    print("worst gradients: " + ", ".join(f"{names[i]} {each[i]:.2e}" for i in order))
    print(f"{len(no_grad)} parameters without a gradient: {no_grad}")
    c = IGEV_TRAIN_STEP_CASE
    grad_idx = np.stack([sample_index(f"g:{n}", p32[n].numel(), SAMPLES) for n in names])
    out_idx = sample_index("out", i32.numel(), PIX)
    arrays = dict(weight_seed=IGEV_TRAIN_WEIGHT_SEED, seed=c["seed"], shape=np.array([c["b"], c["h"], c["w"], c["iters"]]),
                  t=c["t"], grad_names=np.array(names), no_grad_names=np.array(no_grad), grad_idx=grad_idx, out_idx=out_idx,
                  ref_err=np.array([err[k] for k in KINDS]), ref_err_each=np.array(each))
    # the loss function alone on seeded arguments (the CPU test of loss.sequence_loss)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        sl, metrics = sequence_loss(*igev_sequence_loss_inputs(c["seed"], dtype=dt), max_disp=IGEV_TRAIN_ARGS["max_disp"])
        arrays[f"seq_loss_{tag}"] = sl.numpy()
        arrays[f"seq_metrics_{tag}"] = np.array([metrics[k] for k in ("epe", "1px", "3px", "5px")])
    for tag, (params, loss, init, preds) in (("f32", (p32, l32, i32, u32)), ("f64", (p64, l64, i64, u64))):
        idx = torch.from_numpy(out_idx)
        arrays[f"loss_{tag}"] = loss.numpy()
        arrays[f"init_{tag}"] = init.reshape(-1)[idx].numpy()
        arrays[f"preds_{tag}"] = np.stack([u.reshape(-1)[idx].numpy() for u in preds])
        arrays[f"grad_norm_{tag}"] = np.array([float(params[n].grad.double().norm()) for n in names])
        arrays[f"grad_val_{tag}"] = np.stack([params[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                              for n, i in zip(names, grad_idx)])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
