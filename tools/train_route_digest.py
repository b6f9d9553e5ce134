"""What one recorded training step of ACVNet_DDIM and PWCNet_ddim launches and computes, to compare two commits.

The file uses only names both commits have (the model classes, `synth`, the loss functions, `_lib.launch` /
`_lib.timed_launch`, the DV_TRAIN_* variables, `set_train_precision`), so the identical file runs against either package:
`--package-root DIR` names the directory that holds `diffuvolume_amd/` (default: this repository).  Two runs' JSON files
must be equal entry by entry (profiles/train_route_digests.json keeps a `parent` and a `branch` run).

The steps are those of tests/golden/acv_train_step.npz (B = 2, 64 x 160) and tests/golden/pcw_train_step.npz (B = 2,
64 x 128) -- the weights seed, inputs, fixed timestep and NoiseTape of test_gpu_acv_train.step / test_gpu_pcw_train.step --
forward + loss + backward, each on a fresh model.  Every case records the ordered list of entries that went through
`_lib.launch` / `_lib.timed_launch` as count + sha256, and

  hip/<precision>   DV_TRAIN_NET2D=hip, everything else at its default, train precision f32 / f16 / bf16: the digests of
                    every output, the loss, every parameter gradient and every BatchNorm buffer (a step repeats bit for
                    bit in these configurations)
  default, norm=torch, conv3d=torch, conv2d=torch
                    all defaults (NET2D=torch) and one switch at a time on its PyTorch route: `num_batches_tracked` of every
                    BatchNorm and the autograd node names reachable from the last output; no value digests (MIOpen and
                    ATen atomics are in the graph)
  eval/<class>      the eval forward of ACVNet_DDIM, ACVNet, PWCNet_ddim and PWCNet (weights, inputs and seeds of
                    tools/ddim_route_digest.py), plans built before the recording starts: the launch list and the digests
                    of the outputs

    python tools/train_route_digest.py [--package-root DIR] --out FILE"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")       # bounded solver search on the PyTorch routes

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
SWITCHES = ("DV_TRAIN_NET2D", "DV_TRAIN_NORM", "DV_TRAIN_CONV3D", "DV_TRAIN_CONV2D")
VALUE_CASES = [(f"hip/{name}", {"DV_TRAIN_NET2D": "hip"}, prec)
               for name, prec in (("f32", "f32"), ("f16", "f16"), ("bf16", torch.bfloat16))]
ROUTE_CASES = [("default", {}, "f32"), ("norm=torch", {"DV_TRAIN_NORM": "torch"}, "f32"),
               ("conv3d=torch", {"DV_TRAIN_CONV3D": "torch"}, "f32"), ("conv2d=torch", {"DV_TRAIN_CONV2D": "torch"}, "f32")]
OUT = {}


def sha(obj):
    return hashlib.sha256(json.dumps(obj).encode()).hexdigest()


def digest(t):
    t = t.detach().cpu().contiguous()
    return f"{t.dtype}{list(t.shape)}:" + hashlib.sha256(t.numpy().tobytes()).hexdigest()


def inputs(gold, quarter_disp_from_gt):
    from diffuvolume_amd.synth import _gen, synth_stereo_batch
    b, h, w = (int(v) for v in gold["shape"])
    seed = int(gold["input_seed"])
    x = synth_stereo_batch(b, h, w, seed=seed)
    gt = x["gt"].clone()
    bad = torch.rand(b, h, w, generator=_gen(seed, "train_gt_invalid"))
    gt[bad < 0.05] = 0.0
    gt[bad > 0.97] = 200.0
    disp = x["disp"]
    if quarter_disp_from_gt:                                    # KITTI12/main.py:148-150
        disp = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    return [t.cuda() for t in (x["left"], x["right"], disp, gt)]


def node_names(fn):
    """The autograd node names reachable from `fn`, depth first in the order of `next_functions`."""
    names, seen, todo = [], set(), [fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(n.name())
        todo.extend(f for f, _ in reversed(n.next_functions))
    return names


def recorded(_lib, launched):
    """Wrap `_lib.launch` and `_lib.timed_launch` so that every entry name lands in `launched`; returns the two originals."""
    real = (_lib.launch, _lib.timed_launch)

    def launch(name, *a, **k):
        launched.append(name)
        return real[0](name, *a, **k)

    def timed_launch(tag_, flops, nbytes, name, *a, **k):
        launched.append(name)
        return real[1](tag_, flops, nbytes, name, *a, **k)
    _lib.launch, _lib.timed_launch = launch, timed_launch
    return real


def flat(out):
    """Every tensor of a nested tuple / list, in order; a volume handle gives its cost and uncertainty."""
    if isinstance(out, torch.Tensor):
        return [out]
    if hasattr(out, "cost") and hasattr(out, "uncertainty"):
        return [out.cost, out.uncertainty]
    return [t for o in out for t in flat(o)]


def run_eval(dv):
    """The eval forwards: the second call of each model is recorded, so plan builds (first call) stay out of the list."""
    from diffuvolume_amd import _lib
    from diffuvolume_amd.synth import synth_state_dict, synth_stereo_batch
    with np.load(ROOT / "tests" / "golden" / "pcw_forward_eval.npz", allow_pickle=False) as g:
        scale = {str(k): float(v) for k, v in zip(g["scale_keys"].tolist(), g["scale_vals"].tolist())}
    acv = {k: v.cuda() for k, v in synth_stereo_batch(2, 64, 128, seed=3).items()}
    pcw = {k: v.cuda() for k, v in synth_stereo_batch(1, 64, 128, seed=4, shifts=(8,)).items()}
    cases = (("ACVNet_DDIM", lambda: dv.ACVNet_DDIM(192), dict(seed=1, logit_gain=8.0), acv, True),
             ("ACVNet", lambda: dv.ACVNet(192), dict(seed=1, logit_gain=8.0), acv, False),
             ("PWCNet_ddim", lambda: dv.PWCNet_ddim(192, True), dict(seed=2, logit_gain=8.0, scale=scale), pcw, True),
             ("PWCNet", lambda: dv.PWCNet(192, True), dict(seed=2, logit_gain=8.0, scale=scale), pcw, False))
    for name, make, synth_args, x, ddim in cases:
        model = make()
        model.load_state_dict(synth_state_dict(model.state_dict(), **synth_args), strict=True)
        model = model.cuda().eval()
        args = (x["left"], x["right"], x["used"], x["disp"]) if ddim else (x["left"], x["right"])
        with torch.no_grad():
            torch.manual_seed(5)
            model(*args)
            launched = []
            real = recorded(_lib, launched)
            try:
                torch.manual_seed(5)
                outs = model(*args)
                torch.cuda.synchronize()
            finally:
                _lib.launch, _lib.timed_launch = real
        OUT[f"gpu/eval/{name}"] = {"launches": f"{len(launched)} entries:" + sha(launched),
                                   "outputs": sha([digest(t) for t in flat(outs)])}
        print(f"gpu/eval/{name}", OUT[f"gpu/eval/{name}"]["launches"][:40], flush=True)


def run_case(tag, make, loss_fn, gold, quarter_disp, env, precision, values):
    from diffuvolume_amd import _lib
    from diffuvolume_amd.synth import NoiseTape, synth_state_dict
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    model = make()
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(gold["weight_seed"])), strict=True)
    model = model.cuda().train().set_train_precision(precision)
    left, right, disp, gt = inputs(gold, quarter_disp)
    tape, t = NoiseTape(int(gold["tape_seed"])), int(gold["t_step"])
    launched = []
    real = recorded(_lib, launched) + (torch.randint, torch.randn_like)
    torch.randint = lambda low, high, size, *a, device=None, **k: real[2](t, t + 1, size, device=device)
    torch.randn_like = lambda x, *a, **k: tape("q", tuple(x.shape), x.dtype).to(x.device)
    try:
        outs = model(left, right, None, disp, None)
        torch.randint, torch.randn_like = real[2], real[3]
        loss = loss_fn(outs, gt, (gt < 192) & (gt > 0))
        nodes = node_names(outs[-1].grad_fn)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        _lib.launch, _lib.timed_launch, torch.randint, torch.randn_like = real
    rec = {"launches": f"{len(launched)} entries:" + sha(launched)}
    if values:
        rec["outputs"] = sha([digest(o) for o in outs])
        rec["loss"] = digest(loss)
        rec["gradients"] = sha([(n, None if p.grad is None else digest(p.grad)) for n, p in model.named_parameters()])
        rec["buffers"] = sha([(n, digest(b)) for n, b in model.named_buffers()])
        rec["finite"] = all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    else:
        rec["num_batches_tracked"] = sha([(n, int(b)) for n, b in model.named_buffers() if n.endswith("num_batches_tracked")])
        rec["autograd_nodes"] = f"{len(nodes)} nodes:" + sha(nodes)
    OUT[tag] = rec
    print(tag, " ".join(f"{k}={str(v)[-12:]}" for k, v in rec.items()), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", default=str(ROOT), help="the directory that holds diffuvolume_amd/")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, str(Path(a.package_root).resolve()))
    import diffuvolume_amd as dv
    assert Path(dv.__file__).resolve().parents[1] == Path(a.package_root).resolve(), dv.__file__
    assert torch.cuda.is_available(), "needs the MI355X"
    for name, make, loss_fn, quarter in (("acv", lambda: dv.ACVNet_DDIM(192), dv.model_loss_train, False),
                                        ("pcw", lambda: dv.PWCNet_ddim(192), dv.model_loss_kitti12, True)):
        with np.load(ROOT / "tests" / "golden" / f"{name}_train_step.npz") as z:
            gold = {k: z[k] for k in z.files}
        for values, cases in ((True, VALUE_CASES), (False, ROUTE_CASES)):
            for tag, env, precision in cases:
                torch.manual_seed(0)
                run_case(f"gpu/{name}/train/{tag}", make, loss_fn, gold, quarter, env, precision, values)
    for k in SWITCHES:
        os.environ.pop(k, None)
    run_eval(dv)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(OUT, indent=1, sort_keys=True) + "\n")
    print(f"{len(OUT)} entries -> {a.out}")


if __name__ == "__main__":
    main()
