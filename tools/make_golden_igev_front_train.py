"""Golden vectors for one TRAINING step of IGEV's 2-D front (tests/golden/igev_front_train.npz): the reference class
(KITTI15/core/igev_stereo_ddim.py) constructed with `timm.create_model` stubbed to synth.StubMobileNetV2, as in
oracle/make_golden_igev_model.py, and its modules `feature`, `stem_2`, `stem_4`, `conv`, `desc`, `cnet`,
`context_zqr_convs` wired as its forward does (:364-377, :395-398), in train mode after `freeze_bn()`.

The reference gets ``synth_state_dict(template, seed=IGEV_TRAIN_WEIGHT_SEED)`` and runs, in float32 and in float64, the
front on ``synth.igev_train_images`` + ``synth.igev_front_train_loss`` (sum of mean(out * cot) with seeded cotangents over
every output: smooth, so the conditioning is the front's own) + backward.

The loss is smooth but the front is not: it has millions of ReLU / LeakyReLU / ReLU6 inputs, and ONE of them that lies
within float32 rounding of its kink, decided the other way than float64 decides it, moves the gradients of every layer
before it by about 1 / sqrt(elements of that layer's output): 1e-4 .. 1e-2, far above twice the reference's own float32
error (1e-5).  Every float32 implementation decides such signs for itself (another summation order is enough), so a
case measures an implementation only if it has no such input.  Hence the cases (``synth.IGEV_FRONT_TRAIN_CASES``):
  * size: B 1 and B 2 at 32 x 64, the smallest the whole model admits (multiples of 32) with more than one pixel per plane
    at 1/32 resolution, because the number of inputs near a kink grows with the number of pixels (at 96 x 160, 13 million
    activation inputs, the expected count within 3e-7 of a kink is above one);
  * seeds: of SCAN_SEEDS, the seed whose float64 run keeps every activation input FARTHEST from a kink
    (``activation_margin``: distance / RMS of the tensor; `--scan b1` / `--scan b2` prints the table), provided it passes
    the gate below.  The margin is a property of the reference's float64 run alone; it is stored as ``act_margin``.

Stored per case (prefix ``<case>_``; seeds, samples and norms, never weights), float32 and float64:
  loss, out_norm / out_val  per output (synth.igev_front_flat order) the L2 norm and SAMPLES entries (out_idx)
  grad_norm / grad_val      per parameter (order in grad_names) the L2 norm and SAMPLES entries (grad_idx)
  ref_err                   the reference float32's relative L2 error against float64 per full tensor:
                            [weights, biases, outputs] = the worst of that kind (outputs: loss and every output)
The file is written only if every reference float32 gradient is within GATE = 1e-4 relative L2 of its float64 one (a
case that fails -- one InstanceNorm + ReLU sign flip between the precisions is enough -- gets another input seed or
size, never another gate).

Build container only:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_igev_front_train.py [--scan CASE]"""
import contextlib
import io
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from diffuvolume_amd.synth import (IGEV_FRONT_MODULES, IGEV_FRONT_TRAIN_CASES, IGEV_TRAIN_ARGS, IGEV_TRAIN_WEIGHT_SEED,  # noqa: E402
                                   StubMobileNetV2, _gen, igev_front_flat, igev_front_train_loss, igev_train_images,
                                   synth_state_dict)
from oracle.make_golden import REF  # noqa: E402

OUT = REPO / "tests" / "golden" / "igev_front_train.npz"
SAMPLES = 32
GATE = 1e-4
KINDS = ("weights", "biases", "outputs")
SCAN_SEEDS = [s for base in (100, 200, 300, 400) for s in range(base, base + 30)]


def import_reference():
    warnings.filterwarnings("ignore")
    timm = types.ModuleType("timm")
    timm.create_model = lambda *a, **k: StubMobileNetV2()
    sys.modules["timm"] = timm
    oe = types.ModuleType("opt_einsum")
    oe.contract = torch.einsum
    sys.modules.setdefault("opt_einsum", oe)
    sys.path.insert(0, str(REF / "KITTI15"))
    import core.igev_stereo_ddim as R
    return R


def front(m, image1, image2):
    """igev_stereo_ddim.py:364-377 and :395-398 on the reference's modules."""
    image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
    features_left = m.feature(image1)
    features_right = m.feature(image2)
    stem_2x = m.stem_2(image1)
    stem_4x = m.stem_4(stem_2x)
    stem_2y = m.stem_2(image2)
    stem_4y = m.stem_4(stem_2y)
    features_left[0] = torch.cat((features_left[0], stem_4x), 1)
    features_right[0] = torch.cat((features_right[0], stem_4y), 1)
    match_left = m.desc(m.conv(features_left[0]))
    match_right = m.desc(m.conv(features_right[0]))
    cnet_list = m.cnet(image1, num_layers=m.args.n_gru_layers)
    net_list = [torch.tanh(x[0]) for x in cnet_list]
    inp_list = [torch.relu(x[1]) for x in cnet_list]
    inp_list = [list(conv(i).split(split_size=conv.out_channels // 3, dim=1)) for i, conv in zip(inp_list, m.context_zqr_convs)]
    return features_left, stem_2x, match_left, match_right, net_list, inp_list


def sample_index(key: str, numel: int, n: int) -> np.ndarray:
    if numel <= n:
        return np.arange(n, dtype=np.int64) % numel
    return torch.randint(0, numel, (n,), generator=_gen(IGEV_TRAIN_WEIGHT_SEED, key)).numpy().astype(np.int64)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())


def reference_model(R, sd, dtype):
    with contextlib.redirect_stdout(io.StringIO()):
        model = R.IGEVStereo_ddim(types.SimpleNamespace(**IGEV_TRAIN_ARGS))
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).train()
    model.freeze_bn()
    return model


@contextlib.contextmanager
def kink_watch(state):
    """While active, every ReLU / LeakyReLU / ReLU6 call notes in ``state["margin"]`` the smallest distance of an input
    from the activation's kink(s), relative to the RMS of the input tensor.  Exact zeros are left out: they are structural
    (the relu of a sum of two relu outputs) and no rounding moves them."""
    import torch.nn.functional as F

    def note(x, kinks=(0.0,)):
        x = x.detach()
        rms = float(x.pow(2).mean().sqrt())
        for k in kinks if rms > 0 else ():
            d = (x - k).abs()
            d = d[d > 0]
            if d.numel():
                state["margin"] = min(state["margin"], float(d.min()) / rms)

    saved = F.relu, F.leaky_relu, F.hardtanh, F.relu6, torch.relu
    F.relu = lambda x, inplace=False: (note(x), saved[0](x, inplace))[1]
    F.leaky_relu = lambda x, negative_slope=0.01, inplace=False: (note(x), saved[1](x, negative_slope, inplace))[1]
    F.hardtanh = lambda x, min_val=-1.0, max_val=1.0, inplace=False: (note(x, (min_val, max_val)),
                                                                      saved[2](x, min_val, max_val, inplace))[1]
    F.relu6 = lambda x, inplace=False: (note(x, (0.0, 6.0)), saved[3](x, inplace))[1]
    torch.relu = lambda x: (note(x), saved[4](x))[1]
    try:
        yield state
    finally:
        F.relu, F.leaky_relu, F.hardtanh, F.relu6, torch.relu = saved


def activation_margin(model64, case):
    """The float64 reference's smallest relative distance of an activation input from a kink, over the whole front."""
    state = dict(margin=float("inf"))
    img1, img2 = igev_train_images(case["seed"], case["b"], case["h"], case["w"], torch.float64)
    with torch.no_grad(), kink_watch(state):
        front(model64, img1, img2)
    return state["margin"]


def run(R, sd, case, dtype):
    model = reference_model(R, sd, dtype)
    img1, img2 = igev_train_images(case["seed"], case["b"], case["h"], case["w"], dtype)
    outs = front(model, img1, img2)
    loss = igev_front_train_loss(outs, case["seed"])
    loss.backward()
    params = {n: p for n, p in model.named_parameters() if n.split(".")[0] in IGEV_FRONT_MODULES}
    return params, loss.detach(), [t.detach() for t in igev_front_flat(outs)]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = import_reference()
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    template = IGEVStereo_ddim(types.SimpleNamespace(**IGEV_TRAIN_ARGS), feature=Feature(StubMobileNetV2())).state_dict()
    sd = synth_state_dict(template, seed=IGEV_TRAIN_WEIGHT_SEED)
    model64 = reference_model(R, sd, torch.float64)
    if "--scan" in sys.argv:
        case = dict(IGEV_FRONT_TRAIN_CASES[sys.argv[sys.argv.index("--scan") + 1]])
        table = sorted(((activation_margin(model64, dict(case, seed=s)), s) for s in SCAN_SEEDS), reverse=True)
        print("\n".join(f"seed {s}: margin {m:.3e}" for m, s in table))
        return
    arrays = dict(weight_seed=IGEV_TRAIN_WEIGHT_SEED, gate=GATE, cases=np.array(list(IGEV_FRONT_TRAIN_CASES)))
    for cname, case in IGEV_FRONT_TRAIN_CASES.items():
        margin = activation_margin(model64, case)
        p32, l32, o32 = run(R, sd, case, torch.float32)
        p64, l64, o64 = run(R, sd, case, torch.float64)
        names = list(p32)
        assert all(p32[n].grad is not None and p64[n].grad is not None for n in names)
        err = dict.fromkeys(KINDS, 0.0)
        worst = ("", 0.0)
        for n in names:
            r = rel(p32[n].grad, p64[n].grad)
            kind = "biases" if n.endswith("bias") else "weights"
            err[kind] = max(err[kind], r)
            worst = max(worst, (n, r), key=lambda v: v[1])
        if worst[1] > GATE:
            raise SystemExit(f"{cname}: {worst[0]}: fp32 gradient {worst[1]:.2e} from fp64 (> {GATE}): change the input "
                             f"seed or the size of the case")
        for a, b in [(l32, l64)] + list(zip(o32, o64)):
            err["outputs"] = max(err["outputs"], rel(a, b))
        print(f"{cname}: activation margin {margin:.2e}, gate ok (worst {worst[0]} {worst[1]:.2e}), reference fp32 against fp64, worst per kind: " +
              ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        pre = cname + "_"
        grad_idx = np.stack([sample_index(f"{cname}:g:{n}", p32[n].numel(), SAMPLES) for n in names])
        out_idx = np.stack([sample_index(f"{cname}:o:{i}", t.numel(), SAMPLES) for i, t in enumerate(o32)])
        arrays.update({pre + "seed": case["seed"], pre + "shape": np.array([case["b"], case["h"], case["w"]]),
                       pre + "grad_names": np.array(names), pre + "grad_idx": grad_idx, pre + "out_idx": out_idx,
                       pre + "ref_err": np.array([err[k] for k in KINDS]), pre + "act_margin": margin})
        for tag, (params, loss, outs) in (("f32", (p32, l32, o32)), ("f64", (p64, l64, o64))):
            arrays[f"{pre}loss_{tag}"] = loss.numpy()
            arrays[f"{pre}out_norm_{tag}"] = np.array([float(t.double().norm()) for t in outs])
            arrays[f"{pre}out_val_{tag}"] = np.stack([t.reshape(-1)[torch.from_numpy(i)].numpy() for t, i in zip(outs, out_idx)])
            arrays[f"{pre}grad_norm_{tag}"] = np.array([float(params[n].grad.double().norm()) for n in names])
            arrays[f"{pre}grad_val_{tag}"] = np.stack([params[n].grad.reshape(-1)[torch.from_numpy(i)].numpy()
                                                       for n, i in zip(names, grad_idx)])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT.name}: {OUT.stat().st_size / 1024:.1f} KB")


if __name__ == "__main__":
    main()
