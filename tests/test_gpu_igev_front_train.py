"""IGEV's 2-D front (IGEVFront2d: feature pyramid, stems, matching features, context encoder, context_zqr_convs) in train
mode on the MI355X: every convolution an autograd function on the HIP kernels (train2d.conv2d_any /
conv_transpose2d_module), InstanceNorm + activation on dv_instance_norm_act_f32 / _bwd_f32, BatchNorm2d, ReLU6, tanh and
relu PyTorch.

Parity with the reference (tests/golden/igev_front_train.npz, tools/make_golden_igev_front_train.py: the reference's
modules wired as its forward, train mode after freeze_bn(), float32 and float64, loss sum_i mean(out_i * cot_i); cases
`b1` B 1 and `b2` B 2, both 32 x 64 and inside the 1e-4 gate).  Bar per kind of tensor (weights, biases, outputs), as
relative L2 against the fixture's float64 (sampled entries and whole-tensor norms):
    rel(hip, f64) <= 2 * ref_err[kind] + 1e-6
with ref_err the worst relative L2 error of the reference's own float32 step for that kind (stored in the fixture).

Why the cases are this small and how their seeds were picked (the generator's docstring has the whole argument): the loss
is smooth but the front is not.  ONE ReLU / LeakyReLU / ReLU6 input within float32 rounding of its kink, decided the other
way than float64 decides it, moves the gradients of every layer before it by 1e-4 .. 1e-2, and every float32
implementation decides such signs for itself.  At 96 x 160 and 96 x 128 (13 million activation inputs) both this route and
PyTorch's own float32 on the MI355X missed the bar on most seeds for that reason alone, on other layers with every change
of a summation order, while each kernel was within its own bar (tests/test_gpu_igev_front_bwd.py).  So the cases are the
smallest the whole model admits (multiples of 32, more than one pixel at 1/32 resolution), and their seeds are those whose
float64 reference run keeps every activation input farthest from a kink (`act_margin` in the fixture: a property of the
reference alone).  The bar, the gate and the loss are the issue's."""
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVFront2d, IGEVStereo_ddim
from diffuvolume_amd.synth import (IGEV_FRONT_MODULES, IGEV_TRAIN_ARGS, StubMobileNetV2, igev_front_flat,
                                   igev_front_train_loss, igev_train_images, synth_state_dict)

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "outputs")
ARGS = types.SimpleNamespace(**IGEV_TRAIN_ARGS)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_front_train.npz") as z:
        return {k: z[k] for k in z.files}


def case_of(gold, case):
    b, h, w = (int(v) for v in gold[f"{case}_shape"])
    return dict(seed=int(gold[f"{case}_seed"]), b=b, h=h, w=w)


_SD = {}


def state_dict(gold):
    """The fixture's weights: the whole model's synthetic state_dict, as the reference was loaded with."""
    if not _SD:
        template = IGEVStereo_ddim(ARGS, feature=Feature(StubMobileNetV2())).state_dict()
        _SD.update(synth_state_dict(template, seed=int(gold["weight_seed"])))
    return _SD


def fresh_front(gold, freeze=True):
    m = IGEVFront2d(ARGS, Feature(StubMobileNetV2()))
    m.load_state_dict({k: v for k, v in state_dict(gold).items() if k.split(".")[0] in IGEV_FRONT_MODULES}, strict=True)
    m = m.cuda().train()
    if freeze:
        m.freeze_bn()
    return m


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def train_step(model, case):
    img1, img2 = igev_train_images(case["seed"], case["b"], case["h"], case["w"], device="cuda")
    outs = model(img1, img2)
    loss = igev_front_train_loss(outs, case["seed"])
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach(), outs=[t.detach() for t in igev_front_flat(outs)],
                grads={n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()})


_RUNS = {}


def hip_run(gold, case, monkeypatch):
    """The HIP route's step of a fixture case, computed once and shared (never modified)."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    if case not in _RUNS:
        _RUNS[case] = train_step(fresh_front(gold), case_of(gold, case))
    return _RUNS[case]


def assert_parity(gold, case, run, label):
    g = lambda key: gold[f"{case}_{key}"]
    rows = {k: [] for k in KINDS}
    rows["outputs"].append(("loss", rel(float(run["loss"]), g("loss_f64"))))
    assert len(run["outs"]) == len(g("out_idx"))
    for i, t in enumerate(run["outs"]):
        idx = torch.from_numpy(g("out_idx")[i]).cuda()
        rows["outputs"].append((f"out{i}", rel(t.reshape(-1)[idx].cpu().numpy(), g("out_val_f64")[i])))
        rows["outputs"].append((f"out{i}:norm", rel(float(t.double().norm()), g("out_norm_f64")[i])))
    for j, name in enumerate(g("grad_names")):
        name = str(name)
        gr = run["grads"][name]
        assert gr is not None and torch.isfinite(gr).all(), name
        kind = "biases" if name.endswith("bias") else "weights"
        idx = torch.from_numpy(g("grad_idx")[j]).cuda()
        rows[kind].append((name, rel(gr.reshape(-1)[idx].cpu().numpy(), g("grad_val_f64")[j])))
        rows[kind].append((name + ":norm", rel(float(gr.double().norm()), g("grad_norm_f64")[j])))
    bound = {k: 2 * float(g("ref_err")[i]) + 1e-6 for i, k in enumerate(KINDS)}
    for k in KINDS:
        worst = max(rows[k], key=lambda r: r[1])
        print(f"PARITY front {label} {case} {k}: worst {worst[1]:.3e} ({worst[0]})  bar {bound[k]:.2e}")
    bad = [(k, n, e) for k in KINDS for n, e in rows[k] if not e <= bound[k]]
    assert not bad, f"{label} route over the bar {bound}: {sorted(bad, key=lambda t: -t[2])[:12]}"


@pytest.mark.parametrize("case", ["b1", "b2"])
def test_step_matches_reference(gold, case, monkeypatch):
    run = hip_run(gold, case, monkeypatch)
    assert all(g is not None for g in run["grads"].values())                          # images ask for no gradient
    assert_parity(gold, case, run, "hip")


@pytest.mark.parametrize("case", ["b1", "b2"])
def test_two_steps_give_the_same_bits(gold, case, monkeypatch):
    ref = hip_run(gold, case, monkeypatch)
    run = train_step(fresh_front(gold), case_of(gold, case))
    assert torch.equal(run["loss"], ref["loss"]) and all(torch.equal(a, b) for a, b in zip(run["outs"], ref["outs"]))
    for n, g in ref["grads"].items():
        assert torch.equal(run["grads"][n], g), n


@pytest.mark.parametrize("case", ["b1", "b2"])
def test_torch_route_is_within_the_same_bar(gold, case, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)                  # MIOpen: the same solvers in every process
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    assert_parity(gold, case, train_step(fresh_front(gold), case_of(gold, case)), "torch")


def test_batchnorm_in_train_mode_runs_and_updates_its_buffers(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    m = fresh_front(gold, freeze=False)
    before = {k: v.clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    run = train_step(m, case_of(gold, "b2"))
    assert torch.isfinite(run["loss"]) and all(g is not None and torch.isfinite(g).all() for g in run["grads"].values())
    after = m.state_dict()
    assert before and all(not torch.equal(after[k], v) for k, v in before.items())


def test_eval_and_no_grad_equal_the_models_own_front(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    img1, img2 = igev_train_images(int(gold["b2_seed"]), 2, 64, 96, device="cuda")       # H != W, three pixels wide at 1/32
    model = IGEVStereo_ddim(ARGS, feature=Feature(StubMobileNetV2()))
    model.load_state_dict(state_dict(gold), strict=True)
    model = model.cuda().eval()
    with torch.no_grad():
        f, stem_2x, _, net, inp, geo_fn = model._front(img1, img2)
    front = fresh_front(gold).eval()
    outs = front(img1, img2)                                                          # eval mode, grad mode on
    front.train().freeze_bn()
    with torch.no_grad():
        again = front(img1, img2)                                                      # train mode under no_grad
    for got in (outs, again):
        fl, s2, ml, mr, nl, il = got
        assert all(torch.equal(a, b) for a, b in zip(fl, f)) and torch.equal(s2, stem_2x)
        assert all(torch.equal(a, b) for a, b in zip(nl, net))
        assert all(torch.equal(a, b) for ta, tb in zip(il, inp) for a, b in zip(ta, tb))
        ref_fn = type(geo_fn)(ml, mr, geo_fn.geo_volume)
        assert torch.equal(ref_fn.corr0, geo_fn.corr0)                                 # match_left / match_right: the same bits
    assert not any(t.requires_grad for t in igev_front_flat(outs))


def test_refusals(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    m = fresh_front(gold)
    img = torch.zeros(1, 3, 32, 64)
    with pytest.raises(DiffuVolumeError):
        m(img, img.cuda())                                                             # a CPU image
    with pytest.raises(DiffuVolumeError):
        with torch.autocast("cuda", dtype=torch.float16):
            m(img.cuda(), img.cuda())
