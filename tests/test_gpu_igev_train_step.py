"""One whole training step of IGEVStereo_ddim on the MI355X: `forward_train` (2-D front, cost volume, spx heads, geometry
lookup, update block and convex upsampling on their differentiable HIP routes), `loss.sequence_loss`, backward.

Parity with the reference (tests/golden/igev_train_step.npz, tools/make_golden_igev_train_step.py: the reference class's
own `forward` in train mode after freeze_bn() and its `sequence_loss`, float32 and float64, B 2, 64 x 128, 3 iterations,
fixed t and q_sample noise).  Bar per kind of tensor (weights, biases, outputs), as relative L2 against the fixture's
float64 (sampled entries and whole-tensor norms):
    rel(hip, f64) <= 2 * ref_err[kind] + 1e-6
with ref_err the worst relative L2 error of the reference's own float32 step for that kind.  There is no 1e-4 gate on
this fixture: whole-model float32 gradients are not well conditioned (L1 signs, ReLU kinks, the sampler's floor -- the
reference's float32 is 5.2e-2 / 6.0e-2 / 2.3e-3 from its float64 here), so the recorded error is the yardstick.

Measured on the MI355X (weights / biases / outputs): 7.1e-2 / 6.1e-2 / 2.5e-3 under bars of 1.04e-1 / 1.19e-1 / 4.6e-3."""
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
from diffuvolume_amd.loss import sequence_loss
from diffuvolume_amd.synth import IGEV_TRAIN_ARGS, NoiseTape, StubMobileNetV2, igev_train_step_inputs, synth_state_dict

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "outputs")
ARGS = types.SimpleNamespace(**IGEV_TRAIN_ARGS)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_train_step.npz") as z:
        return {k: z[k] for k in z.files}


def case_of(gold):
    b, h, w, iters = (int(v) for v in gold["shape"])
    return dict(seed=int(gold["seed"]), b=b, h=h, w=w, iters=iters, t=int(gold["t"]))


def fresh_model(gold):
    m = IGEVStereo_ddim(ARGS, feature=Feature(StubMobileNetV2()))
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=int(gold["weight_seed"])), strict=True)
    m = m.cuda().train()
    m.freeze_bn()
    return m


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def train_step(model, case):
    x = igev_train_step_inputs(device="cuda", **case)
    init, preds = model.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=x["iters"], t=x["t"],
                                      noise=x["noise"])
    loss, _ = sequence_loss(preds, init, x["flow_full"], x["valid"], max_disp=ARGS.max_disp)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach(), init=init.detach(), preds=[p.detach() for p in preds],
                grads={n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()})


_RUNS = {}


def hip_run(gold, monkeypatch):
    """The HIP route's step (model included), computed once and shared; the model is only modified by the test that says so."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    if "hip" not in _RUNS:
        model = fresh_model(gold)
        _RUNS["hip"] = (model, train_step(model, case_of(gold)))
    return _RUNS["hip"]


def assert_parity(gold, run, label):
    rows = {k: [] for k in KINDS}
    rows["outputs"].append(("loss", rel(float(run["loss"]), gold["loss_f64"])))
    idx = torch.from_numpy(gold["out_idx"]).cuda()
    b, h, w, iters = (int(v) for v in gold["shape"])
    assert tuple(run["init"].shape) == (b, 1, h, w) and len(run["preds"]) == iters
    rows["outputs"].append(("init", rel(run["init"].reshape(-1)[idx].cpu().numpy(), gold["init_f64"])))
    for i, p in enumerate(run["preds"]):
        assert tuple(p.shape) == (b, 1, h, w)
        rows["outputs"].append((f"pred{i}", rel(p.reshape(-1)[idx].cpu().numpy(), gold["preds_f64"][i])))
    for j, name in enumerate(gold["grad_names"]):
        name = str(name)
        gr = run["grads"][name]
        assert gr is not None, name
        kind = "biases" if name.endswith("bias") else "weights"
        gi = torch.from_numpy(gold["grad_idx"][j]).cuda()
        rows[kind].append((name, rel(gr.reshape(-1)[gi].cpu().numpy(), gold["grad_val_f64"][j])))
        rows[kind].append((name + ":norm", rel(float(gr.double().norm()), gold["grad_norm_f64"][j])))
    bound = {k: 2 * float(gold["ref_err"][i]) + 1e-6 for i, k in enumerate(KINDS)}
    for k in KINDS:
        worst = max(rows[k], key=lambda r: r[1])
        print(f"PARITY train step {label} {k}: worst {worst[1]:.3e} ({worst[0]})  bar {bound[k]:.2e}")
    bad = [(k, n, e) for k in KINDS for n, e in rows[k] if not e <= bound[k]]
    assert not bad, f"{label} route over the bar {bound}: {sorted(bad, key=lambda t: -t[2])[:12]}"


def test_step_matches_reference(gold, monkeypatch):
    _, run = hip_run(gold, monkeypatch)
    assert_parity(gold, run, "hip")


def test_parameters_without_a_gradient_are_the_references(gold, monkeypatch):
    _, run = hip_run(gold, monkeypatch)
    assert sorted(n for n, g in run["grads"].items() if g is None) == sorted(str(n) for n in gold["no_grad_names"])
    for n, g in run["grads"].items():
        if g is not None:
            assert torch.isfinite(g).all() and float(g.abs().max()) > 0, n


def test_two_steps_give_the_same_bits(gold, monkeypatch):
    _, ref = hip_run(gold, monkeypatch)
    run = train_step(fresh_model(gold), case_of(gold))
    assert torch.equal(run["loss"], ref["loss"]) and torch.equal(run["init"], ref["init"])
    assert all(torch.equal(a, b) for a, b in zip(run["preds"], ref["preds"]))
    for n, g in ref["grads"].items():
        assert (g is None and run["grads"][n] is None) or torch.equal(run["grads"][n], g), n


def test_test_mode_returns_the_last_prediction(gold, monkeypatch):
    model, ref = hip_run(gold, monkeypatch)
    x = igev_train_step_inputs(device="cuda", **case_of(gold))
    up = model.forward_train(x["image1"], x["image2"], x["flow_full"], x["flow_gt"], iters=x["iters"], test_mode=True,
                             t=x["t"], noise=x["noise"])
    assert torch.equal(up.detach(), ref["preds"][-1])


def test_refusals_and_eval_forward_after_an_optimizer_step(gold, monkeypatch):
    model, _ = hip_run(gold, monkeypatch)              # (its gradients are set: the shared run is not read after this test)
    x = igev_train_step_inputs(device="cuda", **case_of(gold))
    args = (x["image1"], x["image2"], x["flow_full"], x["flow_gt"])
    with pytest.raises(NotImplementedError, match="inference-only"):                   # `forward` keeps the parent's refusal
        model(*args)
    with pytest.raises(DiffuVolumeError):
        with torch.autocast("cuda", dtype=torch.float16):
            model.forward_train(*args, iters=1)
    with pytest.raises(DiffuVolumeError):
        model.forward_train(x["image1"].cpu(), *args[1:], iters=1)
    with pytest.raises(DiffuVolumeError):
        with torch.no_grad():
            model.forward_train(*args, iters=1)
    model.args.mixed_precision = True
    try:
        with pytest.raises(DiffuVolumeError):
            model.forward_train(*args, iters=1)
    finally:
        model.args.mixed_precision = False
    model.eval()
    with pytest.raises(DiffuVolumeError):
        model.forward_train(*args, iters=1)
    with torch.no_grad():
        before, _ = model(*args, iters=2, noise=NoiseTape(3))
    model.train()
    model.freeze_bn()
    torch.optim.AdamW([p for p in model.parameters() if p.grad is not None], lr=1e-3).step()
    model.eval()
    with torch.no_grad():
        after, _ = model(*args, iters=2, noise=NoiseTape(3))                                            # the plans follow the new weights
    assert torch.isfinite(after).all() and not torch.equal(after, before)
