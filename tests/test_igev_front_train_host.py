"""Host-side checks of IGEV's whole-model training route: the C ABI of the two backward kernels of the 2-D front, the
fixtures tests/golden/igev_front_train.npz and igev_train_step.npz (gate, shapes, seeds, names), `loss.sequence_loss`
against the reference's recorded value, and the refusal of CPU tensors."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _lib, synth, train2d
from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVFront2d, IGEVStereo_ddim
from diffuvolume_amd.loss import sequence_loss

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("dv_instance_norm_act_bwd_f32", "dv_conv2d_fewin_wgrad_workspace_floats", "dv_conv2d_fewin_wgrad_f32")
ARGS = types.SimpleNamespace(**synth.IGEV_TRAIN_ARGS)


def load(name):
    with np.load(GOLDEN / name) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def front_gold():
    return load("igev_front_train.npz")


@pytest.fixture(scope="module")
def step_gold():
    return load("igev_train_step.npz")


def model():
    return IGEVStereo_ddim(ARGS, feature=Feature(synth.StubMobileNetV2()))


def test_new_symbols_in_header_and_signatures():
    header = (ROOT / "include" / "diffuvolume_hip.h").read_text()
    source = (ROOT / "diffuvolume_amd" / "csrc" / "igev_front_bwd.hip").read_text()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.SIGNATURES, sym
        decl = re.search(rf"\b{sym}\(([^;]*)\);", header)
        assert decl is not None, sym
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[sym][1]), sym     # one ctypes entry per C parameter
        assert re.search(rf'extern "C" \w+ {sym}\(', source), sym


def test_front_fixture_is_self_consistent(front_gold):
    gold = front_gold
    assert float(gold["gate"]) == 1e-4 and int(gold["weight_seed"]) == synth.IGEV_TRAIN_WEIGHT_SEED == 55
    assert [str(c) for c in gold["cases"]] == list(synth.IGEV_FRONT_TRAIN_CASES) == ["b1", "b2"]
    front = IGEVFront2d(ARGS, Feature(synth.StubMobileNetV2()))
    params = [n for n, _ in front.named_parameters()]
    full = [n for n, _ in model().named_parameters() if n.split(".")[0] in synth.IGEV_FRONT_MODULES]
    assert sorted(params) == sorted(full)                                              # the reference's names
    assert any(c["b"] > 1 for c in synth.IGEV_FRONT_TRAIN_CASES.values())
    for case, c in synth.IGEV_FRONT_TRAIN_CASES.items():
        g = lambda k: gold[f"{case}_{k}"]
        assert int(g("seed")) == c["seed"] and tuple(int(v) for v in g("shape")) == (c["b"], c["h"], c["w"])
        assert np.all(g("ref_err") > 0) and np.all(g("ref_err") < float(gold["gate"]))
        names = [str(n) for n in g("grad_names")]
        assert sorted(names) == sorted(params)                                          # every parameter gets a gradient
        n_out = 4 + 1 + 2 + 3 + 9
        for tag in ("f32", "f64"):
            dt = np.float32 if tag == "f32" else np.float64
            assert g(f"grad_val_{tag}").shape == (len(names), 32) and g(f"grad_val_{tag}").dtype == dt
            assert g(f"out_val_{tag}").shape == (n_out, 32) and g(f"out_norm_{tag}").shape == (n_out,)
            assert np.isfinite(g(f"loss_{tag}")) and np.all(g(f"grad_norm_{tag}") > 0) and np.all(g(f"out_norm_{tag}") > 0)
        r = np.abs(g("grad_norm_f32") - g("grad_norm_f64")) / g("grad_norm_f64")
        assert r.max() < float(gold["gate"])
    assert not any(gold[k].ndim > 2 for k in gold)                                      # seeds and samples, never weights


def test_step_fixture_is_self_consistent(step_gold):
    gold = step_gold
    c = synth.IGEV_TRAIN_STEP_CASE
    assert int(gold["weight_seed"]) == 55 and int(gold["seed"]) == c["seed"] and int(gold["t"]) == c["t"]
    assert tuple(int(v) for v in gold["shape"]) == (c["b"], c["h"], c["w"], c["iters"]) == (2, 64, 128, 3)
    names, none = [str(n) for n in gold["grad_names"]], [str(n) for n in gold["no_grad_names"]]
    assert sorted(names + none) == sorted(n for n, _ in model().named_parameters())
    assert sorted(none) == sorted([n for n, _ in model().named_parameters() if n.startswith("time_embedding.")] +
                                  ["cost_agg.conv1_up.bn.weight", "cost_agg.conv1_up.bn.bias"])
    assert gold["ref_err"].shape == (3,) and np.all(gold["ref_err"] > 0) and gold["ref_err_each"].shape == (len(names),)
    weights = [e for n, e in zip(names, gold["ref_err_each"]) if not n.endswith("bias")]
    assert float(gold["ref_err"][0]) == max(weights)
    for tag in ("f32", "f64"):
        assert gold[f"grad_val_{tag}"].shape == (len(names), 32) and gold[f"preds_{tag}"].shape == (c["iters"], 256)
        assert gold[f"init_{tag}"].shape == (256,) and np.isfinite(gold[f"loss_{tag}"])
        assert np.all(gold[f"grad_norm_{tag}"] > 0)
    assert abs(float(gold["loss_f32"]) - float(gold["loss_f64"])) <= float(gold["ref_err"][2]) * float(gold["loss_f64"])
    x = synth.igev_train_step_inputs(**c)
    assert x["image1"].shape == (2, 3, 64, 128) and x["flow_gt"].shape == (2, 1, 16, 32) and x["noise"].shape == (2, 48, 16, 32)
    assert x["t"].tolist() == [c["t"]] and float(x["image1"].max()) <= 255 and float(x["image1"].min()) >= 0


def test_sequence_loss_matches_the_reference(step_gold):
    seed = synth.IGEV_TRAIN_STEP_CASE["seed"]
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        preds, init, gt, valid = synth.igev_sequence_loss_inputs(seed, dtype=dt)
        assert float((gt >= 192).float().mean()) > 0.05 and float((valid < 0.5).float().mean()) > 0.05
        loss, metrics = sequence_loss(preds, init, gt, valid, max_disp=192)
        ref = float(step_gold[f"seq_loss_{tag}"])
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (tag, float(loss), ref)
        np.testing.assert_allclose([metrics[k] for k in ("epe", "1px", "3px", "5px")], step_gold[f"seq_metrics_{tag}"],
                                   rtol=1e-6)
    preds, init, gt, valid = synth.igev_sequence_loss_inputs(seed)
    one, _ = sequence_loss(preds[-1:], init, gt, valid)                                # a single prediction: weight 1
    assert torch.isfinite(one)
    with pytest.raises(AssertionError):
        sequence_loss([], init, gt, valid)


def test_cpu_tensors_raise():
    x = torch.zeros(1, 3, 8, 8)
    w = torch.zeros(4, 3, 3, 3, requires_grad=True)
    for call in (lambda: train2d.conv2d_fewin(x, w, None, 2),
                 lambda: train2d.conv2d_s2(torch.zeros(1, 8, 8, 8), torch.zeros(4, 8, 3, 3, requires_grad=True)),
                 lambda: train2d.conv2d_k1s2(torch.zeros(1, 8, 8, 8), torch.zeros(4, 8, 1, 1, requires_grad=True)),
                 lambda: train2d.instance_norm_act(torch.zeros(1, 2, 4, 4, requires_grad=True)),
                 lambda: train2d.conv2d_any(torch.nn.Conv2d(3, 4, 3, 2, 1), x)):
        with pytest.raises(DiffuVolumeError):
            call()
    front = IGEVFront2d(ARGS, Feature(synth.StubMobileNetV2())).train()
    with pytest.raises(DiffuVolumeError):
        front(torch.zeros(1, 3, 32, 64), torch.zeros(1, 3, 32, 64))
    m = model().train()
    img = torch.zeros(1, 3, 32, 64)
    with pytest.raises(DiffuVolumeError):
        m.forward_train(img, img, torch.zeros(1, 1, 32, 64), torch.zeros(1, 1, 8, 16), iters=1)
    with pytest.raises(DiffuVolumeError):                                              # the eval entry is `forward`
        m.eval().forward_train(img, img, torch.zeros(1, 1, 32, 64), torch.zeros(1, 1, 8, 16), iters=1)
    with pytest.raises(NotImplementedError, match="inference-only"):                   # and `forward` keeps refusing train mode
        m.train()(img, img, torch.zeros(1, 1, 32, 64), torch.zeros(1, 1, 8, 16))
