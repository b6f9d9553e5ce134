"""IGEV's once-per-pair cost-volume front (IGEVCostVolume: gwc -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier
-> softmax + regression) in train mode on the MI355X: every convolution, transposed convolution and gate an autograd
function on the HIP kernels (train3d / train2d), BatchNorm / LeakyReLU / softmax in PyTorch.

Parity with the reference (tests/golden/igev_volume_train.npz, tools/make_golden_igev_volume_train.py: the imported
reference modules in float32 and float64 on one training step, cases `even` 16 x 32 D 16 and `tall` 8 x 24 D 48).
Bar per kind of tensor (weights, biases, leaves, outputs), as relative L2 against the fixture's float64:
    rel(hip, f64) <= 2 * ref_err[kind] + 1e-6
with ref_err the worst relative L2 error of the reference's own float32 step for that kind (stored in the fixture).

Measured on the MI355X (worst per kind, weights / biases / leaves / outputs; bars 1.2e-5 / 1.0e-5 / 7.4e-6 / 7.5e-6 for
`even`, 1.1e-5 / 1.6e-5 / 8.4e-6 / 6.7e-6 for `tall`):
    HIP   even 4.8e-6 / 4.4e-6 / 2.7e-6 / 2.7e-6,   tall 5.3e-6 / 6.7e-6 / 3.6e-6 / 3.2e-6
    torch even 5.2e-6 / 5.6e-6 / 3.1e-6 / 2.6e-6,   tall 3.9e-6 / 4.6e-6 / 2.6e-6 / 2.2e-6   (DV_TRAIN_CONV3D=torch)"""
import copy

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume
from diffuvolume_amd.submodule import build_gwc_volume, softmax_regress
from diffuvolume_amd.synth import (igev_volume_train_inputs, igev_volume_train_leaves, igev_volume_train_loss,
                                   synth_state_dict)
from test_igev_volume_oracle import igev_inputs, volume_state_dict

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "leaves", "outputs")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_volume_train.npz") as z:
        return {k: z[k] for k in z.files}


def case_of(gold, case):
    b, h, w, max_disp = (int(v) for v in gold[f"{case}_shape"])
    return dict(seed=int(gold[f"{case}_seed"]), b=b, h=h, w=w, max_disp=max_disp)


def fresh_model(gold, max_disp):
    m = IGEVCostVolume(max_disp)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=int(gold["weight_seed"]), logit_gain=float(gold["logit_gain"])),
                      strict=True)
    return m.cuda().train()


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def train_step(model, case, requires_grad=True):
    """forward + loss + backward of the fixture's step -> everything the tests compare, detached."""
    x = igev_volume_train_inputs(device="cuda", requires_grad=requires_grad, **case)
    geo, init = model(x["match_left"], x["match_right"], x["features"])
    loss = igev_volume_train_loss(geo, init, x)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach(), geo=geo.detach(), init=init.detach(),
                grads={n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()},
                leaves={n: t.grad for n, t in igev_volume_train_leaves(x).items()},
                bn={k: v.clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))})


_RUNS = {}


def hip_run(gold, case, monkeypatch):
    """The HIP route's step of a fixture case, computed once and shared (never modified)."""
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    if case not in _RUNS:
        c = case_of(gold, case)
        _RUNS[case] = train_step(fresh_model(gold, c["max_disp"]), c)
    return _RUNS[case]


def parity_rows(gold, case, run):
    """-> {kind: [(name, rel(ours, f64))]} over everything the fixture stores."""
    g = lambda key: gold[f"{case}_{key}"]
    rows = {k: [] for k in KINDS}
    rows["outputs"].append(("loss", rel(float(run["loss"]), g("loss_f64"))))
    for tag in ("geo", "init"):
        assert tuple(run[tag].shape) == tuple(int(v) for v in g(f"{tag}_shape")), tag
        idx = torch.from_numpy(g(f"{tag}_idx")).cuda()
        rows["outputs"].append((tag, rel(run[tag].reshape(-1)[idx].cpu().numpy(), g(f"{tag}_f64"))))
    bn = torch.cat([run["bn"][str(k)].reshape(-1) for k in g("bn_names")]).cpu().numpy()
    rows["outputs"].append(("bn running statistics", rel(bn, g("bn_f64"))))
    for what, tensors, names in (("grad", run["grads"], g("grad_names")), ("leaf", run["leaves"], g("leaf_names"))):
        for j, name in enumerate(names):
            name = str(name)
            gr = tensors[name]
            assert gr is not None and torch.isfinite(gr).all(), name
            kind = "leaves" if what == "leaf" else ("biases" if name.endswith("bias") else "weights")
            idx = torch.from_numpy(g(f"{what}_idx")[j]).cuda()
            rows[kind].append((name, rel(gr.reshape(-1)[idx].cpu().numpy(), g(f"{what}_val_f64")[j])))
            rows[kind].append((name + ":norm", rel(float(gr.double().norm()), g(f"{what}_norm_f64")[j])))
    return rows


def assert_parity(gold, case, run, label):
    rows = parity_rows(gold, case, run)
    bound = {k: 2 * float(gold[f"{case}_ref_err"][i]) + 1e-6 for i, k in enumerate(KINDS)}
    for k in KINDS:
        worst = max(rows[k], key=lambda r: r[1])
        print(f"PARITY {label} {case} {k}: worst {worst[1]:.3e} ({worst[0]})  bar {bound[k]:.2e}")
    bad = [(k, n, e) for k in KINDS for n, e in rows[k] if not e <= bound[k]]
    assert not bad, f"{label} route over the bar {bound}: {sorted(bad, key=lambda t: -t[2])[:12]}"


@pytest.mark.parametrize("case", ["even", "tall"])
def test_step_matches_reference(gold, case, monkeypatch):
    run = hip_run(gold, case, monkeypatch)
    none = sorted(str(n) for n in gold[f"{case}_none_names"])
    assert none == sorted(n for n, g in run["grads"].items() if g is None)            # cost_agg.conv1_up.bn.*: never called
    assert_parity(gold, case, run, "hip")


@pytest.mark.parametrize("case", ["even", "tall"])
def test_frozen_backbone_still_trains_the_volume_weights(gold, case, monkeypatch):
    ref = hip_run(gold, case, monkeypatch)
    c = case_of(gold, case)
    run = train_step(fresh_model(gold, c["max_disp"]), c, requires_grad=False)
    assert all(g is None for g in run["leaves"].values())
    assert torch.equal(run["loss"], ref["loss"])
    for n, g in ref["grads"].items():
        assert (g is None and run["grads"][n] is None) or torch.equal(run["grads"][n], g), n


@pytest.mark.parametrize("case", ["even", "tall"])
def test_two_steps_give_the_same_bits(gold, case, monkeypatch):
    ref = hip_run(gold, case, monkeypatch)
    c = case_of(gold, case)
    run = train_step(fresh_model(gold, c["max_disp"]), c)
    assert torch.equal(run["loss"], ref["loss"]) and torch.equal(run["geo"], ref["geo"]) and torch.equal(run["init"], ref["init"])
    for group in ("grads", "leaves", "bn"):
        for n, g in ref[group].items():
            assert (g is None and run[group][n] is None) or torch.equal(run[group][n], g), (group, n)


@pytest.mark.parametrize("case", ["even", "tall"])
def test_torch_route_is_within_the_same_bar(gold, case, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_CONV3D", "torch")
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    c = case_of(gold, case)
    assert_parity(gold, case, train_step(fresh_model(gold, c["max_disp"]), c), "torch")


def test_optimizer_step_refreshes_the_eval_plans(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    c = case_of(gold, "even")
    model = fresh_model(gold, c["max_disp"])
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    x = igev_volume_train_inputs(device="cuda", requires_grad=False, **c)
    args = (x["match_left"], x["match_right"], x["features"])
    with torch.no_grad():
        before = model.eval()(*args)                     # the eval plans exist before the step
    geo, init = model.train()(*args)
    igev_volume_train_loss(geo, init, x).backward()
    opt.step()
    clone = IGEVCostVolume(c["max_disp"])
    clone.load_state_dict(copy.deepcopy(model.state_dict()))
    with torch.no_grad():
        after, fresh = model.eval()(*args), clone.cuda().eval()(*args)
    assert not torch.equal(before[0], after[0])
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])


def parent_eval_front(m, match_left, match_right, features_left):
    """The eval forward as it stood before the training route existed (_cost_volume and hourglass.forward restated on the
    module's plans)."""
    from diffuvolume_amd.igev_stereo_ddim import _run
    m.refresh_plans()
    stem, classifier = m.plans()
    gwc = stem(build_gwc_volume(match_left, match_right, m.max_disp // 4, 8))
    gwc = m.corr_feature_att(gwc, features_left[0], inplace=True)
    h = m.cost_agg
    p = h.plans()
    conv1 = h.feature_att_8(_run(p["conv1"], gwc), features_left[1], inplace=True)
    conv2 = h.feature_att_16(_run(p["conv2"], conv1), features_left[2], inplace=True)
    conv3 = h.feature_att_32(_run(p["conv3"], conv2), features_left[3], inplace=True)
    conv2 = _run(p["agg_0"], torch.cat((p["conv3_up"](conv3), conv2), dim=1))
    conv2 = h.feature_att_up_16(conv2, features_left[2], inplace=True)
    conv1 = _run(p["agg_1"], torch.cat((p["conv2_up"](conv2), conv1), dim=1))
    conv1 = h.feature_att_up_8(conv1, features_left[1], inplace=True)
    geo = p["conv1_up"](conv1)
    return geo, softmax_regress(classifier(geo)).unsqueeze(1)


def test_eval_and_no_grad_do_what_they_did():
    """On the inputs of tests/golden/igev_volume.npz: eval mode gives the bits of the plan route it always ran (with and
    without grad mode), and train mode under no_grad still refuses its BatchNorm2d, as it did before."""
    g = load_golden("igev_volume")
    m = IGEVCostVolume()
    m.load_state_dict(volume_state_dict(g), strict=True)
    m = m.cuda().eval()
    ml, mr, feats = igev_inputs(int(g["front_seed"]), 1, 8, 32)
    args = (ml.cuda(), mr.cuda(), [f.cuda() for f in feats])
    with torch.no_grad():
        want = parent_eval_front(m, *args)
        got = m(*args)
    got_grad_mode = m(*args)                               # eval with autograd recording: the same route
    for a, b, c in zip(want, got, got_grad_mode):
        assert torch.equal(a, b) and torch.equal(a, c) and not c.requires_grad
    assert float((got[0].cpu().double() - g["geo"].double()).abs().max() / g["geo"].double().abs().max()) < 2e-5
    m.train()
    with torch.no_grad(), pytest.raises(DiffuVolumeError, match="training mode"):
        m(*args)


def test_sizes_off_the_grid_and_cpu_tensors_are_refused(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    model = fresh_model(gold, 64)
    for h, w in ((12, 32), (16, 20)):
        x = igev_volume_train_inputs(seed=1, b=1, h=h, w=w, max_disp=64, device="cuda")
        with pytest.raises(DiffuVolumeError, match="multiples of 8"):
            model(x["match_left"], x["match_right"], x["features"])
    x = igev_volume_train_inputs(seed=1, b=1, h=16, w=32, max_disp=80, device="cuda")
    with pytest.raises(DiffuVolumeError, match="multiples of 8"):
        IGEVCostVolume(80).cuda().train()(x["match_left"], x["match_right"], x["features"])
