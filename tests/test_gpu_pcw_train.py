"""PWCNet_ddim in train mode on the MI355X against one training step of the reference (tests/golden/pcw_train_step.npz,
tools/make_golden_pcw_train.py): the same synthetic weights, inputs and random draws, model_loss_kitti12, backward().

Bar, per stored tensor (loss, the six predictions at the sampled pixels, every parameter's gradient norm and sampled
entries, every BatchNorm running statistic after the step), as relative L2 error against the reference's float64:
    rel(hip) <= 2 * max over the tensors of its kind of rel(reference float32) + 1e-6
(the bar of tests/test_gpu_acv_train.py, for the same reason: in train mode every BatchNorm normalises by batch
statistics, and where one float32 evaluation lands inside the reference's own float32 spread is chance).  The step is
checked with refinenet3 on the HIP 2-D route (the default) and with DV_TRAIN_CONV2D=torch."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, PWCNet_ddim, model_loss_kitti12
from diffuvolume_amd.synth import NoiseTape, _gen, synth_state_dict, synth_stereo_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "pcw_train_step.npz") as z:
        return {k: z[k] for k in z.files}


def inputs(gold):
    """The generator's inputs: images, quarter-resolution disp_net (KITTI12/main.py:148-150), ground truth."""
    b, h, w = (int(v) for v in gold["shape"])
    seed = int(gold["input_seed"])
    x = synth_stereo_batch(b, h, w, seed=seed)
    gt = x["gt"].clone()
    bad = torch.rand(b, h, w, generator=_gen(seed, "train_gt_invalid"))
    gt[bad < 0.05] = 0.0
    gt[bad > 0.97] = 200.0
    disp_net = F.interpolate(torch.clamp(gt, 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    return [t.cuda() for t in (x["left"], x["right"], disp_net, gt)]


def fresh_model(gold):
    model = PWCNet_ddim(192)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=int(gold["weight_seed"])), strict=True)
    return model.cuda().train()


def step(model, gold, monkeypatch):
    """forward + model_loss_kitti12 + backward with the fixture's timestep and q_sample noise."""
    left, right, disp, gt = inputs(gold)
    tape = NoiseTape(int(gold["tape_seed"]))
    t = int(gold["t_step"])
    real_randint = torch.randint
    with monkeypatch.context() as m:
        m.setattr(torch, "randint", lambda low, high, size, *a, device=None, **k:
                  real_randint(t, t + 1, size, device=device))
        m.setattr(torch, "randn_like", lambda x, *a, **k: tape("q", tuple(x.shape), x.dtype).to(x.device))
        outs = model(left, right, None, disp, None)
    loss = model_loss_kitti12(outs, gt, (gt < 192) & (gt > 0))
    loss.backward()
    torch.cuda.synchronize()
    return outs, loss


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


class Bar:
    """Per kind of tensor: every HIP relative error within 2x the worst reference-float32 one of that kind + 1e-6."""

    def __init__(self):
        self.rows = []

    def __call__(self, hip, f32, f64, kind, what):
        self.rows.append((kind, what, rel(hip, f64), rel(f32, f64)))

    def check(self):
        kinds = {k for k, *_ in self.rows}
        bound = {k: 2 * max(r[3] for r in self.rows if r[0] == k) + 1e-6 for k in kinds}
        bad = sorted(((h / bound[k], w) for k, w, h, _ in self.rows if not h <= bound[k]), reverse=True)
        assert not bad, f"{len(bad)} of {len(self.rows)} tensors over the bar {bound}: {bad[:20]}"
        return {k: max(h for kk, _, h, _ in self.rows if kk == k) / bound[k] for k in kinds}


def check_step(gold, model, outs, loss):
    bar = Bar()
    bar(float(loss.detach()), gold["loss_f32"], gold["loss_f64"], "loss", "loss")
    pix = torch.from_numpy(gold["pix_idx"]).cuda()
    for i, p in enumerate(outs):
        bar(p.detach().reshape(-1)[pix].cpu().numpy(), gold[f"pred{i}_f32"], gold[f"pred{i}_f64"], "pred", f"pred{i}")
    params = dict(model.named_parameters())
    for j, name in enumerate(gold["grad_names"]):
        g = params[str(name)].grad
        assert g is not None, name
        bar(float(g.double().norm()), gold["grad_norm_f32"][j], gold["grad_norm_f64"][j], "norm", str(name))
        bar(g.reshape(-1)[torch.from_numpy(gold["grad_idx"][j]).cuda()].cpu().numpy(), gold["grad_val_f32"][j],
            gold["grad_val_f64"][j], "grad", str(name))
    bufs = dict(model.named_buffers())
    for j, name in enumerate(gold["bn_names"]):
        v = bufs[str(name)].reshape(-1)[torch.from_numpy(gold["bn_idx"][j]).cuda()].cpu().numpy()
        bar(v, gold["bn_val_f32"][j], gold["bn_val_f64"][j], "bn", str(name))
    print("largest ratio to the bar per kind:", bar.check())


@pytest.fixture(scope="module")
def stepped(gold):
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("DV_TRAIN_CONV2D", raising=False)
        mp.delenv("DV_TRAIN_CONV3D", raising=False)
        model = fresh_model(gold)
        outs, loss = step(model, gold, mp)
        return model, outs, loss
    finally:
        mp.undo()


def test_step_matches_reference(gold, stepped):
    check_step(gold, *stepped)


def test_single_input_channel_layer_gradient_is_not_rounding_noise(gold, stepped):
    """dispupsample's 1x1 conv has one input channel, so the train-mode BatchNorm behind it cancels its weight gradient
    to almost nothing and a float32 evaluation is mostly rounding noise (the reference's float32: 2e-3 from float64).
    The training path evaluates that layer in float64: its gradient holds float64 to a tenth of that."""
    j = [str(n) for n in gold["grad_names"]].index("dispupsample.0.0.weight")
    g = dict(stepped[0].named_parameters())["dispupsample.0.0.weight"].grad
    idx = torch.from_numpy(gold["grad_idx"][j]).cuda()
    assert rel(g.reshape(-1)[idx].cpu().numpy(), gold["grad_val_f64"][j]) <= 0.1 * rel(gold["grad_val_f32"][j],
                                                                                        gold["grad_val_f64"][j])
    assert rel(float(g.double().norm()), gold["grad_norm_f64"][j]) <= 0.1 * rel(gold["grad_norm_f32"][j],
                                                                                 gold["grad_norm_f64"][j])


def test_six_outputs_of_the_input_size(gold, stepped):
    b, h, w = (int(v) for v in gold["shape"])
    outs = stepped[1]
    assert len(outs) == 6
    for o in outs:
        assert tuple(o.shape) == (b, h, w) and o.dtype == torch.float32 and torch.isfinite(o).all()


def test_time_embedding_gets_no_gradient(gold, stepped):
    model = stepped[0]
    names = {str(n) for n in gold["none_grad_names"]}
    assert names and all(n.startswith("time_embedding.") for n in names)
    for name, p in model.named_parameters():
        assert (p.grad is None) == (name in names), name


def test_batchnorm_statistics_are_updated(gold, stepped):
    model = stepped[0]
    before = fresh_model(gold)
    b0 = dict(before.named_buffers())
    changed = [n for n, v in model.named_buffers() if n.endswith("running_mean") and not torch.equal(v, b0[n])]
    n_bn = sum(1 for n, _ in model.named_buffers() if n.endswith("running_mean"))
    assert len(changed) == n_bn                                     # every BatchNorm of the graph ran in train mode
    assert any(n.startswith("refinenet3.") for n in changed) and any(n.startswith("dres4.") for n in changed)


def test_step_with_torch_refinement_convolutions(gold, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    model = fresh_model(gold)
    outs, loss = step(model, gold, monkeypatch)
    check_step(gold, model, outs, loss)


def test_eval_after_adam_step_uses_fresh_plans(gold, monkeypatch):
    model = fresh_model(gold)
    left, right, disp, _ = inputs(gold)
    used = disp.new_zeros(disp.shape[0], *left.shape[2:]) + 20
    model.eval()
    with torch.no_grad():
        model(left, right, used, disp)                              # plans built pre-step
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    step(model, gold, monkeypatch)
    opt.step()
    model.eval()
    torch.manual_seed(0)
    with torch.no_grad():
        a = model(left, right, used, disp)[0][0]
    clone = PWCNet_ddim(192)
    clone.load_state_dict(copy.deepcopy(model.state_dict()), strict=True)
    clone = clone.cuda().eval()
    torch.manual_seed(0)
    with torch.no_grad():
        b = clone(left, right, used, disp)[0][0]
    assert torch.equal(a, b)


def test_odd_dims_raise_before_the_device(gold):
    model = fresh_model(gold)
    left = torch.zeros(1, 3, 48, 128, device="cuda")                # 48: 1/8 of it is odd at the stride-2 layers
    with pytest.raises(DiffuVolumeError, match="divisible by 32"):
        model(left, left, None, torch.zeros(1, 1, 12, 32, device="cuda"), None)
