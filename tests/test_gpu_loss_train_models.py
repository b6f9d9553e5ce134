"""The recorded training steps of the three models with their loss on the fused HIP route (DV_TRAIN_LOSS=hip), on the
helpers of test_gpu_acv_train.py / test_gpu_pcw_train.py / test_gpu_igev_train_step.py as they are: the steps hold the bars
those tests state, the fused function is what the loss's graph ends in, and two steps from the same state give the same
loss and gradient bits.  ACV and PCW run with DV_TRAIN_NET2D=hip as well, the setting under which every one of their
gradients repeats (test_gpu_net2d_train_models.py)."""
import gc

import pytest
import torch

import test_gpu_acv_train as acv_t
import test_gpu_igev_train_step as igev_t
import test_gpu_pcw_train as pcw_t
from test_gpu_norm_train_models import load

pytestmark = pytest.mark.gpu


def one_step(t, gold):
    gc.collect()
    torch.cuda.empty_cache()
    model = t.fresh_model(gold)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DV_TRAIN_LOSS", "hip")
        mp.setenv("DV_TRAIN_NET2D", "hip")
        outs, loss = t.step(model, gold, mp)
    assert "MaskedLossFn" in loss.grad_fn.name()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return dict(model=model, outs=[o.detach() for o in outs], loss=loss.detach(), grads=grads)


@pytest.fixture(scope="module", params=["acv", "pcw"])
def steps(request):
    t = acv_t if request.param == "acv" else pcw_t
    gold = load(t)
    return request.param, t, gold, [one_step(t, gold), one_step(t, gold)]


def test_recorded_step_holds_its_bars_on_the_fused_loss(steps):
    which, t, gold, runs = steps
    r = runs[0]
    if which == "pcw":
        t.check_step(gold, r["model"], r["outs"], r["loss"])
    else:
        t.test_step_matches_reference(gold, (r["model"], r["outs"], r["loss"]))


def test_two_steps_give_the_same_loss_and_gradient_bits(steps):
    which, _, _, (a, b) = steps
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"]))
    assert sorted(a["grads"]) == sorted(b["grads"]) and len(a["grads"]) > 200
    differ = [n for n in a["grads"] if not torch.equal(a["grads"][n], b["grads"][n])]
    assert not differ, f"{which}: {len(differ)} of {len(a['grads'])} gradients differ: {differ[:12]}"


def test_igev_recorded_step_and_repeat_on_the_fused_loss(monkeypatch):
    with igev_t.np.load(igev_t.GOLDEN / "igev_train_step.npz") as z:
        gold = {k: z[k] for k in z.files}
    monkeypatch.setenv("DV_TRAIN_LOSS", "hip")
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    calls = []
    real = igev_t.sequence_loss
    monkeypatch.setattr(igev_t, "sequence_loss", lambda *a, **k: calls.append(real(*a, **k)) or calls[-1])
    runs = [igev_t.train_step(igev_t.fresh_model(gold), igev_t.case_of(gold)) for _ in range(2)]
    assert len(calls) == 2 and all("MaskedLossFn" in loss.grad_fn.name() for loss, _ in calls)
    assert all(isinstance(v, float) for _, m in calls for v in m.values())
    igev_t.assert_parity(gold, runs[0], "hip loss")
    a, b = runs
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["init"], b["init"])
    assert all(torch.equal(x, y) for x, y in zip(a["preds"], b["preds"]))
    for n, g in a["grads"].items():
        assert (g is None and b["grads"][n] is None) or torch.equal(b["grads"][n], g), n
