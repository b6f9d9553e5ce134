"""ACVNet_DDIM and PWCNet_ddim training steps with their 2-D networks on the HIP route (DV_TRAIN_NET2D=hip) and on the
nn.Modules (DV_TRAIN_NET2D=torch), on the recorded steps of test_gpu_acv_train.py / test_gpu_pcw_train.py (their
`fresh_model`, `step` and checks are used as they are).

Per model the module runs two steps on `hip` and one on `torch`, once, and every test below reads those.  No step sets
`torch.backends.cudnn.deterministic`: on `hip` no convolution, BatchNorm or resize of the step is MIOpen's or ATen's choice,
and that nothing depends on such a choice is what the repeat test is about -- the loss, the outputs, EVERY parameter
gradient (291 for ACV, 452 for PCW) and every BatchNorm buffer have the same bits on both `hip` steps."""
import gc

import pytest
import torch

import test_gpu_acv_train as acv_t
import test_gpu_pcw_train as pcw_t
from test_gpu_norm_train_models import in_graph, load

pytestmark = pytest.mark.gpu

COUNTS = {"acv": 291, "pcw": 452}
# PyTorch operators on a gradient's path that this route does not own, by parameter-name prefix.  None: every gradient of
# both models repeats.  (Nothing under `feature_extraction.` or `refinenet3.` may ever be listed.)
NOT_OWNED = {"acv": {}, "pcw": {}}


def one_step(t, gold, route):
    gc.collect()
    torch.cuda.empty_cache()
    model = t.fresh_model(gold)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DV_TRAIN_NET2D", route)
        for k in ("DV_TRAIN_NORM", "DV_TRAIN_CONV2D", "DV_TRAIN_CONV3D", "DV_TRAIN_TAIL", "DV_TRAIN_VOLUME",
                  "DV_TRAIN_REFINE", "DV_TRAIN_PATCH", "DV_TRAIN_ATTN"):
            mp.delenv(k, raising=False)
        assert torch.backends.cudnn.deterministic is False
        outs, loss = t.step(model, gold, mp)
    found = {fn: in_graph(outs[-1].grad_fn, fn) for fn in ("ConvCatFnBackward", "ResizeBilinearFnBackward")}
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return dict(model=model, outs=[o.detach() for o in outs], loss=loss.detach(), found=found, grads=grads)


@pytest.fixture(scope="module", params=["acv", "pcw"])
def steps(request):
    t = acv_t if request.param == "acv" else pcw_t
    gold = load(t)
    runs = {"hip": one_step(t, gold, "hip"), "torch": one_step(t, gold, "torch"), "hip2": one_step(t, gold, "hip")}
    return request.param, t, gold, runs


def test_the_functions_are_in_the_graph_on_hip_and_not_on_torch(steps):
    which, _, _, runs = steps
    for name in ("hip", "hip2"):
        assert runs[name]["found"]["ConvCatFnBackward"], which
        assert runs[name]["found"]["ResizeBilinearFnBackward"] == (which == "pcw")
    assert not any(runs["torch"]["found"].values()), which


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_recorded_training_step_on_both_routes(steps, route):
    which, t, gold, runs = steps
    r = runs[route]
    if which == "pcw":
        t.check_step(gold, r["model"], r["outs"], r["loss"])
    else:
        t.test_step_matches_reference(gold, (r["model"], r["outs"], r["loss"]))
    tracked = {n: int(v) for n, v in r["model"].named_buffers() if n.endswith("num_batches_tracked")}
    assert tracked == {n: int(v) for n, v in runs["torch"]["model"].named_buffers() if n.endswith("num_batches_tracked")}
    assert min(v for n, v in tracked.items() if n.startswith("feature_extraction.")) == 2      # left and right image


def test_two_hip_steps_give_the_same_bits_everywhere(steps):
    which, _, _, runs = steps
    a, b = runs["hip"], runs["hip2"]
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"]))
    names = sorted(a["grads"])
    assert names == sorted(b["grads"]) and len(names) == COUNTS[which], len(names)
    differ = [n for n in names if not torch.equal(a["grads"][n], b["grads"][n])]
    allowed = tuple(NOT_OWNED[which])
    assert not any(p.startswith(("feature_extraction.", "refinenet3.")) for p in allowed)
    left = [n for n in differ if not (allowed and n.startswith(allowed))]
    assert not left, f"{which}: {len(left)} of {len(names)} gradients differ: {left[:12]}"
    bufs_a, bufs_b = dict(a["model"].named_buffers()), dict(b["model"].named_buffers())
    bn = [n for n in bufs_a if n.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert len(bn) >= 150
    differ = [n for n in bn if not torch.equal(bufs_a[n], bufs_b[n])]
    assert not differ, f"{which}: {len(differ)} BatchNorm buffers differ: {differ[:12]}"
