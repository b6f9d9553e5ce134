"""ACVNet_DDIM and PWCNet_ddim training steps with the BatchNorm3d + activation of their 3-D stacks on the fused HIP
kernels (DV_TRAIN_NORM=hip) and on the PyTorch statement (DV_TRAIN_NORM=torch), on the recorded steps of
test_gpu_acv_train.py / test_gpu_pcw_train.py (their `fresh_model`, `step` and checks are used as they are).

Per model the module runs two steps on `hip` and one on `torch`, once, and every test below reads those.  The steps run with
`torch.backends.cudnn.deterministic = True`: MIOpen's default choice for a stride-2 convolution of PWCNet_ddim's feature
extractor does not give the same bits twice (tests/test_gpu_train_tail_models.py), and the repeat test below is about the
3-D stacks, whose inputs must repeat for it to say anything."""
import gc

import pytest
import torch
from torch import nn

import test_gpu_acv_train as acv_t
import test_gpu_pcw_train as pcw_t

pytestmark = pytest.mark.gpu

FN = "BatchNormActFnBackward"


def in_graph(fn, name):
    seen, stack = set(), [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if f.name() == name:
            return True
        stack.extend(g for g, _ in f.next_functions)
    return False


def stack_parameters(model):
    """name -> parameter of the 3-D stacks: every Conv3d, ConvTranspose3d and BatchNorm3d of the model."""
    out = {}
    for mname, m in model.named_modules():
        if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d, nn.BatchNorm3d)):
            out.update({f"{mname}.{k}": p for k, p in m.named_parameters(recurse=False)})
    return out


def one_step(t, gold, route):
    gc.collect()
    torch.cuda.empty_cache()
    model = t.fresh_model(gold)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DV_TRAIN_NORM", route)
        mp.setattr(torch.backends.cudnn, "deterministic", True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rest = torch.cuda.memory_allocated()
        outs, loss = t.step(model, gold, mp)
        peak = torch.cuda.max_memory_allocated() - rest
    found = in_graph(outs[-1].grad_fn, FN)
    grads = {k: p.grad.clone() for k, p in stack_parameters(model).items() if p.grad is not None}
    return dict(model=model, outs=[o.detach() for o in outs], loss=loss.detach(), peak=peak, found=found, grads=grads)


def load(t):
    import numpy as np
    from conftest import GOLDEN
    with np.load(GOLDEN / ("acv_train_step.npz" if t is acv_t else "pcw_train_step.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module", params=["acv", "pcw"])
def steps(request):
    t = acv_t if request.param == "acv" else pcw_t
    gold = load(t)
    runs = {"hip": one_step(t, gold, "hip"), "torch": one_step(t, gold, "torch"), "hip2": one_step(t, gold, "hip")}
    return request.param, t, gold, runs


def test_the_function_is_in_the_graph_on_hip_and_not_on_torch(steps):
    which, _, _, runs = steps
    assert runs["hip"]["found"] and runs["hip2"]["found"] and not runs["torch"]["found"], which


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_recorded_training_step_on_both_routes(steps, route):
    which, t, gold, runs = steps
    r = runs[route]
    if which == "pcw":
        t.check_step(gold, r["model"], r["outs"], r["loss"])
    else:
        t.test_step_matches_reference(gold, (r["model"], r["outs"], r["loss"]))
    # the modules count their batches as on the PyTorch route (ACV's stacks up to dres1 twice: the unfiltered pass is first)
    tracked = {n: int(v) for n, v in r["model"].named_buffers() if n.endswith("num_batches_tracked")}
    assert tracked == {n: int(v) for n, v in runs["torch"]["model"].named_buffers() if n.endswith("num_batches_tracked")}
    assert max(tracked.values()) >= 1


def test_two_hip_steps_give_the_same_bits_in_the_3d_stacks(steps):
    which, _, _, runs = steps
    a, b = runs["hip"], runs["hip2"]
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(x, y) for x, y in zip(a["outs"], b["outs"]))
    names = sorted(a["grads"])
    assert names == sorted(b["grads"])
    bn = [n for n, p in stack_parameters(a["model"]).items() if p.dim() == 1 and n in a["grads"]]
    assert len(bn) >= 20, len(bn)                                            # BatchNorm weights and biases are among them
    differ = [n for n in names if not torch.equal(a["grads"][n], b["grads"][n])]
    assert not differ, f"{which}: {len(differ)} of {len(names)} differ: {differ[:10]}"
    bufs_a, bufs_b = dict(a["model"].named_buffers()), dict(b["model"].named_buffers())
    stack_bn = [n for n, m in a["model"].named_modules() if isinstance(m, nn.BatchNorm3d)]
    for n in stack_bn:
        for k in ("running_mean", "running_var"):
            assert torch.equal(bufs_a[f"{n}.{k}"], bufs_b[f"{n}.{k}"]), (n, k)


def test_step_peak_memory_of_pcw_is_lower_on_hip(steps):
    """PyTorch keeps the normalised tensor, softplus and tanh of every Mish layer for its backward; the HIP route keeps the
    convolution output alone.  (ACV's ReLU layers keep the same two tensors on both routes: printed, not asserted.)"""
    which, _, gold, runs = steps
    hip, ref = runs["hip"]["peak"], runs["torch"]["peak"]
    print(f"{which} step at {tuple(int(v) for v in gold['shape'])}: peak above rest {hip / 2 ** 20:.1f} MiB on hip, "
          f"{ref / 2 ** 20:.1f} MiB on torch")
    assert which != "pcw" or hip < ref
