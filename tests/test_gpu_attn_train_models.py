"""ACVNet_DDIM training steps with the hourglasses' bottleneck window attention on the fused HIP kernels (DV_TRAIN_ATTN=hip)
and on the PyTorch statements (DV_TRAIN_ATTN=torch), on the recorded step of test_gpu_acv_train.py (its `fresh_model`, `step`
and checks are used as they are).  PWCNet_ddim and IGEV have no attention block.

The module runs one step per route, once, and the tests below read those."""
import gc

import numpy as np
import pytest
import torch

import test_gpu_acv_train as acv_t
from diffuvolume_amd import window_attention_train

pytestmark = pytest.mark.gpu

FN = "WindowAttentionFnBackward"
HOURGLASSES = ("dres2_att_", "dres2", "dres3")
ATTN = tuple(f"{h}.attention_block.{p}" for h in HOURGLASSES
             for p in ("qkv_3d.weight", "qkv_3d.bias", "final1x1.weight", "final1x1.bias"))


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


def one_step(gold, route):
    gc.collect()
    torch.cuda.empty_cache()
    model = acv_t.fresh_model(gold)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DV_TRAIN_ATTN", route)
        outs, loss = acv_t.step(model, gold, mp)
    return dict(model=model, outs=[o.detach() for o in outs], loss=loss.detach(), found=in_graph(outs[0].grad_fn, FN))


@pytest.fixture(scope="module")
def steps():
    from conftest import GOLDEN
    with np.load(GOLDEN / "acv_train_step.npz") as z:
        gold = {k: z[k] for k in z.files}
    return gold, {"hip": one_step(gold, "hip"), "torch": one_step(gold, "torch")}


def test_the_function_is_in_the_graph_on_hip_and_not_on_torch(steps):
    _, runs = steps
    assert runs["hip"]["found"] and not runs["torch"]["found"]
    for r in runs.values():
        grads = dict(r["model"].named_parameters())
        mine = [n for n in grads if ".attention_block." in n and n.split(".")[0] in HOURGLASSES]
        assert set(ATTN) <= set(mine)
        assert all(grads[n].grad is not None and bool((grads[n].grad != 0).any()) for n in mine)
    assert list(runs["hip"]["model"].state_dict()) == list(runs["torch"]["model"].state_dict())


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_recorded_training_step_on_both_routes(steps, route):
    gold, runs = steps
    r = runs[route]
    acv_t.test_step_matches_reference(gold, (r["model"], r["outs"], r["loss"]))


def test_the_same_input_twice_gives_the_attention_gradients_bit_for_bit(steps, monkeypatch):
    """The call site's expression on the model's own parameters, fed one bottleneck tensor and one cotangent twice."""
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    gold, runs = steps
    ab = runs["hip"]["model"].dres2.attention_block
    b, h, w = (int(v) for v in gold["shape"])
    gen = torch.Generator().manual_seed(43)
    c4 = torch.randn(b, 128, 12, h // 16, w // 16, generator=gen).cuda()
    g = torch.randn(c4.shape, generator=gen).cuda()
    params = [ab.qkv_3d.weight, ab.qkv_3d.bias, ab.final1x1.weight, ab.final1x1.bias]
    got = []
    for _ in range(2):
        x = c4.clone().requires_grad_(True)
        out = window_attention_train(x, *params, ab.num_heads)
        assert out.grad_fn.name() == FN
        got.append(torch.autograd.grad(out, [x] + params, g))
    assert [tuple(t.shape) for t in got[0][1:]] == [tuple(p.shape) for p in params]
    assert all(bool((t != 0).any()) for t in got[0])
    assert all(torch.equal(p, q) for p, q in zip(*got))
