"""The training routes on the differentiable cost-volume builders (train_volume.py; DV_TRAIN_VOLUME): the autograd graphs
of ACVNet_DDIM.train_forward and PWCNet_ddim.train_forward hold the new functions' backward nodes on the default route and
none with DV_TRAIN_VOLUME=torch; IGEVCostVolume in train mode holds none on either: its call site stays on the PyTorch
statement, because with the eval kernel's forward (8.97e-8 relative L2 from the statement's) the recorded step `even` of
test_gpu_igev_volume_train.py leaves its bar -- every gradient in front of cost_agg.agg_1.2 lands 1.2e-3 .. 3.8e-3 from
float64 against bars of 7.4e-6 .. 1.2e-5, the layers behind it stay at 3e-6 -- and that bar is not this file's to move.
A frozen IGEV backbone gives the same bits, and the volume stage of each model -- features as leaves -> volumes -> a fixed random linear loss -- gives the same gradient
bits on two backward passes from the same state.  Sizes: the smallest the training routes accept (a 64 x 160 / 64 x 128
pair, an 8 x 16 quarter-resolution plane); the graph checks need only the forward.  Parity of whole training steps on this
route with the reference's recorded steps is held by test_gpu_acv_train / test_gpu_pcw_train / test_gpu_igev_volume_train."""
import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import (ACVNet_DDIM, PWCNet_ddim, build_concat_volume, build_concat_volume_train, build_gwc_volume,
                             build_gwc_volume_train)
from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume
from diffuvolume_amd.synth import igev_volume_train_inputs, synth_state_dict, synth_stereo_batch

pytestmark = pytest.mark.gpu
NODES = ("GwcVolumeFnBackward", "ConcatVolumeFnBackward")


def backward_nodes(*outs):
    """Names of all nodes of the autograd graph below `outs`."""
    seen, names = set(), []
    stack = [o.grad_fn for o in outs if o.grad_fn is not None]
    while stack:
        fn = stack.pop()
        if fn in seen:
            continue
        seen.add(fn)
        names.append(fn.name())
        stack.extend(f for f, _ in fn.next_functions if f is not None)
    return names


def count(names):
    return tuple(sum(n == node for n in names) for node in NODES)


def seeded(model, seed):
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed), strict=True)
    return model.cuda().train()


def pair_forward(model, h, w, quarter_disp):
    x = synth_stereo_batch(1, h, w, seed=3)
    disp = x["disp"]
    if quarter_disp:                        # PWCNet_ddim trains on the quarter-resolution disparity
        disp = F.interpolate(torch.clamp(x["gt"], 0, 191).unsqueeze(1), size=(h // 4, w // 4), mode="bilinear") / 4
    return model(x["left"].cuda(), x["right"].cuda(), None, disp.cuda(), None)


def igev_forward(model, requires_grad=True):
    x = igev_volume_train_inputs(seed=5, b=1, h=8, w=16, max_disp=64, device="cuda", requires_grad=requires_grad)
    return model(x["match_left"], x["match_right"], x["features"])


@pytest.fixture(scope="module")
def models():
    return dict(acv=seeded(ACVNet_DDIM(192), 11), pcw=seeded(PWCNet_ddim(192), 12), igev=seeded(IGEVCostVolume(64), 13))


FORWARD = {
    # model -> (forward, (gwc nodes, concat nodes) on the default route)
    "acv": (lambda m: pair_forward(m, 64, 160, False), (1, 1)),     # the un-filtered volume is built under no_grad
    "pcw": (lambda m: pair_forward(m, 64, 128, True), (4, 4)),      # four scales
    "igev": (lambda m: igev_forward(m), (0, 0)),                   # stays on the statement: see the module docstring
}


@pytest.mark.parametrize("which", list(FORWARD))
def test_graph_holds_the_new_backward_nodes_on_the_default_route_only(models, which, monkeypatch):
    forward, expected = FORWARD[which]
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    assert count(backward_nodes(*forward(models[which]))) == expected
    monkeypatch.setenv("DV_TRAIN_VOLUME", "torch")
    assert count(backward_nodes(*forward(models[which]))) == (0, 0)


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_igev_geo_bits_do_not_depend_on_requires_grad(models, route, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_VOLUME", route)
    geo, init = igev_forward(models["igev"], requires_grad=True)
    geo_frozen, init_frozen = igev_forward(models["igev"], requires_grad=False)
    assert geo.requires_grad and geo_frozen.requires_grad          # the weights still want their gradients
    assert torch.equal(geo.detach(), geo_frozen.detach()) and torch.equal(init.detach(), init_frozen.detach())


def leaves(gen, *shapes):
    return [torch.randn(*s, generator=gen).cuda().requires_grad_(True) for s in shapes]


def acv_stage(gen):
    """ACVNet_DDIM.train_forward's volumes at a 64 x 160 pair: gwc 320 channels in 40 groups, the concat volume times
    softmax(att) * noisy."""
    fl, fr, cl, cr, att = leaves(gen, (1, 320, 16, 40), (1, 320, 16, 40), (1, 32, 16, 40), (1, 32, 16, 40), (1, 1, 48, 16, 40))
    noisy = torch.rand(1, 1, 48, 16, 40, generator=gen).cuda()
    vols = [build_gwc_volume(fl, fr, 48, 40),
            build_concat_volume_train(cl, cr, 48, scale=(F.softmax(att, dim=2) * noisy)[:, 0])]
    return [fl, fr, cl, cr, att], vols


def pcw_stage(gen):
    """PWCNet_ddim.train_forward's volumes at a 64 x 128 pair: gwc and zero_left concat at 1/4 .. 1/32."""
    ins, vols = [], []
    for div in (4, 8, 16, 32):
        h, w, d = 64 // div, 128 // div, 192 // div
        fl, fr, cl, cr = leaves(gen, (1, 320, h, w), (1, 320, h, w), (1, 12, h, w), (1, 12, h, w))
        ins += [fl, fr, cl, cr]
        vols += [build_gwc_volume(fl, fr, d, 40), build_concat_volume(cl, cr, d, zero_left=True)]
    return ins, vols


def igev_stage(gen):
    ml, mr = leaves(gen, (1, 96, 8, 16), (1, 96, 8, 16))
    return [ml, mr], [build_gwc_volume_train(ml, mr, 16, 8)]


@pytest.mark.parametrize("stage", [acv_stage, pcw_stage, igev_stage])
def test_two_backward_passes_of_the_volume_stage_repeat_bit_for_bit(stage, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    gen = torch.Generator().manual_seed(21)
    ins, vols = stage(gen)
    assert sum(count(backward_nodes(*vols))) == len(vols)
    weights = [torch.randn(v.shape, generator=gen).cuda() for v in vols]          # the fixed random linear loss
    loss = sum((v * w).sum() for v, w in zip(vols, weights))
    first = torch.autograd.grad(loss, ins, retain_graph=True)
    again = torch.autograd.grad(loss, ins)
    for i, (a, b) in enumerate(zip(first, again)):
        assert a is not None and bool(a.abs().sum() > 0), i
        assert torch.equal(a, b), i
