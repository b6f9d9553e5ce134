"""IGEV's convex-upsampling head (IGEVUpsampler: spx_2_gru -> spx_gru -> softmax + context_upsample once per GRU
iteration, spx_4 / spx_2 / spx -> the upsampled initial disparity once per pair) in train mode on the MI355X: both
transposed convolutions, the 3x3 over the virtual concatenation and the convex upsampling autograd functions on the HIP
kernels (train2d, ContextUpsampleFn; the once-per-pair spx convolutions on the same functions), BatchNorm /
InstanceNorm / LeakyReLU in PyTorch.

Parity with the reference (tests/golden/igev_upsample_train.npz, tools/make_golden_igev_upsample_train.py: the imported
reference modules in float32 and float64 on one training step, cases `even` B 2, 8 x 16, T 3 and `odd` B 1, 5 x 7, T 2).
Bar per kind of tensor (weights, biases, leaves, outputs), as relative L2 against the fixture's float64:
    rel(hip, f64) <= 2 * ref_err[kind] + 1e-6
with ref_err the worst relative L2 error of the reference's own float32 step for that kind (stored in the fixture).

Measured on the MI355X (worst per kind, weights / biases / leaves / outputs; bars 2.4e-6 / 2.3e-6 / 2.1e-6 / 1.2e-6 for
`even`, 2.1e-6 / 1.8e-6 / 2.1e-6 / 1.2e-6 for `odd`):
    HIP   even 1.0e-6 / 4.4e-7 / 7.8e-7 / 1.0e-7,   odd 8.9e-7 / 5.7e-7 / 7.6e-7 / 1.0e-7
    torch even 9.1e-7 / 4.7e-7 / 7.0e-7 / 9.0e-8,   odd 6.8e-7 / 4.8e-7 / 5.6e-7 / 9.4e-8   (DV_TRAIN_CONV2D=torch)
Chain test (update block -> upsampler, two iterations): HIP against the torch route 1.8e-6 at worst (gate 1e-4)."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError
from diffuvolume_amd.igev_stereo_ddim import IGEVUpsampler, context_upsample
from diffuvolume_amd.synth import (UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, _gen, igev_upsample_state_dict,
                                   igev_upsample_train_inputs, igev_upsample_train_leaves, igev_upsample_train_step,
                                   synth_state_dict, update_train_inputs)

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "leaves", "outputs")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_upsample_train.npz") as z:
        return {k: z[k] for k in z.files}


def case_of(gold, case):
    b, h, w, iters = (int(v) for v in gold[f"{case}_shape"])
    return dict(seed=int(gold[f"{case}_seed"]), b=b, h=h, w=w, iters=iters)


def fresh_model(gold):
    m = IGEVUpsampler()
    m.load_state_dict(igev_upsample_state_dict(m.state_dict(), int(gold["weight_seed"]), float(gold["logit_gain"])),
                      strict=True)
    return m.cuda().train()


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def train_step(model, case, requires_grad=True):
    """forward + loss + backward of the fixture's step -> everything the tests compare, detached."""
    x = igev_upsample_train_inputs(device="cuda", requires_grad=requires_grad, **case)
    loss, init_up, ups = igev_upsample_train_step(model, x)
    loss.backward()
    torch.cuda.synchronize()
    return dict(loss=loss.detach(), init=init_up.detach(), ups=[u.detach() for u in ups],
                grads={n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()},
                leaves={n: t.grad for n, t in igev_upsample_train_leaves(x).items()},
                bn={k: v.clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))})


_RUNS = {}


def hip_run(gold, case, monkeypatch):
    """The HIP route's step of a fixture case, computed once and shared (never modified)."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    if case not in _RUNS:
        _RUNS[case] = train_step(fresh_model(gold), case_of(gold, case))
    return _RUNS[case]


def parity_rows(gold, case, run):
    """-> {kind: [(name, rel(ours, f64))]} over everything the fixture stores."""
    g = lambda key: gold[f"{case}_{key}"]
    rows = {k: [] for k in KINDS}
    rows["outputs"].append(("loss", rel(float(run["loss"]), g("loss_f64"))))
    idx = torch.from_numpy(g("up_idx")).cuda()
    shape = tuple(int(v) for v in g("up_shape"))
    assert tuple(run["init"].shape) == shape and all(tuple(u.shape) == shape for u in run["ups"])
    rows["outputs"].append(("init", rel(run["init"].reshape(-1)[idx].cpu().numpy(), g("init_f64"))))
    for i, u in enumerate(run["ups"]):
        rows["outputs"].append((f"up{i}", rel(u.reshape(-1)[idx].cpu().numpy(), g("up_f64")[i])))
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


@pytest.mark.parametrize("case", ["even", "odd"])
def test_step_matches_reference(gold, case, monkeypatch):
    run = hip_run(gold, case, monkeypatch)
    assert all(g is not None for g in run["grads"].values())
    assert_parity(gold, case, run, "hip")


@pytest.mark.parametrize("case", ["even", "odd"])
def test_frozen_leaves_still_train_the_weights(gold, case, monkeypatch):
    ref = hip_run(gold, case, monkeypatch)
    run = train_step(fresh_model(gold), case_of(gold, case), requires_grad=False)
    assert all(g is None for g in run["leaves"].values())
    assert torch.equal(run["loss"], ref["loss"])
    for n, g in ref["grads"].items():
        assert torch.equal(run["grads"][n], g), n


@pytest.mark.parametrize("case", ["even", "odd"])
def test_two_steps_give_the_same_bits(gold, case, monkeypatch):
    ref = hip_run(gold, case, monkeypatch)
    run = train_step(fresh_model(gold), case_of(gold, case))
    assert torch.equal(run["loss"], ref["loss"]) and torch.equal(run["init"], ref["init"])
    assert all(torch.equal(a, b) for a, b in zip(run["ups"], ref["ups"]))
    for group in ("grads", "leaves", "bn"):
        for n, g in ref[group].items():
            assert torch.equal(run[group][n], g), (group, n)


@pytest.mark.parametrize("case", ["even", "odd"])
def test_torch_route_is_within_the_same_bar(gold, case, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    assert_parity(gold, case, train_step(fresh_model(gold), case_of(gold, case)), "torch")


def test_optimizer_step_refreshes_the_eval_plans(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    c = case_of(gold, "even")
    model = fresh_model(gold)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    x = igev_upsample_train_inputs(device="cuda", requires_grad=False, **c)
    args = (x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])
    with torch.no_grad():
        before = model.eval()(*args)                     # the eval plans exist before the step
    model.train()
    first = model(*args)                                 # the train plans exist before the step
    igev_upsample_train_step(model, x)[0].backward()
    opt.step()
    stepped = model(*args)                               # train mode after the step: the new weights
    clone = IGEVUpsampler()
    clone.load_state_dict(copy.deepcopy(model.state_dict()))
    with torch.no_grad():
        after, fresh = model.eval()(*args), clone.cuda().eval()(*args)
    assert not torch.equal(before, after) and not torch.equal(first, stepped)
    assert torch.equal(after, fresh)


def parent_upsample_disp(m, disp, mask_feat_4, stem_2x):
    """`upsample_disp` as it stood before the training route existed (IGEVStereo_ddim.upsample_disp restated on the
    module's plans)."""
    up, mix, head = m.plans()
    x = up(mask_feat_4)
    if x.shape != stem_2x.shape:
        x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
    spx_pred = head(mix([x, stem_2x]))
    return context_upsample(disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


def test_eval_and_no_grad_do_what_they_did(gold):
    """Eval mode gives the bits of the plan route it always ran (with and without grad mode), and agrees with the
    reference's eval expression; train mode under no_grad refuses its BatchNorm2d."""
    c = case_of(gold, "odd")
    m = fresh_model(gold).eval()
    x = igev_upsample_train_inputs(device="cuda", requires_grad=False, **c)
    args = (x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])
    with torch.no_grad():
        want = parent_upsample_disp(m, *args)
        got = m(*args)
        ref = context_upsample(args[0], m.spx_gru(m.spx_2_gru.conv2(torch.cat((m.spx_2_gru.conv1(args[1]), args[2]), 1))),
                               scale=4.0, apply_softmax=True).unsqueeze(1)
        init = m.init_forward(x["feat0"], x["stem_2x"], x["init_disp"])
    got_grad_mode = m(*args)                               # eval with autograd recording: the same route
    assert torch.equal(want, got) and torch.equal(want, got_grad_mode) and not got_grad_mode.requires_grad
    assert float((got - ref).abs().max() / ref.abs().max()) < 2e-5
    assert init.shape == got.shape and not init.requires_grad and torch.isfinite(init).all()
    m.train()
    with torch.no_grad(), pytest.raises(DiffuVolumeError, match="training mode"):
        m(*args)
    m.spx_2_gru.conv1.bn.eval(), m.spx_2_gru.conv2.bn.eval()      # the reference's freeze_bn(): the plan route again
    with torch.no_grad():
        assert torch.equal(m(*args), want)


def test_refusals(gold, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    c = case_of(gold, "odd")
    m = fresh_model(gold)
    x = igev_upsample_train_inputs(device="cuda", **c)
    args = (x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])
    for dt in (torch.float16, torch.bfloat16):
        with torch.autocast("cuda", dtype=dt), pytest.raises(DiffuVolumeError, match="autocast"):
            m(*args)
        with torch.autocast("cuda", dtype=dt), pytest.raises(DiffuVolumeError, match="autocast"):
            m.init_forward(x["feat0"], x["stem_2x"], x["init_disp"])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        m(args[0].detach().cpu(), args[1], args[2])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        m(args[0], args[1], args[2].detach().cpu())
    with pytest.raises(RuntimeError, match="up_weights"):                       # logits that are not [B,9,4h,4w]
        context_upsample(x["disp"][0], torch.zeros(1, 9, 20, 24, device="cuda", requires_grad=True), 4.0, True)
    with pytest.raises(RuntimeError, match="up_weights"):                       # a disparity of another plane
        m(x["disp"][0][:, :, :4], args[1], args[2])


def test_model_upsample_disp_trains_and_forward_still_refuses(gold, monkeypatch):
    """IGEVStereo_ddim.upsample_disp delegates to the same function: in train mode it gives the module's bits and
    gradients; IGEVStereo_ddim.forward keeps refusing train mode."""
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    from diffuvolume_amd.synth import StubMobileNetV2
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    c = case_of(gold, "odd")
    ref = fresh_model(gold)
    args = dict(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2, corr_radius=4,
                slow_fast_gru=False, max_disp=192, mixed_precision=False)
    model = IGEVStereo_ddim(types.SimpleNamespace(**args), feature=Feature(StubMobileNetV2()))
    model.load_state_dict(ref.state_dict(), strict=False)
    model = model.cuda().train()
    outs = []
    for m in (ref, model):
        x = igev_upsample_train_inputs(device="cuda", **c)
        up = (m if m is ref else m.upsample_disp)(x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])
        (up - x["gt"]).abs().mean().backward()
        outs.append((up.detach(), x["disp"][0].grad, x["mask_feat_4"][0].grad, m.spx_gru[0].weight.grad,
                     m.spx_2_gru.conv1.conv.weight.grad))
    for a, b in zip(*outs):
        assert a is not None and torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="inference-only"):
        model(torch.zeros(1, 3, 64, 128, device="cuda"), torch.zeros(1, 3, 64, 128, device="cuda"),
              torch.zeros(1, 1, 64, 128, device="cuda"), torch.zeros(1, 1, 16, 32, device="cuda"))


def chain_step(block_sd, up_sd, x, stem_2x, gt):
    """Two iterations of the reference's train loop (igev_stereo_ddim.py:441-457) on the update block and the upsampling
    head, a full-resolution L1 loss per iteration -> the update block's gradients."""
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    block = BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)
    block.load_state_dict(block_sd, strict=True)
    ups = IGEVUpsampler()
    ups.load_state_dict(up_sd, strict=True)
    block, ups = block.cuda().train(), ups.cuda().train()
    net, disp, loss = list(x["net"]), x["disp"], 0.0
    for i in range(len(x["corr"])):
        disp = disp.detach()
        net, mask_feat_4, delta = block(net, x["inp"], x["corr"][i], disp, iter16=True, iter08=True)
        disp = disp + delta
        loss = loss + (ups(disp, mask_feat_4, stem_2x) - gt).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad for n, p in block.named_parameters()}


def test_update_block_trains_through_the_upsampler(gold, monkeypatch):
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    b, h, w = 1, 8, 16
    template = BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)
    block_sd = synth_state_dict(template.state_dict(), seed=7)
    up_sd = igev_upsample_state_dict(IGEVUpsampler().state_dict(), int(gold["weight_seed"]), float(gold["logit_gain"]))
    stem_2x = torch.randn(b, 32, 2 * h, 2 * w, generator=_gen(61, "stem_2x")).cuda()
    gt = (torch.randn(b, 1, 4 * h, 4 * w, generator=_gen(61, "gt")).abs() * 16 + 1).cuda()
    inputs = lambda: update_train_inputs(61, b, h, w, 2, device="cuda")
    first = chain_step(block_sd, up_sd, inputs(), stem_2x, gt)
    again = chain_step(block_sd, up_sd, inputs(), stem_2x, gt)
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    torch_route = chain_step(block_sd, up_sd, inputs(), stem_2x, gt)
    worst = ("", 0.0)
    for n, g in first.items():
        assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0, n     # mask feature and delta_disp reach it
        assert torch.equal(g, again[n]), n
        e = rel(g.cpu().numpy(), torch_route[n].double().cpu().numpy())
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e <= 1e-4, (n, e)
    print(f"PARITY chain hip against torch route: worst {worst[1]:.3e} ({worst[0]})")
