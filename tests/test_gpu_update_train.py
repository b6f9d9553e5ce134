"""IGEV's update block in train mode on the MI355X (update.BasicMultiUpdateBlock, train2d.ConvGRUFn / ConvCatFn).

Parity with the reference (tests/golden/update_train_loop.npz, tools/make_golden_update_train.py: the imported reference
block in float32 and float64 on an unrolled loop, cases `even` 16 x 32 T = 6 and `ragged` 20 x 28 T = 4).  Bar per kind
of tensor (weights, biases, leaves, outputs), as relative L2 against the fixture's float64:
    rel <= min(max(2 * worst reference-float32 error of that kind, 1e-5), 1e-4)
twice the reference float32's own error (the rule of the ACV and PCW steps), not below 1e-5 -- the error at which
tests/test_gpu_wino3.py accepts the Winograd kernels the forward and the input gradients run on -- and never above the
fixture's gate.  The HIP route is held to it; the errors of both routes (HIP, DV_TRAIN_CONV2D=torch) are printed.

Measured on the MI355X (worst per kind, weights / biases / leaves / outputs; reference float32 2.7e-6 / 3.7e-6 / 2.1e-6 /
1.6e-6):   HIP   even 3.2e-6 / 1.2e-6 / 3.4e-6 / 2.6e-6,   ragged 2.9e-6 / 8.8e-7 / 2.3e-6 / 1.8e-6
           torch even 2.6e-3 / 4.9e-4 / 3.5e-6 / 2.8e-6,   ragged 2.6e-6 / 9.8e-7 / 2.3e-6 / 2.0e-6
The torch route's figures depend on the run: its `ragged` weights came out between 2.61e-6 and 2.68e-6 over six runs, and
`even` gave 2.6e-3 / 4.9e-4 in every process that ran it first but 3.1e-6 / 1.5e-6 once in a process that had timed other
convolutions before it (MIOpen picks its solver from what the process has seen).  Where 2.6e-3 appears it is one ReLU
that lands on the other side of zero: ONE of the 130 048 outputs of encoder.conv in iteration 3 (float64 pre-activation
6.9e-6, next to values up to 14) comes out <= 0, which removes that element's gradient from the four encoder layers
below it (convc1 / convc2 / convd1 / convd2; everything else stays at 3e-6).  That is the conditioning the generator's
docstring describes, met by another float32 evaluation order than the reference's own; it is why the torch route is
printed and not asserted.  The HIP route's kernels sum in a fixed order: its figures are the same on every run."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _lib, train2d
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import (UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, synth_state_dict, update_train_inputs,
                                   update_train_loop)
from diffuvolume_amd.update import BasicMultiUpdateBlock

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "leaves", "outputs")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "update_train_loop.npz") as z:
        return {k: z[k] for k in z.files}


def fresh_block(seed=7, n_gru_layers=3):
    args = types.SimpleNamespace(**{**UPDATE_TRAIN_ARGS, "n_gru_layers": n_gru_layers})
    m = BasicMultiUpdateBlock(args, hidden_dims=UPDATE_TRAIN_HIDDEN)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=seed), strict=True)
    return m.cuda().train()


def rel(a, ref):
    a, ref = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (a, ref))
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def leaves_of(x):
    d = {f"net{i}": t for i, t in enumerate(x["net"])}
    d.update({f"inp{i}{j}": t for i, lv in enumerate(x["inp"]) for j, t in enumerate(lv)})
    return d


def run_case(gold, case, route, monkeypatch):
    """The fixture's loop on the GPU -> {kind: [(name, rel(ours), rel(reference f32))]}"""
    if route == "torch":
        monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    else:
        monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    b, h, w, iters = (int(v) for v in gold[f"{case}_shape"])
    block = fresh_block(int(gold["weight_seed"]))
    x = update_train_inputs(int(gold[f"{case}_seed"]), b, h, w, iters, device="cuda")
    loss, disps, masks, _ = update_train_loop(block, x)
    loss.backward()
    torch.cuda.synchronize()
    g = lambda key: gold[f"{case}_{key}"]
    rows = {k: [] for k in KINDS}
    rows["outputs"].append(("loss", rel(float(loss.detach()), g("loss_f64")), rel(g("loss_f32"), g("loss_f64"))))
    pix, mpix = torch.from_numpy(g("pix_idx")).cuda(), torch.from_numpy(g("mask_idx")).cuda()
    for i in range(iters):
        for tag, t, idx in (("disp", disps[i], pix), ("mask", masks[i], mpix)):
            rows["outputs"].append((f"{tag}{i}", rel(t.detach().reshape(-1)[idx].cpu().numpy(), g(f"{tag}{i}_f64")),
                                    rel(g(f"{tag}{i}_f32"), g(f"{tag}{i}_f64"))))
    for what, tensors, names in (("grad", dict(block.named_parameters()), g("grad_names")),
                                 ("leaf", leaves_of(x), g("leaf_names"))):
        for j, name in enumerate(names):
            name = str(name)
            gr = tensors[name].grad
            assert gr is not None and torch.isfinite(gr).all(), name
            kind = "leaves" if what == "leaf" else ("biases" if name.endswith("bias") else "weights")
            idx = torch.from_numpy(g(f"{what}_idx")[j]).cuda()
            rows[kind].append((name, rel(gr.reshape(-1)[idx].cpu().numpy(), g(f"{what}_val_f64")[j]),
                               rel(g(f"{what}_val_f32")[j], g(f"{what}_val_f64")[j])))
            rows[kind].append((name + ":norm", rel(float(gr.double().norm()), g(f"{what}_norm_f64")[j]),
                               rel(g(f"{what}_norm_f32")[j], g(f"{what}_norm_f64")[j])))
    return rows


def bars(rows):
    return {k: min(max(2 * max(r[2] for r in rows[k]), 1e-5), 1e-4) for k in KINDS}


@pytest.mark.parametrize("case", ["even", "ragged"])
def test_loop_matches_reference(gold, case, monkeypatch):
    hip = run_case(gold, case, "hip", monkeypatch)
    tor = run_case(gold, case, "torch", monkeypatch)
    bound = bars(hip)
    for k in KINDS:
        print(f"PARITY {case} {k}: hip {max(r[1] for r in hip[k]):.3e}  torch {max(r[1] for r in tor[k]):.3e}  "
              f"reference f32 {max(r[2] for r in hip[k]):.3e}  bar {bound[k]:.1e}")
    bad = [(k, n, e) for k in KINDS for n, e, _ in hip[k] if not e <= bound[k]]
    assert not bad, f"HIP route over the bar {bound}: {sorted(bad, key=lambda t: -t[2])[:12]}"


def gru_ref(gru, h, cz, cr, cq, *xs):
    """update.py:33-40 restated in torch."""
    x = torch.cat(xs, dim=1)
    hx = torch.cat([h, x], dim=1)
    z = torch.sigmoid(gru.convz(hx) + cz)
    r = torch.sigmoid(gru.convr(hx) + cr)
    q = torch.tanh(gru.convq(torch.cat([r * h, x], dim=1)) + cq)
    return (1 - z) * h + z * q


def test_conv_gru_function_against_float64(monkeypatch):
    """ConvGRU alone (three x sources: all seven inputs and the six parameters), float32 on the HIP route against the
    float64 restatement: every gradient within 1e-5 relative L2 (the Winograd kernels' bar)."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    from diffuvolume_amd.update import ConvGRU
    gen = torch.Generator().manual_seed(11)
    gru = ConvGRU(128, 64 + 40 + 24)
    gru.load_state_dict(synth_state_dict(gru.state_dict(), seed=3))
    shapes = [128, 128, 128, 128, 64, 40, 24]
    vals = [torch.randn(2, c, 13, 21, generator=gen) for c in shapes]
    vals[0] = torch.tanh(vals[0])
    gy = torch.randn(2, 128, 13, 21, generator=gen)
    ref_gru = copy.deepcopy(gru).double()
    a64 = [v.double().requires_grad_(True) for v in vals]
    gru_ref(ref_gru, *a64).backward(gy.double())
    gru = gru.cuda().train()
    a32 = [v.cuda().requires_grad_(True) for v in vals]
    out = gru(*a32)
    out.backward(gy.cuda())
    assert rel(out.detach().cpu().numpy(), gru_ref(ref_gru, *a64).detach().numpy()) <= 1e-5
    for i, (a, b) in enumerate(zip(a32, a64)):
        assert rel(a.grad.cpu().numpy(), b.grad.numpy()) <= 1e-5, f"input {i}"
    for (n, p), q in zip(gru.named_parameters(), ref_gru.parameters()):
        assert rel(p.grad.cpu().numpy(), q.grad.numpy()) <= 1e-5, n


@pytest.mark.parametrize("n,offset", [(4096, 0), (4099, 0), (1027, 1), (3, 0), (5000, 3)])
def test_gate_kernels_tails_and_misaligned_views(n, offset):
    """The elementwise gate kernels on lengths that are no multiple of 4 and on views that are not 16-byte aligned (the
    scalar body), against the torch expressions in float64."""
    gen = torch.Generator().manual_seed(n + offset)
    mk = lambda: torch.randn(n + offset, generator=gen).cuda()[offset:]
    d, h, q = mk(), torch.tanh(mk()), torch.tanh(mk())
    z, r = torch.sigmoid(mk()), torch.sigmoid(mk())
    out = [torch.full((n + offset,), float("nan"), device="cuda")[offset:] for _ in range(6)]
    rh, hn, dq, dz, dh, dr = out
    train2d._gates("dv_gru_reset_mul_f32", r, h, rh, n)
    train2d._gates("dv_gru_blend_f32", z, q, h, hn, n)
    train2d._gates("dv_gru_gates_bwd_blend_f32", d, z, q, h, dq, dz, dh, n)
    dh0 = dh.clone()
    train2d._gates("dv_gru_gates_bwd_reset_f32", d, r, h, dr, dh, n)
    D, H, Q, Z, R = (t.double() for t in (d, h, q, z, r))
    for got, want in ((rh, R * H), (hn, (1 - Z) * H + Z * Q), (dq, D * Z * (1 - Q * Q)), (dz, D * (Q - H) * Z * (1 - Z)),
                      (dh0, D * (1 - Z)), (dr, D * H * R * (1 - R)), (dh, D * (1 - Z) + D * R)):
        assert torch.all((got.double() - want).abs() <= 4 * 2.0 ** -24 * (want.abs() + D.abs().max()))


def call_block(block, x, i=0, **kw):
    return block(list(x["net"]), x["inp"], x["corr"][i], x["disp"], **kw)


def test_training_forward_equals_eval_forward(monkeypatch):
    """Same kernels for the convolutions; r*h and the blend are computed by the gate kernels instead of the epilogues, in
    the epilogues' form (h + z (q - h)), and encoder.conv runs without its padded 128th channel.  Measured maximum
    |train - eval| / max|eval| on the MI355X: 0 ulp for every hidden state, the mask features and delta_disp (with
    (1-z) h + z q in the gate kernel it was 26 ulp of delta_disp's maximum); the test asserts twice that: equality."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    x = update_train_inputs(5, 2, 20, 28, 1, device="cuda")
    net_t, mask_t, delta_t = call_block(block, x)
    block.eval()
    with torch.no_grad():
        net_e, mask_e, delta_e = call_block(block, {**x, "net": [t.detach() for t in x["net"]],
                                                    "inp": [[t.detach() for t in lv] for lv in x["inp"]]})
    worst = 0.0
    for a, b in zip([*net_t, mask_t, delta_t], [*net_e, mask_e, delta_e]):
        worst = max(worst, float((a.detach() - b).abs().max() / b.abs().max()) / 2.0 ** -24)
    print(f"TRAIN_VS_EVAL worst {worst:.2f} ulp of the tensor maximum")
    assert worst <= 2 * MEASURED_ULP


MEASURED_ULP = 0.0


def test_train_mode_without_grad_is_the_eval_path(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    x = update_train_inputs(5, 1, 20, 28, 1, device="cuda")
    with torch.no_grad():
        a = call_block(block, x)
        block.eval()
        b = call_block(block, x)
    for u, v in zip([*a[0], a[1], a[2]], [*b[0], b[1], b[2]]):
        assert torch.equal(u, v) and not u.requires_grad


@pytest.fixture
def counts(monkeypatch):
    """Calls into the library's entry points, the plans, F.conv2d and torch.cat during one training call."""
    lib = _lib.load()
    c = {"cat": []}
    for name in ("dv_conv2d_wgrad_cat_f32", "dv_conv2d_wgrad_f32", "dv_gru_reset_mul_f32", "dv_gru_blend_f32", "dv_gru_gates_bwd_blend_f32",
                 "dv_gru_gates_bwd_reset_f32", "dv_conv2d_1in_f32", "dv_conv2d_1in_wgrad_f32"):
        def counting(*args, _real=getattr(lib, name), _name=name):
            c[_name] = c.get(_name, 0) + 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)
    depth = [0]
    real_pair, real_plan, real_conv, real_cat = S.Conv2dPairPlan.__call__, S.Conv2dPlan.__call__, F.conv2d, torch.cat

    def pair(self, *a, **k):
        c["pair"] = c.get("pair", 0) + 1
        depth[0] += 1
        try:
            return real_pair(self, *a, **k)
        finally:
            depth[0] -= 1

    def plan(self, *a, **k):
        if not depth[0]:                                   # (a pair too small for its launch runs its two single plans)
            c["plan"] = c.get("plan", 0) + 1
        return real_plan(self, *a, **k)

    def conv2d(*a, **k):
        c["F.conv2d"] = c.get("F.conv2d", 0) + 1
        return real_conv(*a, **k)

    def cat(tensors, *a, **k):
        c["cat"].append(tuple(t.shape[1] for t in tensors if t.dim() == 4))
        return real_cat(tensors, *a, **k)
    monkeypatch.setattr(S.Conv2dPairPlan, "__call__", pair)
    monkeypatch.setattr(S.Conv2dPlan, "__call__", plan)
    monkeypatch.setattr(F, "conv2d", conv2d)
    monkeypatch.setattr(torch, "cat", cat)
    return c


def one_training_call(block):
    x = update_train_inputs(5, 2, 20, 28, 1, device="cuda")
    net, mask, delta = call_block(block, x)
    (delta.sum() + mask.sum() + sum(t.sum() for t in net)).backward()
    torch.cuda.synchronize()


def test_what_runs_on_the_hip_route(monkeypatch, counts):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    block.plans("train"), [m.plans("train") for m in (block.gru04, block.gru08, block.gru16, block.encoder, block.disp_head)]
    counts.clear()
    counts["cat"] = []
    one_training_call(block)
    # weight gradients: 3 ConvGRUs x 3, encoder convc1 / convc2 / convd2 / conv, disp_head.conv1 / conv2, mask_feat_4 on
    # the new kernel, none on refinenet3's
    assert counts.get("dv_conv2d_wgrad_cat_f32") == 9 + 4 + 2 + 1
    assert not counts.get("dv_conv2d_wgrad_f32")
    # forward: one pair launch and one candidate per ConvGRU, 4 encoder layers, 2 head layers, mask_feat_4
    # input gradients: 2 per ConvGRU; convc2, convd2, conv, conv1, mask_feat_4 (convc1's input, corr, asks for none);
    # disp_head.conv2's on the single-channel kernel
    assert counts.get("pair") == 3
    assert counts.get("plan") == (3 + 4 + 2 + 1) + (6 + 5)
    assert counts.get("dv_conv2d_1in_f32") == 2                         # convd1's forward, disp_head.conv2's input gradient
    assert counts.get("dv_conv2d_1in_wgrad_f32") == 1                   # convd1
    # gate kernels: r*h and the blend per ConvGRU forward, r*h again in its backward; one of each backward kernel
    assert counts.get("dv_gru_reset_mul_f32") == 6 and counts.get("dv_gru_blend_f32") == 3
    assert counts.get("dv_gru_gates_bwd_blend_f32") == 3 and counts.get("dv_gru_gates_bwd_reset_f32") == 3
    assert not counts.get("F.conv2d")                                   # (convd1 too runs on its own kernels)
    assert counts["cat"] == [(127, 1)]                                  # the motion features' disparity channel only


def test_what_runs_on_the_torch_route(monkeypatch, counts):
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    one_training_call(fresh_block())
    assert not counts.get("dv_conv2d_wgrad_cat_f32") and not counts.get("dv_conv2d_wgrad_f32")
    assert not counts.get("dv_gru_reset_mul_f32") and not counts.get("dv_gru_blend_f32") and not counts.get("plan") and not counts.get("pair")
    assert counts.get("F.conv2d") == 9 + 5 + 2 + 1


def test_corr_and_disp_receive_gradients(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    x = update_train_inputs(5, 1, 10, 14, 1, device="cuda")
    corr, disp = x["corr"][0].requires_grad_(True), x["disp"].requires_grad_(True)
    net, mask, delta = block(list(x["net"]), x["inp"], corr, disp)
    (delta.sum() + mask.sum()).backward()
    assert corr.grad is not None and float(corr.grad.abs().sum()) > 0
    assert disp.grad is not None and float(disp.grad.abs().sum()) > 0
    assert block.encoder.convd1.weight.grad is not None and float(block.encoder.convd1.weight.grad.abs().sum()) > 0


def test_fewer_gru_levels_and_slow_fast(monkeypatch):
    """n_gru_layers 1 and 2, update=False and mask=False against the torch route (same bar as the fixture cases' floor)."""
    for n in (1, 2, 3):
        grads = {}
        for route in ("hip", "torch"):
            monkeypatch.setenv("DV_TRAIN_CONV2D", route)
            block = fresh_block(n_gru_layers=n)
            x = update_train_inputs(9, 1, 12, 20, 1, device="cuda")
            net = list(x["net"])
            if n == 3:
                net = block(net, x["inp"], iter16=True, iter08=False, iter04=False, update=False)
            if n >= 2:
                net = block(net, x["inp"], iter16=n == 3, iter08=True, iter04=False, update=False)
            net, mask, delta = block(net, x["inp"], x["corr"][0], x["disp"], iter16=n == 3, iter08=n >= 2, mask=False)
            assert mask is None
            (delta * x["m"][:, :1]).sum().backward()
            grads[route] = {k: p.grad for k, p in block.named_parameters() if p.grad is not None}
        assert grads["hip"].keys() == grads["torch"].keys() and "gru04.convq.weight" in grads["hip"]
        assert ("gru16.convz.weight" in grads["hip"]) == (n == 3)
        for k in grads["hip"]:
            assert rel(grads["hip"][k].cpu().numpy(), grads["torch"][k].cpu().numpy()) <= 2e-5, (n, k)


def test_optimizer_step_refreshes_the_packed_weights(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    opt = torch.optim.AdamW(block.parameters(), lr=1e-2)
    x = update_train_inputs(5, 1, 20, 28, 1, device="cuda")
    net, mask, delta = call_block(block, x)
    first = delta.detach().clone()
    (delta.sum() + mask.sum()).backward()
    opt.step()
    _, _, second = call_block(block, x)
    assert not torch.equal(first, second)
    clone = fresh_block()
    clone.load_state_dict(copy.deepcopy(block.state_dict()))
    _, _, third = call_block(clone, x)
    assert torch.equal(second.detach(), third.detach())        # the second forward ran on the stepped weights, all of them


def test_optimizer_step_is_seen_by_a_module_trained_on_its_own(monkeypatch):
    """ConvGRU, DispHead and BasicMotionEncoder are training entries of their own: their packed weights (forward and
    flipped) follow the weight key without the block's forward."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    x = update_train_inputs(5, 1, 10, 14, 1, device="cuda")
    calls = {"gru": lambda m: m.gru04(x["net"][0], *x["inp"][0], x["net"][0].detach(), x["inp"][0][0].detach()),
             "head": lambda m: m.disp_head(x["net"][0]),
             "encoder": lambda m: m.encoder(x["disp"], x["corr"][0])}
    for name, call in calls.items():
        first = call(block)
        g = torch.autograd.grad(first.sum(), [p for p in block.parameters() if p.requires_grad], allow_unused=True)
        with torch.no_grad():
            for p, gp in zip(block.parameters(), g):
                if gp is not None:
                    p.add_(gp.sign(), alpha=-1e-2)                        # an in-place step, as an optimizer writes it
        second = call(block)
        assert not torch.equal(first, second), name
        clone = fresh_block()
        clone.load_state_dict(copy.deepcopy(block.state_dict()))
        third = call(clone)
        assert torch.equal(second.detach(), third.detach()), name
        gb = torch.autograd.grad(second.sum(), x["net"][0], allow_unused=True)[0]
        gc = torch.autograd.grad(third.sum(), x["net"][0], allow_unused=True)[0]
        assert (gb is None and gc is None) or torch.equal(gb, gc), name    # the flipped weights too


def test_lookup_request_is_materialised(monkeypatch):
    """`corr` as a GeoLookupRequest (what this build's IGEVDiffusionLoop hands over): the training route materialises it,
    the same bits and gradients as with the lookup's tensor."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
    gen = torch.Generator().manual_seed(61)
    b, c, d, h, w = 2, 8, 48, 8, 24
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()
    vol = Combined_Geo_Encoding_Volume(rnd(b, 16, h, w), rnd(b, 16, h, w), rnd(b, c, d, h, w), num_levels=2, radius=4)
    disp = (torch.rand(b, 1, h, w, generator=gen) * 40).cuda()
    coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous().cuda()
    noisy = torch.rand(b, d, h, w, generator=gen).cuda()
    outs = []
    for corr in (vol.request(disp, coords, noisy), vol(disp, coords, noisy)):
        block = fresh_block()
        x = update_train_inputs(5, b, h, w, 1, device="cuda")
        net, mask, delta = block(list(x["net"]), x["inp"], corr, disp)
        (delta.sum() + mask.sum()).backward()
        outs.append((delta.detach(), block.encoder.convc1.weight.grad.clone(), x["net"][0].grad.clone()))
    assert outs[0][0].shape == (b, 1, h, w) and float(outs[0][1].abs().sum()) > 0
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_autocast_and_cpu_are_refused(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block()
    x = update_train_inputs(5, 1, 10, 14, 1, device="cuda")
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(DiffuVolumeError):
        call_block(block, x)
    with pytest.raises(DiffuVolumeError):
        call_block(block, update_train_inputs(5, 1, 10, 14, 1))


def kinds_of(block, x, disps, masks, loss):
    out = {"weights": [p.grad for n, p in block.named_parameters() if not n.endswith("bias")],
           "biases": [p.grad for n, p in block.named_parameters() if n.endswith("bias")],
           "leaves": [t.grad for t in leaves_of(x).values()],
           "outputs": [loss.detach().reshape(1), *[d.detach() for d in disps], *[m.detach() for m in masks]]}
    return {k: [t.detach().double().cpu() for t in v] for k, v in out.items()}


def worst_rel(a, b):
    return {k: max(float((u - v).norm() / v.norm().clamp_min(1e-300)) for u, v in zip(a[k], b[k])) for k in KINDS}


def long_loop(route, monkeypatch, iters=22, b=1, h=80, w=184):
    monkeypatch.setenv("DV_TRAIN_CONV2D", route)
    block = fresh_block()
    x = update_train_inputs(41, b, h, w, iters, device="cuda")
    loss, disps, masks, _ = update_train_loop(block, x)
    loss.backward()
    torch.cuda.synchronize()
    return kinds_of(block, x, disps, masks, loss)


def block_f64_cpu(block, net, inp, corr, disp):
    """BasicMultiUpdateBlock.forward (n_gru_layers 3) restated in torch for the float64 CPU leg."""
    pool = lambda t: F.avg_pool2d(t, 3, stride=2, padding=1)
    interp = lambda t, d: F.interpolate(t, d.shape[2:], mode="bilinear", align_corners=True)
    e = block.encoder
    net[2] = gru_ref(block.gru16, net[2], *inp[2], pool(net[1]))
    net[1] = gru_ref(block.gru08, net[1], *inp[1], pool(net[0]), interp(net[2], net[1]))
    cor = F.relu(e.convc2(F.relu(e.convc1(corr))))
    dsp = F.relu(e.convd2(F.relu(e.convd1(disp))))
    mf = torch.cat([F.relu(e.conv(torch.cat([cor, dsp], dim=1))), disp], dim=1)
    net[0] = gru_ref(block.gru04, net[0], *inp[0], mf, interp(net[1], net[0]))
    delta = block.disp_head.conv2(F.relu(block.disp_head.conv1(net[0])))
    return net, F.relu(block.mask_feat_4[0](net[0])), delta


def test_full_length_loop(monkeypatch):
    """T = 22 at B 1, 80 x 184 (the reference's train_iters on one crop's 1/4 plane): finite, the same bits on a second
    run, peak memory and the distance to the torch route printed.  DV_FULL_PARITY=1 adds the float64 CPU restatement:
    the HIP route's error against it is at most twice the torch route's float32 error against it, per kind.  Measured
    (weights / biases / leaves / outputs): HIP 1.7e-3 / 5.3e-4 / 1.4e-3 / 4.3e-5, torch route 1.7e-3 / 6.1e-4 / 1.3e-3 /
    4.4e-5 against float64, 1.5e-3 / 4.5e-4 / 1.3e-3 / 3.4e-5 between the two routes; 2.5 GiB peak."""
    torch.cuda.reset_peak_memory_stats()
    a = long_loop("hip", monkeypatch)
    print(f"LONG max_memory_allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    for k in KINDS:
        assert all(torch.isfinite(t).all() for t in a[k]), k
    b = long_loop("hip", monkeypatch)
    for k in KINDS:
        assert all(torch.equal(u, v) for u, v in zip(a[k], b[k])), k
    t = long_loop("torch", monkeypatch)
    print("LONG hip vs torch route, relative L2 per kind:", {k: f"{v:.3e}" for k, v in worst_rel(a, t).items()})
    if os.environ.get("DV_FULL_PARITY") != "1":
        return
    block = fresh_block().cpu().double()

    class Ref:
        def __call__(self, net, inp, corr=None, disp=None, **kw):
            return block_f64_cpu(block, net, inp, corr, disp)
    x = update_train_inputs(41, 1, 80, 184, 22, dtype=torch.float64)
    loss, disps, masks, _ = update_train_loop(Ref(), x)
    loss.backward()
    r = kinds_of(block, x, disps, masks, loss)
    eh, et = worst_rel(a, r), worst_rel(t, r)
    print("LONG against float64: hip", eh, "torch", et)
    for k in KINDS:
        assert eh[k] <= 2 * et[k], (k, eh[k], et[k])
