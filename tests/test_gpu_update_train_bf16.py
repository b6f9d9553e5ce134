"""Training of IGEV's update block at train precision "bf16" on the MI355X:
``BasicMultiUpdateBlock.set_train_precision(torch.bfloat16)`` (train2d's bf16 plans in the ``plans("trainbf16")`` slot,
dv_conv2d_wgrad_cat_bf16, the bf16 gate kernels, dv_conv2d_1in_bf16).  The method and the helpers are
tests/test_gpu_update_train_amp.py's; no loss scale is applied anywhere but in the range test.

Yardstick for the gradients: the float64 restatement on the CPU, triangulated with the SAME torch expressions under a real
``torch.autocast("cuda", dtype=torch.bfloat16)`` (``DV_TRAIN_CONV2D=torch`` at "bf16").  The HIP route's relative L2 error
against float64 is at most twice the torch-autocast route's -- the project's standing rule -- per tensor for a ConvGRU
alone, per kind of tensor (weights, biases, leaves, outputs; the worst tensor of each kind) for the unrolled loops.  The
expectation before the first run was about eight times the fp16 figures of tests/test_gpu_update_train_amp.py (three
mantissa bits fewer); it is no bar.  Measured figures: the docstrings of the two tests below and DESIGN.md, "IGEV's update
block in bfloat16"."""
import copy

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import DiffuVolumeError, _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import synth_state_dict, update_train_inputs, update_train_loop
from diffuvolume_amd.update import ConvGRU
from test_gpu_update_train_amp import (KINDS, call_block, fresh_block, gru_ref, kinds_of, leaves_of, loop_f64, rel,
                                       rel_per_tensor)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CHILDREN = ("gru04", "gru08", "gru16", "encoder", "disp_head")


def exactb16(t):
    return torch.equal(t.bfloat16().float(), t)


def test_conv_gru_alone_against_float64(monkeypatch):
    """ConvGRU alone (x sources of 64, 40 and 24 channels, B 2, 13 x 21): all seven inputs and the six parameters, no
    scale.  Per tensor: HIP "bf16" error against float64 <= 2 x the error of the same expression under real bf16 autocast.

    Measured on the MI355X (relative L2 against float64, HIP | torch bf16 autocast): output 3.87e-3 | 4.20e-3; the seven
    input gradients 3.43e-3 .. 6.98e-3 | 5.40e-3 .. 8.82e-3; the six parameter gradients 4.14e-3 .. 7.39e-3 | 5.83e-3 ..
    9.14e-3 -- every tensor 0.63 .. 0.92 of the autocast route, about eight times the fp16 figures (4.2e-4 .. 9.1e-4)."""
    gen = torch.Generator().manual_seed(11)
    proto = ConvGRU(128, 64 + 40 + 24)
    proto.load_state_dict(synth_state_dict(proto.state_dict(), seed=3))
    vals = [torch.randn(2, c, 13, 21, generator=gen) for c in [128, 128, 128, 128, 64, 40, 24]]
    vals[0] = torch.tanh(vals[0])
    gy = torch.randn(2, 128, 13, 21, generator=gen)
    ref_gru = copy.deepcopy(proto).double()
    a64 = [v.double().requires_grad_(True) for v in vals]
    out64 = gru_ref(ref_gru, *a64)
    out64.backward(gy.double())
    want = {"out": out64, **{f"input{i}": a.grad for i, a in enumerate(a64)},
            **{n: p.grad for n, p in ref_gru.named_parameters()}}
    errs = {}
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_CONV2D", route)
        gru = copy.deepcopy(proto).cuda().train().set_train_precision(BF16)
        assert gru.train_precision == "bf16"
        a = [v.cuda().requires_grad_(True) for v in vals]
        out = gru(*a)
        assert out.dtype == torch.float32
        out.backward(gy.cuda())
        got = {"out": out, **{f"input{i}": t.grad for i, t in enumerate(a)}, **{n: p.grad for n, p in gru.named_parameters()}}
        assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in got.values())
        errs[route] = {k: rel(got[k], want[k]) for k in want}
    for k in want:
        print(f"GRUBF16 {k}: hip {errs['hip'][k]:.3e}  torch autocast {errs['torch'][k]:.3e}")
    bad = {k: (errs["hip"][k], errs["torch"][k]) for k in want if not errs["hip"][k] <= 2 * errs["torch"][k]}
    assert not bad, bad


def loop_gpu(case, route, monkeypatch, scale=1.0):
    monkeypatch.setenv("DV_TRAIN_CONV2D", route)
    b, h, w, iters, seed = case
    block = fresh_block(BF16)
    x = update_train_inputs(seed, b, h, w, iters, device="cuda")
    loss, disps, masks, _ = update_train_loop(block, x)
    (loss * scale).backward()
    torch.cuda.synchronize()
    return kinds_of(block, x, disps, masks, loss * scale, scale)


@pytest.mark.parametrize("case", [(2, 16, 32, 3, 21), (2, 20, 28, 2, 22)], ids=["even_T3", "ragged_T2"])
def test_unrolled_loop_against_float64(case, monkeypatch):
    """synth.update_train_loop (B 2; 16 x 32 with T = 3, 20 x 28 with T = 2), no loss scale: per kind the worst tensor's
    error of the HIP "bf16" route against the float64 CPU restatement <= 2 x the worst tensor's error of the torch bf16
    autocast route.

    Measured on the MI355X (weights / biases / leaves / outputs, HIP | torch bf16 autocast):
        16 x 32, T 3   1.45e-1 / 5.14e-2 / 1.24e-1 / 1.20e-2  |  1.50e-1 / 5.38e-2 / 1.27e-1 / 1.47e-2
        20 x 28, T 2   1.26e-1 / 6.02e-2 / 9.87e-2 / 9.23e-3  |  1.34e-1 / 6.02e-2 / 1.07e-1 / 1.13e-2
    (worst tensors on both routes: encoder.convc1.weight, gru16.convr.bias / gru08.convr.bias, inp01, the mask features).
    Against the fp16 figures of tests/test_gpu_update_train_amp.py: 2.1 .. 3.7 times on weights, biases and leaves, eight
    times on the outputs."""
    ref = loop_f64(case)
    eh = rel_per_tensor(loop_gpu(case, "hip", monkeypatch), ref)
    et = rel_per_tensor(loop_gpu(case, "torch", monkeypatch), ref)
    worst = lambda e, k: max(e[k].items(), key=lambda kv: kv[1])
    for k in KINDS:
        (nh, vh), (nt, vt) = worst(eh, k), worst(et, k)
        print(f"LOOPBF16 {case} {k}: hip {vh:.3e} ({nh})  torch autocast {vt:.3e} ({nt})")
    bad = {k: (worst(eh, k), worst(et, k)) for k in KINDS if not worst(eh, k)[1] <= 2 * worst(et, k)[1]}
    assert not bad, bad


def test_training_forward_is_float32_bf16_exact_and_its_own(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = update_train_inputs(5, 2, 20, 28, 1, device="cuda")
    outs = {}
    for precision in (BF16, "f16", "f32"):
        net, mask, delta = call_block(fresh_block(precision), x)
        outs[precision] = [t.detach() for t in (*net, mask, delta)]
        assert delta.requires_grad and all(t.dtype == torch.float32 for t in outs[precision])
    for name, t in zip(("net0", "net1", "net2", "mask_feat_4", "delta_disp"), outs[BF16]):
        assert exactb16(t) and torch.isfinite(t).all(), name
    assert not torch.equal(outs[BF16][-1], outs["f32"][-1]) and not torch.equal(outs[BF16][-1], outs["f16"][-1])
    assert not torch.equal(outs[BF16][0], outs["f16"][0])


@pytest.fixture
def counts(monkeypatch):
    """Calls into the library's entry points, the plans and F.conv2d during one training call."""
    lib = _lib.load()
    c = {}
    names = ["dv_conv2d_wgrad_cat_bf16", "dv_conv2d_wgrad_cat_f16", "dv_conv2d_wgrad_cat_f32", "dv_conv2d_wgrad_f32",
             "dv_gru_reset_mul_bf16", "dv_gru_blend_bf16", "dv_gru_reset_mul_f16", "dv_gru_blend_f16", "dv_gru_reset_mul_f32",
             "dv_gru_blend_f32", "dv_gru_gates_bwd_blend_f32", "dv_gru_gates_bwd_reset_f32", "dv_conv2d_1in_bf16",
             "dv_conv2d_1in_f16", "dv_conv2d_1in_f32", "dv_conv2d_1in_wgrad_f32", "dv_conv2d_cat_f32", "dv_conv2d_cat_ksplit_f32",
             "dv_conv2d_wino_cat_f32", "dv_conv2d_wino_cat_pair_f32", "dv_conv2d_wino_cat_ksplit_f32",
             "dv_conv2d_wino_cat_pair_ksplit_f32"]
    names += [f"dv_conv2d_{e}_cat{s}" for e in ("f16", "bf16") for s in ("", "_ksplit", "_pair", "_pair_ksplit")]
    for name in names:
        def counting(*args, _real=getattr(lib, name), _name=name):
            c[_name] = c.get(_name, 0) + 1
            return _real(*args)
        monkeypatch.setattr(lib, name, counting)

    def wrap(cls, key):
        real = cls.__call__

        def call(self, *a, **k):
            c[key] = c.get(key, 0) + 1
            return real(self, *a, **k)
        monkeypatch.setattr(cls, "__call__", call)
    wrap(S.Conv2dPairPlan, "pair")
    wrap(S.Conv2dPlan, "plan")
    real_conv = F.conv2d

    def conv2d(*a, **k):
        c["F.conv2d"] = c.get("F.conv2d", 0) + 1
        return real_conv(*a, **k)
    monkeypatch.setattr(F, "conv2d", conv2d)
    return c


def one_training_call(block):
    x = update_train_inputs(5, 2, 20, 28, 1, device="cuda")
    net, mask, delta = call_block(block, x)
    (delta.sum() + mask.sum() + sum(t.sum() for t in net)).backward()
    torch.cuda.synchronize()


def test_what_runs_at_bf16(monkeypatch, counts):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block(BF16)
    block.plans("trainbf16"), [getattr(block, m).plans("trainbf16") for m in CHILDREN]
    counts.clear()
    one_training_call(block)
    # weight gradients: 3 ConvGRUs x 3, encoder convc1 / convc2 / convd2 / conv, disp_head.conv1 / conv2, mask_feat_4
    assert counts.get("dv_conv2d_wgrad_cat_bf16") == 9 + 4 + 2 + 1
    assert counts.get("dv_gru_reset_mul_bf16") == 6 and counts.get("dv_gru_blend_bf16") == 3
    assert counts.get("dv_conv2d_1in_bf16") == 2                                           # convd1, disp_head.conv2's dx
    # forward: pair + candidate per ConvGRU, 4 encoder layers, 2 head layers, mask_feat_4; input gradients: 2 per ConvGRU,
    # convc2, convd2, conv, conv1, mask_feat_4 -- all on the bf16 convolution entries
    assert sum(v for k, v in counts.items() if k.startswith("dv_conv2d_bf16_cat")) == (6 + 4 + 2 + 1) + (6 + 5)
    # none of the f16 twins, none of the f32 forward entries, not F.conv2d
    assert not [k for k in counts if k.endswith("_f16") or "_f16_" in k], counts
    assert not [k for k in counts if k.startswith(("dv_conv2d_cat", "dv_conv2d_wino", "dv_conv2d_wgrad_cat_f32",
                                                   "dv_conv2d_wgrad_f32", "dv_gru_reset_mul_f32", "dv_gru_blend_f32",
                                                   "dv_conv2d_1in_f32"))], counts
    assert not counts.get("F.conv2d") and not counts.get("plan") and not counts.get("pair")
    # the gate backward and convd1's weight gradient run as at "f16": float32
    assert counts.get("dv_gru_gates_bwd_blend_f32") == 3 and counts.get("dv_gru_gates_bwd_reset_f32") == 3
    assert counts.get("dv_conv2d_1in_wgrad_f32") == 1


def grads_of_one_step(block, x, scale=1.0):
    for p in block.parameters():
        p.grad = None
    for t in leaves_of(x).values():
        t.grad = None
    loss, _, _, _ = update_train_loop(block, x)
    (loss * scale).backward()
    torch.cuda.synchronize()
    return {**{n: p.grad.clone() for n, p in block.named_parameters()}, **{n: t.grad.clone() for n, t in leaves_of(x).items()}}


def test_round_trip_through_the_precisions_and_identical_steps(monkeypatch):
    """One block taken through "f32" -> bf16 -> "f16" -> "f32" gives, at each precision, the gradient bits of a fresh
    block set to that precision (the three plan slots do not leak into each other); two identical bf16 steps give identical
    bits."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = update_train_inputs(31, 2, 12, 20, 2, device="cuda")
    fresh = {p: grads_of_one_step(fresh_block(p), x) for p in ("f32", BF16, "f16")}
    block = fresh_block("f32")
    for p in ("f32", BF16, "f16", "f32"):
        block.set_train_precision(p)
        got = grads_of_one_step(block, x)
        assert got.keys() == fresh[p].keys()
        assert all(torch.equal(got[n], fresh[p][n]) for n in got), p
    assert not torch.equal(fresh[BF16]["gru04.convq.weight"], fresh["f16"]["gru04.convq.weight"])
    block.set_train_precision(BF16)
    a, b = grads_of_one_step(block, x), grads_of_one_step(block, x)
    assert all(torch.equal(a[n], b[n]) and torch.isfinite(a[n]).all() for n in a)


def test_optimizer_step_refreshes_the_bf16_packed_weights(monkeypatch):
    """The `trainbf16` packed weights, forward and flipped, follow the weight key."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block(BF16)
    opt = torch.optim.AdamW(block.parameters(), lr=1e-2)
    x = update_train_inputs(5, 1, 12, 20, 1, device="cuda")
    net, mask, delta = call_block(block, x)
    first = delta.detach().clone()
    (delta.sum() + mask.sum()).backward()
    opt.step()
    net2, mask2, second = call_block(block, x)
    assert not torch.equal(first, second)
    clone = fresh_block(BF16)
    clone.load_state_dict(copy.deepcopy(block.state_dict()))
    net3, mask3, third = call_block(clone, x)
    for a, b in zip([*net2, mask2, second], [*net3, mask3, third]):
        assert torch.equal(a.detach(), b.detach())             # the second forward ran on the stepped weights, all of them
    gb = torch.autograd.grad(second.sum() + mask2.sum(), x["net"][0])[0]
    gc = torch.autograd.grad(third.sum() + mask3.sum(), x["net"][0])[0]
    assert torch.equal(gb, gc)                                 # the flipped weights too


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_gru_levels_with_update_and_mask_off(n, monkeypatch):
    """n_gru_layers 1 and 2 with the update=False calls and mask=False: finite, and the same parameters receive gradients
    as at "f32"."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    grads = {}
    for precision in (BF16, "f32"):
        block = fresh_block(precision, n_gru_layers=n)
        x = update_train_inputs(9, 1, 12, 20, 1, device="cuda")
        net = list(x["net"])
        if n >= 2:
            net = block(net, x["inp"], iter16=False, iter08=True, iter04=False, update=False)
        net, mask, delta = block(net, x["inp"], x["corr"][0], x["disp"], iter16=False, iter08=n >= 2, mask=False)
        assert mask is None and delta.dtype == torch.float32
        (delta * x["m"][:, :1]).sum().backward()
        grads[precision] = {k: p.grad for k, p in block.named_parameters() if p.grad is not None}
    assert grads[BF16].keys() == grads["f32"].keys() and "gru04.convq.weight" in grads[BF16]
    assert ("gru08.convz.weight" in grads[BF16]) == (n >= 2) and "gru16.convz.weight" not in grads[BF16]
    assert all(torch.isfinite(g).all() for g in grads[BF16].values())


def test_range_a_loss_scaled_by_2_to_the_20_keeps_every_gradient_finite(monkeypatch):
    """The loop whose fp16 twin needs a GradScaler to stay in range: at bf16 the range is float32's."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = update_train_inputs(22, 2, 20, 28, 2, device="cuda")
    g = grads_of_one_step(fresh_block(BF16), x, scale=2.0 ** 20)
    assert all(torch.isfinite(t).all() for t in g.values())
    assert max(float(t.abs().max()) for t in g.values()) > 65504.0          # (beyond what an fp16 gradient could hold)


def test_autocast_matrix(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = update_train_inputs(5, 1, 10, 14, 1, device="cuda")
    block = fresh_block(BF16)
    with torch.autocast("cuda", dtype=BF16):                      # at "bf16" the caller's bf16 autocast is accepted
        net, mask, delta = call_block(block, x)
    assert delta.dtype == torch.float32 and mask.dtype == torch.float32 and all(t.dtype == torch.float32 for t in net)
    # bf16 inputs are converted to float32 once on entry
    xb = {**x, "net": [t.detach().bfloat16() for t in x["net"]], "inp": [[t.detach().bfloat16() for t in lv] for lv in x["inp"]],
          "corr": [t.bfloat16() for t in x["corr"]], "disp": x["disp"].bfloat16()}
    netb, maskb, deltab = call_block(block, xb)
    assert deltab.dtype == torch.float32 and all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in netb)
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(DiffuVolumeError):
        call_block(block, x)
    for child in CHILDREN:                                        # every child is an entry of its own
        assert getattr(block, child).train_precision == "bf16"
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(DiffuVolumeError):
        block.disp_head(x["net"][0])
    # at "f16" a bf16 autocast keeps raising; at "f32" both keep raising
    block.set_train_precision("f16")
    with torch.autocast("cuda", dtype=BF16), pytest.raises(DiffuVolumeError):
        call_block(block, x)
    block.set_train_precision("f32")
    for dt in (BF16, torch.float16):
        with torch.autocast("cuda", dtype=dt), pytest.raises(DiffuVolumeError):
            call_block(block, x)
    # eval under bf16 autocast keeps raising, whatever the train precision
    block.set_train_precision(BF16).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16), pytest.raises(DiffuVolumeError):
        call_block(block, {**x, "net": [t.detach() for t in x["net"]]})
    with pytest.raises(ValueError):
        block.set_train_precision("bf16")
