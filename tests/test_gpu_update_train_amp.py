"""Mixed-precision training of IGEV's update block on the MI355X: ``BasicMultiUpdateBlock.set_train_precision("f16")``
(train2d's fp16 plans, dv_conv2d_wgrad_cat_f16, the fp16 gate kernels).

Yardstick for the gradients: the float64 restatement on the CPU, triangulated with the SAME torch expressions under a real
``torch.autocast("cuda", dtype=torch.float16)`` (``DV_TRAIN_CONV2D=torch`` at "f16" precision).  The HIP route's error
against float64 is at most twice the torch-autocast route's error against float64 -- the project's "twice the reference's
own error" rule -- per tensor for a ConvGRU alone, per kind of tensor (weights, biases, leaves, outputs; the worst tensor
of each kind) for the unrolled loop.  The upstream gradient / the loss is scaled by a power of two as a GradScaler would
and the results are unscaled afterwards (exact).

Measured on the MI355X (relative L2 against float64): ConvGRU alone, HIP 4.2e-4 .. 9.1e-4 per tensor against 8.4e-4 ..
1.9e-3 for torch autocast (every tensor about half: dW is not rounded to fp16 and the gate backward is float32); the
unrolled loops: test_unrolled_loop_against_float64's docstring."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import DiffuVolumeError, _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import (UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN, synth_state_dict, update_train_inputs,
                                   update_train_loop)
from diffuvolume_amd.update import BasicMultiUpdateBlock, ConvGRU

pytestmark = pytest.mark.gpu
KINDS = ("weights", "biases", "leaves", "outputs")
SCALE = 1024.0


def fresh_block(precision="f16", seed=7, n_gru_layers=3):
    args = types.SimpleNamespace(**{**UPDATE_TRAIN_ARGS, "n_gru_layers": n_gru_layers})
    m = BasicMultiUpdateBlock(args, hidden_dims=UPDATE_TRAIN_HIDDEN)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=seed), strict=True)
    return m.cuda().train().set_train_precision(precision)


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def call_block(block, x, i=0, **kw):
    return block(list(x["net"]), x["inp"], x["corr"][i], x["disp"], **kw)


def exact16(t):
    return torch.equal(t.half().float(), t)


def test_default_precision_still_refuses_autocast_and_bf16_is_refused(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = update_train_inputs(5, 1, 10, 14, 1, device="cuda")
    block = fresh_block("f32")
    assert block.train_precision == "f32"
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(DiffuVolumeError):
        call_block(block, x)
    with pytest.raises(ValueError):
        block.set_train_precision("bf16")
    block.set_train_precision("f16")
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(DiffuVolumeError):
        call_block(block, x)
    with torch.autocast("cuda", dtype=torch.float16):           # with "f16" the caller's fp16 autocast is fine
        net, mask, delta = call_block(block, x)
    assert delta.dtype == torch.float32 and mask.dtype == torch.float32 and all(t.dtype == torch.float32 for t in net)


def test_training_forward_has_the_bits_of_the_eval_forward_under_autocast(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block("f16")
    x = update_train_inputs(5, 2, 20, 28, 1, device="cuda")
    net_t, mask_t, delta_t = call_block(block, x)
    assert delta_t.requires_grad
    block.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        net_e, mask_e, delta_e = call_block(block, {**x, "net": [t.detach() for t in x["net"]],
                                                    "inp": [[t.detach() for t in lv] for lv in x["inp"]]})
    for name, a, b in zip(("net0", "net1", "net2", "mask_feat_4", "delta_disp"), [*net_t, mask_t, delta_t],
                          [*net_e, mask_e, delta_e]):
        assert a.dtype == torch.float32 and torch.equal(a.detach(), b), name
        assert exact16(a.detach()), name
    # ... and differs from the float32 training forward
    _, _, delta_32 = call_block(fresh_block("f32"), x)
    assert not torch.equal(delta_32.detach(), delta_t.detach())


def gru_ref(gru, h, cz, cr, cq, *xs):
    """update.py:33-40 restated in torch."""
    x = torch.cat(xs, dim=1)
    hx = torch.cat([h, x], dim=1)
    z = torch.sigmoid(gru.convz(hx) + cz)
    r = torch.sigmoid(gru.convr(hx) + cr)
    q = torch.tanh(gru.convq(torch.cat([r * h, x], dim=1)) + cq)
    return (1 - z) * h + z * q


def test_conv_gru_alone_against_float64(monkeypatch):
    """ConvGRU alone (x sources of 64, 40 and 24 channels, 13 x 21): all seven inputs and the six parameters.  The
    upstream gradient is handed over scaled by 2^10 and the results unscaled.  Per tensor: HIP "f16" error against float64
    <= 2 x the error of the same expression under real fp16 autocast."""
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
        gru = copy.deepcopy(proto).cuda().train().set_train_precision("f16")
        a = [v.cuda().requires_grad_(True) for v in vals]
        out = gru(*a)
        assert out.dtype == torch.float32
        out.backward(gy.cuda() * SCALE)
        got = {"out": out, **{f"input{i}": t.grad / SCALE for i, t in enumerate(a)},
               **{n: p.grad / SCALE for n, p in gru.named_parameters()}}
        assert all(t.dtype == torch.float32 and torch.isfinite(t).all() for t in got.values())
        errs[route] = {k: rel(got[k], want[k]) for k in want}
    for k in want:
        print(f"GRU16 {k}: hip {errs['hip'][k]:.3e}  torch autocast {errs['torch'][k]:.3e}")
    bad = {k: (errs["hip"][k], errs["torch"][k]) for k in want if not errs["hip"][k] <= 2 * errs["torch"][k]}
    assert not bad, bad


def leaves_of(x):
    d = {f"net{i}": t for i, t in enumerate(x["net"])}
    d.update({f"inp{i}{j}": t for i, lv in enumerate(x["inp"]) for j, t in enumerate(lv)})
    return d


def kinds_of(block, x, disps, masks, loss, scale):
    out = {"weights": {n: p.grad / scale for n, p in block.named_parameters() if not n.endswith("bias")},
           "biases": {n: p.grad / scale for n, p in block.named_parameters() if n.endswith("bias")},
           "leaves": {n: t.grad / scale for n, t in leaves_of(x).items()},
           "outputs": {"loss": loss.detach().reshape(1) / scale, **{f"disp{i}": d.detach() for i, d in enumerate(disps)},
                       **{f"mask{i}": m.detach() for i, m in enumerate(masks)}}}
    return {k: {n: t.detach().double().cpu() for n, t in v.items()} for k, v in out.items()}


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


_F64 = {}


def loop_f64(case):
    """The float64 restatement of a case on the CPU, computed once and shared (never modified)."""
    if case not in _F64:
        b, h, w, iters, seed = case
        block = fresh_block("f32").cpu().double()

        class Ref:
            def __call__(self, net, inp, corr=None, disp=None, **kw):
                return block_f64_cpu(block, net, inp, corr, disp)
        x = update_train_inputs(seed, b, h, w, iters, dtype=torch.float64)
        loss, disps, masks, _ = update_train_loop(Ref(), x)
        loss.backward()
        _F64[case] = kinds_of(block, x, disps, masks, loss, 1.0)
    return _F64[case]


def loop_gpu(case, route, monkeypatch, precision="f16"):
    monkeypatch.setenv("DV_TRAIN_CONV2D", route)
    b, h, w, iters, seed = case
    block = fresh_block(precision)
    x = update_train_inputs(seed, b, h, w, iters, device="cuda")
    loss, disps, masks, _ = update_train_loop(block, x)
    (loss * SCALE).backward()
    torch.cuda.synchronize()
    return kinds_of(block, x, disps, masks, loss * SCALE, SCALE)


def rel_per_tensor(a, ref):
    return {k: {n: float((a[k][n] - ref[k][n]).norm() / ref[k][n].norm().clamp_min(1e-300)) for n in ref[k]} for k in KINDS}


@pytest.mark.parametrize("case", [(2, 16, 32, 3, 21), (2, 20, 28, 2, 22)], ids=["even_T3", "ragged_T2"])
def test_unrolled_loop_against_float64(case, monkeypatch):
    """synth.update_train_loop (B 2; 16 x 32 with T = 3, 20 x 28 with T = 2), the loss scaled by 1024: per kind the worst
    tensor's error of the HIP "f16" route against the float64 CPU restatement <= 2 x the worst tensor's error of the
    torch-autocast route.

    Measured on the MI355X (weights / biases / leaves / outputs, HIP | torch autocast):
        16 x 32, T 3   3.97e-2 / 1.34e-2 / 2.23e-2 / 1.50e-3  |  5.81e-2 / 1.98e-2 / 4.35e-2 / 3.14e-3
        20 x 28, T 2   5.94e-2 / 2.83e-2 / 4.84e-2 / 1.12e-3  |  6.27e-2 / 2.82e-2 / 4.96e-2 / 2.36e-3
    (worst tensors: encoder.convc1.weight on both routes, mask_feat_4.0.bias / gru08.convr.bias, inp0x / net0, the mask
    features).  The rule held per kind on the worst tensor; the pooled form the conditioning note of
    tests/test_gpu_update_train.py would allow was not needed."""
    ref = loop_f64(case)
    eh = rel_per_tensor(loop_gpu(case, "hip", monkeypatch), ref)
    et = rel_per_tensor(loop_gpu(case, "torch", monkeypatch), ref)
    worst = lambda e, k: max(e[k].items(), key=lambda kv: kv[1])
    for k in KINDS:
        (nh, vh), (nt, vt) = worst(eh, k), worst(et, k)
        print(f"LOOP16 {case} {k}: hip {vh:.3e} ({nh})  torch autocast {vt:.3e} ({nt})")
    bad = {k: (worst(eh, k), worst(et, k)) for k in KINDS if not worst(eh, k)[1] <= 2 * worst(et, k)[1]}
    assert not bad, bad


@pytest.fixture
def counts(monkeypatch):
    """Calls into the library's entry points, the plans and F.conv2d during one training call."""
    lib = _lib.load()
    c = {}
    for name in ("dv_conv2d_wgrad_cat_f16", "dv_conv2d_wgrad_cat_f32", "dv_conv2d_wgrad_f32", "dv_gru_reset_mul_f16",
                 "dv_gru_blend_f16", "dv_gru_reset_mul_f32", "dv_gru_blend_f32", "dv_gru_gates_bwd_blend_f32",
                 "dv_gru_gates_bwd_reset_f32", "dv_conv2d_1in_f16", "dv_conv2d_1in_f32", "dv_conv2d_1in_wgrad_f32"):
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
    wrap(S.Conv2dF16Plan, "plan16")
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


def test_what_runs_at_each_precision(monkeypatch, counts):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block("f16")
    block.plans("train16"), [m.plans("train16") for m in (block.gru04, block.gru08, block.gru16, block.encoder, block.disp_head)]
    counts.clear()
    one_training_call(block)
    # weight gradients: 3 ConvGRUs x 3, encoder convc1 / convc2 / convd2 / conv, disp_head.conv1 / conv2, mask_feat_4
    assert counts.get("dv_conv2d_wgrad_cat_f16") == 9 + 4 + 2 + 1
    assert not counts.get("dv_conv2d_wgrad_cat_f32") and not counts.get("dv_conv2d_wgrad_f32")
    assert not counts.get("F.conv2d") and not counts.get("plan") and not counts.get("pair")
    # forward: pair + candidate per ConvGRU, 4 encoder layers, 2 head layers, mask_feat_4; input gradients: 2 per ConvGRU,
    # convc2, convd2, conv, conv1, mask_feat_4
    assert counts.get("plan16") == (6 + 4 + 2 + 1) + (6 + 5)
    assert counts.get("dv_conv2d_1in_f16") == 2 and not counts.get("dv_conv2d_1in_f32")   # convd1, disp_head.conv2's dx
    assert counts.get("dv_conv2d_1in_wgrad_f32") == 1                                       # convd1 stays on it
    assert counts.get("dv_gru_reset_mul_f16") == 6 and counts.get("dv_gru_blend_f16") == 3
    assert not counts.get("dv_gru_reset_mul_f32") and not counts.get("dv_gru_blend_f32")
    assert counts.get("dv_gru_gates_bwd_blend_f32") == 3 and counts.get("dv_gru_gates_bwd_reset_f32") == 3
    block.set_train_precision("f32")                       # the other way round
    counts.clear()
    one_training_call(block)
    assert counts.get("dv_conv2d_wgrad_cat_f32") == 16 and not counts.get("dv_conv2d_wgrad_cat_f16")
    assert not counts.get("plan16") and not counts.get("dv_conv2d_1in_f16") and not counts.get("F.conv2d")
    assert not counts.get("dv_gru_reset_mul_f16") and not counts.get("dv_gru_blend_f16")
    assert counts.get("plan") and counts.get("dv_gru_blend_f32") == 3


def grads_of_one_step(block, x):
    for p in block.parameters():
        p.grad = None
    for t in leaves_of(x).values():
        t.grad = None
    loss, _, _, _ = update_train_loop(block, x)
    (loss * SCALE).backward()
    torch.cuda.synchronize()
    return {**{n: p.grad.clone() for n, p in block.named_parameters()}, **{n: t.grad.clone() for n, t in leaves_of(x).items()}}


def test_two_identical_steps_give_identical_gradient_bits(monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block("f16")
    x = update_train_inputs(31, 2, 20, 28, 2, device="cuda")
    a, b = grads_of_one_step(block, x), grads_of_one_step(block, x)
    assert len(a) == len(b) and all(torch.equal(a[n], b[n]) and torch.isfinite(a[n]).all() for n in a)


def test_optimizer_step_refreshes_the_fp16_packed_weights(monkeypatch):
    """The `train16` packed weights, forward and flipped, follow the weight key."""
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    block = fresh_block("f16")
    opt = torch.optim.AdamW(block.parameters(), lr=1e-2)
    x = update_train_inputs(5, 1, 20, 28, 1, device="cuda")
    net, mask, delta = call_block(block, x)
    first = delta.detach().clone()
    (delta.sum() + mask.sum()).backward()
    opt.step()
    net2, mask2, second = call_block(block, x)
    assert not torch.equal(first, second)
    clone = fresh_block("f16")
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
    for precision in ("f16", "f32"):
        block = fresh_block(precision, n_gru_layers=n)
        x = update_train_inputs(9, 1, 12, 20, 1, device="cuda")
        net = list(x["net"])
        if n >= 2:
            net = block(net, x["inp"], iter16=False, iter08=True, iter04=False, update=False)
        net, mask, delta = block(net, x["inp"], x["corr"][0], x["disp"], iter16=False, iter08=n >= 2, mask=False)
        assert mask is None and delta.dtype == torch.float32
        ((delta * x["m"][:, :1]).sum() * SCALE).backward()
        grads[precision] = {k: p.grad for k, p in block.named_parameters() if p.grad is not None}
    assert grads["f16"].keys() == grads["f32"].keys() and "gru04.convq.weight" in grads["f16"]
    assert ("gru08.convz.weight" in grads["f16"]) == (n >= 2) and "gru16.convz.weight" not in grads["f16"]
    assert all(torch.isfinite(g).all() for g in grads["f16"].values())
