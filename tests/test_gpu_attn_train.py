"""The bottleneck window attention of ACVNet_DDIM's hourglasses in training on HIP (diffuvolume_amd/train_attn.py,
csrc/window_attn.hip forward, csrc/window_attn_bwd.hip backward) against `oracle.acv_oracle.attention_block` under autograd
in float64 on the CPU.  The yardstick is the same oracle in float32 on the CPU.  Bar (test_gpu_regress_train.Bar): per kind
of tensor (y, dx, dWqkv, dbqkv, dWp, dbp) and per input gain, every HIP relative L2 error is at most 2x the worst float32
one of that kind and gain + 1e-6; the ratios are printed.  The weights are `_attention_weights(seed)` of test_gpu_parity.py.

Cases (x shape, input gain), the smallest that reach each path of the backward (one block per 4x4x4 window; 16-byte stores
when W % 4 == 0; the -1000 mask only when H AND W are padded):
  one_window   (1,128,4,4,4)   1    one window
  windows      (2,128,8,4,8)   1    several windows, batch 2
  h_padded     (1,128,4,6,4)   1    only H padded: mask off, padded tokens are real keys
  w_padded     (1,128,4,4,6)   1    only W padded: mask off, element stores
  both_padded  (2,128,4,5,7)   1    both padded: masked
  saturated    (2,128,4,6,20)  20   saturated softmax
  sat_masked   (1,128,4,5,7)   20   saturated softmax, masked"""
import ctypes

import pytest
import torch

from diffuvolume_amd import DiffuVolumeError, _lib, train_attn, window_attention_train
from diffuvolume_amd.submodule import window_attention
from oracle import acv_oracle as O
from test_gpu_parity import _attention_weights
from test_gpu_regress_train import Bar, rel

pytestmark = pytest.mark.gpu

CASES = {
    "one_window": ((1, 128, 4, 4, 4), 1.0),
    "windows": ((2, 128, 8, 4, 8), 1.0),
    "h_padded": ((1, 128, 4, 6, 4), 1.0),
    "w_padded": ((1, 128, 4, 4, 6), 1.0),
    "both_padded": ((2, 128, 4, 5, 7), 1.0),
    "saturated": ((2, 128, 4, 6, 20), 20.0),
    "sat_masked": ((1, 128, 4, 5, 7), 20.0),
}
KINDS = ("y", "dx", "dWqkv", "dbqkv", "dWp", "dbp")
GRADS = KINDS[1:]
NAMES = ("a.qkv_3d.weight", "a.qkv_3d.bias", "a.final1x1.weight", "a.final1x1.bias")
PAD, SENT = 37, -7.0e5                                       # 37 floats: the carved view starts 4 bytes off a 16-byte line
FN = "WindowAttentionFnBackward"


def make_inputs(name):
    """x, the four parameters and the cotangent g of a case (CPU, float32)."""
    shape, gain = CASES[name]
    idx = sorted(CASES).index(name)
    gen = torch.Generator().manual_seed(idx + 61)
    x = torch.randn(shape, generator=gen) * gain
    sd = _attention_weights(idx + 5)
    g = torch.randn(shape, generator=gen)
    return (x, *(sd[n].float() for n in NAMES), g)


def oracle(x, wq, bq, wp, bp, g, dtype):
    """The oracle and its autograd on the CPU -> the six kinds."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, wq, bq, wp, bp)]
    sd = dict(zip(NAMES, leaves[1:]))
    y = O.attention_block(leaves[0], sd, "a")
    y.backward(g.to(dtype))
    out = dict(zip(GRADS, (t.grad for t in leaves)))
    out["dWp"] = out["dWp"].reshape(128, 128)
    out["y"] = y.detach()
    return out


def run(x, wq, bq, wp, bp, g, want=(True,) * 5):
    """window_attention_train on the GPU and its backward; want = which of the five inputs require a gradient."""
    leaves = [t.detach().cuda().requires_grad_(k) for t, k in zip((x, wq, bq, wp, bp), want)]
    y = window_attention_train(*leaves)
    y.backward(g.cuda())
    out = dict(zip(GRADS, (t.grad for t in leaves)))
    if out["dWp"] is not None:
        out["dWp"] = out["dWp"].reshape(128, 128)
    out["y"] = y.detach()
    return out, y


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, float64 reference, float32 yardstick); computed once, left unchanged."""
    out = {}
    for name in CASES:
        x = make_inputs(name)
        out[name] = (x, oracle(*x, torch.float64), oracle(*x, torch.float32))
    return out


def kind_of(k, name):
    return f"{k}/gain{CASES[name][1]:g}"


def test_inputs_reach_what_they_are_meant_to_reach(refs):
    pads = {n: (CASES[n][0][3] % 4 != 0, CASES[n][0][4] % 4 != 0) for n in CASES}
    assert pads["h_padded"] == (True, False) and pads["w_padded"] == (False, True)
    assert pads["both_padded"] == (True, True) and pads["sat_masked"] == (True, True) and pads["saturated"] == (True, False)
    assert pads["one_window"] == (False, False) and pads["windows"] == (False, False)
    for name, (_, f64, _) in refs.items():                                   # every gradient is live
        assert all(bool((f64[k] != 0).any()) for k in KINDS), name


def test_values_and_gradients_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    bar = Bar()
    for name, (x, f64, f32) in refs.items():
        got, y = run(*x)
        assert y.grad_fn.name() == FN
        for k in KINDS:
            assert got[k].shape == f64[k].shape and got[k].dtype == torch.float32, (name, k)
            assert bool(torch.isfinite(got[k]).all()), (name, k)
            bar(got[k], f32[k], f64[k], kind_of(k, name), name)
    bar.check()


@pytest.mark.parametrize("name", ["h_padded", "w_padded"])
def test_padded_tokens_are_keys_the_k_and_v_thirds_of_the_bias_gradient(refs, name, monkeypatch):
    """With one of H and W whole the mask is off: real queries attend to the padded tokens, whose dK and dV rows enter
    qkv_3d.bias.grad and nothing else.  The thirds on their own, to the bar of the bias gradient.  The k third is zero in
    exact arithmetic (a constant added to every key moves every logit of a query alike; float64 leaves ~1e-16 of the
    gradient's size there), but only as the sum over ALL 64 keys of a window -- without the padded rows it is as large as
    the other thirds.  A relative error against that zero would compare rounding with rounding, so the error of the k third
    is taken relative to the norm of the whole bias gradient; the q and v thirds are relative to themselves."""
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    x, f64, f32 = refs[name]
    got, _ = run(*x)
    whole = float(f64["dbqkv"].norm())
    assert float(f64["dbqkv"][128:256].norm()) < 1e-12 * whole < float(f64["dbqkv"][256:].norm())
    for third, sl in (("q", slice(0, 128)), ("k", slice(128, 256)), ("v", slice(256, 384))):
        scale = whole if third == "k" else float(f64["dbqkv"][sl].norm())
        hip = float((got["dbqkv"][sl].double().cpu() - f64["dbqkv"][sl]).norm()) / scale
        f32_ = float((f32["dbqkv"][sl].double() - f64["dbqkv"][sl]).norm()) / scale
        bound = 2 * f32_ + 1e-6
        print(f"dbqkv[{third}] {name:10s} hip {hip:.3e}  float32 {f32_:.3e}  ratio to the bar {hip / bound:.3f}")
        assert hip <= bound, (third, hip, bound)


def test_forward_has_the_bits_of_the_eval_kernel(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    for name in ("one_window", "w_padded", "both_padded"):
        x = refs[name][0]
        got, _ = run(*x)
        with torch.no_grad():
            assert torch.equal(got["y"], window_attention(*(t.cuda() for t in x[:5]), heads=16)), name


def test_two_runs_give_the_same_bits(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    for name in ("windows", "both_padded"):
        x = refs[name][0]
        a, _ = run(*x)
        b, _ = run(*x)
        assert all(torch.equal(a[k], b[k]) for k in KINDS), name


def test_a_batch_gives_the_input_gradient_bits_of_its_items(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    for name in ("windows", "both_padded"):
        x, wq, bq, wp, bp, g = refs[name][0]
        whole, _ = run(x, wq, bq, wp, bp, g)
        for i in range(x.shape[0]):
            item, _ = run(x[i:i + 1], wq, bq, wp, bp, g[i:i + 1])
            assert torch.equal(item["dx"], whole["dx"][i:i + 1]), (name, i)
            assert torch.equal(item["y"], whole["y"][i:i + 1]), (name, i)


def test_frozen_inputs_get_no_gradient_and_leave_the_others_bit_for_bit(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    x = refs["both_padded"][0]
    full, _ = run(*x)
    for want in ((True, False, False, False, False), (False, True, True, True, True), (False, False, True, False, False),
                 (False, False, False, True, False), (False, False, False, False, True), (True, True, False, False, True)):
        got, _ = run(*x, want=want)
        assert torch.equal(got["y"], full["y"]), want
        for k, wanted in zip(GRADS, want):
            assert (got[k] is None) if not wanted else torch.equal(got[k], full[k]), (want, k)


def test_changing_the_cotangent_inside_one_window_changes_dx_only_inside_it(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    x, wq, bq, wp, bp, g = refs["windows"][0]
    base, _ = run(x, wq, bq, wp, bp, g)
    g2 = g.clone()
    g2[1, :, 4:8, 0:4, 4:8] += 1.0                                            # batch item 1, window (1, 0, 1)
    got, _ = run(x, wq, bq, wp, bp, g2)
    inside = torch.zeros(x.shape, dtype=torch.bool)
    inside[1, :, 4:8, 0:4, 4:8] = True
    inside = inside.cuda()
    assert torch.equal(got["dx"][~inside], base["dx"][~inside])
    assert bool((got["dx"][inside] != base["dx"][inside]).any())


def test_returns_a_fresh_tensor_saves_exactly_its_five_inputs_and_takes_a_strided_cotangent(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    x = refs["one_window"][0]
    leaves = [t.cuda().requires_grad_(True) for t in x[:5]]
    leaves[3] = x[3].reshape(128, 128).cuda().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = window_attention_train(*leaves)
    assert y.grad_fn.name() == FN
    assert y.data_ptr() != leaves[0].data_ptr() and y.shape == leaves[0].shape
    assert sorted(t.data_ptr() for t in saved) == sorted(t.data_ptr() for t in leaves)
    g = x[5].cuda()
    strided = g.permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)
    assert not strided.is_contiguous() and torch.equal(strided, g)
    a = torch.autograd.grad(y, leaves, g, retain_graph=True)
    b = torch.autograd.grad(y, leaves, strided, retain_graph=True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    (gx,) = torch.autograd.grad(y.sum(), leaves[0], create_graph=True)
    with pytest.raises(RuntimeError):                                        # once_differentiable: no double backward
        gx.sum().backward()


def test_torch_route_is_the_statement_and_bad_arguments_raise(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "torch")
    for name in ("w_padded", "both_padded"):
        x, f64, _ = refs[name]
        got, y = run(*x)
        assert "WindowAttentionFn" not in y.grad_fn.name()
        assert all(rel(got[k], f64[k]) < 1e-5 for k in KINDS), name
    x = [t.cuda() for t in refs["one_window"][0][:5]]
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_ATTN", route)
        with pytest.raises(TypeError):
            window_attention_train(*(t.double() for t in x))
        with pytest.raises(DiffuVolumeError):
            window_attention_train(*(t.cpu() for t in x))
        with pytest.raises(RuntimeError):
            window_attention_train(x[0], x[1][:-1], *x[2:])
        with pytest.raises(RuntimeError):
            window_attention_train(x[0][0], *x[1:])
    monkeypatch.setenv("DV_TRAIN_ATTN", "eager")
    with pytest.raises(ValueError):
        window_attention_train(*x)


def carve(t, fill=None):
    """t's values (or `fill`) in the middle of a sentinel-filled arena -> (arena, view), 4 bytes off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD,), SENT, device="cuda")
    v = arena[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return arena, v


def intact(arena, n):
    return bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + n:] == SENT).all())


@pytest.mark.parametrize("name", ["windows", "w_padded", "both_padded"])
def test_attn_bwd_abi_offset_views_bounds_and_refusals(refs, name, monkeypatch):
    """dv_window_attn3d_bwd_f32 as a C caller sees it.  x, dout, dx and the workspace one float off a 16-byte line send the
    entry to the element stores: its results hold the bar and have the bits of the aligned call.  Outputs and workspace lie
    between sentinels that survive; outputs pre-filled with NaN come back finite, so every element is written; outputs
    that are not wanted are not touched; NULL pointers, no wanted output, a missing workspace, bad sizes, unsupported
    channel / head counts and unaligned weights are refused with their codes and write nothing."""
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    lib, st = _lib.load(), _lib.stream_ptr()
    f = lib.dv_window_attn3d_bwd_f32
    shape = CASES[name][0]
    b, c, d, h, w = shape
    size = (b, c, d, h, w, 16)
    inputs, f64, f32 = refs[name]
    n_ws = lib.dv_window_attn3d_bwd_workspace_floats(*size)
    assert n_ws > 0
    want, _ = run(*inputs)
    nan = float("nan")
    x, g = carve(inputs[0].cuda())[1], carve(inputs[5].cuda())[1]
    wq, bq, wp = inputs[1].cuda(), inputs[2].cuda(), inputs[3].reshape(128, 128).cuda().contiguous()
    shapes = dict(dx=shape, dWqkv=(384, 128), dbqkv=(384,), dWp=(128, 128), dbp=(128,))
    outs = {k: carve(torch.empty(s), fill=nan) for k, s in shapes.items()}
    a_ws, v_ws = carve(torch.empty(n_ws), fill=nan)
    o = {k: v for k, (_, v) in outs.items()}
    ins = [x.data_ptr(), wq.data_ptr(), bq.data_ptr(), wp.data_ptr(), g.data_ptr()]
    ptrs = [o[k].data_ptr() for k in GRADS]
    assert f(*ins, *ptrs, v_ws.data_ptr(), *size, st) == 0
    torch.cuda.synchronize()
    bar = Bar()
    for k, (a, v) in outs.items():
        assert intact(a, v.numel()), k
        assert bool(torch.isfinite(v).all()), k
        bar(v, f32[k], f64[k], kind_of(k, name), f"{name} carved")
        assert torch.equal(v, want[k]), k
    assert intact(a_ws, n_ws)

    # every proper subset of the outputs: those not wanted and (without dqkv_w, dqkv_b, dproj_w) the workspace are not
    # touched, those wanted have the bits of the full call; the workspace may be NULL exactly when it is not needed
    null = ctypes.c_void_p(None)
    for mask in range(1, 31):
        wanted = [k for i, k in enumerate(GRADS) if mask >> i & 1]
        for v in o.values():
            v.fill_(nan)
        v_ws.fill_(nan)
        some = [ptrs[i] if mask >> i & 1 else null for i in range(5)]
        needs_ws = any(k in wanted for k in ("dWqkv", "dbqkv", "dWp"))
        if needs_ws:
            assert f(*ins, *some, null, *size, st) == -1, wanted              # a missing workspace
        assert f(*ins, *some, v_ws.data_ptr() if needs_ws else null, *size, st) == 0, wanted
        torch.cuda.synchronize()
        assert all(torch.equal(o[k], want[k]) for k in wanted), wanted
        assert all(bool(torch.isnan(o[k]).all()) for k in GRADS if k not in wanted), wanted
        assert needs_ws or bool(torch.isnan(v_ws).all()), wanted
    assert all(intact(a, v.numel()) for a, v in outs.values()) and intact(a_ws, n_ws)
    bar.check()

    # refusals: nothing is launched, nothing is written
    arenas = [a for a, _ in outs.values()] + [a_ws]
    for a in arenas:
        a.fill_(SENT)
    full = ins + ptrs + [v_ws.data_ptr()]
    for i in range(5):
        a = list(full)
        a[i] = null
        assert f(*a, *size, st) == -1, i
    assert f(*ins, null, null, null, null, null, full[10], *size, st) == -1              # nothing wanted
    for i in (0, 2, 3, 4):
        bad = list(size)
        bad[i] = 0
        assert f(*full, *bad, st) == -2, i
        bad[i] = -size[i]
        assert f(*full, *bad, st) == -2, i
    assert f(*full, b, c, 6, h, w, 16, st) == -2                                         # D % 4 != 0
    assert f(*full, b, 64, d, h, w, 16, st) == -3                                        # C = 64
    assert f(*full, b, c, d, h, w, 8, st) == -3                                          # heads = 8
    off_w = carve(wq)[1]
    assert f(ins[0], off_w.data_ptr(), *ins[2:], *ptrs, full[10], *size, st) == lib.dv_window_attn3d_f32(
        ins[0], off_w.data_ptr(), ins[2], ins[3], ins[2], ptrs[0], *size, st) != 0       # the forward's alignment code
    torch.cuda.synchronize()
    assert all(bool((a == SENT).all()) for a in arenas)


def test_the_table_names_this_file(monkeypatch):
    monkeypatch.setenv("DV_TRAIN_ATTN", "hip")
    why = _lib.VOLUME_TRAIN_SIGNATURES["dv_window_attn3d_bwd_f32"][2]
    assert why == _lib.held_by("test_gpu_attn_train.py::test_attn_bwd_abi_offset_views_bounds_and_refusals")
    assert train_attn.route() == "hip"
