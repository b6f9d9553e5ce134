"""The differentiable cost-volume builders (train_volume.build_gwc_volume_train / build_concat_volume_train: the eval
kernels forward, csrc/volume_bwd.hip backward) against the PyTorch statements they replace
(submodule._gwc_volume_autograd / _concat_volume_autograd, the latter times a scale [B,D,H,W] where one is given).

Reference: float64 autograd of the statement on the CPU.  Yardstick: the same statement in float32 on the CPU.  Bar (the
`Bar` of test_gpu_regress_train.py), per kind of tensor (vol, dref, dtgt, ds of each builder):
    rel_L2(hip, f64) <= 2 * max over the cases of rel_L2(statement_f32, f64) + 1e-6
Shapes: the smallest at which a kernel takes another path -- D = 1, each channels-per-group of the row kernel (4, 8, 12),
D not a multiple of 4, W < D, ACV's 320 channels in 40 groups, channels-per-group and odd W that only the generic kernel
takes, more than 64 quads per row, and for the concatenation H not a multiple of 4, more than one chunk of 8 channels
(the workspace route of ds) and D = 48.  Every concat shape runs plain, with zero_left and with a random scale.
Gradients of the volume are randn with about 30 % exact zeros."""
import ctypes

import pytest
import torch

from diffuvolume_amd import (_lib, build_concat_volume, build_concat_volume_train, build_gwc_volume,
                             build_gwc_volume_train, train_volume)
from diffuvolume_amd.submodule import _concat_volume_autograd, _gwc_volume_autograd
from test_gpu_regress_train import Bar, rel

pytestmark = pytest.mark.gpu

GWC_SHAPES = [(1, 32, 1, 4, 1, 4), (2, 16, 3, 8, 4, 4), (1, 64, 2, 12, 9, 8), (1, 96, 2, 8, 12, 8), (1, 320, 2, 12, 6, 40),
              (1, 24, 2, 7, 9, 8), (2, 20, 3, 10, 4, 4), (1, 32, 1, 260, 48, 4)]            # (B, C, H, W, D, G)
CONCAT_SHAPES = [(1, 1, 1, 4, 1), (2, 6, 3, 11, 5), (2, 8, 5, 8, 4), (1, 12, 2, 8, 12), (1, 32, 2, 12, 48),
                 (1, 3, 1, 260, 7)]                                                         # (B, C, H, W, D)
MODES = ("plain", "zero_left", "scale")
SENT, PAD = -7777.25, 37                    # 37 floats: a carved tensor starts 4 bytes off a 16-byte line
ALIGNED_PAD = 36                            # 36 floats: on a 16-byte line, so that the row kernels write between sentinels too


def gwc_inputs(shape):
    b, c, h, w, d, g = shape
    gen = torch.Generator().manual_seed(100 + GWC_SHAPES.index(shape))
    ref, tgt = torch.randn(b, c, h, w, generator=gen), torch.randn(b, c, h, w, generator=gen)
    dvol = torch.randn(b, g, d, h, w, generator=gen)
    dvol[torch.rand(dvol.shape, generator=gen) < 0.3] = 0.0
    return ref, tgt, dvol


def concat_inputs(shape, mode):
    b, c, h, w, d = shape
    gen = torch.Generator().manual_seed(1000 + 10 * CONCAT_SHAPES.index(shape) + MODES.index(mode))
    ref, tgt = torch.randn(b, c, h, w, generator=gen), torch.randn(b, c, h, w, generator=gen)
    scale = torch.rand(b, d, h, w, generator=gen) + 0.1 if mode == "scale" else None
    dvol = torch.randn(b, 2 * c, d, h, w, generator=gen)
    dvol[torch.rand(dvol.shape, generator=gen) < 0.3] = 0.0
    return ref, tgt, scale, dvol


def gwc_statement(ref, tgt, dvol, shape, dtype):
    ref, tgt = (t.detach().clone().to(dtype).requires_grad_(True) for t in (ref, tgt))
    vol = _gwc_volume_autograd(ref, tgt, shape[4], shape[5])
    vol.backward(dvol.to(dtype))
    return dict(vol=vol.detach(), dref=ref.grad, dtgt=tgt.grad)


def concat_statement(ref, tgt, scale, dvol, shape, mode, dtype):
    ref, tgt = (t.detach().clone().to(dtype).requires_grad_(True) for t in (ref, tgt))
    vol = _concat_volume_autograd(ref, tgt, shape[4], mode == "zero_left")
    if scale is not None:
        scale = scale.detach().clone().to(dtype).requires_grad_(True)
        vol = scale.unsqueeze(1) * vol
    vol.backward(dvol.to(dtype))
    out = dict(vol=vol.detach(), dref=ref.grad, dtgt=tgt.grad)
    if scale is not None:
        out["ds"] = scale.grad
    return out


@pytest.fixture(scope="module")
def refs():
    """Per case: inputs, float64 reference and float32 yardstick, computed once and left unchanged."""
    out = {}
    for s in GWC_SHAPES:
        x = gwc_inputs(s)
        out["gwc", s, None] = (x, gwc_statement(*x, s, torch.float64), gwc_statement(*x, s, torch.float32))
    for s in CONCAT_SHAPES:
        for m in MODES:
            x = concat_inputs(s, m)
            out["concat", s, m] = (x, concat_statement(*x, s, m, torch.float64), concat_statement(*x, s, m, torch.float32))
    return out


@pytest.fixture(scope="module")
def bounds(refs):
    """kind -> 2 * (the statement's worst float32 error of that kind) + 1e-6."""
    worst = {}
    for (builder, _, _), (_, f64, f32) in refs.items():
        for k in f64:
            worst[f"{builder}/{k}"] = max(worst.get(f"{builder}/{k}", 0.0), rel(f32[k], f64[k]))
    return {k: 2 * v + 1e-6 for k, v in worst.items()}


def gwc_run(ref, tgt, dvol, shape, want=(True, True)):
    ref, tgt = (t.detach().cuda().requires_grad_(w) for t, w in zip((ref, tgt), want))
    vol = build_gwc_volume_train(ref, tgt, shape[4], shape[5])
    vol.backward(dvol.cuda())
    return dict(vol=vol.detach(), dref=ref.grad, dtgt=tgt.grad)


def concat_run(ref, tgt, scale, dvol, shape, mode, want=(True, True, True)):
    ref, tgt = (t.detach().cuda().requires_grad_(w) for t, w in zip((ref, tgt), want))
    if scale is not None:
        scale = scale.detach().cuda().requires_grad_(want[2])
    vol = build_concat_volume_train(ref, tgt, shape[4], zero_left=mode == "zero_left", scale=scale)
    vol.backward(dvol.cuda())
    out = dict(vol=vol.detach(), dref=ref.grad, dtgt=tgt.grad)
    if scale is not None:
        out["ds"] = scale.grad
    return out


def run_case(key, x, **kw):
    builder, shape, mode = key
    return gwc_run(*x, shape, **kw) if builder == "gwc" else concat_run(*x, shape, mode, **kw)


def hold_to_the_bar(refs):
    bar = Bar()
    for key, (x, f64, f32) in refs.items():
        got = run_case(key, x)
        for k in f64:
            assert got[k].shape == f64[k].shape, (key, k)
            bar(got[k], f32[k], f64[k], f"{key[0]}/{k}", f"{key[1]} {key[2] or ''}")
    bar.check()


def test_values_and_gradients_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    hold_to_the_bar(refs)


def test_torch_route_is_the_statement_and_bad_route_raises(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_VOLUME", "torch")
    assert train_volume.route() == "torch"
    hold_to_the_bar(refs)
    ref, tgt, scale, _ = (t.cuda() for t in concat_inputs((2, 8, 5, 8, 4), "scale"))
    ref.requires_grad_(True)
    names = ("GwcVolumeFnBackward", "ConcatVolumeFnBackward")
    assert build_gwc_volume_train(ref, tgt, 4, 4).grad_fn.name() not in names
    assert build_concat_volume_train(ref, tgt, 4, scale=scale).grad_fn.name() not in names
    assert build_gwc_volume(ref, tgt, 4, 4).grad_fn.name() not in names          # the builders follow the switch
    monkeypatch.setenv("DV_TRAIN_VOLUME", "eager")
    with pytest.raises(ValueError):
        build_gwc_volume_train(ref, tgt, 4, 4)
    with pytest.raises(ValueError):
        build_concat_volume_train(ref, tgt, 4)
    monkeypatch.delenv("DV_TRAIN_VOLUME")
    assert train_volume.route() == "hip"
    assert build_gwc_volume_train(ref, tgt, 4, 4).grad_fn.name() == names[0]
    assert build_concat_volume_train(ref, tgt, 4, scale=scale).grad_fn.name() == names[1]
    assert build_gwc_volume(ref, tgt, 4, 4).grad_fn.name() == names[0]          # CUDA tensors that want a gradient
    assert build_concat_volume(ref, tgt, 4, zero_left=True).grad_fn.name() == names[1]


def test_forward_is_the_eval_builder_bit_for_bit_and_the_wedge_is_zero(refs):
    for (builder, shape, mode), (x, _, _) in refs.items():
        ref, tgt = x[0].cuda(), x[1].cuda()
        d, w = shape[4], shape[3]
        wedge = (torch.arange(w).view(1, w) < torch.arange(d).view(d, 1)).cuda()          # [D,W]: x < d
        if builder == "gwc":
            vol = build_gwc_volume_train(ref.clone().requires_grad_(True), tgt, d, shape[5])
            with torch.no_grad():
                assert torch.equal(vol.detach(), build_gwc_volume(ref, tgt, d, shape[5])), shape
            assert not bool(vol.detach()[:, :, wedge.unsqueeze(1).expand(d, shape[2], w)].any()), shape
            continue
        c = shape[1]
        scale = None if x[2] is None else x[2].cuda()
        vol = build_concat_volume_train(ref.clone().requires_grad_(True), tgt, d, zero_left=mode == "zero_left", scale=scale)
        assert vol.requires_grad
        with torch.no_grad():
            ev = build_concat_volume(ref, tgt, d, zero_left=mode == "zero_left")
            if scale is not None:                              # one product per element: the eval path's dv_mul_f32 order
                ev = scale.unsqueeze(1) * ev
        assert torch.equal(vol.detach(), ev), (shape, mode)
        m = wedge.unsqueeze(1).expand(d, shape[2], w)
        assert not bool(vol.detach()[:, c:][:, :, m].any()), (shape, mode)
        if mode == "zero_left":
            assert not bool(vol.detach()[:, :c][:, :, m].any()), shape


def test_backward_repeats_and_a_batch_is_its_items(refs):
    for key, (x, _, _) in refs.items():
        first, again = run_case(key, x), run_case(key, x)
        for k in first:
            assert torch.equal(first[k], again[k]), (key, k)
        if key[1][0] != 2:
            continue
        items = [run_case((key[0], (1,) + key[1][1:], key[2]), tuple(None if t is None else t[i:i + 1] for t in x))
                 for i in range(2)]
        for k in first:
            assert torch.equal(first[k], torch.cat([items[0][k], items[1][k]])), (key, k)


def test_zero_gradient_gives_exact_zeros(refs):
    for key, (x, _, _) in refs.items():
        got = run_case(key, x[:-1] + (torch.zeros_like(x[-1]),))
        for k in got:
            if k != "vol":
                assert torch.equal(got[k], torch.zeros_like(got[k])), (key, k)


def test_a_frozen_side_gets_none_and_the_other_sides_bits_are_unchanged(refs):
    for key, (x, _, _) in refs.items():
        full = run_case(key, x)
        grads = [k for k in full if k != "vol"]
        for i, frozen in enumerate(grads):
            want = tuple(j != i for j in range(3 if key[0] == "concat" else 2))
            got = run_case(key, x, want=want)
            assert got[frozen] is None, (key, frozen)
            for k in grads:
                if k != frozen:
                    assert torch.equal(got[k], full[k]), (key, frozen, k)


def test_a_non_contiguous_gradient_is_accepted(refs):
    for key in (("gwc", (2, 16, 3, 8, 4, 4), None), ("concat", (2, 8, 5, 8, 4), "scale"), ("concat", (2, 6, 3, 11, 5), "plain")):
        x, _, _ = refs[key]
        dvol = x[-1]
        strided = torch.empty(dvol.shape + (2,), device="cuda")[..., 0]
        strided.copy_(dvol)
        assert not strided.is_contiguous()
        want, got = run_case(key, x), run_case(key, x[:-1] + (strided,))
        for k in want:
            assert torch.equal(want[k], got[k]), (key, k)


def carve(t, pad=PAD):
    """t's values in the middle of a sentinel-filled arena -> (arena, view): 4 bytes off a 16-byte line with PAD, on one
    with ALIGNED_PAD."""
    arena = torch.full((t.numel() + 2 * pad,), SENT, device="cuda")
    v = arena[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * pad) % 16 and v.is_contiguous()
    return arena, v


def intact(arena, n, written, pad=PAD):
    """The sentinel survives outside the carved tensor and, if the tensor was written, nowhere inside."""
    ok = bool((arena[:pad] == SENT).all()) and bool((arena[pad + n:] == SENT).all())
    return ok and (not written or not bool((arena[pad:pad + n] == SENT).any()))


@pytest.mark.parametrize("shape", [(2, 16, 3, 8, 4, 4), (1, 96, 2, 8, 12, 8), (1, 24, 2, 7, 9, 8)])
def test_gwc_abi_offset_views_bounds_and_refusals(refs, bounds, shape):
    """dv_gwc_volume_bwd_f32 as a C caller sees it: operands 4 bytes off a 16-byte line (the generic kernel) agree with
    the aligned run to the bar, both outputs lie between sentinels that survive, and NULL pointers, both outputs NULL and
    bad shapes are refused with their codes and write nothing."""
    lib = _lib.load()
    b, c, h, w, d, g = shape
    (ref, tgt, dvol), f64, _ = refs["gwc", shape, None]
    ref, tgt, dvol = ref.cuda(), tgt.cuda(), dvol.cuda()
    dims, st = (b, c, h, w, d, g), _lib.stream_ptr()
    (g_ref, dref), (g_tgt, dtgt) = carve(ref, ALIGNED_PAD), carve(tgt, ALIGNED_PAD)
    g_ref.fill_(SENT), g_tgt.fill_(SENT)
    assert lib.dv_gwc_volume_bwd_f32(ref.data_ptr(), tgt.data_ptr(), dvol.data_ptr(), dref.data_ptr(), dtgt.data_ptr(), *dims, st) == 0
    torch.cuda.synchronize()
    assert intact(g_ref, ref.numel(), True, ALIGNED_PAD) and intact(g_tgt, tgt.numel(), True, ALIGNED_PAD)
    (_, oref), (_, otgt), (_, odvol) = carve(ref), carve(tgt), carve(dvol)
    a_ref, v_ref = carve(dref)
    a_tgt, v_tgt = carve(dtgt)
    a_ref.fill_(SENT), a_tgt.fill_(SENT)
    assert lib.dv_gwc_volume_bwd_f32(oref.data_ptr(), otgt.data_ptr(), odvol.data_ptr(), v_ref.data_ptr(), v_tgt.data_ptr(), *dims, st) == 0
    torch.cuda.synchronize()
    assert intact(a_ref, ref.numel(), True) and intact(a_tgt, tgt.numel(), True)
    for got in ((dref, dtgt), (v_ref, v_tgt)):
        assert rel(got[0], f64["dref"]) <= bounds["gwc/dref"] and rel(got[1], f64["dtgt"]) <= bounds["gwc/dtgt"]
    # one side only: the other arena is not touched, the bits of the wanted side do not change
    keep = v_ref.clone()
    a_ref.fill_(SENT), a_tgt.fill_(SENT)
    assert lib.dv_gwc_volume_bwd_f32(oref.data_ptr(), otgt.data_ptr(), odvol.data_ptr(), v_ref.data_ptr(), None, *dims, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(v_ref, keep) and bool((a_tgt == SENT).all())

    a_ref.fill_(SENT), a_tgt.fill_(SENT)
    ptrs = [ref.data_ptr(), tgt.data_ptr(), dvol.data_ptr(), v_ref.data_ptr(), v_tgt.data_ptr()]
    null = ctypes.c_void_p(None)
    for i in range(3):
        a = list(ptrs)
        a[i] = null
        assert lib.dv_gwc_volume_bwd_f32(*a, *dims, st) == -1
    assert lib.dv_gwc_volume_bwd_f32(*ptrs[:3], null, null, *dims, st) == -1
    assert lib.dv_error_string(-1).decode().lower().count("null")
    for i in range(6):
        bad = list(dims)
        bad[i] = 0
        assert lib.dv_gwc_volume_bwd_f32(*ptrs, *bad, st) == -2
    assert lib.dv_gwc_volume_bwd_f32(*ptrs, b, c, h, w, d, c + 1, st) == -2          # C % G != 0
    torch.cuda.synchronize()
    assert bool((a_ref == SENT).all()) and bool((a_tgt == SENT).all())          # a refused call writes nothing


@pytest.mark.parametrize("shape,mode", [((2, 8, 5, 8, 4), "scale"), ((1, 12, 2, 8, 12), "scale"), ((1, 12, 2, 8, 12), "zero_left"),
                                        ((2, 6, 3, 11, 5), "scale"), ((1, 32, 2, 12, 48), "plain")])
def test_concat_abi_offset_views_bounds_and_refusals(refs, bounds, shape, mode):
    """dv_concat_volume_bwd_f32 as a C caller sees it: see test_gwc_abi_offset_views_bounds_and_refusals; the workspace of
    dv_concat_volume_bwd_workspace_floats lies between sentinels too."""
    lib = _lib.load()
    b, c, h, w, d = shape
    (ref, tgt, scale, dvol), f64, _ = refs["concat", shape, mode]
    ref, tgt, dvol = ref.cuda(), tgt.cuda(), dvol.cuda()
    scale = None if scale is None else scale.cuda()
    dims, st = (b, c, h, w, d, int(mode == "zero_left")), _lib.stream_ptr()
    n_ws = lib.dv_concat_volume_bwd_workspace_floats(b, c, h, w, d)
    chunks = (c + 7) // 8
    assert n_ws == (chunks * b * d * h * w if w % 4 == 0 and chunks > 1 else 0)
    for bad in ((0, c, h, w, d), (b, 0, h, w, d), (b, c, -1, w, d), (b, c, h, 0, d), (b, c, h, w, 0)):
        assert lib.dv_concat_volume_bwd_workspace_floats(*bad) == 0
    kinds = ["dref", "dtgt"] + (["ds"] if scale is not None else [])
    like = dict(dref=ref, dtgt=tgt, ds=scale)

    def call(ins, outs, ws):
        code = lib.dv_concat_volume_bwd_f32(ins[0].data_ptr(), ins[1].data_ptr(), _lib.ptr(ins[2]), ins[3].data_ptr(),
                                            *(_lib.ptr(outs.get(k)) for k in ("dref", "dtgt", "ds")), _lib.ptr(ws), *dims, st)
        torch.cuda.synchronize()
        return code

    guards = {k: carve(like[k], ALIGNED_PAD) for k in kinds}
    aligned = {k: v for k, (_, v) in guards.items()}
    g_ws, ws = carve(torch.empty(n_ws), ALIGNED_PAD) if n_ws and scale is not None else (None, None)
    for a, _ in list(guards.values()) + ([(g_ws, None)] if ws is not None else []):
        a.fill_(SENT)
    assert call((ref, tgt, scale, dvol), aligned, ws) == 0
    for k, (a, v) in guards.items():
        assert intact(a, v.numel(), True, ALIGNED_PAD), k
    if ws is not None:                                        # the row kernel's chunk sums: all of it, nothing beyond
        assert intact(g_ws, n_ws, True, ALIGNED_PAD)
    offs = tuple(None if t is None else carve(t)[1] for t in (ref, tgt, scale, dvol))
    arenas = {k: carve(like[k]) for k in kinds}
    a_ws, v_ws = carve(torch.empty(n_ws)) if ws is not None else (None, None)
    for a, _ in list(arenas.values()) + ([(a_ws, None)] if ws is not None else []):
        a.fill_(SENT)
    assert call(offs, {k: v for k, (_, v) in arenas.items()}, v_ws) == 0
    for k, (a, v) in arenas.items():
        assert intact(a, v.numel(), True), k
        for got in (aligned[k], v):
            assert rel(got, f64[k]) <= bounds[f"concat/{k}"], k
    if ws is not None:
        assert intact(a_ws, n_ws, False)                      # the generic kernels the offset views take leave it alone
        # the aligned operands with the workspace between sentinels (4 bytes off: the generic kernels again)
        assert call((ref, tgt, scale, dvol), aligned, v_ws) == 0 and intact(a_ws, n_ws, False)
    # a single output: the others are not touched, its bits do not change
    keep = arenas["dtgt"][1].clone()
    for a, _ in arenas.values():
        a.fill_(SENT)
    assert call(offs, {"dtgt": arenas["dtgt"][1]}, None) == 0
    assert torch.equal(arenas["dtgt"][1], keep) and bool((arenas["dref"][0] == SENT).all())

    for a, _ in arenas.values():
        a.fill_(SENT)
    outs = {k: v for k, (_, v) in arenas.items()}
    null = ctypes.c_void_p(None)
    o = [_lib.ptr(outs.get(k)) for k in ("dref", "dtgt", "ds")]
    f = lib.dv_concat_volume_bwd_f32
    assert f(ref.data_ptr(), tgt.data_ptr(), _lib.ptr(scale), null, *o, _lib.ptr(ws), *dims, st) == -1          # dvol
    assert f(ref.data_ptr(), tgt.data_ptr(), _lib.ptr(scale), dvol.data_ptr(), null, null, null, _lib.ptr(ws), *dims, st) == -1
    for i in range(5):
        bad = list(dims)
        bad[i] = 0
        assert f(ref.data_ptr(), tgt.data_ptr(), _lib.ptr(scale), dvol.data_ptr(), *o, _lib.ptr(ws), *bad, st) == -2
    if scale is not None:
        assert f(ref.data_ptr(), tgt.data_ptr(), null, dvol.data_ptr(), *o, _lib.ptr(ws), *dims, st) == -1      # ds without s
        assert f(null, tgt.data_ptr(), scale.data_ptr(), dvol.data_ptr(), *o, _lib.ptr(ws), *dims, st) == -1    # ds without ref
        assert f(ref.data_ptr(), null, scale.data_ptr(), dvol.data_ptr(), *o, _lib.ptr(ws), *dims, st) == -1    # ds without tgt
        assert f(ref.data_ptr(), tgt.data_ptr(), scale.data_ptr(), dvol.data_ptr(), *o, _lib.ptr(ws), b, c, h, w, d, 1, st) == -3
        if n_ws:
            assert f(ref.data_ptr(), tgt.data_ptr(), scale.data_ptr(), dvol.data_ptr(), *o, null, *dims, st) == -1
    else:
        assert f(ref.data_ptr(), tgt.data_ptr(), null, dvol.data_ptr(), o[0], o[1], o[0], null, *dims, st) == -1    # ds without s
        assert f(null, null, null, dvol.data_ptr(), o[0], o[1], null, null, *dims, st) == 0       # ref / tgt only serve ds
        torch.cuda.synchronize()
        assert torch.equal(outs["dref"], aligned["dref"]) or rel(outs["dref"], f64["dref"]) <= bounds["concat/dref"]
        for a, _ in arenas.values():
            a.fill_(SENT)
    torch.cuda.synchronize()
    for k, (a, _) in arenas.items():
        assert bool((a == SENT).all()), k                                        # a refused call writes nothing


@pytest.mark.parametrize("which", ["gwc", "concat"])
def test_backward_allocates_its_outputs_and_the_declared_workspace_only(which, monkeypatch):
    """A condition, not a measurement: during backward the peak grows by less than the gradients handed back + the
    declared workspace + 1 MiB -- nothing of the volume's size (3 MiB / 6 MiB here) is allocated."""
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    b, c, h, w, d = 2, 16, 16, 64, 24
    ref = torch.randn(b, c, h, w, device="cuda").requires_grad_(True)
    tgt = torch.randn(b, c, h, w, device="cuda").requires_grad_(True)
    scale = torch.rand(b, d, h, w, device="cuda").requires_grad_(True)

    def forward():
        if which == "gwc":
            return build_gwc_volume_train(ref, tgt, 4 * d, 4)          # [2,4,96,16,64]: 3 MiB
        return build_concat_volume_train(ref, tgt, d, scale=scale)          # [2,32,24,16,64]: 6 MiB

    vol = forward()
    g = torch.randn_like(vol)
    vol.backward(g)                                              # library loaded, allocator warm
    ref.grad = tgt.grad = scale.grad = None
    vol = forward()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    vol.backward(g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    outputs = 4 * (ref.numel() + tgt.numel() + (scale.numel() if which == "concat" else 0))
    n_ws = 4 * _lib.load().dv_concat_volume_bwd_workspace_floats(b, c, h, w, d) if which == "concat" else 0
    print(f"{which}: peak growth {grown} B; outputs {outputs} B, workspace {n_ws} B, the volume {4 * vol.numel()} B")
    assert which == "gwc" or n_ws == 4 * 2 * scale.numel()
    assert grown < outputs + n_ws + (1 << 20) < 4 * vol.numel()


def test_refusals_of_the_python_functions():
    ref = torch.randn(1, 8, 2, 4, device="cuda", requires_grad=True)
    tgt = torch.randn(1, 8, 2, 4, device="cuda")
    with pytest.raises(TypeError):
        build_gwc_volume_train(ref.double(), tgt.double(), 2, 4)
    with pytest.raises(_lib.DiffuVolumeError):
        build_concat_volume_train(ref.detach().cpu(), tgt.cpu(), 2)
    with pytest.raises(RuntimeError):
        build_gwc_volume_train(ref, tgt[:, :4], 2, 4)
    with pytest.raises(RuntimeError):
        build_concat_volume_train(ref, tgt, 2, scale=torch.ones(1, 3, 2, 4, device="cuda"))
    with pytest.raises(RuntimeError):
        build_concat_volume_train(ref, tgt, 2, zero_left=True, scale=torch.ones(1, 2, 2, 4, device="cuda"))
    vol = build_gwc_volume_train(ref, tgt, 2, 4)
    (grad,) = torch.autograd.grad(vol.sum(), ref, create_graph=True)
    with pytest.raises(RuntimeError):                          # once_differentiable: no double backward
        grad.sum().backward()
