"""The differentiable warp + correlation of PWCNet_ddim's refinement input (train_refine.warp_corr_train: csrc/warp_corr.hip
forward and backward) against the PyTorch statements it replaces (pwcnet_ddim.warp + groupwise_corr_pm).

Reference: float64 autograd of the statements on the CPU.  Yardstick: the same statements in float32 on the CPU.  Bar (the
`Bar` of test_gpu_regress_train.py), per kind of tensor (diff, corr, dleft, dright, ddisp):
    rel_L2(hip, f64) <= 2 * max over the cases of rel_L2(statement_f32, f64) + 1e-6
Shapes: the smallest live one (W = 24), a tile whose wrap-around columns overlap it, two and three tiles of 128 columns
with their halos, all 32 channels (two LDS chunks of 16) with negative disparities, every output column sampling the same
two source columns (fan-in), samples far outside the image, zero disparity, and H = 1, 2, where the reference's grid
makes every pixel invalid (rows 0 and H-1 always are).  Gradients are randn with about 30 % exact zeros.

`warp` takes two hard decisions: floor() of the sample column (it fixes ddisp) and the 0.999 validity.  Both sit where the
fractional part of ix = (x - d) W / (W - 1) - 0.5 is within 1e-3 of an integer, so disp is nudged by 2^-7 until that
fractional part lies in [2e-3, 1 - 2e-3] at every pixel; no pixel is left out of any comparison."""
import ctypes

import pytest
import torch

from diffuvolume_amd import DiffuVolumeError, _lib, train_refine, warp_corr_train
from diffuvolume_amd.pwcnet_ddim import groupwise_corr_pm, warp
from diffuvolume_amd.submodule import refine_inputs
from test_gpu_pcw_train import check_step, fresh_model, gold, step  # noqa: F401  (gold is a fixture)
from test_gpu_regress_train import Bar, rel

pytestmark = pytest.mark.gpu

MD = 24
CASES = {                                                   # name: ((B, C, H, W), disparity)
    "smallest": ((1, 1, 3, 24), "u0_6"),
    "wrap_overlaps_tile": ((2, 3, 3, 25), "u0_30"),
    "two_tiles": ((1, 20, 4, 150), "u0_30"),
    "full_channels_negative": ((1, 32, 5, 40), "u-30_30"),
    "fan_in": ((1, 8, 3, 64), "fan"),
    "three_tiles_far_outside": ((2, 5, 4, 300), "wide"),
    "zero_disparity": ((1, 4, 4, 32), "zero"),
    "all_invalid_h1": ((1, 4, 1, 32), "u0_30"),
    "all_invalid_h2": ((1, 4, 2, 32), "u0_30"),
}
LIVE = [k for k in CASES if not k.startswith("all_invalid")]
KINDS = ("diff", "corr", "dleft", "dright", "ddisp")
SENT, PAD = -7777.25, 37                    # 37 floats: a carved tensor starts 4 bytes off a 16-byte line


def frac_ix(disp):
    """Fractional part of the float64 sample column of every pixel."""
    w = disp.shape[-1]
    x = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    ix = (x - disp.double()) * w / (w - 1) - 0.5
    return ix - torch.floor(ix)


def near_a_decision(disp):
    f = frac_ix(disp)
    return (f < 2e-3) | (f > 1 - 2e-3)


def make_inputs(name):
    (b, c, h, w), kind = CASES[name]
    gen = torch.Generator().manual_seed(4200 + list(CASES).index(name))
    left, right = torch.randn(b, c, h, w, generator=gen), torch.randn(b, c, h, w, generator=gen)
    r = torch.rand(b, 1, h, w, generator=gen)
    x = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    disp = {"u0_6": 6 * r, "u0_30": 30 * r, "u-30_30": 60 * r - 30, "fan": x - 3.3 + 0.2 * r,
            "wide": w * r - w / 4, "zero": torch.zeros_like(r)}[kind].contiguous()
    for _ in range(64):
        bad = near_a_decision(disp)
        if not bool(bad.any()):
            break
        disp = torch.where(bad, disp + 2.0 ** -7, disp)
    assert not bool(near_a_decision(disp).any()), name
    g_diff, g_corr = torch.randn(b, c, h, w, generator=gen), torch.randn(b, 2 * MD + 1, h, w, generator=gen)
    g_diff[torch.rand(g_diff.shape, generator=gen) < 0.3] = 0.0
    g_corr[torch.rand(g_corr.shape, generator=gen) < 0.3] = 0.0
    return left, right, disp, g_diff, g_corr


def statement(left, right, disp, g_diff, g_corr, dtype):
    left, right, disp = (t.detach().clone().to(dtype).requires_grad_(True) for t in (left, right, disp))
    warped = warp(right, disp)
    diff, corr = left - warped, groupwise_corr_pm(left, warped, MD)
    torch.autograd.backward([diff, corr], [g_diff.to(dtype), g_corr.to(dtype)])
    return dict(diff=diff.detach(), corr=corr.detach(), dleft=left.grad, dright=right.grad, ddisp=disp.grad)


def valid_pixels(right, disp):
    """[B,1,H,W] bool: where the reference's mask is 1 (float64)."""
    with torch.no_grad():
        return warp(torch.ones_like(right[:, :1]).double(), disp.double()) > 0


@pytest.fixture(scope="module")
def refs():
    """Per case: inputs, float64 reference, float32 yardstick and the validity, computed once and left unchanged."""
    out = {}
    for name in CASES:
        x = make_inputs(name)
        out[name] = (x, statement(*x, torch.float64), statement(*x, torch.float32), valid_pixels(x[1], x[2]))
    return out


@pytest.fixture(scope="module")
def bounds(refs):
    worst = {k: max(rel(f32[k], f64[k]) for _, f64, f32, _ in refs.values()) for k in KINDS}
    return {k: 2 * v + 1e-6 for k, v in worst.items()}


def run(left, right, disp, g_diff, g_corr, want=(True, True, True)):
    left, right, disp = (t.detach().cuda().requires_grad_(w) for t, w in zip((left, right, disp), want))
    diff, corr = warp_corr_train(left, right, disp)
    torch.autograd.backward([diff, corr], [g_diff.cuda(), g_corr.cuda()])
    return dict(diff=diff.detach(), corr=corr.detach(), dleft=left.grad, dright=right.grad, ddisp=disp.grad)


def hold_to_the_bar(refs):
    bar = Bar()
    for name, (x, f64, f32, _) in refs.items():
        got = run(*x)
        for k in KINDS:
            assert got[k].shape == f64[k].shape, (name, k)
            bar(got[k], f32[k], f64[k], k, f"{name} {CASES[name][0]}")
    bar.check()


def test_inputs_are_live_and_away_from_the_decisions(refs):
    for name, (x, f64, f32, valid) in refs.items():
        assert not bool(near_a_decision(x[2]).any()), name
        share, tail = float(valid.double().mean()), float(valid[..., -MD:].double().mean())
        print(f"{name}: valid pixels {share:.2f}, of the last {MD} columns {tail:.2f}")
        if name in LIVE:
            assert share >= 0.10 and tail >= 0.10, name              # a kernel that zeroes everything cannot pass
            assert all(float(f64[k].abs().max()) > 0 for k in KINDS), name
        else:
            assert share == 0.0, name
        # the float32 statement takes the same decisions as the float64 one
        assert torch.equal(f32["diff"] == x[0], f64["diff"] == x[0].double()), name


def test_values_and_gradients_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    hold_to_the_bar(refs)


def test_all_invalid_rows_give_exact_values(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    for name in ("all_invalid_h1", "all_invalid_h2"):
        x = refs[name][0]
        got = run(*x)
        assert torch.equal(got["diff"], x[0].cuda()), name
        for k in ("corr", "dright", "ddisp"):
            assert torch.equal(got[k], torch.zeros_like(got[k])), (name, k)
        assert torch.equal(got["dleft"], x[3].cuda()), name         # only g_diff reaches left


def test_forward_has_the_bits_of_the_eval_kernel(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    for name, (x, *_) in refs.items():
        left, right, disp = (t.cuda() for t in x[:3])
        c = left.shape[1]
        diff, corr = warp_corr_train(left.clone().requires_grad_(True), right, disp)
        assert diff.requires_grad and corr.requires_grad
        gen = torch.Generator().manual_seed(7)
        du_a, du_b = torch.randn(c, generator=gen).cuda(), torch.randn(c, generator=gen).cuda()
        with torch.no_grad():
            ev = refine_inputs(left, right, disp, du_a, du_b, MD)
        assert torch.equal(diff.detach(), ev[:, :c]), name
        assert torch.equal(corr.detach(), ev[:, 3 * c + 1:]), name


def test_a_single_wanted_input_gets_the_bits_of_the_full_run(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    grads = ("dleft", "dright", "ddisp")
    for name, (x, *_) in refs.items():
        full = run(*x)
        for i, k in enumerate(grads):
            got = run(*x, want=tuple(j == i for j in range(3)))
            assert torch.equal(got[k], full[k]), (name, k)
            assert all(got[o] is None for o in grads if o != k), (name, k)
            assert torch.equal(got["diff"], full["diff"]) and torch.equal(got["corr"], full["corr"])


def test_backward_repeats_and_a_batch_is_its_items(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    for name, (x, *_) in refs.items():
        first, again = run(*x), run(*x)
        for k in KINDS:
            assert torch.equal(first[k], again[k]), (name, k)
        if CASES[name][0][0] != 2:
            continue
        items = [run(*(t[i:i + 1] for t in x)) for i in range(2)]
        for k in KINDS:
            assert torch.equal(first[k], torch.cat([items[0][k], items[1][k]])), (name, k)


def test_invalid_pixels_pass_no_gradient_to_right_and_disp(refs, monkeypatch):
    """ddisp is exactly 0 where diff == left, and whatever gradient arrives at an invalid pixel of the warped map -- g_diff
    there, and every g_corr entry whose partner in the warped map is that pixel -- changes no bit of dright and ddisp."""
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    for name, (x, _, _, valid) in refs.items():
        left, right, disp, g_diff, g_corr = x
        w = left.shape[-1]
        first = run(*x)
        untouched = (first["diff"] == left.cuda()).all(dim=1, keepdim=True)
        assert torch.equal(untouched.cpu(), ~valid), name
        assert not bool(first["ddisp"][untouched].any()), name
        gen = torch.Generator().manual_seed(99)
        inval = ~valid                                              # [B,1,H,W]
        g_diff2 = torch.where(inval, torch.randn(g_diff.shape, generator=gen), g_diff)
        hit = torch.zeros(g_corr.shape, dtype=torch.bool)
        for i in range(0, MD + 1):                                  # corr[i+MD, x] pairs left[x] with warped[x-i]
            hit[:, i + MD, :, i:] = inval[:, 0, :, :w - i]
        for k in range(1, MD + 1):                                  # corr[MD-k, x], x < k, pairs left[x] with warped[W-k+x]
            hit[:, MD - k, :, :k] = inval[:, 0, :, w - k:]
        g_corr2 = torch.where(hit, torch.randn(g_corr.shape, generator=gen), g_corr)
        assert name not in LIVE or (bool(hit.any()) and not torch.equal(g_corr2, g_corr))
        second = run(left, right, disp, g_diff2, g_corr2)
        assert torch.equal(second["dright"], first["dright"]) and torch.equal(second["ddisp"], first["ddisp"]), name
        assert not torch.equal(second["dleft"], first["dleft"]) or not bool(inval.any()), name


def carve(t):
    """t's values in the middle of a sentinel-filled arena -> (arena, view), 4 bytes off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD,), SENT, device="cuda")
    v = arena[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return arena, v


def intact(arena, n, written):
    """The sentinel survives outside the carved tensor and, if the tensor was written, nowhere inside."""
    ok = bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + n:] == SENT).all())
    return ok and (not written or not bool((arena[PAD:PAD + n] == SENT).any()))


@pytest.mark.parametrize("name", ["wrap_overlaps_tile", "two_tiles", "three_tiles_far_outside"])
def test_warp_corr_abi_offset_views_bounds_and_refusals(refs, bounds, name):
    """dv_warp_corr_f32 and dv_warp_corr_bwd_f32 as a C caller sees them: every operand 4 bytes off a 16-byte line gives
    the bits of the aligned run, outputs and workspace lie between sentinels that survive, and NULL pointers, no wanted
    output, a wanted dright without workspace, bad shapes and unsupported C / maxshift / W are refused with their codes
    and write nothing."""
    lib = _lib.load()
    x, f64, _, _ = refs[name]
    b, c, h, w = CASES[name][0]
    want = run(*x)
    left, right, disp, g_diff, g_corr = (carve(t.cuda())[1] for t in x)
    dims, st = (b, c, h, w, MD), _lib.stream_ptr()
    n_ws = lib.dv_warp_corr_bwd_workspace_floats(b, c, h, w)
    assert n_ws == b * c * h * w
    like = dict(diff=left, corr=g_corr, dleft=left, dright=right, ddisp=disp)
    arenas = {k: carve(torch.empty_like(like[k])) for k in KINDS}
    a_ws, v_ws = carve(torch.empty(n_ws))

    def refill():
        for a, _ in arenas.values():
            a.fill_(SENT)
        a_ws.fill_(SENT)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((a == SENT).all()) for a, _ in arenas.values()) and bool((a_ws == SENT).all())

    out = {k: v for k, (_, v) in arenas.items()}
    ins = [t.data_ptr() for t in (left, right, disp)]
    gs = [g_diff.data_ptr(), g_corr.data_ptr()]
    refill()
    assert lib.dv_warp_corr_f32(*ins, out["diff"].data_ptr(), out["corr"].data_ptr(), *dims, st) == 0
    assert lib.dv_warp_corr_bwd_f32(*ins, *gs, out["dleft"].data_ptr(), out["dright"].data_ptr(), out["ddisp"].data_ptr(),
                                    v_ws.data_ptr(), *dims, st) == 0
    torch.cuda.synchronize()
    for k, (a, v) in arenas.items():
        assert intact(a, v.numel(), True), k
        assert torch.equal(v, want[k]) and rel(v, f64[k]) <= bounds[k], k
    assert intact(a_ws, n_ws, True)
    # a single output: nothing else is touched (the workspace only serves dright), its bits do not change
    for k in ("dleft", "dright", "ddisp"):
        refill()
        ptrs = [out[o].data_ptr() if o == k else None for o in ("dleft", "dright", "ddisp")]
        assert lib.dv_warp_corr_bwd_f32(*ins, *gs, *ptrs, v_ws.data_ptr(), *dims, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(out[k], want[k]) and intact(arenas[k][0], out[k].numel(), True), k
        assert all(bool((arenas[o][0] == SENT).all()) for o in KINDS if o != k), k
        assert intact(a_ws, n_ws, k == "dright") and (k == "dright" or bool((a_ws == SENT).all())), k
    refill()
    assert lib.dv_warp_corr_bwd_f32(*ins, *gs, out["dleft"].data_ptr(), None, out["ddisp"].data_ptr(), None, *dims, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out["dleft"], want["dleft"]) and torch.equal(out["ddisp"], want["ddisp"])

    refill()
    null = ctypes.c_void_p(None)
    fwd = ins + [out["diff"].data_ptr(), out["corr"].data_ptr()]
    bwd = ins + gs + [out["dleft"].data_ptr(), out["dright"].data_ptr(), out["ddisp"].data_ptr(), v_ws.data_ptr()]
    for i in range(5):
        a = list(fwd)
        a[i] = null
        assert lib.dv_warp_corr_f32(*a, *dims, st) == -1
        a = list(bwd)
        a[i] = null
        assert lib.dv_warp_corr_bwd_f32(*a, *dims, st) == -1
    assert lib.dv_warp_corr_bwd_f32(*bwd[:5], null, null, null, bwd[8], *dims, st) == -1          # nothing wanted
    assert lib.dv_warp_corr_bwd_f32(*bwd[:8], null, *dims, st) == -1                               # dright without workspace
    assert lib.dv_error_string(-1).decode().lower().count("null")
    for i in range(4):
        bad = list(dims)
        bad[i] = 0
        assert lib.dv_warp_corr_f32(*fwd, *bad, st) == -2 and lib.dv_warp_corr_bwd_f32(*bwd, *bad, st) == -2
    for bad in ((65536, c, h, w, MD), (b, c, 65536, w, MD)):
        assert lib.dv_warp_corr_f32(*fwd, *bad, st) == -2 and lib.dv_warp_corr_bwd_f32(*bwd, *bad, st) == -2
    for bad in ((b, 33, h, w, MD), (b, c, h, w, MD - 1), (b, c, h, w, MD + 1), (b, c, h, MD - 1, MD)):
        assert lib.dv_warp_corr_f32(*fwd, *bad, st) == -3 and lib.dv_warp_corr_bwd_f32(*bwd, *bad, st) == -3
    assert untouched()                                                       # a refused call writes nothing


def test_torch_route_is_the_statement_and_bad_route_raises(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "torch")
    assert train_refine.route() == "torch"
    hold_to_the_bar(refs)
    x = refs["two_tiles"][0]
    left, right, disp = (t.cuda().requires_grad_(True) for t in x[:3])
    diff, corr = warp_corr_train(left, right, disp)
    assert "WarpCorrFn" not in diff.grad_fn.name() and "WarpCorrFn" not in corr.grad_fn.name()
    warped = warp(right, disp)
    assert torch.equal(diff, left - warped) and torch.equal(corr, groupwise_corr_pm(left, warped, MD))
    monkeypatch.setenv("DV_TRAIN_REFINE", "eager")
    with pytest.raises(ValueError):
        warp_corr_train(left, right, disp)
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    diff, corr = warp_corr_train(left, right, disp)
    assert diff.grad_fn.name() == "WarpCorrFnBackward" and corr.grad_fn is diff.grad_fn


def test_refusals_and_empty_tensors_of_the_python_function(monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", "hip")
    left = torch.randn(1, 4, 2, 24, device="cuda", requires_grad=True)
    right, disp = torch.randn(1, 4, 2, 24, device="cuda"), torch.rand(1, 1, 2, 24, device="cuda")
    with pytest.raises(TypeError):
        warp_corr_train(left.double(), right.double(), disp.double())
    with pytest.raises(DiffuVolumeError):
        warp_corr_train(left.detach().cpu(), right.cpu(), disp.cpu())
    with pytest.raises(RuntimeError):
        warp_corr_train(left, right[:, :2], disp)
    with pytest.raises(RuntimeError):
        warp_corr_train(left, right, disp[:, 0])
    with pytest.raises(DiffuVolumeError):                          # no silent change of route
        warp_corr_train(left, right, disp, maxshift=23)
    with pytest.raises(DiffuVolumeError):
        warp_corr_train(left[..., :23], right[..., :23], disp[..., :23])
    with pytest.raises(DiffuVolumeError):
        warp_corr_train(left.repeat(1, 9, 1, 1), right.repeat(1, 9, 1, 1), disp)
    e = torch.zeros(0, 4, 2, 24, device="cuda", requires_grad=True)
    diff, corr = warp_corr_train(e, e.detach(), torch.zeros(0, 1, 2, 24, device="cuda"))
    assert tuple(diff.shape) == (0, 4, 2, 24) and tuple(corr.shape) == (0, 49, 2, 24)
    (diff.sum() + corr.sum()).backward()
    assert tuple(e.grad.shape) == (0, 4, 2, 24)
    diff, corr = warp_corr_train(left, right, disp)
    (grad,) = torch.autograd.grad(diff.sum() + corr.sum(), left, create_graph=True)
    with pytest.raises(RuntimeError):                              # once_differentiable: no double backward
        grad.sum().backward()


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


@pytest.mark.parametrize("route", ["hip", "torch"])
def test_recorded_training_step_on_both_routes(gold, route, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_REFINE", route)
    model = fresh_model(gold)
    outs, loss = step(model, gold, monkeypatch)
    check_step(gold, model, outs, loss)
    assert in_graph(outs[-1].grad_fn, "WarpCorrFnBackward") == (route == "hip")
