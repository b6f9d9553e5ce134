"""The fused masked training losses (csrc/masked_loss.hip, diffuvolume_amd/train_loss.py) on the MI355X.

Reference: the reference's own float64 record where one exists (tests/golden/loss_train.npz for the five model_loss_*
functions, seq_loss_f64 / seq_metrics_f64 of igev_train_step.npz for sequence_loss), the float64 CPU evaluation of the torch
expression on the same inputs elsewhere.  Yardstick: the same in float32.  Bar, relative L2 for gradients and relative for
scalars:   err(hip) <= 2 * err(float32) + 1e-6.

Shapes (B,H,W): one element; a tail with no full quad; the synth case; odd sizes with misaligned rows; and 2 * GRID_ELEMENTS
+ 3 elements, where every block of the capped grid loops more than once and the last quad is partial.  K: 1, 4, 6, 23 and
30 (above the 24 of one launch: two launches of each kind)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from diffuvolume_amd import _lib, loss as L, masked_loss_train, sequence_loss_train, synth, train_loss

pytestmark = pytest.mark.gpu

FN = {"smooth_l1": F.smooth_l1_loss, "l1": F.l1_loss}
SHAPES = {"one": (1, 1, 1), "tail": (1, 3, 5), "synth": (2, 16, 24), "odd": (2, 37, 129),
          "loop": (1, 1, 2 * train_loss.GRID_ELEMENTS + 3)}
CASES = [(s, k) for s in ("one", "tail", "synth", "odd") for k in (1, 4, 6, 23, 30)] + [("loop", 1), ("loop", 4)]
MODEL_LOSSES = {"model_loss_train": L.model_loss_train, "model_loss_train_freeze_attn": L.model_loss_train_freeze_attn,
                "model_loss_train_attn_only": L.model_loss_train_attn_only, "model_loss_test": L.model_loss_test,
                "model_loss_kitti12": L.model_loss_kitti12}
SENT, PAD = -777.0, 1025


def rel(a, ref):
    a, ref = (torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in (a, ref))
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


def within(hip, f32, f64, what):
    e, y = rel(hip, f64), rel(f32, f64)
    print(f"{what}: hip {e:.3g}  float32 {y:.3g}")
    assert e <= 2 * y + 1e-6, what


def operands(shape, k, seed=0):
    """k predictions around a ground truth, a mask that selects ~3/4 of the pixels (always the first), both kinds of loss in
    turn, and d == 0 exactly at every 7th pixel of prediction 0."""
    b, h, w = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 * k + h * 31 + w % 9973 + seed)
    gt = torch.rand(b, h, w, generator=g) * 180 + 1
    mask = torch.rand(b, h, w, generator=g) > 0.25
    mask.view(-1)[0] = True
    preds = [gt + torch.randn(b, h, w, generator=g) * (2.5 / (i % 6 + 1)) for i in range(k)]
    preds[0].view(-1)[::7] = gt.view(-1)[::7]
    weights = [0.5 + 0.1 * (i % 9) for i in range(k)]
    kinds = ["smooth_l1" if i % 2 == 0 else "l1" for i in range(k)]
    return preds, gt, mask, weights, kinds


def torch_expr(preds, gt, mask, weights, kinds, dtype=None, device=None, gout=None):
    """The reference's expression with autograd -> (loss, gradients)."""
    preds = [p.detach().to(device=device, dtype=dtype).requires_grad_(True) for p in preds]
    gt, mask = gt.to(device=device, dtype=dtype), mask.to(device=device)
    loss = sum(w * FN[kd](p[mask], gt[mask], reduction="mean") for p, w, kd in zip(preds, weights, kinds))
    (loss if gout is None else loss * gout).backward()
    return loss.detach(), [p.grad for p in preds]


def hip_run(preds, gt, mask, weights, kinds, gout=None, frozen=()):
    preds = [p.detach().cuda().requires_grad_(i not in frozen) for i, p in enumerate(preds)]
    loss = masked_loss_train(preds, gt.cuda(), mask.cuda(), weights, kinds)
    assert loss.shape == () and loss.dtype == torch.float32 and "MaskedLossFn" in loss.grad_fn.name()
    (loss if gout is None else loss * gout).backward()
    torch.cuda.synchronize()
    return loss.detach(), [p.grad for p in preds]


@pytest.fixture(scope="module")
def refs():
    """(operands, float64 result, float32 result) per case, computed once on the CPU and left unchanged."""
    out = {}
    for shape, k in CASES:
        ops = operands(shape, k)
        out[shape, k] = (ops, torch_expr(*ops, dtype=torch.float64), torch_expr(*ops, dtype=torch.float32))
    return out


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "loss_train.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def step_gold():
    with np.load(GOLDEN / "igev_train_step.npz") as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(MODEL_LOSSES))
def test_model_losses_against_the_reference_record(gold, name, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_LOSS", "hip")
    preds, gt, mask = synth.loss_train_inputs(**synth.LOSS_TRAIN_CASE)
    preds = [p.cuda().requires_grad_(True) for p in preds]
    loss = MODEL_LOSSES[name](preds, gt.cuda(), mask.cuda())
    assert "MaskedLossFn" in loss.grad_fn.name()
    loss.backward()
    within(loss, gold[f"{name}_loss_f32"], gold[f"{name}_loss_f64"], f"{name} loss")
    g32, g64 = gold[f"{name}_grad_f32"], gold[f"{name}_grad_f64"]
    used = [p for p in preds if p.grad is not None]
    assert len(used) == len(g64) and all(p.grad is None for p in preds[len(g64):])       # zip: the shorter list
    for i, p in enumerate(used):
        within(p.grad, g32[i], g64[i], f"{name} dpred{i}")
        sel = mask.cuda()
        assert bool((p.grad[~sel] == 0).all())


@pytest.mark.parametrize("shape,k", CASES)
def test_against_float64(refs, shape, k):
    ops, (l64, g64), (l32, g32) = refs[shape, k]
    loss, grads = hip_run(*ops)
    within(loss, l32, l64, f"{shape} K={k} loss")
    for i, g in enumerate(grads):
        assert g.shape == ops[0][i].shape
        within(g, g32[i], g64[i], f"{shape} K={k} dpred{i}")
        assert bool((g[~ops[2].cuda()] == 0).all())


@pytest.mark.parametrize("shape,k", [("odd", 6), ("tail", 4), ("loop", 1)])
def test_unselected_pixels_are_zero_by_selection(refs, shape, k):
    """NaN and +-Inf behind the mask, in the predictions and in gt, reach neither the loss nor a gradient: same bits as with
    finite values there; d == 0 at a selected pixel gives 0."""
    (preds, gt, mask, weights, kinds), _, _ = refs[shape, k]
    want_loss, want = hip_run(preds, gt, mask, weights, kinds)
    zero = mask.clone().view(-1)
    zero[:] = False
    zero[::7] = True
    zero = zero.view(mask.shape) & mask
    if bool(zero.any()):
        assert bool((want[0][zero.cuda()] == 0).all())                  # d == 0 exactly: sign(0) = 0 and d = 0
    if not bool((~mask).any()):
        return
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")]).repeat(mask.numel() // 3 + 1)[:mask.numel()]
    poison = poison.view(mask.shape)
    bad_preds = [torch.where(mask, p, poison if i % 2 == 0 else p) for i, p in enumerate(preds)]
    bad_gt = torch.where(mask, gt, poison.roll(1))
    loss, grads = hip_run(bad_preds, bad_gt, mask, weights, kinds)
    assert torch.equal(loss, want_loss) and bool(torch.isfinite(loss))
    for g, w in zip(grads, want):
        assert torch.equal(g, w) and bool((g[~mask.cuda()] == 0).all())


def test_an_empty_selection_gives_nan_and_zero_gradients(refs):
    (preds, gt, mask, weights, kinds), _, _ = refs["odd", 4]
    loss, grads = hip_run(preds, gt, torch.zeros_like(mask), weights, kinds)
    assert bool(torch.isnan(loss))
    assert all(bool((g == 0).all()) for g in grads)


@pytest.mark.parametrize("kind", ["l1", "smooth_l1"])
def test_nan_at_a_selected_pixel_reaches_the_loss_and_that_gradient_only(refs, kind):
    (preds, gt, mask, weights, _), _, _ = refs["odd", 4]
    at = int(mask.view(-1).nonzero()[5])
    preds = [p.clone() for p in preds]
    preds[1].view(-1)[at] = float("nan")
    loss, grads = hip_run(preds, gt, mask, weights, [kind] * 4)
    assert bool(torch.isnan(loss))
    for i, g in enumerate(grads):
        nan = torch.isnan(g.view(-1))
        assert int(nan.sum()) == (1 if i == 1 else 0) and (i != 1 or bool(nan[at]))
        assert bool((g[~mask.cuda()] == 0).all())


@pytest.mark.parametrize("shape,k", [("odd", 6), ("synth", 30), ("loop", 4)])
def test_same_bits_on_every_launch(refs, shape, k):
    (preds, gt, mask, weights, kinds), _, _ = refs[shape, k]
    dev = [p.cuda() for p in preds]
    kd = [train_loss.KINDS[s] for s in kinds]
    m8 = mask.cuda().view(torch.uint8)
    runs = []
    for _ in range(2):
        loss, stats = train_loss.masked_loss_forward(dev, gt.cuda(), m8, train_loss.MASK_U8, 0.0, weights, kd, k - 1)
        _, grads = hip_run(preds, gt, mask, weights, kinds)
        runs.append((loss.clone(), stats.clone(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    stats = runs[0][1].cpu()
    assert stats.shape == ((k + 23) // 24, 30)
    kl = k - (stats.shape[0] - 1) * 24
    assert float(stats[-1][kl]) == float(mask.sum()) and float(stats[-1][kl + 5]) == 0
    d = (preds[-1] - gt)[mask].abs()
    assert [float(v) for v in stats[-1][kl + 2:kl + 5]] == [float((d < t).sum()) for t in (1, 3, 5)]
    assert abs(float(stats[-1][kl + 1]) - float(d.double().sum())) <= 1e-6 * float(d.double().sum())


def test_hip_and_torch_routes_agree(refs, monkeypatch):
    """`loss.model_loss_kitti12` and `loss.sequence_loss` on GPU tensors under both values of DV_TRAIN_LOSS."""
    (preds, gt, mask, _, _), _, _ = refs["odd", 6]
    weights, kinds = [0.5, 0.5, 0.5, 0.7, 1.0, 1.3], ["smooth_l1"] * 6
    l64, g64 = torch_expr(preds, gt, mask, weights, kinds, dtype=torch.float64)
    l32, g32 = torch_expr(preds, gt, mask, weights, kinds, dtype=torch.float32)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_LOSS", route)
        dev = [p.cuda().requires_grad_(True) for p in preds]
        loss = L.model_loss_kitti12(dev, gt.cuda(), mask.cuda())
        assert ("MaskedLossFn" in loss.grad_fn.name()) == (route == "hip")
        loss.backward()
        within(loss, l32, l64, f"{route} loss")
        for i, p in enumerate(dev):
            within(p.grad, g32[i], g64[i], f"{route} dpred{i}")
    # what the fused route does not take stays the torch expression, without raising
    monkeypatch.setenv("DV_TRAIN_LOSS", "hip")
    dev = [p.cuda().double().requires_grad_(True) for p in preds]
    assert "MaskedLossFn" not in L.model_loss_kitti12(dev, gt.cuda().double(), mask.cuda()).grad_fn.name()
    gtg = gt.cuda().requires_grad_(True)
    L.model_loss_kitti12([p.cuda() for p in preds], gtg, mask.cuda()).backward()
    assert gtg.grad is not None
    col = L.model_loss_test([preds[0].cuda()[:, :, :1].requires_grad_(True)], gt.cuda()[:, :, :1], mask.cuda()[:, :, :1])
    assert "MaskedLossFn" in col.grad_fn.name()                                   # a non-contiguous view is made contiguous
    within(col, *(torch_expr([preds[0][:, :, :1]], gt[:, :, :1], mask[:, :, :1], [1.0], ["l1"], dtype=dt)[0]
                  for dt in (torch.float32, torch.float64)), "strided view")


def test_a_frozen_prediction_gets_no_gradient_and_the_others_keep_their_bits(refs):
    (preds, gt, mask, weights, kinds), _, _ = refs["odd", 6]
    _, want = hip_run(preds, gt, mask, weights, kinds)
    loss, grads = hip_run(preds, gt, mask, weights, kinds, frozen=(0, 3))
    assert grads[0] is None and grads[3] is None
    assert all(torch.equal(grads[i], want[i]) for i in (1, 2, 4, 5))


def test_a_scaled_loss_scales_every_gradient(refs):
    (preds, gt, mask, weights, kinds), _, _ = refs["odd", 6]
    scale = 1024.0 * 1.37
    _, g64 = torch_expr(preds, gt, mask, weights, kinds, dtype=torch.float64, gout=scale)
    _, g32 = torch_expr(preds, gt, mask, weights, kinds, dtype=torch.float32, gout=scale)
    _, dev = torch_expr(preds, gt, mask, weights, kinds, device="cuda", gout=scale)
    _, grads = hip_run(preds, gt, mask, weights, kinds, gout=scale)
    for i, g in enumerate(grads):
        within(g, g32[i], g64[i], f"scaled dpred{i}")
        within(dev[i], g32[i], g64[i], f"scaled dpred{i} torch route")


# ---- the sequence_loss form ------------------------------------------------------------------------------------------

def seq_run(fn, preds, init, gt, valid, **kw):
    preds = [p.detach().cuda().requires_grad_(True) for p in preds]
    init = init.detach().cuda().requires_grad_(True)
    loss, metrics = fn(preds, init, gt.cuda(), valid.cuda(), **kw)
    loss.backward()
    return loss.detach(), metrics, [init.grad, *[p.grad for p in preds]]


def seq_cpu(preds, init, gt, valid, dtype, **kw):
    preds = [p.detach().to(dtype).requires_grad_(True) for p in preds]
    init = init.detach().to(dtype).requires_grad_(True)
    loss, metrics = L.sequence_loss(preds, init, gt.to(dtype), valid, **kw)
    loss.backward()
    return loss.detach(), metrics, [init.grad, *[p.grad for p in preds]]


def test_sequence_loss_against_the_reference_record(step_gold, monkeypatch):
    seed = synth.IGEV_TRAIN_STEP_CASE["seed"]
    args = synth.igev_sequence_loss_inputs(seed)
    c64, c32 = seq_cpu(*args, torch.float64, max_disp=192), seq_cpu(*args, torch.float32, max_disp=192)
    assert abs(float(c64[0]) - float(step_gold["seq_loss_f64"])) <= 1e-12 * float(c64[0])
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_LOSS", route)
        loss, metrics, grads = seq_run(L.sequence_loss, *args, max_disp=192)
        within(loss, step_gold["seq_loss_f32"], step_gold["seq_loss_f64"], f"{route} sequence loss")
        for j, key in enumerate(("epe", "1px", "3px", "5px")):
            assert isinstance(metrics[key], float)
            within(metrics[key], step_gold["seq_metrics_f32"][j], step_gold["seq_metrics_f64"][j], f"{route} {key}")
        for i, g in enumerate(grads):
            within(g, c32[2][i], c64[2][i], f"{route} sequence grad{i}")
    # 23 predictions, the shape of a real step's list
    gen = torch.Generator().manual_seed(3)
    many = [args[2] + torch.randn(args[2].shape, generator=gen) * 2 for _ in range(22)]
    big = (many, *args[1:])
    c64, c32 = seq_cpu(*big, torch.float64), seq_cpu(*big, torch.float32)
    loss, metrics, grads = seq_run(sequence_loss_train, *big)
    within(loss, c32[0], c64[0], "22 + 1 loss")
    for key in metrics:
        within(metrics[key], c32[1][key], c64[1][key], f"22 + 1 {key}")
    for i, g in enumerate(grads):
        within(g, c32[2][i], c64[2][i], f"22 + 1 grad{i}")


def test_sequence_loss_single_prediction_gets_weight_one():
    preds, init, gt, valid = synth.igev_sequence_loss_inputs(7)
    args = (preds[-1:], init, gt, valid)
    c64, c32 = seq_cpu(*args, torch.float64), seq_cpu(*args, torch.float32)
    loss, _, grads = seq_run(sequence_loss_train, *args)
    assert bool(torch.isfinite(loss))
    within(loss, c32[0], c64[0], "single prediction loss")
    within(grads[1], c32[2][1], c64[2][1], "single prediction grad")
    with pytest.raises(AssertionError):
        sequence_loss_train([], init.cuda(), gt.cuda(), valid.cuda())


def test_sequence_selection_is_the_torch_expressions():
    """Edge values of ``valid`` (around 0.5, NaN) and of gt (around +-max_disp, zeros, a square that overflows, one that
    underflows) select exactly the pixels of ``(valid >= 0.5) & (sqrt(gt ** 2) < max_disp)``: an L1 prediction gt + 2 has a
    non-zero gradient exactly at the selected pixels."""
    half, top = torch.tensor(0.5), torch.tensor(192.0)
    vals = torch.stack([half, torch.nextafter(half, torch.tensor(0.0)), torch.nextafter(half, torch.tensor(1.0)),
                        torch.tensor(0.0), torch.tensor(1.0), torch.tensor(float("nan")), torch.tensor(0.49999997)])
    gts = torch.stack([top, torch.nextafter(top, torch.tensor(0.0)), torch.nextafter(top, torch.tensor(999.0)), -top,
                       -torch.nextafter(top, torch.tensor(0.0)), torch.tensor(0.0), torch.tensor(-0.0),
                       torch.tensor(1e20), torch.tensor(1e-30), torch.tensor(100.0), torch.tensor(3e38)])
    valid = vals.repeat_interleave(len(gts)).view(1, 7, 11)
    gt = gts.repeat(len(vals)).view(1, 1, 7, 11)
    want = ((valid >= 0.5) & (torch.sum(gt ** 2, dim=1).sqrt() < 192)).unsqueeze(1)
    assert 0 < int(want.sum()) < want.numel()
    for max_disp, expect in ((192, want), (float(torch.nextafter(top, torch.tensor(0.0))), None)):
        if expect is None:
            expect = ((valid >= 0.5) & (torch.sum(gt ** 2, dim=1).sqrt() < max_disp)).unsqueeze(1)
        pred = (gt + 2).cuda().requires_grad_(True)
        loss, _ = sequence_loss_train([pred], (gt + 2).cuda(), gt.cuda(), valid.cuda(), max_disp=max_disp)
        loss.backward()
        assert torch.equal((pred.grad != 0).cpu(), expect), max_disp


def test_the_infinity_flag_raises_from_the_stats_copy(refs):
    """Under the ``valid`` selection an infinite gt is never selected (inf < max_disp is false for every max_disp; the
    reference's assert cannot fire either), so the flag is raised where it can be: a byte mask that selects an infinite gt."""
    (preds, gt, mask, weights, kinds), _, _ = refs["odd", 4]
    kd = [train_loss.KINDS[s] for s in kinds]
    dev, m8 = [p.cuda() for p in preds], mask.cuda().view(torch.uint8)
    _, stats = train_loss.masked_loss_forward(dev, gt.cuda(), m8, train_loss.MASK_U8, 0.0, weights, kd, 3)
    assert set(train_loss.sequence_metrics(stats, 4)) == {"epe", "1px", "3px", "5px"}
    bad = gt.clone()
    bad.view(-1)[int(mask.view(-1).nonzero()[3])] = -float("inf")
    _, stats = train_loss.masked_loss_forward(dev, bad.cuda(), m8, train_loss.MASK_U8, 0.0, weights, kd, 3)
    assert float(stats[0, 4 + 5]) == 1.0
    with pytest.raises(AssertionError):
        train_loss.sequence_metrics(stats, 4)
    hidden = torch.where(mask, gt, torch.tensor(float("inf")))                # infinite only behind the mask: no flag
    _, stats = train_loss.masked_loss_forward(dev, hidden.cuda(), m8, train_loss.MASK_U8, 0.0, weights, kd, 3)
    assert float(stats[0, 4 + 5]) == 0.0
    v = torch.ones(gt.shape)
    loss, _ = sequence_loss_train([preds[0].cuda().unsqueeze(1)], preds[1].cuda().unsqueeze(1), bad.cuda().unsqueeze(1),
                                  v.cuda(), max_disp=float("inf"))
    assert bool(torch.isfinite(loss))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------

def carve(t, off, fill=None):
    """t's values (or `fill`) in the middle of a sentinel-filled arena of t's dtype -> (arena, view, start); the view starts
    `off` elements past a 16-byte line."""
    per16 = 16 // t.element_size()
    arena = torch.full((t.numel() + 2 * PAD + per16,), SENT if t.dtype.is_floating_point else 0x5A, dtype=t.dtype,
                       device="cuda")
    start = PAD + (off - PAD) % per16
    v = arena[start:start + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == t.element_size() * off and v.is_contiguous()
    return arena, v, start


def intact(arena, start, n):
    s = SENT if arena.dtype.is_floating_point else 0x5A
    return bool((arena[:start] == s).all()) and bool((arena[start + n:] == s).all())


def host(ptrs, weights, kinds):
    k = len(ptrs)
    return ((ctypes.c_void_p * k)(*ptrs), (ctypes.c_double * k)(*weights), (ctypes.c_int * k)(*kinds))


@pytest.mark.parametrize("mode", ["u8", "valid_f32"])
def test_masked_loss_abi_offset_views_bounds_and_refusals(refs, mode):
    """dv_masked_loss_workspace_floats, dv_masked_loss_fwd_f32 and dv_masked_loss_bwd_f32 as a C caller sees them.  Every
    tensor operand 1-3 elements off a 16-byte line (the element accesses) gives the bits of the run on 16-byte lines; stats,
    loss, the workspace and the gradients lie between sentinels that survive, and the gradients, pre-filled with NaN, come
    back finite; every refused argument returns its code and nothing is written."""
    lib, st = _lib.load(), _lib.stream_ptr()
    (preds, gt, mask, weights, kinds), _, _ = refs["odd", 6]
    k, n = 6, gt.numel()
    kd = [train_loss.KINDS[s] for s in kinds]
    if mode == "u8":
        m, code, max_disp = mask.view(torch.uint8) * 3, 0, 0.0              # any non-zero byte selects
    else:
        m, code, max_disp = (torch.rand(gt.shape, generator=torch.Generator().manual_seed(1)) > 0.3).float(), 1, 150.0
    size = lib.dv_masked_loss_workspace_floats
    assert size(k, n) == 2 * ((n + 1023) // 1024) * (k + 6) and size(4, 100) == 20
    assert size(24, 10 ** 10) == 2 * 1024 * 30 and size(1, 2 * train_loss.GRID_ELEMENTS + 3) == 2 * 1024 * 7
    assert size(0, n) == 0 and size(25, n) == 0 and size(-1, n) == 0 and size(1, 0) == 0 and size(1, -5) == 0
    gout = torch.tensor([1.5], device="cuda")

    results = []
    for offs in ((0, 0, 0), (1, 2, 3)):
        ps = [carve(p, offs[i % 3])[1] for i, p in enumerate(preds)]
        g = carve(gt, offs[1])[1]
        mk = carve(m, offs[2])[1]
        ws_a, ws, ws_s = carve(torch.empty(size(k, n)), 2, fill=0.0)              # 8 bytes past a 16-byte line
        st_a, stats, st_s = carve(torch.empty(k + 6, dtype=torch.float64), 1, fill=0.0)
        lo_a, loss, lo_s = carve(torch.empty(1), offs[0], fill=0.0)
        pa, wa, ka = host([p.data_ptr() for p in ps], weights, kd)
        assert lib.dv_masked_loss_fwd_f32(pa, wa, ka, g.data_ptr(), mk.data_ptr(), code, max_disp, k, n, k - 1,
                                          ws.data_ptr(), stats.data_ptr(), loss.data_ptr(), st) == 0
        grads = [carve(torch.empty(p.shape), offs[(i + 1) % 3], fill=float("nan")) for i, p in enumerate(preds)]
        grads[2] = None                                                            # one prediction wants no gradient
        ga = (ctypes.c_void_p * k)(*[None if x is None else x[1].data_ptr() for x in grads])
        assert lib.dv_masked_loss_bwd_f32(pa, wa, ka, g.data_ptr(), mk.data_ptr(), code, max_disp, stats.data_ptr(),
                                          gout.data_ptr(), ga, k, n, st) == 0
        torch.cuda.synchronize()
        assert intact(ws_a, ws_s, ws.numel()) and intact(st_a, st_s, k + 6) and intact(lo_a, lo_s, 1), offs
        for x in grads:
            assert x is None or (intact(x[0], x[2], n) and bool(torch.isfinite(x[1]).all())), offs
        results.append((loss.clone(), stats.clone(), [None if x is None else x[1].clone() for x in grads]))
    (l0, s0, g0), (l1, s1, g1) = results
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g0, g1))
    # ... and they are the values of the torch expression with this selection
    sel = (m != 0) if mode == "u8" else ((m >= 0.5) & ((gt ** 2).sqrt() < max_disp))
    l64, g64 = torch_expr(preds, gt, sel, weights, kinds, dtype=torch.float64, gout=1.5)
    l32, g32 = torch_expr(preds, gt, sel, weights, kinds, dtype=torch.float32, gout=1.5)
    within(l0, l32, l64, f"abi {mode} loss")
    assert float(s0[k]) == float(sel.sum())
    for i in (0, 1, 3, 4, 5):
        within(g0[i], g32[i], g64[i], f"abi {mode} dpred{i}")

    # refusals: nothing is launched, nothing is written
    for a in (ws_a, st_a, lo_a, *[x[0] for x in grads if x is not None]):
        a.fill_(SENT)
    null = ctypes.c_void_p(None)
    good_f = [pa, wa, ka, g.data_ptr(), mk.data_ptr(), code, max_disp, k, n, k - 1, ws.data_ptr(), stats.data_ptr(),
              loss.data_ptr()]
    good_b = [pa, wa, ka, g.data_ptr(), mk.data_ptr(), code, max_disp, stats.data_ptr(), gout.data_ptr(), ga, k, n]

    def refused(entry, good, at, value, want):
        args = list(good)
        args[at] = value
        assert entry(*args, st) == want, (entry.__name__, at, value)

    fwd, bwd = lib.dv_masked_loss_fwd_f32, lib.dv_masked_loss_bwd_f32
    holed = (ctypes.c_void_p * k)(*[p.data_ptr() if i != 4 else None for i, p in enumerate(ps)])
    bad_kind = (ctypes.c_int * k)(*[kd[0], 2, *kd[2:]])
    for at in (0, 1, 2, 3, 4, 10, 11, 12):
        refused(fwd, good_f, at, null, -1)
    for at in (0, 1, 2, 3, 4, 7, 8, 9):
        refused(bwd, good_b, at, null, -1)
    refused(fwd, good_f, 0, holed, -1)
    refused(bwd, good_b, 0, holed, -1)
    refused(bwd, good_b, 9, (ctypes.c_void_p * k)(*[None] * k), -1)               # no gradient wanted at all
    for entry, good, at_k, at_n in ((fwd, good_f, 7, 8), (bwd, good_b, 10, 11)):
        for bad in (0, -1, train_loss.MAX_K + 1):
            refused(entry, good, at_k, bad, -2)
        for bad in (0, -1):
            refused(entry, good, at_n, bad, -2)
        refused(entry, good, 2, bad_kind, -3)
        refused(entry, good, 5, 2, -3)
        refused(entry, good, 5, -1, -3)
    for bad in (k, -2):
        refused(fwd, good_f, 9, bad, -2)
    if mode == "valid_f32":
        refused(fwd, good_f, 6, float("nan"), -3)
        refused(bwd, good_b, 6, float("nan"), -3)
    refused(fwd, good_f, 10, ws.data_ptr() + 4, -4)
    refused(fwd, good_f, 11, stats.data_ptr() + 4, -4)
    refused(bwd, good_b, 7, stats.data_ptr() + 4, -4)
    torch.cuda.synchronize()
    for a in (ws_a, st_a, lo_a, *[x[0] for x in grads if x is not None]):
        assert bool((a == SENT).all())
    assert train_loss.MAX_K >= 24
