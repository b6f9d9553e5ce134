"""The differentiable regression tail (train_tail.upsample_softmax_regress_train, csrc/regress_bwd.hip) against the torch
expression it replaces: F.interpolate(trilinear, x4) + F.softmax(dim=1) + disparity_regression.

Reference: that expression in float64 on the CPU, for disp and, through autograd with a given g, for dcost.  Yardstick: the
same expression in float32 on the CPU.  Bar (the form of test_gpu_acv_train.Bar), per kind of tensor (disp, dcost) and per
conditioning class (mild = randn costs, steep = randn * 40):
    rel_L2(hip, f64) <= 2 * max over the cases of rel_L2(torch_f32, f64) + 1e-6
Shapes: the smallest at which the kernel takes another path -- one coarse pixel (every tap clamped), 2x2, a ragged single
tile with B = 2, more than one tile (4 x 16 coarse pixels) in x, three tiles per axis with ragged remainders (11 x 37), and
two D != 48 shapes for the two-pass route through the workspace.  At (1,48,1,1) the steep float32 gradient is cancellation
noise (3e-2 of float64) and no yardstick, so that shape is mild only.  g is randn with about 30 % exact zeros."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import _lib, upsample_softmax_regress, upsample_softmax_regress_train
from diffuvolume_amd import train_tail

pytestmark = pytest.mark.gpu

SHAPES = [(1, 48, 1, 1), (1, 48, 2, 2), (2, 48, 3, 5), (1, 48, 9, 17), (1, 48, 11, 37), (1, 12, 4, 6), (2, 5, 3, 4)]
CASES = [(s, ac, cls) for s in SHAPES for ac in (False, True) for cls in ("mild", "steep")
         if not (cls == "steep" and s == (1, 48, 1, 1))]


def expression(cost, ac):
    """cost [B,D,h,w] -> disp [B,4h,4w]: the expression of the models' training heads."""
    b, d, h, w = cost.shape
    kw = {"align_corners": True} if ac else {}
    up = F.interpolate(cost.unsqueeze(1), [4 * d, 4 * h, 4 * w], mode="trilinear", **kw).squeeze(1)
    k = torch.arange(4 * d, dtype=cost.dtype).view(1, -1, 1, 1)
    return torch.sum(F.softmax(up, dim=1) * k, 1)


def make_inputs(shape, ac, cls):
    b, d, h, w = shape
    gen = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + 10 * int(ac) + (cls == "steep"))
    cost = torch.randn(b, d, h, w, generator=gen) * (40.0 if cls == "steep" else 1.0)
    g = torch.randn(b, 4 * h, 4 * w, generator=gen)
    g[torch.rand(b, 4 * h, 4 * w, generator=gen) < 0.3] = 0.0
    return cost, g


def on_cpu(cost, g, ac, dtype):
    c = cost.detach().clone().to(dtype).requires_grad_(True)
    disp = expression(c, ac)
    disp.backward(g.to(dtype))
    return disp.detach(), c.grad


@pytest.fixture(scope="module")
def refs():
    """Per case: inputs, float64 reference and float32 yardstick, computed once and left unchanged."""
    out = {}
    for shape, ac, cls in CASES:
        cost, g = make_inputs(shape, ac, cls)
        out[shape, ac, cls] = (cost, g, on_cpu(cost, g, ac, torch.float64), on_cpu(cost, g, ac, torch.float32))
    return out


def rel(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    return float((a - ref).norm() / max(float(ref.norm()), 1e-30))


class Bar:
    """test_gpu_acv_train.Bar: every relative error within 2x the worst float32 one of its kind + 1e-6."""

    def __init__(self):
        self.rows = []

    def __call__(self, hip, f32, f64, kind, what):
        self.rows.append((kind, what, rel(hip, f64), rel(f32, f64)))

    def check(self):
        kinds = sorted({k for k, *_ in self.rows})
        bound = {k: 2 * max(r[3] for r in self.rows if r[0] == k) + 1e-6 for k in kinds}
        for k, what, h, y in self.rows:
            print(f"{k:12s} {what:34s} hip {h:.3e}  float32 {y:.3e}  ratio to the bar {h / bound[k]:.3f}")
        print("bars:", bound)
        bad = sorted(((h / bound[k], w) for k, w, h, _ in self.rows if not h <= bound[k]), reverse=True)
        assert not bad, f"{len(bad)} of {len(self.rows)} tensors over the bar {bound}: {bad[:20]}"


def run(cost, g, ac):
    c = cost.detach().cuda().requires_grad_(True)
    disp = upsample_softmax_regress_train(c, align_corners=ac)
    disp.backward(g.cuda())
    return disp.detach(), c.grad


def hold_to_the_bar(refs):
    bar = Bar()
    for (shape, ac, cls), (cost, g, (d64, g64), (d32, g32)) in refs.items():
        disp, dcost = run(cost, g, ac)
        assert disp.shape == d64.shape and dcost.shape == cost.shape
        what = f"{shape} ac={int(ac)}"
        bar(disp, d32, d64, f"disp/{cls}", what)
        bar(dcost, g32, g64, f"dcost/{cls}", what)
    bar.check()


def test_disp_and_dcost_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_TAIL", raising=False)
    hold_to_the_bar(refs)


def test_torch_route_is_the_expression_and_bad_route_raises(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_TAIL", "torch")
    assert train_tail.route() == "torch"
    hold_to_the_bar(refs)
    c = make_inputs((2, 48, 3, 5), False, "mild")[0].cuda().requires_grad_(True)
    assert upsample_softmax_regress_train(c).grad_fn.name() != "UpsampleSoftmaxRegressFnBackward"
    monkeypatch.setenv("DV_TRAIN_TAIL", "eager")
    with pytest.raises(ValueError):
        upsample_softmax_regress_train(c)
    monkeypatch.delenv("DV_TRAIN_TAIL")
    assert train_tail.route() == "hip"
    assert upsample_softmax_regress_train(c).grad_fn.name() == "UpsampleSoftmaxRegressFnBackward"


@pytest.mark.parametrize("shape", [(2, 48, 3, 5), (1, 48, 11, 37), (2, 5, 3, 4)])
@pytest.mark.parametrize("ac", [False, True])
def test_forward_is_the_eval_launch_bit_for_bit(refs, shape, ac):
    cost = refs[shape, ac, "steep"][0].cuda()
    for c in (cost, cost.unsqueeze(1)):                       # [B,D,h,w] and [B,1,D,h,w]
        disp = upsample_softmax_regress_train(c.clone().requires_grad_(True), align_corners=ac)
        assert disp.requires_grad and tuple(disp.shape) == (shape[0], 4 * shape[2], 4 * shape[3])
        assert torch.equal(disp.detach(), upsample_softmax_regress(cost, False, ac)[0])


@pytest.mark.parametrize("shape", [(2, 48, 3, 5), (2, 48, 9, 17), (2, 5, 3, 4)])
@pytest.mark.parametrize("ac", [False, True])
def test_gradient_repeats_and_a_batch_is_its_items(shape, ac):
    gen = torch.Generator().manual_seed(7)
    cost = (torch.randn(*shape, generator=gen) * 10).cuda()
    g = torch.randn(shape[0], 4 * shape[2], 4 * shape[3], generator=gen).cuda()

    def grad(c, gg):
        c = c.clone().requires_grad_(True)
        upsample_softmax_regress_train(c, align_corners=ac).backward(gg)
        return c.grad

    first = grad(cost, g)
    assert torch.equal(first, grad(cost, g))
    assert torch.equal(first, torch.cat([grad(cost[:1], g[:1]), grad(cost[1:], g[1:])]))


@pytest.mark.parametrize("shape", [(1, 48, 9, 17), (2, 5, 3, 4)])
@pytest.mark.parametrize("ac", [False, True])
def test_zero_gradient_is_exactly_zero_and_nan_goes_where_torch_puts_it(shape, ac):
    gen = torch.Generator().manual_seed(11)
    cost = torch.randn(*shape, generator=gen) * 40                      # near one-hot softmax
    g = torch.zeros(shape[0], 4 * shape[2], 4 * shape[3])
    _, dcost = run(cost, g, ac)
    assert torch.equal(dcost, torch.zeros_like(dcost))
    # a masked-out pixel next to a live one: only the live one contributes
    g[0, 1, 2] = 1.5
    _, one = run(cost, g, ac)
    d64 = on_cpu(cost, g, ac, torch.float64)[1]
    assert bool((one != 0).any()) and not bool(((one != 0).cpu() & (d64 == 0)).any())
    # non-finite gradients are not filtered: NaN lands on every tap of its pixel, as in torch's backward, and nowhere else
    g[0, 2, 1] = float("nan")
    _, bad = run(cost, g, ac)
    assert torch.equal(torch.isnan(bad).cpu(), torch.isnan(on_cpu(cost, g, ac, torch.float32)[1]))
    assert torch.isnan(bad).any() and not torch.isnan(bad).all()


def _call(lib, cost, disp, g, dcost, ws, shape, ac):
    b, d, h, w = shape
    code = lib.dv_upsample_softmax_regress_bwd_f32(cost.data_ptr(), disp.data_ptr(), g.data_ptr(), dcost.data_ptr(),
                                                   _lib.ptr(ws), b, d, h, w, int(ac), _lib.stream_ptr())
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("shape", [(2, 48, 3, 5), (1, 48, 9, 17), (2, 5, 3, 4)])
@pytest.mark.parametrize("ac", [False, True])
def test_abi_offset_views_bounds_and_refusals(shape, ac):
    """The entry's pointer and bounds contract, called as a C caller would: views offset by one float give the bits of
    aligned operands; dcost and the workspace lie in the middle of sentinel-filled buffers, the sentinel survives outside
    and nowhere inside; NULL pointers and non-positive shapes are refused with their codes and write nothing."""
    lib = _lib.load()
    b, d, h, w = shape
    gen = torch.Generator().manual_seed(3)
    cost = (torch.randn(*shape, generator=gen) * 5).cuda()
    g = torch.randn(b, 4 * h, 4 * w, generator=gen).cuda()
    disp = upsample_softmax_regress(cost, False, ac)[0]
    n_ws = lib.dv_upsample_softmax_regress_bwd_workspace_floats(b, d, h, w)
    assert (n_ws == 0) == (d == 48) and n_ws in (0, b * d * 16 * h * w)
    aligned = torch.empty_like(cost)
    ws = torch.empty(n_ws, device="cuda") if n_ws else None
    assert _call(lib, cost, disp, g, aligned, ws, shape, ac) == 0

    def offset(t):
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    SENT, PAD = -7777.25, 37                                  # 37 floats: the carved tensors start 4 bytes off a 16-byte line
    arena = torch.full((cost.numel() + 2 * PAD,), SENT, device="cuda")
    dcost = arena[PAD:PAD + cost.numel()].view(cost.shape)
    ws_arena = torch.full((n_ws + 2 * PAD,), SENT, device="cuda")
    ws_v = ws_arena[PAD:PAD + n_ws] if n_ws else None
    assert _call(lib, offset(cost), offset(disp), offset(g), dcost, ws_v, shape, ac) == 0
    assert torch.equal(dcost, aligned)
    assert bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + cost.numel():] == SENT).all())
    assert not bool((dcost == SENT).any())
    assert bool((ws_arena[:PAD] == SENT).all()) and bool((ws_arena[PAD + n_ws:] == SENT).all())
    if n_ws:
        assert not bool((ws_v == SENT).any())

    arena.fill_(SENT)
    null = ctypes.c_void_p(None)
    ptrs = [cost.data_ptr(), disp.data_ptr(), g.data_ptr(), dcost.data_ptr()]
    for i in range(4):
        a = list(ptrs)
        a[i] = null
        assert lib.dv_upsample_softmax_regress_bwd_f32(*a, _lib.ptr(ws_v), b, d, h, w, int(ac), _lib.stream_ptr()) == -1
    if n_ws:
        assert lib.dv_upsample_softmax_regress_bwd_f32(*ptrs, null, b, d, h, w, int(ac), _lib.stream_ptr()) == -1
    for bad in ((0, d, h, w), (b, 0, h, w), (b, d, -1, w), (b, d, h, 0)):
        assert lib.dv_upsample_softmax_regress_bwd_f32(*ptrs, _lib.ptr(ws_v), *bad, int(ac), _lib.stream_ptr()) == -2
        assert lib.dv_upsample_softmax_regress_bwd_workspace_floats(*bad) == 0
    torch.cuda.synchronize()
    assert bool((arena == SENT).all())                        # a refused call writes nothing


def test_nothing_of_the_size_of_the_fine_volume_is_allocated(monkeypatch):
    """A condition, not a measurement: forward + backward at (2,48,16,32) grow the peak by less than 1/8 of one
    [B,192,4h,4w] float32 tensor (the torch expression keeps several of them)."""
    monkeypatch.delenv("DV_TRAIN_TAIL", raising=False)
    b, d, h, w = 2, 48, 16, 32
    cost = torch.randn(b, d, h, w, device="cuda").requires_grad_(True)
    g = torch.randn(b, 4 * h, 4 * w, device="cuda")
    upsample_softmax_regress_train(cost).backward(g)          # library loaded, allocator warm
    cost.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    upsample_softmax_regress_train(cost).backward(g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    fine = b * 4 * d * 4 * h * 4 * w * 4
    print(f"peak growth {grown} B against {fine} B for one fine volume")
    assert grown < fine // 8


def test_refusals_of_the_python_function():
    cost = torch.randn(1, 48, 2, 2, device="cuda", requires_grad=True)
    with pytest.raises(TypeError):
        upsample_softmax_regress_train(cost.double())
    with pytest.raises(_lib.DiffuVolumeError):
        upsample_softmax_regress_train(cost.detach().cpu())
    with pytest.raises(RuntimeError):
        upsample_softmax_regress_train(torch.randn(1, 2, 48, 2, 2, device="cuda"))
    disp = upsample_softmax_regress_train(cost)
    (grad,) = torch.autograd.grad(disp.sum(), cost, create_graph=True)
    with pytest.raises(RuntimeError):                          # once_differentiable: no double backward
        grad.sum().backward()
