"""The patch stencils of ACVNet_DDIM's attention branch in training on HIP (diffuvolume_amd/train_patch.py,
csrc/patch_volume.hip forward, csrc/patch_volume_bwd.hip backward) against the statement of the call site,

    gwc   = patch(gwc)
    patch = torch.cat((patch_l1(gwc[:, :8]), patch_l2(gwc[:, 8:24]), patch_l3(gwc[:, 24:40])), dim=1)

built from nn.Conv3d modules and evaluated with float64 autograd on the CPU.  The yardstick is the same statement in
float32 on the CPU.  Bar (test_gpu_regress_train.Bar): per kind of tensor (out, dgwc, dw1, dw2) every HIP relative L2 error
is at most 2x the worst float32 one of that kind + 1e-6; the ratios are printed.

Shapes are the smallest that reach each path of the backward (a block owns a 16 x 128 tile of one (b, g, d) plane; 16-byte
accesses when W % 4 == 0 and the tensors lie on 16-byte lines; at most 65535 planes per launch), all with G = 40 and the
network's dilations [1]*8 + [2]*16 + [3]*16:
  tiny        [1,40,1,2,3]      image smaller than every halo, odd W
  row_tiles   [2,40,2,17,12]    two row tiles, 16-byte path
  col_tiles   [1,40,1,5,140]    two column tiles
  odd_w       [1,40,2,9,50]     W % 4 != 0: element-wise accesses
  many_blocks [2,40,2,33,140]   3 x 2 tiles per plane, 24 partials per group
  many_planes [2,40,2100,1,4]   2 * 16 * 2100 = 67200 planes in one dilation run: two launches
  mixed_runs  [2,5,2,18,20]     G = 5 with dilations (2,1,1,3,2): four runs of unequal length, one dilation twice"""
import ctypes

import pytest
import torch
from torch import nn

from diffuvolume_amd import DiffuVolumeError, _lib, patch_volume_train, train_patch
from diffuvolume_amd.submodule import patch_volume
from test_gpu_regress_train import Bar, rel

pytestmark = pytest.mark.gpu

NET = (1,) * 8 + (2,) * 16 + (3,) * 16
SHAPES = {
    "tiny": (1, 40, 1, 2, 3),
    "row_tiles": (2, 40, 2, 17, 12),
    "col_tiles": (1, 40, 1, 5, 140),
    "odd_w": (1, 40, 2, 9, 50),
    "many_blocks": (2, 40, 2, 33, 140),
    "many_planes": (2, 40, 2100, 1, 4),
    "mixed_runs": (2, 5, 2, 18, 20),
}
DILATION = {"mixed_runs": (2, 1, 1, 3, 2)}
KINDS = ("out", "dgwc", "dw1", "dw2")
PAD, SENT = 37, -7.0e5                                       # 37 floats: the carved view starts 4 bytes off a 16-byte line


def dil_of(name):
    return DILATION.get(name, NET)


def runs_of(dilation):
    return train_patch._runs(tuple(dilation))[4]


def make_inputs(name):
    """gwc, w1, w2 and the cotangent g of a case (CPU, float32)."""
    shape = SHAPES[name]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 23)
    gwc = torch.randn(shape, generator=gen)
    w1 = torch.randn(shape[1], 9, generator=gen) / 3
    w2 = torch.randn(shape[1], 9, generator=gen) / 3
    g = torch.randn(shape, generator=gen)
    return gwc, w1, w2, g


def statement(gwc, w1, w2, g, dilation, dtype=None, device="cpu"):
    """The call site's statement from nn.Conv3d modules and its autograd -> the four kinds (+ the output's grad_fn)."""
    dtype = dtype or gwc.dtype
    ng_all = gwc.shape[1]
    x = gwc.detach().to(device=device, dtype=dtype).requires_grad_(True)
    patch = nn.Conv3d(ng_all, ng_all, (1, 3, 3), 1, (0, 1, 1), 1, groups=ng_all, bias=False).to(device=device, dtype=dtype)
    layers = [nn.Conv3d(n, n, (1, 3, 3), 1, (0, dl, dl), dl, groups=n, bias=False).to(device=device, dtype=dtype)
              for _, n, dl in runs_of(dilation)]
    with torch.no_grad():
        patch.weight.copy_(w1.reshape(ng_all, 1, 1, 3, 3))
        for m, (g0, n, _) in zip(layers, runs_of(dilation)):
            m.weight.copy_(w2[g0:g0 + n].reshape(n, 1, 1, 3, 3))
    mid = patch(x)
    out = torch.cat([m(mid[:, g0:g0 + n]) for m, (g0, n, _) in zip(layers, runs_of(dilation))], dim=1)
    out.backward(g.to(device=device, dtype=dtype))
    return dict(out=out.detach(), dgwc=x.grad, dw1=patch.weight.grad.reshape(ng_all, 9),
                dw2=torch.cat([m.weight.grad.reshape(-1, 9) for m in layers])), out.grad_fn


def run(gwc, w1, w2, g, dilation, want=(True, True, True)):
    """patch_volume_train on the GPU and its backward; want = (gwc, w1, w2) require a gradient."""
    x, a, c = (t.detach().cuda().requires_grad_(k) for t, k in zip((gwc, w1, w2), want))
    out = patch_volume_train(x, a, c, dilation)
    out.backward(g.cuda())
    return dict(out=out.detach(), dgwc=x.grad, dw1=a.grad, dw2=c.grad), out


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, float64 reference, float32 yardstick); computed once, left unchanged."""
    out = {}
    for name in SHAPES:
        x = make_inputs(name)
        out[name] = (x, statement(*x, dil_of(name), torch.float64)[0], statement(*x, dil_of(name), torch.float32)[0])
    return out


def test_inputs_reach_what_they_are_meant_to_reach(refs):
    lib = _lib.load()
    slots = lambda name: lib.dv_patch_volume_bwd_workspace_floats(*SHAPES[name]) // (SHAPES[name][1] * 18)
    assert slots("many_blocks") == 24 and slots("row_tiles") == 2 * 2 * 2 and slots("col_tiles") == 2
    assert slots("tiny") == 1 and slots("many_planes") == 2 * 2100
    b, _, d, h, w = SHAPES["many_planes"]
    assert max(b * n * d for _, n, _ in runs_of(NET)) > 65535 and w % 4 == 0
    # tiny: no row lies beyond the smallest halo (1 + 1), no column beyond the halo of dilation 2; both widths are odd
    assert SHAPES["tiny"][3] <= 1 + 1 and SHAPES["tiny"][4] <= 1 + 2 and SHAPES["tiny"][4] % 4 and SHAPES["odd_w"][4] % 4
    assert all(SHAPES[n][4] % 4 == 0 for n in ("row_tiles", "col_tiles", "many_blocks", "mixed_runs"))
    assert len(runs_of(dil_of("mixed_runs"))) == 4 and len(runs_of(NET)) == 3
    for name, (_, f64, _) in refs.items():                                   # every gradient is live
        assert all(bool((f64[k] != 0).any()) for k in KINDS), name


def test_values_and_gradients_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    bar = Bar()
    for name, (x, f64, f32) in refs.items():
        got, _ = run(*x, dil_of(name))
        for k in KINDS:
            assert got[k].shape == f64[k].shape and got[k].dtype == torch.float32, (name, k)
            assert bool(torch.isfinite(got[k]).all()), (name, k)
            bar(got[k], f32[k], f64[k], k, name)
    bar.check()


def test_forward_has_the_bits_of_the_eval_kernel(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    for name in ("row_tiles", "odd_w", "many_blocks", "mixed_runs"):
        x = refs[name][0]
        got, _ = run(*x, dil_of(name))
        table = torch.tensor(dil_of(name), dtype=torch.int32, device="cuda")
        with torch.no_grad():
            assert torch.equal(got["out"], patch_volume(x[0].cuda(), x[1].cuda(), x[2].cuda(), table)), name


@pytest.mark.parametrize("name", ["many_blocks", "odd_w"])
def test_frozen_inputs_get_no_gradient_and_leave_the_others_bit_for_bit(refs, name, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    x = refs[name][0]
    full, _ = run(*x, dil_of(name))
    for want in ((True, False, False), (False, True, True), (True, True, False), (True, False, True), (False, True, False),
                 (False, False, True)):
        got, _ = run(*x, dil_of(name), want=want)
        assert torch.equal(got["out"], full["out"]), want
        for k, wanted in zip(("dgwc", "dw1", "dw2"), want):
            assert (got[k] is None) if not wanted else torch.equal(got[k], full[k]), (want, k)


def test_two_runs_give_the_same_bits(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    for name in ("many_blocks", "odd_w", "many_planes"):
        x = refs[name][0]
        a, _ = run(*x, dil_of(name))
        b, _ = run(*x, dil_of(name))
        assert all(torch.equal(a[k], b[k]) for k in KINDS), name


def test_a_batch_gives_the_input_gradient_bits_of_its_items(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    for name in ("many_blocks", "row_tiles", "mixed_runs"):
        gwc, w1, w2, g = refs[name][0]
        whole, _ = run(gwc, w1, w2, g, dil_of(name))
        for i in range(gwc.shape[0]):
            item, _ = run(gwc[i:i + 1], w1, w2, g[i:i + 1], dil_of(name))
            assert torch.equal(item["dgwc"], whole["dgwc"][i:i + 1]), (name, i)
            assert torch.equal(item["out"], whole["out"][i:i + 1]), (name, i)


def test_returns_a_fresh_tensor_and_saves_exactly_its_three_inputs(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    x, a, c = (t.cuda().requires_grad_(True) for t in refs["row_tiles"][0][:3])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        out = patch_volume_train(x, a, c, NET)
    assert out.grad_fn.name() == "PatchVolumeFnBackward"
    assert out.data_ptr() != x.data_ptr() and out.shape == x.shape
    assert sorted(t.data_ptr() for t in saved) == sorted(t.data_ptr() for t in (x, a, c))
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):                                        # once_differentiable: no double backward
        gx.sum().backward()


def test_torch_route_is_the_statement_and_bad_arguments_raise(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_PATCH", "torch")
    for name in ("odd_w", "mixed_runs"):
        x = refs[name][0]
        got, out = run(*x, dil_of(name))
        assert "PatchVolumeFn" not in out.grad_fn.name()
        want, _ = statement(*x, dil_of(name), device="cuda")
        assert torch.equal(got["out"], want["out"]), name
        # the same convolution calls behind it; their backward is MIOpen's, whose summation order is not this project's
        assert all(rel(got[k], refs[name][1][k]) < 1e-5 and rel(got[k], want[k].cpu()) < 1e-5 for k in KINDS), name
    x, a, c = (t.cuda() for t in refs["odd_w"][0][:3])
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_PATCH", route)
        with pytest.raises(TypeError):
            patch_volume_train(x.double(), a.double(), c.double(), NET)
        with pytest.raises(DiffuVolumeError):
            patch_volume_train(x.cpu(), a.cpu(), c.cpu(), NET)
        with pytest.raises(RuntimeError):
            patch_volume_train(x, a[:-1], c, NET)
        with pytest.raises(RuntimeError):
            patch_volume_train(x[0], a, c, NET)
        with pytest.raises(ValueError):
            patch_volume_train(x, a, c, NET[:-1])
        with pytest.raises(ValueError):
            patch_volume_train(x, a, c, (4,) + NET[1:])
    monkeypatch.setenv("DV_TRAIN_PATCH", "eager")
    with pytest.raises(ValueError):
        patch_volume_train(x, a, c, NET)


def carve(t, fill=None):
    """t's values (or `fill`) in the middle of a sentinel-filled arena -> (arena, view), 4 bytes off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD,), SENT, device="cuda")
    v = arena[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return arena, v


def intact(arena, n):
    return bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + n:] == SENT).all())


@pytest.mark.parametrize("name", ["row_tiles", "odd_w", "mixed_runs"])
def test_patch_bwd_abi_offset_views_bounds_and_refusals(refs, name, monkeypatch):
    """dv_patch_volume_bwd_f32 as a C caller sees it.  Every operand one float off a 16-byte line sends the entry to the
    element-wise accesses: its results hold the bar and have the bits of the aligned call (which takes the 16-byte accesses
    where W % 4 == 0; both do the same arithmetic).  Outputs and workspace lie between sentinels that survive; outputs
    pre-filled with NaN come back finite, so every element is written; outputs that are not wanted are not touched; NULL
    pointers, no wanted output, a missing workspace, bad sizes and malformed runs are refused with their codes and write
    nothing."""
    monkeypatch.setenv("DV_TRAIN_PATCH", "hip")
    lib, st = _lib.load(), _lib.stream_ptr()
    f = lib.dv_patch_volume_bwd_f32
    shape = SHAPES[name]
    b, ng, d, h, w = shape
    x, f64, f32 = refs[name]
    n, g0, gn, dl, _ = train_patch._runs(tuple(dil_of(name)))
    runs = (n, g0, gn, dl)
    n_ws = lib.dv_patch_volume_bwd_workspace_floats(*shape)
    want, _ = run(*x, dil_of(name))
    nan = float("nan")
    gwc, w1, w2, g = (carve(t.cuda())[1] for t in x)
    outs = {k: carve(torch.empty(shape if k == "dgwc" else (ng, 9)), fill=nan) for k in ("dgwc", "dw1", "dw2")}
    a_ws, v_ws = carve(torch.empty(n_ws), fill=nan)
    o = {k: v for k, (_, v) in outs.items()}
    ins = [gwc.data_ptr(), w1.data_ptr(), w2.data_ptr(), g.data_ptr()]
    assert f(*ins, o["dgwc"].data_ptr(), o["dw1"].data_ptr(), o["dw2"].data_ptr(), v_ws.data_ptr(), *shape, *runs, st) == 0
    torch.cuda.synchronize()
    bar = Bar()
    for k, (a, v) in outs.items():
        assert intact(a, v.numel()), k
        assert bool(torch.isfinite(v).all()), k
        bar(v, f32[k], f64[k], k, f"{name} carved")
        assert torch.equal(v, want[k]), k
    bar.check()
    assert intact(a_ws, n_ws)

    # only dgwc: no workspace needed, dw1 / dw2 and the workspace are not touched; only dw2: dgwc is not touched
    for k in outs:
        outs[k][1].fill_(nan)
    v_ws.fill_(nan)
    null = ctypes.c_void_p(None)
    assert f(*ins, o["dgwc"].data_ptr(), null, null, null, *shape, *runs, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o["dgwc"], want["dgwc"]) and bool(torch.isnan(v_ws).all())
    assert bool(torch.isnan(o["dw1"]).all()) and bool(torch.isnan(o["dw2"]).all())
    o["dgwc"].fill_(nan)
    assert f(*ins, null, null, o["dw2"].data_ptr(), v_ws.data_ptr(), *shape, *runs, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(o["dw2"], want["dw2"]) and bool(torch.isnan(o["dgwc"]).all()) and bool(torch.isnan(o["dw1"]).all())
    assert all(intact(a, v.numel()) for a, v in outs.values()) and intact(a_ws, n_ws)

    # refusals: nothing is launched, nothing is written
    arenas = [a for a, _ in outs.values()] + [a_ws]
    for a in arenas:
        a.fill_(SENT)
    full = ins + [o["dgwc"].data_ptr(), o["dw1"].data_ptr(), o["dw2"].data_ptr(), v_ws.data_ptr()]
    for i in (0, 1, 2, 3):
        a = list(full)
        a[i] = null
        assert f(*a, *shape, *runs, st) == -1, i
    assert f(*ins, null, null, null, full[7], *shape, *runs, st) == -1                     # nothing wanted
    assert f(*full[:7], null, *shape, *runs, st) == -1                                     # dw1 / dw2 without a workspace
    for i in (1, 2, 3):
        r = list(runs)
        r[i] = None
        assert f(*full, *shape, *r, st) == -1, i
    for i in range(5):
        bad = list(shape)
        bad[i] = 0
        assert f(*full, *bad, *runs, st) == -2, i
        bad[i] = -shape[i]
        assert f(*full, *bad, *runs, st) == -2, i
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    assert f(*full, *shape, 0, g0, gn, dl, st) == -2
    assert f(*full, *shape, n - 1, g0, gn, dl, st) == -2                                   # the runs stop short of G
    assert f(*full, b, ng + 1, d, h, w, *runs, st) == -2
    assert f(*full, *shape, 1, ints(1), ints(ng), ints(1), st) == -2                       # does not start at group 0
    assert f(*full, *shape, 2, ints(0, 2), ints(1, ng - 1), ints(1, 2), st) == -2          # a gap
    assert f(*full, *shape, 2, ints(0, ng), ints(ng, 0), ints(1, 2), st) == -2             # an empty run
    for bad_dl in (0, 4, -1):
        assert f(*full, *shape, 1, ints(0), ints(ng), ints(bad_dl), st) == -2, bad_dl
    torch.cuda.synchronize()
    assert all(bool((a == SENT).all()) for a in arenas)
