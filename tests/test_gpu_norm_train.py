"""BatchNorm3d (batch statistics) + skip + activation on HIP (diffuvolume_amd/train_norm.py, csrc/bn3d_act.hip) against the
PyTorch statement  act(F.batch_norm(x, ..., training=True) + skip)  evaluated with float64 autograd on the CPU.  The
yardstick is the same statement in float32 on the CPU.  Bar (test_gpu_regress_train.Bar, the form of test_gpu_acv_train.Bar):
per kind of tensor (y, dx, dskip, dgamma, dbeta, running_mean, running_var) every HIP relative L2 error is at most 2x the
worst float32 one of that kind + 1e-6; the ratios are printed.

Shapes are the smallest that reach each path of the kernels (one block per chunk of 8192 floats of a (b,c) slab, 16-byte
accesses when S % 4 == 0 and everything lies on a 16-byte line):
  sub_wave   [2,3,1,1,5]     fewer elements than a wave, odd S
  one_item   [1,32,4,6,8]    B = 1, S % 4 == 0 but a single short chunk per slab
  odd_s      [2,8,3,5,7]     S % 4 != 0: the scalar kernels
  vector     [2,4,16,32,64]  S = 32768 = 4 chunks per slab, 2 * 4 = 8 partials per channel (>= 3), more than one block
  big_mean*  per-channel mean 1e3 and std 1 (a plain sum of squares loses every digit of the variance there), at odd_s and
             at vector (the merge of partials whose means are large).  Held with "none" and "mish" only: at that mean a
             float32 `mean` is 6e-5 coarse, z moves by as much, and a ReLU whose z lies that close to 0 takes another
             decision in float32 than in float64 -- in the yardstick as well as in the kernel -- which measures the
             data's distance to 0, not the arithmetic
  mish_tails gamma = 15: z reaches beyond +-20 (softplus' threshold, and exp(z) -> 0)
  relu_zeros gamma = beta = 0 on two channels and exact zeros in skip: z == 0 exactly, where ReLU' is 0
Every case runs with each of the three activations and with no skip, a skip that wants a gradient and one that does not."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from diffuvolume_amd import DiffuVolumeError, _lib, batch_norm_act_train, train_norm
from test_gpu_regress_train import Bar, rel

pytestmark = pytest.mark.gpu

EPS = 1e-5
ACTS = ("none", "relu", "mish")
ACT_CODE = {"none": 0, "relu": 1, "mish": 2}
KINDS = ("y", "dx", "dskip", "dgamma", "dbeta", "running_mean", "running_var")
SHAPES = {
    "sub_wave": (2, 3, 1, 1, 5),
    "one_item": (1, 32, 4, 6, 8),
    "odd_s": (2, 8, 3, 5, 7),
    "vector": (2, 4, 16, 32, 64),
    "big_mean": (2, 8, 3, 5, 7),
    "big_mean_vector": (2, 4, 16, 32, 64),
    "mish_tails": (2, 8, 3, 5, 7),
    "relu_zeros": (2, 8, 3, 5, 7),
}
MOMENTUM = {"odd_s": 0.3, "vector": 0.01}                    # elsewhere the default 0.1
SKIPS = ("no_skip", "skip_grad", "skip_const")
PAD, SENT = 37, -7.0e5                                       # 37 floats: the carved view starts 4 bytes off a 16-byte line


def acts_of(name):
    return ("none", "mish") if name.startswith("big_mean") else ACTS


def make_inputs(name):
    """x, weight, bias, skip, the cotangent g and the initial running buffers of a case (CPU, float32)."""
    shape = SHAPES[name]
    c = shape[1]
    gen = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 11)
    x = torch.randn(shape, generator=gen) * (0.5 + torch.rand(1, c, 1, 1, 1, generator=gen)) + torch.randn(1, c, 1, 1, 1, generator=gen)
    w = 0.5 + torch.rand(c, generator=gen)
    b = 0.3 * torch.randn(c, generator=gen)
    skip = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    if name.startswith("big_mean"):
        x = torch.randn(shape, generator=gen) + 1e3
    if name == "mish_tails":
        w = torch.full((c,), 15.0)
    if name == "relu_zeros":
        w[:2], b[:2] = 0.0, 0.0
        skip[torch.rand(shape, generator=gen) < 0.3] = 0.0
    rm, rv = 0.2 * torch.randn(c, generator=gen), 0.5 + torch.rand(c, generator=gen)
    return x, w, b, skip, g, rm, rv


def statement(x, w, b, skip, g, rm, rv, act, mode, momentum, dtype):
    """The PyTorch statement and its autograd on the CPU in `dtype` -> the seven kinds (+ z)."""
    x, w, b = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    skip = None if mode == "no_skip" else skip.detach().to(dtype).requires_grad_(mode == "skip_grad")
    rm, rv = rm.clone().to(dtype), rv.clone().to(dtype)
    z = F.batch_norm(x, rm, rv, w, b, True, momentum, EPS)
    if skip is not None:
        z = z + skip
    y = F.relu(z) if act == "relu" else z * torch.tanh(F.softplus(z)) if act == "mish" else z
    y.backward(g.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dskip=None if skip is None else skip.grad, dgamma=w.grad, dbeta=b.grad,
                running_mean=rm, running_var=rv, z=z.detach())


def run(x, w, b, skip, g, rm, rv, act, mode, momentum, want=(True, True, True)):
    """batch_norm_act_train on the GPU and its backward; want = (x, weight, bias) require a gradient."""
    x, w, b = (t.detach().cuda().requires_grad_(k) for t, k in zip((x, w, b), want))
    skip = None if mode == "no_skip" else skip.detach().cuda().requires_grad_(mode == "skip_grad")
    rm, rv = rm.clone().cuda(), rv.clone().cuda()
    y = batch_norm_act_train(x, w, b, rm, rv, momentum=momentum, eps=EPS, act=act, skip=skip)
    y.backward(g.cuda())
    return dict(y=y.detach(), dx=x.grad, dskip=None if skip is None else skip.grad, dgamma=w.grad, dbeta=b.grad,
                running_mean=rm, running_var=rv), y


@pytest.fixture(scope="module")
def refs():
    """(case, act, skip mode) -> (inputs, momentum, float64 reference, float32 yardstick); computed once, left unchanged."""
    out = {}
    for name in SHAPES:
        x = make_inputs(name)
        mo = MOMENTUM.get(name, 0.1)
        for act in acts_of(name):
            for mode in SKIPS:
                out[name, act, mode] = (x, mo, statement(*x, act, mode, mo, torch.float64),
                                        statement(*x, act, mode, mo, torch.float32))
    return out


def hold_to_the_bar(refs):
    bar = Bar()
    for (name, act, mode), (x, mo, f64, f32) in refs.items():
        got, _ = run(*x, act, mode, mo)
        for k in KINDS:
            if f64[k] is None:
                assert got[k] is None, (name, act, mode, k)
                continue
            assert got[k].shape == f64[k].shape and got[k].dtype == torch.float32, (name, act, mode, k)
            assert bool(torch.isfinite(got[k]).all()), (name, act, mode, k)
            bar(got[k], f32[k], f64[k], k, f"{name} {act} {mode}")
    bar.check()


def test_inputs_reach_what_they_are_meant_to_reach(refs):
    z = refs["mish_tails", "mish", "no_skip"][2]["z"]
    assert bool((z > 20).any()) and bool((z < -20).any())
    for mode in SKIPS:
        _, _, f64, f32 = refs["relu_zeros", "relu", mode]
        zero = f64["z"] == 0
        assert int(zero.sum()) >= 50 and torch.equal(zero, f32["z"] == 0), mode
        assert bool((f64["dx"][:, 2:] != 0).any())
    x = refs["big_mean", "none", "no_skip"][0][0]
    m, s = x.double().mean(dim=(0, 2, 3, 4)), x.double().std(dim=(0, 2, 3, 4))
    assert bool(((m - 1e3).abs() < 1).all()) and bool(((s - 1).abs() < 0.2).all())
    lib = _lib.load()
    b, c, *dhw = SHAPES["vector"]
    s = dhw[0] * dhw[1] * dhw[2]
    partials = (lib.dv_bn3d_train_workspace_floats(b, c, s) // c - 2) // 3
    assert partials >= 3 and s % 4 == 0, partials
    assert (lib.dv_bn3d_train_workspace_floats(*SHAPES["one_item"][:2], 4 * 6 * 8) // 32 - 2) // 3 == 1


def test_values_and_gradients_within_twice_float32_of_float64(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    hold_to_the_bar(refs)


def test_relu_gradient_is_zero_where_z_is_exactly_zero(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    x, mo, f64, _ = refs["relu_zeros", "relu", "skip_grad"]
    got, _ = run(*x, "relu", "skip_grad", mo)
    zero = (f64["z"] == 0).cuda()
    assert bool((got["dskip"][zero] == 0).all()) and bool((got["y"][zero] == 0).all())
    live = (f64["z"] > 1e-3).cuda()
    assert torch.equal(got["dskip"][live], x[4].cuda()[live])               # dz = dy where z > 0


@pytest.mark.parametrize("name", ["odd_s", "vector"])
def test_frozen_inputs_get_no_gradient_and_leave_the_others_bit_for_bit(refs, name, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    for act in ("relu", "mish", "none"):
        x, mo, _, _ = refs[name, act, "skip_grad"]
        full, _ = run(*x, act, "skip_grad", mo)
        frozen, _ = run(*x, act, "skip_grad", mo, want=(True, False, False))
        assert frozen["dgamma"] is None and frozen["dbeta"] is None
        assert torch.equal(frozen["dx"], full["dx"]) and torch.equal(frozen["dskip"], full["dskip"]), act
        one, _ = run(*x, act, "skip_grad", mo, want=(True, True, False))
        assert one["dbeta"] is None and torch.equal(one["dgamma"], full["dgamma"]) and torch.equal(one["dx"], full["dx"])
        nox, _ = run(*x, act, "skip_grad", mo, want=(False, True, True))
        assert nox["dx"] is None and torch.equal(nox["dskip"], full["dskip"]), act
        assert torch.equal(nox["dgamma"], full["dgamma"]) and torch.equal(nox["dbeta"], full["dbeta"]), act
        const, _ = run(*x, act, "skip_const", mo)
        assert const["dskip"] is None and torch.equal(const["y"], full["y"]), act
        for k in ("dx", "dgamma", "dbeta", "running_mean", "running_var"):
            assert torch.equal(const[k], full[k]), (act, k)
        only_skip, _ = run(*x, act, "skip_grad", mo, want=(False, False, False))
        assert only_skip["dx"] is None and torch.equal(only_skip["dskip"], full["dskip"]), act


def test_two_runs_give_the_same_bits(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    for key in (("vector", "mish", "skip_grad"), ("vector", "relu", "no_skip"), ("odd_s", "none", "skip_grad"),
                ("one_item", "mish", "no_skip")):
        x, mo, _, _ = refs[key]
        a, _ = run(*x, key[1], key[2], mo)
        b, _ = run(*x, key[1], key[2], mo)
        for k in KINDS:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (key, k)


def test_returns_a_fresh_tensor_and_saves_only_inputs_statistics_and_parameters(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    x, mo, _, _ = refs["vector", "mish", "skip_grad"]
    saved = []
    xc, sc = x[0].cuda().requires_grad_(True), x[3].cuda().requires_grad_(True)
    w, b = x[1].cuda().requires_grad_(True), x[2].cuda().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = batch_norm_act_train(xc, w, b, None, None, act="mish", skip=sc)
    assert y.grad_fn.name() == "BatchNormActFnBackward"
    assert y.data_ptr() not in (xc.data_ptr(), sc.data_ptr())
    big = [t for t in saved if t.numel() == xc.numel()]
    assert len(saved) == 6 and sorted(t.data_ptr() for t in big) == sorted((xc.data_ptr(), sc.data_ptr()))
    assert sorted(t.numel() for t in saved if t.numel() != xc.numel()) == [xc.shape[1]] * 4
    (gx,) = torch.autograd.grad(y.sum(), xc, create_graph=True)
    with pytest.raises(RuntimeError):                                        # once_differentiable: no double backward
        gx.sum().backward()


def test_bn_act_on_a_module_counts_batches_honours_momentum_and_works_without_grad(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    x, _, _, _ = refs["odd_s", "relu", "skip_grad"]
    c = x[0].shape[1]
    for momentum in (0.1, 0.45):
        bn = torch.nn.BatchNorm3d(c, eps=EPS, momentum=momentum).cuda().train()
        twin = torch.nn.BatchNorm3d(c, eps=EPS, momentum=momentum).double().train()
        with torch.no_grad():
            for m in (bn, twin):
                m.weight.copy_(x[1]), m.bias.copy_(x[2]), m.running_mean.copy_(x[5]), m.running_var.copy_(x[6])
        xc, sc = x[0].cuda(), x[3].cuda()
        with torch.no_grad():                                                # forward only, the buffers still move
            y0 = train_norm.bn_act(bn, xc, "relu", skip=sc)
            ref = F.relu(twin(x[0].double()) + x[3].double())
        assert y0.grad_fn is None and int(bn.num_batches_tracked) == 1
        assert rel(y0, ref) < 1e-6
        assert rel(bn.running_mean, twin.running_mean) < 1e-6 and rel(bn.running_var, twin.running_var) < 1e-6
        assert not torch.equal(bn.running_mean.cpu(), x[5])
        y1 = train_norm.bn_act(bn, xc.requires_grad_(True), "relu", skip=sc)
        twin(x[0].double())
        assert int(bn.num_batches_tracked) == 2 and torch.equal(y1.detach(), y0)          # same bits with and without grad
        assert y1.grad_fn.name() == "BatchNormActFnBackward"
        assert rel(bn.running_mean, twin.running_mean) < 1e-6 and rel(bn.running_var, twin.running_var) < 1e-6
        assert not bn.running_mean.requires_grad and bn.running_mean.grad_fn is None
    # outside the kernel's case the module's own forward runs, on either route
    bn.eval()
    y = train_norm.bn_act(bn, xc, "relu", skip=sc)
    assert "BatchNormActFn" not in y.grad_fn.name() and int(bn.num_batches_tracked) == 2
    assert torch.equal(y, F.relu(bn(xc) + sc))


def test_torch_route_is_the_statement_and_bad_arguments_raise(refs, monkeypatch):
    monkeypatch.setenv("DV_TRAIN_NORM", "torch")
    x, mo, f64, _ = refs["odd_s", "mish", "skip_grad"]
    got, y = run(*x, "mish", "skip_grad", mo)
    assert "BatchNormActFn" not in y.grad_fn.name()
    assert all(rel(got[k], f64[k]) < 1e-5 for k in KINDS)
    xc, w, b, sc = (x[i].cuda() for i in (0, 1, 2, 3))
    z = F.batch_norm(xc, None, None, w, b, True, mo, EPS) + sc
    assert torch.equal(got["y"], z * torch.tanh(F.softplus(z)))
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_NORM", route)
        with pytest.raises(ValueError):
            batch_norm_act_train(xc, w, b, None, None, act="gelu")
        with pytest.raises(ValueError):                                      # one value per channel: PyTorch raises too
            batch_norm_act_train(xc[:1, :, :1, :1, :1], w, b, None, None)
        with pytest.raises(TypeError):
            batch_norm_act_train(xc.double(), w.double(), b.double(), None, None)
        with pytest.raises(DiffuVolumeError):
            batch_norm_act_train(xc.cpu(), w.cpu(), b.cpu(), None, None)
        with pytest.raises(RuntimeError):
            batch_norm_act_train(xc, w[:-1], b, None, None)
        with pytest.raises(RuntimeError):
            batch_norm_act_train(xc, w, b, None, None, skip=sc[:1])
        with pytest.raises(RuntimeError):
            batch_norm_act_train(xc, w, b, x[5].cuda(), None)
    monkeypatch.setenv("DV_TRAIN_NORM", "eager")
    with pytest.raises(ValueError):
        batch_norm_act_train(xc, w, b, None, None)


def carve(t, fill=None):
    """t's values (or `fill`) in the middle of a sentinel-filled arena -> (arena, view), 4 bytes off a 16-byte line."""
    arena = torch.full((t.numel() + 2 * PAD,), SENT, device="cuda")
    v = arena[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t) if fill is None else v.fill_(fill)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return arena, v


def intact(arena, n):
    return bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + n:] == SENT).all())


@pytest.mark.parametrize("name", ["vector", "one_item", "odd_s", "sub_wave"])
def test_bn3d_abi_offset_views_bounds_and_refusals(refs, name, monkeypatch):
    """dv_bn3d_stats_f32, dv_bn3d_apply_act_f32 and dv_bn3d_act_bwd_f32 as a C caller sees them.  Every operand one float off
    a 16-byte line sends the entries to the scalar kernels: their outputs have the bits of the aligned run (which takes
    the 16-byte kernels where S % 4 == 0).  Outputs and workspace lie between sentinels that survive; outputs pre-filled
    with NaN come back finite, so every element is written; NULL pointers, no wanted output, B*S == 1, a bad act and bad
    sizes are refused with their codes and write nothing."""
    monkeypatch.setenv("DV_TRAIN_NORM", "hip")
    lib, st = _lib.load(), _lib.stream_ptr()
    shape = SHAPES[name]
    b, c = shape[:2]
    s = shape[2] * shape[3] * shape[4]
    n_ws = lib.dv_bn3d_train_workspace_floats(b, c, s)
    nan = float("nan")
    for act, mode in (("relu", "skip_grad"), ("mish", "no_skip"), ("none", "no_skip"), ("none", "skip_grad")):
        x, mo, f64, _ = refs[name, act, mode]
        want, _ = run(*x, act, mode, mo)
        xs, w, bb, sk, g, rm, rv = (carve(t.cuda())[1] for t in x)
        a_rm, rm = carve(x[5].cuda())
        a_rv, rv = carve(x[6].cuda())
        skp = sk.data_ptr() if mode != "no_skip" else None
        outs = {k: carve(torch.empty(shape if k in ("y", "dx", "dskip") else (c,)), fill=nan)
                for k in ("y", "dx", "dskip", "dgamma", "dbeta", "mean", "invstd")}
        a_ws, v_ws = carve(torch.empty(n_ws), fill=nan)
        o = {k: v for k, (_, v) in outs.items()}
        assert lib.dv_bn3d_stats_f32(xs.data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(), rm.data_ptr(),
                                     rv.data_ptr(), v_ws.data_ptr(), b, c, s, mo, EPS, st) == 0
        assert lib.dv_bn3d_apply_act_f32(xs.data_ptr(), skp, o["mean"].data_ptr(), o["invstd"].data_ptr(), w.data_ptr(),
                                         bb.data_ptr(), o["y"].data_ptr(), b, c, s, ACT_CODE[act], st) == 0
        assert lib.dv_bn3d_act_bwd_f32(g.data_ptr(), xs.data_ptr(), skp, o["mean"].data_ptr(), o["invstd"].data_ptr(),
                                       w.data_ptr(), bb.data_ptr(), o["dx"].data_ptr(),
                                       o["dskip"].data_ptr() if skp else None, o["dgamma"].data_ptr(),
                                       o["dbeta"].data_ptr(), v_ws.data_ptr(), b, c, s, ACT_CODE[act], st) == 0
        torch.cuda.synchronize()
        for k, (a, v) in outs.items():
            assert intact(a, v.numel()), (act, mode, k)
            if k == "dskip" and not skp:
                assert bool(torch.isnan(v).all())                            # not wanted: not touched
                continue
            assert bool(torch.isfinite(v).all()), (act, mode, k)
            if k in want:
                assert torch.equal(v, want[k]), (act, mode, k)
        assert intact(a_ws, n_ws) and intact(a_rm, c) and intact(a_rv, c)
        assert torch.equal(rm, want["running_mean"]) and torch.equal(rv, want["running_var"])
        assert rel(o["mean"], x[0].double().mean(dim=(0, 2, 3, 4))) < 1e-6
        # without running buffers: the same statistics, nothing else
        m2, i2 = torch.empty_like(o["mean"]), torch.empty_like(o["invstd"])
        assert lib.dv_bn3d_stats_f32(xs.data_ptr(), m2.data_ptr(), i2.data_ptr(), None, None, v_ws.data_ptr(), b, c, s,
                                     mo, EPS, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(m2, o["mean"]) and torch.equal(i2, o["invstd"])
        assert torch.equal(rm, want["running_mean"]) and intact(a_ws, n_ws)

    # refusals: nothing is launched, nothing is written
    arenas = [a for a, _ in outs.values()] + [a_ws, a_rm, a_rv]
    for a in arenas:
        a.fill_(SENT)
    null = ctypes.c_void_p(None)
    stats = [xs.data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(), rm.data_ptr(), rv.data_ptr(), v_ws.data_ptr()]
    apply = [xs.data_ptr(), sk.data_ptr(), o["mean"].data_ptr(), o["invstd"].data_ptr(), w.data_ptr(), bb.data_ptr(),
             o["y"].data_ptr()]
    bwd = [g.data_ptr(), xs.data_ptr(), sk.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr(), bb.data_ptr(),
           o["dx"].data_ptr(), o["dskip"].data_ptr(), o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), v_ws.data_ptr()]
    for i in (0, 1, 2, 5):
        a = list(stats)
        a[i] = null
        assert lib.dv_bn3d_stats_f32(*a, b, c, s, 0.1, EPS, st) == -1
    assert lib.dv_bn3d_stats_f32(*stats[:3], null, stats[4], stats[5], b, c, s, 0.1, EPS, st) == -1
    for i in (0, 2, 3, 4, 5, 6):
        a = list(apply)
        a[i] = null
        assert lib.dv_bn3d_apply_act_f32(*a, b, c, s, 1, st) == -1
    for i in (0, 1, 3, 4, 5, 6, 11):
        a = list(bwd)
        a[i] = null
        assert lib.dv_bn3d_act_bwd_f32(*a, b, c, s, 1, st) == -1
    assert lib.dv_bn3d_act_bwd_f32(*bwd[:7], null, null, null, null, bwd[11], b, c, s, 1, st) == -1      # nothing wanted
    assert lib.dv_bn3d_act_bwd_f32(*bwd[:2], null, *bwd[3:], b, c, s, 1, st) == -1                       # dskip without skip
    for bad in ((0, c, s), (b, 0, s), (b, c, 0), (b, c, -s)):
        assert lib.dv_bn3d_stats_f32(*stats, *bad, 0.1, EPS, st) == -2
        assert lib.dv_bn3d_apply_act_f32(*apply, *bad, 1, st) == -2
        assert lib.dv_bn3d_act_bwd_f32(*bwd, *bad, 1, st) == -2
    assert lib.dv_bn3d_stats_f32(*stats, 1, c, 1, 0.1, EPS, st) == -3                                    # B*S == 1
    assert lib.dv_bn3d_act_bwd_f32(*bwd, 1, c, 1, 1, st) == -3
    for act in (-1, 3, 4, 5):
        assert lib.dv_bn3d_apply_act_f32(*apply, b, c, s, act, st) == -3
        assert lib.dv_bn3d_act_bwd_f32(*bwd, b, c, s, act, st) == -3
    torch.cuda.synchronize()
    assert all(bool((a == SENT).all()) for a in arenas)
