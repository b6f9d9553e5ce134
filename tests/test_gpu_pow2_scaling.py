"""Exact power-of-two equivariance of the linear kernels.

Any sequence of fp32 ``+``, ``*``, ``fma`` and MFMA accumulations commutes bit for bit with scaling an operand by a power
of two as long as nothing under- or overflows, and so do the Winograd transforms (their factors are +-1, 1/2 and 1/4).  So
for every row of the table below, with unit ``randn`` operands (every intermediate then stays within 2^+-70):

    torch.equal(op(a * x), a * op(x))    for a = 2^30 and a = 2^-30
    torch.equal(op(-x), -op(x))          unless the row rectifies (ReLU, leaky ReLU: positive scaling is all they keep)

with each operand of a bilinear op scaled on its own, a bias / residual / skip scaled along with the operand it is added
to, BatchNorm folded with zero shift.  No float64 reference is involved: what this catches is what a reference compared
at amplitude 1 cannot -- an absolute threshold, a flush, a fixed pre-scale, an accumulator that starts from something
other than zero.  The 16-bit training entries are in the table with a = 2^+-4, where every rounded operand stays a normal
number -- and WITHOUT the sign flip, see below.  Each row names the C entry it is there for, and the test asserts that this
entry ran.

Measured on the MI355X: every float32 row holds for 2^30, 2^-30 and -1 -- no float32 kernel here has an absolute
threshold, a flush or a stale accumulator -- and every 16-bit row holds for 2^4 and 2^-4.  The sign flip does NOT hold for
the 16-bit rows: op(-x) and -op(x) differ in 0.4 .. 9 % of the elements, by up to 1.2 units of 2^-24 * sum |operands|
(largest difference 9.5e-7 .. 7.6e-6 on unit operands), in all seven of them -- three kernels with three different
stagings (csrc/conv3d_mp.h, csrc/conv3d_wgrad_mp.h, csrc/conv2d_wgrad_cat_f16.hip), at fp16 and at bf16, while the fp32
rows of the same shapes are exact.  What the seven share is v_mfma_f32_16x16x32_{f16,bf16}, and the instruction alone shows
it: one wave, one instruction, C = 0, unit normal A and B, and 3.3 % (f16) / 0.3 % (bf16) of the 16 x 16 outputs of D(-A, B)
are not -D(A, B) (largest difference 1.9e-6 / 9.5e-7).  The rounding inside its 32-product sum is not symmetric about
zero; the fp32 instruction is an fmaf chain and is.  The operands' own rounding is symmetric (round to nearest) and
nothing in the kernels' code depends on a sign, so there is nothing to fix in them; the
per-element bars of tests/test_gpu_amp_magnitudes.py count a rounding per product and hold either way (sign-coherent
operands, where such a one-sided rounding adds up, reach 13 of c = 224 .. 1120 there against 1 .. 2 for signed ones).

Left out, and why:
  * everything with a softmax, sigmoid, tanh, Mish or ReLU6 IN THE SCALED OPERAND is not homogeneous: the regression tails'
    forward, the feature gate's logit, window attention's forward, the ConvGRU gates, ``dv_refine_inputs_f32`` (Mish), the
    DDIM state updates (clamps and thresholds), instance norm and batch norm forward (they divide by the scale); their
    backward entries are here as functions of the cotangent, which they are linear in;
  * the metrics are counts;
  * ``f16x3`` has a fixed pre-scale: tests/test_gpu_conv_f16x3_floor.py is about it.
"""
import pytest
import torch

from diffuvolume_amd import _lib, train2d, train3d
from diffuvolume_amd import submodule as S
from diffuvolume_amd import train_attn, train_loss, train_net2d, train_norm, train_patch, train_tail, train_volume
from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
from diffuvolume_amd.igev_upsample import context_upsample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG, SMALL = 2.0 ** 30, 2.0 ** -30
TABLE = []


class Row:
    def __init__(self, name, entry, make, signed, alphas):
        self.name, self.entry, self.make, self.signed, self.alphas = name, entry, make, signed, alphas


def row(name, entry, signed=True, alphas=(BIG, SMALL)):
    """``make() -> (fn, operands, groups)``: ``fn(**operands)`` is a tensor or a tuple of tensors; each group names the
    operands that are scaled together, and the result must scale with them."""
    def deco(make):
        TABLE.append(Row(name, entry, make, signed, alphas))
        return make
    return deco


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def unit_bn(cout, seed):
    """BatchNorm that folds to a per-channel scale in [0.6, 1.5] and a shift of exactly zero."""
    g = torch.Generator().manual_seed(seed)
    return tuple(t.to(DEV) for t in (torch.rand(cout, generator=g) + 0.5, torch.zeros(cout), torch.zeros(cout),
                                     torch.rand(cout, generator=g) + 0.5))


@pytest.fixture(autouse=True)
def hip_routes(monkeypatch):
    for knob in ("CONV3D", "CONV2D", "LOOKUP", "TAIL", "VOLUME", "NORM", "PATCH", "ATTN", "NET2D", "LOSS"):
        monkeypatch.setenv(f"DV_TRAIN_{knob}", "hip")


@pytest.fixture
def launched(monkeypatch):
    """The names of the entries that ran (every launch reports its return code to ``_lib.check`` under its name)."""
    seen, real = [], _lib.check

    def spy(code, what):
        seen.append(what)
        return real(code, what)

    monkeypatch.setattr(_lib, "check", spy)
    return seen


def as_tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


@pytest.mark.parametrize("r", TABLE, ids=lambda r: r.name)
def test_scaling_an_operand_by_a_power_of_two_scales_the_result_bit_for_bit(r, launched):
    fn, operands, groups = r.make()
    base = as_tuple(fn(**operands))
    assert r.entry in launched, (r.entry, sorted(set(launched)))
    assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in base)
    for group in groups:
        assert set(group) <= set(operands), group
        for alpha in (*r.alphas, *((-1.0,) if r.signed else ())):
            scaled = {k: (v * alpha if k in group else v) for k, v in operands.items()}
            for i, (got, want) in enumerate(zip(as_tuple(fn(**scaled)), base)):
                assert torch.isfinite(got).all()
                assert torch.equal(got, want * alpha), (r.name, group, alpha, i, float((got - want * alpha).abs().max()))


def test_the_table_names_every_route_it_promises():
    entries = {r.entry for r in TABLE}
    for e in ("dv_conv3d_wino_f32", "dv_conv3d_wino3_f32", "dv_conv3d_s2pp_f32", "dv_conv3d_f32", "dv_deconv3d_k3s2_f32",
              "dv_deconv3d_k3s2_redir_f32", "dv_deconv3d_k4s2_f32", "dv_conv2d_gated_f32", "dv_conv2d_wino_dil_cat_f32",
              "dv_conv2d_s2_f32", "dv_conv2d_cat_f32", "dv_conv2d_cat_ksplit_f32", "dv_conv2d_wino_cat_ksplit_f32",
              "dv_conv2d_fewin_f32", "dv_dwconv3x3_f32", "dv_gwc_volume_f32", "dv_concat_volume_f32",
              "dv_concat_attn_volume_f32", "dv_patch_volume_runs_f32", "dv_allpairs_corr_f32", "dv_geo_filter_lookup_f32",
              "dv_conv3d_wgrad_f32", "dv_conv2d_wgrad_f32", "dv_deconv3d_k4s2_wgrad_f32", "dv_deconv3d_k4s2_dgrad_f32",
              "dv_feature_gate_bwd_f32", "dv_resize_bilinear_ac_bwd_f32", "dv_context_upsample_bwd_f32",
              "dv_geo_filter_lookup_bwd_f32", "dv_gwc_volume_bwd_f32", "dv_concat_volume_bwd_f32", "dv_patch_volume_bwd_f32",
              "dv_upsample_softmax_regress_bwd_f32", "dv_window_attn3d_bwd_f32", "dv_bn3d_act_bwd_f32",
              "dv_masked_loss_fwd_f32", "dv_masked_loss_bwd_f32", "dv_conv3d_k3s1_f16_f32", "dv_conv3d_k3s1_bf16_f32",
              "dv_conv3d_wgrad_f16_f32", "dv_conv3d_wgrad_bf16_f32", "dv_conv2d_wgrad_cat_f16"):
        assert e in entries, e


# ------------------------------------------------------------------ Conv3dPlan at f32
ACTS = {"none": S.ACT_NONE, "relu": S.ACT_RELU, "leaky": S.ACT_LEAKY}
# route -> (entry without in_scale, entry with in_scale, cin, cout, (B, D, H, W), k, stride, precision)
CONV3D = {
    "wino": ("dv_conv3d_wino_f32", "dv_conv3d_wino_f32", 8, 16, (1, 3, 5, 18), 3, 1, "f32"),
    "wino3": ("dv_conv3d_wino3_f32", "dv_conv3d_wino_f32", 64, 32, (1, 3, 5, 12), 3, 1, "f32"),      # Cin >= 64, W % 4 == 0
    "s2pp": ("dv_conv3d_s2pp_f32", "dv_conv3d_f32", 8, 64, (1, 3, 5, 8), 3, 2, "f32"),
    "s2_odd_w": ("dv_conv3d_f32", "dv_conv3d_f32", 8, 64, (1, 3, 5, 9), 3, 2, "f32"),
    "k1": ("dv_conv3d_f32", "dv_conv3d_f32", 12, 20, (1, 3, 5, 18), 1, 1, "f32"),
    "head": ("dv_conv3d_f32", "dv_conv3d_f32", 32, 1, (1, 3, 5, 18), 3, 1, "f32"),                  # Cout == 1
    "direct": ("dv_conv3d_f32", "dv_conv3d_f32", 8, 16, (1, 3, 5, 18), 3, 1, "f32_direct"),
}
# (in_scale, residual, activation)
CONV3D_FORMS = [(False, False, "none"), (True, True, "relu"), (False, True, "leaky"), (True, False, "none")]


def conv3d_row(route, form):
    plain, filt, cin, cout, dims, k, stride, precision = CONV3D[route]
    with_scale, with_res, act = form

    def make():
        bn = unit_bn(cout, 1)
        x, w = rnd(dims[0], cin, *dims[1:], seed=2), rnd(cout, cin, k, k, k, seed=3, scale=0.2)

        def fn(x, w, in_scale=None, residual=None):
            plan = S.Conv3dPlan(w, bn, stride=stride, act=ACTS[act], precision=precision)
            return plan(x, in_scale=in_scale, residual=residual)

        ops, groups = dict(x=x, w=w), [["x"], ["w"]]
        if with_scale:
            ops["in_scale"] = torch.rand(dims[0], *dims[1:], generator=torch.Generator().manual_seed(4)).to(DEV) + 0.25
            groups.append(["in_scale"])
        if with_res:
            ops["residual"] = rnd(*S.Conv3dPlan(w, bn, stride=stride, precision=precision).out_shape(x.shape), seed=5)
            groups = [g + ["residual"] for g in groups]
        return fn, ops, groups

    name = f"conv3d {route}" + (" in_scale" if with_scale else "") + (" residual" if with_res else "") + f" {act}"
    row(name, filt if with_scale else plain, signed=act == "none")(make)


for _route in CONV3D:
    for _form in CONV3D_FORMS:
        conv3d_row(_route, _form)


# ------------------------------------------------------------------ Deconv3dPlan
def deconv3d_row(name, entry, k, impl, cin, cout, dims, act, mode):
    def make():
        bn = unit_bn(cout, 6)
        x, w = rnd(dims[0], cin, *dims[1:], seed=7), rnd(cin, cout, k, k, k, seed=8, scale=0.2)
        odims = (dims[0], cout, *(2 * n for n in dims[1:]))
        ops, groups = dict(x=x, w=w), [["x"], ["w"]]
        if mode == "res":
            ops["residual"] = rnd(*odims, seed=9)
            groups = [g + ["residual"] for g in groups]
        if mode == "redir":
            cskip = 8
            rbn = unit_bn(cout, 10)
            ops["skip"], ops["rw"] = rnd(dims[0], cskip, *odims[2:], seed=11), rnd(cout, cskip, 1, 1, 1, seed=12, scale=0.3)
            groups = [["x", "skip"], ["w", "rw"], ["x", "rw"], ["w", "skip"]]

        def fn(x, w, residual=None, skip=None, rw=None):
            lib = _lib.load()
            assert lib.dv_deconv3d_set_impl(impl) == 0               # 1: one tile per block, 2: the persistent kernel
            try:
                plan = S.Deconv3dPlan(w, bn, act=ACTS[act], redir=None if rw is None else (rw, rbn))
                return plan(x, residual=residual, skip=skip)
            finally:
                lib.dv_deconv3d_set_impl(0)

        return fn, ops, groups

    row(name, entry, signed=act == "none")(make)


deconv3d_row("deconv3d k3 one-tile", "dv_deconv3d_k3s2_f32", 3, 1, 16, 32, (1, 3, 5, 20), "none", "plain")
deconv3d_row("deconv3d k3 one-tile residual leaky", "dv_deconv3d_k3s2_f32", 3, 1, 16, 32, (1, 3, 5, 20), "leaky", "res")
deconv3d_row("deconv3d k3 persistent", "dv_deconv3d_k3s2_f32", 3, 2, 16, 32, (1, 3, 5, 20), "none", "plain")
deconv3d_row("deconv3d k3 persistent relu", "dv_deconv3d_k3s2_f32", 3, 2, 16, 32, (1, 3, 5, 20), "relu", "plain")
deconv3d_row("deconv3d k3 persistent redir", "dv_deconv3d_k3s2_redir_f32", 3, 2, 16, 32, (1, 3, 5, 20), "none", "redir")
deconv3d_row("deconv3d k3 one-tile redir relu", "dv_deconv3d_k3s2_redir_f32", 3, 1, 16, 32, (1, 3, 5, 20), "relu", "redir")
deconv3d_row("deconv3d k4", "dv_deconv3d_k4s2_f32", 4, 0, 16, 8, (1, 2, 3, 10), "none", "plain")
deconv3d_row("deconv3d k4 residual leaky", "dv_deconv3d_k4s2_f32", 4, 0, 16, 8, (1, 2, 3, 10), "leaky", "res")


# ------------------------------------------------------------------ the 2-D plans
def conv2d_row(name, entry, chans, cout, hw, k=3, dilation=1, stride=1, act="none", res=False, bias=False):
    def make():
        cin = sum(chans)
        bn = unit_bn(cout, 13)
        parts = {f"x{i}": rnd(2, c, *hw, seed=14 + i) for i, c in enumerate(chans)}
        ops = dict(parts, w=rnd(cout, cin, k, k, seed=20, scale=0.2))
        groups = [list(parts), ["w"]]
        oh, ow = ((n - 1) // stride + 1 for n in hw)
        if bias:                                           # a conv bias instead of the BatchNorm: it scales with the result
            ops["b"] = rnd(cout, seed=21)
            groups = [g + ["b"] for g in groups]
        if res:
            ops["residual"] = rnd(2, cout, oh, ow, seed=22)
            groups = [g + ["residual"] for g in groups]

        def fn(w, residual=None, b=None, **xs):
            plan = S.Conv2dPlan(w, None if bias else bn, dilation=dilation, act=ACTS[act], bias=b, stride=stride)
            x = [xs[n] for n in parts]
            return plan(x if len(x) > 1 else x[0], residual=residual)

        return fn, ops, groups

    row(name, entry, signed=act == "none")(make)


conv2d_row("conv2d direct", "dv_conv2d_gated_f32", (8,), 16, (9, 21))
conv2d_row("conv2d direct bias residual relu", "dv_conv2d_gated_f32", (8,), 16, (9, 21), act="relu", res=True, bias=True)
conv2d_row("conv2d direct k1", "dv_conv2d_gated_f32", (16,), 16, (9, 21), k=1)
conv2d_row("conv2d winograd", "dv_conv2d_wino_dil_cat_f32", (16,), 64, (33, 130))
conv2d_row("conv2d winograd residual leaky", "dv_conv2d_wino_dil_cat_f32", (16,), 64, (33, 130), act="leaky", res=True)
conv2d_row("conv2d winograd dilation 2", "dv_conv2d_wino_dil_cat_f32", (16,), 64, (70, 130), dilation=2)
conv2d_row("conv2d direct dilation 16", "dv_conv2d_gated_f32", (16,), 16, (9, 21), dilation=16)
conv2d_row("conv2d stride 2", "dv_conv2d_s2_f32", (8,), 16, (9, 21), stride=2)
conv2d_row("conv2d stride 2 residual relu", "dv_conv2d_s2_f32", (8,), 16, (9, 21), stride=2, act="relu", res=True)
conv2d_row("conv2d cat direct", "dv_conv2d_cat_f32", (5, 3), 16, (9, 21))
conv2d_row("conv2d cat winograd", "dv_conv2d_wino_dil_cat_f32", (9, 7), 64, (33, 130))
conv2d_row("conv2d direct K-split", "dv_conv2d_cat_ksplit_f32", (256,), 32, (9, 21), res=True)
conv2d_row("conv2d winograd K-split", "dv_conv2d_wino_cat_ksplit_f32", (100, 28), 64, (33, 130))


@row("conv2d fewin k7 s2", "dv_conv2d_fewin_f32")
def _fewin():
    fn = lambda x, w, b: train2d.conv2d_fewin(x, w, b, stride=2)
    return fn, dict(x=rnd(2, 3, 9, 21, seed=23), w=rnd(16, 3, 7, 7, seed=24, scale=0.2), b=rnd(16, seed=25)), [["x", "b"], ["w", "b"]]


@row("depthwise 3x3 s1", "dv_dwconv3x3_f32")
def _dw1():
    return (lambda x, w: train2d.dwconv2d(x, w, 1)), dict(x=rnd(2, 5, 7, 9, seed=26), w=rnd(5, 1, 3, 3, seed=27)), [["x"], ["w"]]


@row("depthwise 3x3 s2", "dv_dwconv3x3_f32")
def _dw2():
    return (lambda x, w: train2d.dwconv2d(x, w, 2)), dict(x=rnd(2, 5, 33, 130, seed=28), w=rnd(5, 1, 3, 3, seed=29)), [["x"], ["w"]]


# ------------------------------------------------------------------ builders and lookups
def features(seed, c=24, h=3, w=39):
    return dict(left=rnd(1, c, h, w, seed=seed), right=rnd(1, c, h, w, seed=seed + 1))


@row("gwc volume", "dv_gwc_volume_f32")
def _gwc():
    return (lambda left, right: S.build_gwc_volume(left, right, 12, 8)), features(30), [["left"], ["right"]]


@row("concat volume", "dv_concat_volume_f32")
def _concat():
    return (lambda left, right: S.build_concat_volume(left, right, 6)), features(32, c=12), [["left", "right"]]


@row("concat volume zero_left", "dv_concat_volume_f32")
def _concat_zl():
    return (lambda left, right: S.build_concat_volume(left, right, 6, zero_left=True)), features(34, c=12), [["left", "right"]]


@row("concat attention volume", "dv_concat_attn_volume_f32")
def _concat_att():
    """The softmax is over the attention logits, which are not scaled."""
    att = rnd(1, 1, 6, 3, 39, seed=36)
    return (lambda left, right: S.build_concat_attention_volume(left, right, att, 6)), features(37, c=12), [["left", "right"]]


def patch_operands(seed):
    return dict(gwc=rnd(1, 6, 3, 5, 19, seed=seed), w1=rnd(6, 9, seed=seed + 1), w2=rnd(6, 9, seed=seed + 2))


@row("patch stencils", "dv_patch_volume_runs_f32")
def _patch():
    dil = torch.tensor([1, 1, 2, 2, 3, 3], dtype=torch.int32, device=DEV)
    return (lambda gwc, w1, w2: S.patch_volume(gwc, w1, w2, dil)), patch_operands(40), [["gwc"], ["w1"], ["w2"]]


@row("all-pairs correlation and its pooled level", "dv_allpairs_corr_f32")
def _corr():
    ops = dict(fmap1=rnd(1, 7, 2, 17, seed=43), fmap2=rnd(1, 7, 2, 33, seed=44))
    return Combined_Geo_Encoding_Volume._corr_levels, ops, [["fmap1"], ["fmap2"]]


def lookup_operands(seed, b=1, c=3, d=13, h=3, w=21):
    n = b * h * w
    disp = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * (d + 10) - 5).view(b, 1, h, w).to(DEV)
    coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous().to(DEV)
    return dict(geo=rnd(b, c, d, h, w, seed=seed + 1), fmap1=rnd(b, 6, h, w, seed=seed + 2), fmap2=rnd(b, 6, h, w, seed=seed + 3),
                disp=disp, coords=coords, noisy=rnd(b, d, h, w, seed=seed + 4))


@row("geometry lookup", "dv_geo_filter_lookup_f32")
def _lookup():
    """Jointly linear in (geo, fmap1) -- the correlation rows are bilinear in the two feature maps -- at fixed positions."""
    def fn(geo, fmap1, fmap2, disp, coords, noisy):
        return Combined_Geo_Encoding_Volume(fmap1, fmap2, geo)(disp, coords, noisy)
    return fn, lookup_operands(45), [["geo", "fmap1"], ["geo", "fmap2"]]


# ------------------------------------------------------------------ backward entries
def vjp(forward, wrt):
    """``fn(g, **operands)``: the gradients of ``forward(**operands)`` with respect to the operands ``wrt`` for the cotangent g."""
    def fn(g, **ops):
        leaves = {k: (v.detach().clone().requires_grad_(True) if k in wrt else v) for k, v in ops.items()}
        out = forward(**leaves)
        return torch.autograd.grad(out, [leaves[k] for k in wrt], g)
    return fn


@row("conv3d weight gradient", "dv_conv3d_wgrad_f32")
def _wgrad3d():
    fn = lambda x, g: train3d.conv3d_weight_grad(x, g, 3, 1, 7)
    return fn, dict(x=rnd(1, 5, 2, 3, 17, seed=50), g=rnd(1, 7, 2, 3, 17, seed=51)), [["x"], ["g"]]


@row("conv3d weight gradient stride 2", "dv_conv3d_wgrad_f32")
def _wgrad3d_s2():
    fn = lambda x, g: train3d.conv3d_weight_grad(x, g, 3, 2, 7)
    return fn, dict(x=rnd(1, 5, 4, 6, 18, seed=52), g=rnd(1, 7, 2, 3, 9, seed=53)), [["x"], ["g"]]


@row("conv2d weight gradient", "dv_conv2d_wgrad_f32")
def _wgrad2d():
    fn = lambda x, g: train2d.conv2d_weight_grad(x, g, 3, 1, 7)
    return fn, dict(x=rnd(2, 5, 6, 9, seed=54), g=rnd(2, 7, 6, 9, seed=55)), [["x"], ["g"]]


@row("conv2d weight gradient dilation 2", "dv_conv2d_wgrad_f32")
def _wgrad2d_d2():
    fn = lambda x, g: train2d.conv2d_weight_grad(x, g, 3, 2, 7)
    return fn, dict(x=rnd(2, 5, 9, 33, seed=56), g=rnd(2, 7, 9, 33, seed=57)), [["x"], ["g"]]


@row("deconv3d k4 weight gradient", "dv_deconv3d_k4s2_wgrad_f32")
def _wgrad_k4():
    return train3d.deconv3d_k4_weight_grad, dict(x=rnd(1, 6, 2, 3, 5, seed=58), g=rnd(1, 5, 4, 6, 10, seed=59)), [["x"], ["g"]]


@row("deconv3d k4 input gradient", "dv_deconv3d_k4s2_dgrad_f32")
def _dgrad_k4():
    return train3d.deconv3d_k4_input_grad, dict(g=rnd(1, 5, 4, 6, 10, seed=60), w=rnd(6, 5, 4, 4, 4, seed=61, scale=0.2)), [["g"], ["w"]]


@row("deconv2d k4 input and weight gradient", "dv_deconv2d_k4s2_wgrad_f32")
def _deconv2d_k4():
    """dx is linear in g; dW is bilinear in x and g (x does not reach dx)."""
    fwd = lambda x, w: train2d.conv_transpose2d_k4(x, w)
    return vjp(fwd, ["x", "w"]), dict(g=rnd(2, 5, 10, 18, seed=62), x=rnd(2, 6, 5, 9, seed=63), w=rnd(6, 5, 4, 4, seed=64, scale=0.2)), [["g"]]


@row("feature gate backward", "dv_feature_gate_bwd_f32")
def _gate():
    """(dcv, dlogit): both linear in g; the logit passes through a sigmoid and is left alone."""
    ops = dict(cv=rnd(1, 6, 3, 5, 9, seed=65), logit=rnd(1, 6, 5, 9, seed=66), g=rnd(1, 6, 3, 5, 9, seed=67))
    return train3d.feature_gate_grads, ops, [["g"]]


@row("bilinear resize backward", "dv_resize_bilinear_ac_bwd_f32")
def _resize():
    fwd = lambda x: train_net2d.resize_bilinear_train(x, (11, 23))
    return vjp(fwd, ["x"]), dict(g=rnd(2, 3, 11, 23, seed=68), x=rnd(2, 3, 5, 9, seed=69)), [["g"]]


@row("convex upsampling backward", "dv_context_upsample_bwd_f32")
def _context():
    fwd = lambda disp, weights: context_upsample(disp, weights, scale=4.0, apply_softmax=True)
    ops = dict(g=rnd(1, 12, 28, seed=70), disp=rnd(1, 1, 3, 7, seed=71), weights=rnd(1, 9, 12, 28, seed=72))
    return vjp(fwd, ["disp", "weights"]), ops, [["g"]]


@row("geometry lookup backward", "dv_geo_filter_lookup_bwd_f32")
def _lookup_bwd():
    """(dgeo, dfmap1, dfmap2) for a cotangent g: dv_geo_filter_lookup_bwd_f32, and dv_allpairs_corr_bwd_f32 behind it."""
    def fwd(geo, fmap1, fmap2, disp, coords, noisy):
        return Combined_Geo_Encoding_Volume(fmap1, fmap2, geo)(disp, coords, noisy)
    ops = lookup_operands(73)
    return vjp(fwd, ["geo", "fmap1", "fmap2"]), dict(ops, g=rnd(1, 2 * (9 * 3 + 9), 3, 21, seed=78)), [["g"]]


@row("gwc volume backward", "dv_gwc_volume_bwd_f32")
def _gwc_bwd():
    """(dref, dtgt): linear in dvol, and each linear in the other feature map."""
    fn = lambda left, right, dvol: train_volume.gwc_volume_grad(left, right, dvol, 8)
    return fn, dict(features(79), dvol=rnd(1, 8, 12, 3, 39, seed=81)), [["dvol"]]


@row("concat volume backward", "dv_concat_volume_bwd_f32")
def _concat_bwd():
    """(dref, dtgt, dscale) with a scale [B,D,H,W]: all three linear in dvol."""
    fn = lambda left, right, scale, dvol: train_volume.concat_volume_grad(left, right, scale, dvol, want_scale=True)
    ops = dict(features(82, c=12), scale=rnd(1, 6, 3, 39, seed=84), dvol=rnd(1, 24, 6, 3, 39, seed=85))
    return fn, ops, [["dvol"]]


@row("patch stencils backward", "dv_patch_volume_bwd_f32")
def _patch_bwd():
    fwd = lambda gwc, w1, w2: train_patch.patch_volume_train(gwc, w1, w2, (1, 1, 2, 2, 3, 3))
    return vjp(fwd, ["gwc", "w1", "w2"]), dict(patch_operands(86), g=rnd(1, 6, 3, 5, 19, seed=89)), [["g"]]


@row("regression tail backward", "dv_upsample_softmax_regress_bwd_f32")
def _tail():
    fwd = lambda cost: train_tail.upsample_softmax_regress_train(cost)
    return vjp(fwd, ["cost"]), dict(g=rnd(2, 12, 16, seed=90), cost=rnd(2, 5, 3, 4, seed=91)), [["g"]]


@row("window attention backward", "dv_window_attn3d_bwd_f32")
def _attn():
    c = 128
    fwd = lambda x, qkv_w, qkv_b, proj_w, proj_b: train_attn.window_attention_train(x, qkv_w, qkv_b, proj_w, proj_b, 16)
    ops = dict(x=rnd(1, c, 4, 5, 6, seed=92), qkv_w=rnd(3 * c, c, seed=93, scale=c ** -0.5), qkv_b=rnd(3 * c, seed=94, scale=0.1),
               proj_w=rnd(c, c, seed=95, scale=c ** -0.5), proj_b=rnd(c, seed=96, scale=0.1), g=rnd(1, c, 4, 5, 6, seed=97))
    return vjp(fwd, ["x", "qkv_w", "qkv_b", "proj_w", "proj_b"]), ops, [["g"]]


@row("bn3d + skip backward", "dv_bn3d_act_bwd_f32")
def _bn3d():
    """(dx, dgamma, dbeta, dskip) of batch-statistics BatchNorm + skip, no activation: linear in dy."""
    fwd = lambda x, weight, bias, skip: train_norm.batch_norm_act_train(x, weight, bias, None, None, act="none", skip=skip)
    ops = dict(x=rnd(2, 5, 3, 4, 7, seed=98), weight=rnd(5, seed=99), bias=rnd(5, seed=100), skip=rnd(2, 5, 3, 4, 7, seed=101),
               g=rnd(2, 5, 3, 4, 7, seed=102))
    return vjp(fwd, ["x", "weight", "bias", "skip"]), ops, [["g"]]


@row("bn3d + relu backward", "dv_bn3d_act_bwd_f32")
def _bn3d_relu():
    """The ReLU's mask comes from the forward's operands, which are not scaled: the backward stays linear in dy."""
    fwd = lambda x, weight, bias: train_norm.batch_norm_act_train(x, weight, bias, None, None, act="relu")
    ops = dict(x=rnd(2, 5, 3, 4, 7, seed=103), weight=rnd(5, seed=104), bias=rnd(5, seed=105), g=rnd(2, 5, 3, 4, 7, seed=106))
    return vjp(fwd, ["x", "weight", "bias"]), ops, [["g"]]


def loss_operands(seed):
    mask = (torch.rand(2, 9, 21, generator=torch.Generator().manual_seed(seed)) < 0.7).to(torch.uint8).to(DEV)
    return dict(p0=rnd(2, 9, 21, seed=seed + 1), p1=rnd(2, 9, 21, seed=seed + 2), gt=rnd(2, 9, 21, seed=seed + 3)), mask


@row("masked L1 loss", "dv_masked_loss_fwd_f32", signed=False)
def _l1():
    """L1 is absolutely homogeneous in (pred, gt) together -- loss(-p, -gt) = loss(p, gt), so no sign flip; u8 mask."""
    ops, mask = loss_operands(107)
    fn = lambda p0, p1, gt: train_loss.masked_loss_train([p0, p1], gt, mask, [0.5, 1.0], kind="l1")
    return fn, ops, [["p0", "p1", "gt"]]


@row("masked L1 loss backward", "dv_masked_loss_bwd_f32")
def _l1_bwd():
    ops, mask = loss_operands(111)
    fwd = lambda p0, p1, gt: train_loss.masked_loss_train([p0, p1], gt, mask, [0.5, 1.0], kind="l1")
    return vjp(fwd, ["p0", "p1"]), dict(ops, g=rnd(1, seed=115).reshape(()).abs() + 0.5), [["g"]]


# ------------------------------------------------------------------ the 16-bit training entries, a = 2^+-4, no sign flip
MP = dict(alphas=(2.0 ** 4, 2.0 ** -4), signed=False)     # (the 16-bit matrix instruction is not sign-symmetric: module docstring)


def mp_rows(elem):
    conv = getattr(train3d, f"conv3d_k3s1_{elem}")
    wgrad = getattr(train3d, f"conv3d_weight_grad_{elem}")

    def clear(t):
        """Unit draws kept away from zero: scaled by 2^-4 every rounded operand is still an fp16 normal."""
        return torch.where(t.abs() < 2.0 ** -6, torch.full_like(t, 2.0 ** -6).copysign(t), t)

    @row(f"conv3d k3s1 {elem}", f"dv_conv3d_k3s1_{elem}_f32", **MP)
    def _fwd():
        return (lambda x, w: conv(x, w)), dict(x=clear(rnd(1, 9, 3, 5, 49, seed=120)), w=clear(rnd(16, 9, 3, 3, 3, seed=121))), [["x"], ["w"]]

    @row(f"conv3d k3s1 {elem} transpose_flip", f"dv_conv3d_k3s1_{elem}_f32", **MP)
    def _dgrad():
        ops = dict(x=clear(rnd(1, 9, 3, 5, 49, seed=122)), w=clear(rnd(9, 16, 3, 3, 3, seed=123)))
        return (lambda x, w: conv(x, w, transpose_flip=True)), ops, [["x"], ["w"]]

    @row(f"conv3d weight gradient {elem}", f"dv_conv3d_wgrad_{elem}_f32", **MP)
    def _wgrad():
        return wgrad, dict(x=clear(rnd(1, 9, 3, 5, 49, seed=124)), g=clear(rnd(1, 16, 3, 5, 49, seed=125))), [["x"], ["g"]]


mp_rows("f16")
mp_rows("bf16")


@row("conv2d cat weight gradient f16", "dv_conv2d_wgrad_cat_f16", **MP)
def _wgrad_cat16():
    clear = lambda t: torch.where(t.abs() < 2.0 ** -6, torch.full_like(t, 2.0 ** -6).copysign(t), t)
    fn = lambda a, b, g: train2d.conv2d_cat_weight_grad([a, b], g, 3, f16=True)
    ops = dict(a=clear(rnd(3, 16, 2, 3, seed=126)), b=clear(rnd(3, 8, 2, 3, seed=127)), g=clear(rnd(3, 24, 2, 3, seed=128)))
    return fn, ops, [["a", "b"], ["g"]]


@pytest.mark.parametrize("elem", ["f16", "bf16"])
def test_the_sign_flip_of_the_16_bit_entries_stays_within_twice_their_bar(elem):
    """What replaces the bit-for-bit sign flip for the 16-bit rows.  op(x) and op(-x) are each within the sibling bar
    c * 2^-24 * sum |operands| of the same float64 reference up to its sign, so |op(-x) + op(x)| <= 2 c 2^-24 sum |operands|
    (triangle inequality; c and the sum from the sibling files, nothing new).  Measured: fp16 forward 2.8 % of the elements
    differ, the worst at 1.18 of the 2 c = 896 allowed; fp16 weight gradient 9.1 %, 0.27 of 280; bf16 forward 0.4 %, 0.46 of
    896; bf16 weight gradient 0.7 %, 0.21 of 280.  (In units of the element's own last place the difference reaches 256
    where the sum cancels: it is a unit of the summands' scale, not of the result's.)"""
    import test_gpu_conv3d_bf16 as CB16
    import test_gpu_conv3d_f16 as C16
    import test_gpu_conv3d_wgrad_bf16 as WB16
    import test_gpu_conv3d_wgrad_f16 as W16
    conv_mod, wgrad_mod = (C16, W16) if elem == "f16" else (CB16, WB16)
    conv, wgrad = getattr(train3d, f"conv3d_k3s1_{elem}"), getattr(train3d, f"conv3d_weight_grad_{elem}")
    b, cin, cout, d, h, w = 1, 9, 16, 3, 5, 49
    x, wt, g = rnd(b, cin, d, h, w, seed=130), rnd(cout, cin, 3, 3, 3, seed=131), rnd(b, cout, d, h, w, seed=132)
    rd = (lambda t: t.half().double()) if elem == "f16" else (lambda t: t.bfloat16().double())
    cases = [("forward", conv(x, wt), conv(-x, wt), conv_mod.reference(x.cpu(), wt.cpu())[1], conv_mod.depth_c(cin)),
             ("weight gradient", wgrad(x, g), wgrad(-x, g), W16.ref_wgrad(rd(x.cpu()).abs(), rd(g.cpu()).abs()),
              wgrad_mod.depth_c(b, cin, d, h, w, cout))]
    for what, pos, neg, mag, c in cases:
        diff = (pos.cpu().double() + neg.cpu().double()).abs()
        ulp = torch.exp2(torch.floor(torch.log2(pos.cpu().double().abs().clamp_min(1e-30))) - 23)
        print(f"SIGNFLIP {elem} {what}: {float((diff > 0).double().mean()):.4f} of the elements differ, by at most "
              f"{float((diff / ulp).max()):.1f} ulp; worst {float((diff / (C16.U * mag)).max()):.2f} of 2 c = {2 * c}")
        assert torch.all(diff <= 2 * c * C16.U * mag)
