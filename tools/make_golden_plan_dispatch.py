#!/usr/bin/env python
"""Record which kernel every inference plan and every reference-named operation dispatches to, and the bits it produces:
tests/golden/plan_dispatch.json, replayed by tests/test_gpu_plan_dispatch.py.

    python tools/make_golden_plan_dispatch.py [out.json]        # on the MI355X

For each case: weights and inputs drawn on the CPU from a seed derived from the case's name, a recorder in
``KernelTimer.active`` (tag, flops, bytes, issued, valu of every timed launch), the name of every entry launched (timed or
not, the weight packing included), the SHA-256 of every output and of every packed weight image the plan holds.  Two
recordings of one commit must agree (the kernels sum in a fixed order); the fixture is rewritten only by a change that
means to alter a route, a tag or a kernel's arithmetic, and says so.

Every case names the branches it takes; ``BRANCHES`` gives the entry (and tag pattern) that proves a branch was taken, so a
shape that drifts to another route fails by name.  The shapes are the smallest that take each branch, chosen with the
library's own host queries (the ``*_auto_kslices`` / ``*_supported`` entries and the WINO_MIN_BLOCKS count).  Every plan and
operation is reached through ``diffuvolume_amd.submodule``, the public home of these names.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import re
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from diffuvolume_amd import submodule as S  # noqa: E402
from diffuvolume_amd.profiling import KernelTimer  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "plan_dispatch.json"
DEV = "cuda"

# branch -> (entry that must be launched, regex the launch's tag must match; None: the entry is untimed / any tag)
BRANCHES = {
    "conv3d.f16x3": ("dv_conv3d_f16x3_f32", r"conv3d_f16x3_co\d+$"),
    "conv3d.f16x3_in_scale": ("dv_conv3d_f16x3_f32", r"conv3d_f16x3_co\d+_filter$"),
    "conv3d.wino3": ("dv_conv3d_wino3_f32", r"conv3d_k3s1_co\d+$"),
    "conv3d.wino": ("dv_conv3d_wino_f32", r"conv3d_k3s1_co\d+$"),
    "conv3d.wino_in_scale": ("dv_conv3d_wino_f32", r"conv3d_k3s1_co\d+_filter$"),
    "conv3d.s2pp": ("dv_conv3d_s2pp_f32", r"conv3d_k3s2_co\d+$"),
    "conv3d.s2_in_scale": ("dv_conv3d_f32", r"conv3d_k3s2_co\d+_filter$"),
    "conv3d.k1": ("dv_conv3d_f32", r"conv3d_k1s1_co\d+$"),
    "conv3d.head": ("dv_conv3d_f32", r"conv3d_k3s1_co1$"),
    "conv3d.f32_direct": ("dv_conv3d_f32", r"conv3d_k3s1_co\d+$"),
    "conv3d.residual": (None, None),
    "conv2d.s2_k1": ("dv_conv2d_s2_f32", r"conv2d_k1s2_co\d+$"),
    "conv2d.s2_k3": ("dv_conv2d_s2_f32", r"conv2d_k3s2_co\d+$"),
    "conv2d.s2b_out": ("dv_conv2d_wino_s2b_f32", r"conv2d_k3d1_co\d+_s2b$"),
    "conv2d.wino_ksplit": ("dv_conv2d_wino_cat_ksplit_f32", r"conv2d_k3d1_co\d+_wksplit$"),
    "conv2d.wino_d1": ("dv_conv2d_wino_dil_cat_f32", r"conv2d_k3d1_co\d+$"),
    "conv2d.wino_d2": ("dv_conv2d_wino_dil_cat_f32", r"conv2d_k3d2_co\d+$"),
    "conv2d.direct_ksplit": ("dv_conv2d_cat_ksplit_f32", r"conv2d_k3d1_co\d+_ksplit$"),
    "conv2d.direct_cat": ("dv_conv2d_cat_f32", r"conv2d_k\dd1_co\d+$"),
    "conv2d.gated": ("dv_conv2d_gated_f32", r"conv2d_k\dd1_co\d+$"),
    "conv2d.residual": (None, None), "conv2d.mul": (None, None), "conv2d.blend": (None, None),
    "conv2d.parts2": (None, None), "conv2d.parts4": (None, None),
    "conv2d.group": ("dv_conv2d_wino_dil_cat_f32", r"conv2d_k3d1_co\d+$"),
    "pair.pair": ("dv_conv2d_wino_cat_pair_f32", r"conv2d_k3d1_co\d+\+\d+$"),
    "pair.ksplit": ("dv_conv2d_wino_cat_pair_ksplit_f32", r"conv2d_k3d1_co\d+\+\d+_ksplit$"),
    "pair.singles": ("dv_conv2d_cat_f32", r"conv2d_k3d1_co\d+$"),
    "f16.single": ("dv_conv2d_f16_cat", r"conv2d_f16_k\d_co\d+$"),
    "f16.single_ksplit": ("dv_conv2d_f16_cat_ksplit", r"conv2d_f16_k3_co\d+_ksplit$"),
    "f16.pair": ("dv_conv2d_f16_cat_pair", r"conv2d_f16_k3_co\d+\+\d+$"),
    "f16.pair_ksplit": ("dv_conv2d_f16_cat_pair_ksplit", r"conv2d_f16_k3_co\d+\+\d+_ksplit$"),
    "f16.blend": (None, None),
    "deconv3d.k3": ("dv_deconv3d_k3s2_f32", r"deconv3d_k3s2$"),
    "deconv3d.k4": ("dv_deconv3d_k4s2_f32", r"deconv3d_k4s2$"),
    "deconv3d.redir": ("dv_deconv3d_k3s2_redir_f32", r"deconv3d_k3s2_redir$"),
    "deconv3d.redir_fallback": ("dv_conv3d_f32", r"conv3d_k1s1_co\d+$"),
    "deconv3d.residual": (None, None),
    "deconv2d_k4s2": ("dv_conv2d_gated_f32", r"conv2d_k3d1_co\d+$"),
    "pointwise_expand": ("dv_pointwise_expand_f32", r"pointwise_expand_co\d+$"),
    "rank1.noise": ("dv_mul_f32", None),
    "rank1.plain": ("dv_conv3d_rank1_filter_f32", r"conv3d_k3s1_co\d+_filter_rank1$"),
    "gwc_volume": ("dv_gwc_volume_f32", r"gwc_volume$"),
    "concat_volume": ("dv_concat_volume_f32", None),
    "empty_volume": (None, None),
    "attn_volume.tensor": ("dv_concat_attn_volume_f32", r"concat_attn_volume$"),
    "attn_volume.lazy": ("dv_concat_prob_volume_f32", r"concat_attn_volume$"),
    "disparity_regression": ("dv_disparity_regression_f32", None),
    "upsample_softmax_regress": ("dv_upsample_softmax_regress_f32", r"upsample_softmax_regress$"),
    "softmax_regress": ("dv_softmax_regress_f32", r"softmax_regress$"),
    "feature_gate": ("dv_feature_gate_f32", r"feature_gate$"),
    "refine_inputs": ("dv_refine_inputs_f32", r"refine_inputs$"),
    "patch_volume": ("dv_patch_volume_runs_f32", r"patch_volume$"),
    "window_attention": ("dv_window_attn3d_f32", r"window_attn3d$"),
}

CASES = {}       # name -> (branches, fn(rnd) -> (outputs, plans))


def case(*branches):
    def add(fn):
        CASES[fn.__name__] = (branches, fn)
        return fn
    return add


def _rnd(name):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).to(DEV)


def _w(rnd, cout, cin, *k):
    fan = cin
    for n in k:
        fan *= n
    return rnd(cout, cin, *k, scale=fan ** -0.5)


def _bn(rnd, c):
    return (rnd(c).abs() + 0.5, rnd(c, scale=0.1), rnd(c, scale=0.1), rnd(c).abs() + 0.5)


# ------------------------------------------------------------------------------------------------ Conv3dPlan
def _conv3d(rnd, cin, cout, dims, k=3, stride=1, precision="f32", in_scale=False, residual=False, act=S.ACT_RELU):
    plan = S.Conv3dPlan(_w(rnd, cout, cin, k, k, k), _bn(rnd, cout), stride=stride, act=act, precision=precision)
    x = rnd(dims[0], cin, *dims[1:])
    kw = {}
    if in_scale:
        kw["in_scale"] = rnd(*dims).abs()
    if residual:
        kw["residual"] = rnd(*plan.out_shape(x.shape))
    return [plan(x, **kw)], [plan]


@case("conv3d.f16x3")
def conv3d_f16x3(rnd):
    return _conv3d(rnd, 32, 16, (1, 3, 9, 30), precision="f16x3")


@case("conv3d.f16x3_in_scale", "conv3d.residual")
def conv3d_f16x3_in_scale(rnd):
    return _conv3d(rnd, 32, 16, (1, 3, 9, 30), precision="f16x3", in_scale=True, residual=True)


@case("conv3d.wino3", "conv3d.residual")
def conv3d_wino3(rnd):
    return _conv3d(rnd, 64, 32, (1, 2, 4, 8), residual=True)


@case("conv3d.wino")
def conv3d_wino(rnd):
    return _conv3d(rnd, 16, 32, (2, 3, 5, 10))


@case("conv3d.wino_in_scale")
def conv3d_wino_in_scale(rnd):          # a layer the F(2x2x2) kernel would take: the filter prologue keeps it in-plane
    return _conv3d(rnd, 64, 32, (1, 2, 4, 8), in_scale=True)


@case("conv3d.s2pp")
def conv3d_s2pp(rnd):
    return _conv3d(rnd, 8, 64, (1, 4, 6, 12), stride=2, act=S.ACT_NONE)


@case("conv3d.s2_in_scale")
def conv3d_s2_in_scale(rnd):
    return _conv3d(rnd, 8, 64, (1, 4, 6, 12), stride=2, in_scale=True)


@case("conv3d.k1")
def conv3d_k1(rnd):
    return _conv3d(rnd, 16, 8, (1, 3, 5, 7), k=1, act=S.ACT_MISH)


@case("conv3d.head")
def conv3d_head(rnd):
    return _conv3d(rnd, 16, 1, (1, 3, 5, 7), act=S.ACT_NONE)


@case("conv3d.f32_direct", "conv3d.residual")
def conv3d_f32_direct(rnd):
    return _conv3d(rnd, 16, 32, (1, 3, 5, 10), precision="f32_direct", residual=True)


# ------------------------------------------------------------------------------------------------ Conv2dPlan
def _conv2d(rnd, chans, cout, hw, k=3, dilation=1, stride=1, b=1, residual=False, mul=False, blend=False, act=S.ACT_RELU, **kw):
    cin = sum(chans) if isinstance(chans, tuple) else chans
    plan = S.Conv2dPlan(_w(rnd, cout, cin, k, k), _bn(rnd, cout), dilation=dilation, act=act, stride=stride)
    x = [rnd(b, c, *hw) for c in chans] if isinstance(chans, tuple) else rnd(b, cin, *hw)
    oshape = (b, cout, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1)
    if residual:
        kw["residual"] = rnd(*oshape)
    if mul:
        kw["mul"] = rnd(*oshape)
    if blend:
        kw["blend"] = (torch.sigmoid(rnd(*oshape)), rnd(*oshape))
    return [plan(x, **kw)], [plan]


@case("conv2d.s2_k1")
def conv2d_s2_k1(rnd):
    return _conv2d(rnd, 8, 16, (9, 13), k=1, stride=2)


@case("conv2d.s2_k3", "conv2d.residual")
def conv2d_s2_k3(rnd):
    return _conv2d(rnd, 8, 16, (9, 13), stride=2, residual=True)


@case("conv2d.s2b_out", "conv2d.parts2")
def conv2d_s2b_out(rnd):
    return _conv2d(rnd, (3, 5), 32, (8, 12), s2b_out=True)


@case("conv2d.wino_ksplit", "conv2d.residual", "conv2d.mul")
def conv2d_wino_ksplit(rnd):
    return _conv2d(rnd, 128, 128, (33, 47), residual=True, mul=True, act=S.ACT_SIGMOID)


@case("conv2d.wino_d1", "conv2d.parts4", "conv2d.blend")
def conv2d_wino_d1(rnd):
    return _conv2d(rnd, (1, 2, 2, 3), 128, (33, 47), blend=True, act=S.ACT_TANH)


@case("conv2d.wino_d2")
def conv2d_wino_d2(rnd):
    return _conv2d(rnd, 8, 128, (33, 47), dilation=2)


@case("conv2d.group")
def conv2d_group(rnd):                  # 4 blocks per batch entry: only the group of 8 reaches WINO_MIN_BLOCKS
    return _conv2d(rnd, 8, 128, (16, 16), b=8, group=8)


@case("conv2d.direct_ksplit", "conv2d.residual")
def conv2d_direct_ksplit(rnd):
    return _conv2d(rnd, 64, 32, (8, 12), residual=True)


@case("conv2d.direct_cat", "conv2d.parts2", "conv2d.mul")
def conv2d_direct_cat(rnd):
    return _conv2d(rnd, (3, 5), 32, (9, 13), b=2, mul=True)


@case("conv2d.direct_cat", "conv2d.parts4")
def conv2d_direct_cat4(rnd):
    return _conv2d(rnd, (1, 2, 2, 3), 32, (9, 13), k=1)


@case("conv2d.gated", "conv2d.residual", "conv2d.mul", "conv2d.blend")
def conv2d_gated(rnd):
    return _conv2d(rnd, 8, 32, (9, 13), b=2, residual=True, mul=True, blend=True, act=S.ACT_TANH)


@case("conv2d.gated")
def conv2d_gated_k1(rnd):
    return _conv2d(rnd, 8, 32, (9, 13), k=1, act=S.ACT_LEAKY)


# ------------------------------------------------------------------------------------------------ the pair plans
def _pair(rnd, cin, hw, c=64):
    plan = S.Conv2dPairPlan((_w(rnd, c, cin, 3, 3), rnd(c, scale=0.1)), (_w(rnd, c, cin, 3, 3), rnd(c, scale=0.1)), act=S.ACT_SIGMOID)
    x = [rnd(1, cin - 3, *hw), rnd(1, 3, *hw)]
    o = (1, c, *hw)
    return list(plan(x, residual=(rnd(*o), None), mul=(None, rnd(*o)))), [plan]


@case("pair.pair")
def pair_pair(rnd):
    return _pair(rnd, 8, (33, 47))


@case("pair.ksplit")
def pair_ksplit(rnd):
    return _pair(rnd, 128, (33, 47))


@case("pair.singles")
def pair_singles(rnd):
    return _pair(rnd, 8, (8, 12))


def _f16(rnd, cin, pair, blend=False, k=3, hw=(8, 12), c=64):
    plan = S.Conv2dF16Plan(_w(rnd, c, cin, k, k), rnd(c, scale=0.1), act=S.ACT_TANH if blend else S.ACT_SIGMOID,
                           pair=(_w(rnd, c, cin, k, k), rnd(c, scale=0.1)) if pair else None)
    x = [rnd(2, cin - 8, *hw).half().float(), rnd(2, 8, *hw).half().float()]
    o = (2, c, *hw)
    if pair:
        return list(plan(x, residual=(rnd(*o).half().float(), None), mul=(None, rnd(*o).half().float()))), [plan]
    kw = dict(blend=(torch.sigmoid(rnd(*o)).half().float(), rnd(*o).half().float())) if blend else dict(mul=rnd(*o).half().float())
    return [plan(x, residual=rnd(*o).half().float(), **kw)], [plan]


@case("f16.single")
def f16_single(rnd):
    return _f16(rnd, 64, False)


@case("f16.single")
def f16_single_k1(rnd):
    return _f16(rnd, 64, False, k=1)


@case("f16.single_ksplit", "f16.blend")
def f16_single_ksplit(rnd):
    return _f16(rnd, 128, False, blend=True)


@case("f16.pair")
def f16_pair(rnd):
    return _f16(rnd, 64, True)


@case("f16.pair_ksplit")
def f16_pair_ksplit(rnd):
    return _f16(rnd, 128, True)


# ------------------------------------------------------------------------------------------------ transposed / small plans
def _deconv3d(rnd, k, dims, cin=16, cout=8, redir=None, residual=False):
    kw = {}
    if redir is not None:
        kw["redir"] = (_w(rnd, cout, redir, 1, 1, 1), _bn(rnd, cout))
    plan = S.Deconv3dPlan(rnd(cin, cout, k, k, k, scale=(cin * k ** 3 / 8) ** -0.5), _bn(rnd, cout), act=S.ACT_RELU, **kw)
    x = rnd(dims[0], cin, *dims[1:])
    o = (dims[0], cout, 2 * dims[1], 2 * dims[2], 2 * dims[3])
    call = {}
    if redir is not None:
        call["skip"] = rnd(o[0], redir, *o[2:])
    if residual:
        call["residual"] = rnd(*o)
    return [plan(x, **call)], [plan]


@case("deconv3d.k3")
def deconv3d_k3(rnd):
    return _deconv3d(rnd, 3, (1, 2, 3, 5))


@case("deconv3d.k4", "deconv3d.residual")
def deconv3d_k4(rnd):
    return _deconv3d(rnd, 4, (1, 2, 3, 5), residual=True)


@case("deconv3d.redir")
def deconv3d_redir(rnd):
    return _deconv3d(rnd, 3, (1, 2, 3, 4), redir=8)


@case("deconv3d.redir_fallback", "deconv3d.k3")
def deconv3d_redir_fallback(rnd):
    return _deconv3d(rnd, 3, (1, 2, 3, 5), redir=8)


@case("deconv2d_k4s2")
def deconv2d_k4s2(rnd):
    plan = S.Deconv2dK4S2Plan(rnd(8, 4, 4, 4, scale=0.2), _bn(rnd, 4), bias=rnd(4, scale=0.1), act=S.ACT_LEAKY)
    return [plan(rnd(1, 8, 5, 7))], [plan]


@case("pointwise_expand")
def pointwise_expand(rnd):
    plan = S.PointwiseExpandPlan(_w(rnd, 54, 8, 1, 1))
    return [plan(rnd(2, 8, 5, 7))], [plan]


def _rank1(rnd, noise):
    b, c, d, h, w, cout = 1, 8, 12, 4, 9, 6
    vol = S.build_concat_attention_volume(rnd(b, c, h, w), rnd(b, c, h, w), rnd(b, 1, d, h, w), d, lazy=True)
    plan = S.Rank1FilterPlan(_w(rnd, cout, 2 * c, 3, 3, 3), _bn(rnd, cout))
    assert plan.applies(vol)
    return [plan(vol, torch.sigmoid(rnd(b, d, h, w)) if noise else None)], [plan]


@case("rank1.noise", "pointwise_expand")
def rank1_noise(rnd):
    return _rank1(rnd, True)


@case("rank1.plain")
def rank1_plain(rnd):
    return _rank1(rnd, False)


# ------------------------------------------------------------------------------------------------ module functions
@case("gwc_volume")
def gwc_volume(rnd):
    return [S.build_gwc_volume(rnd(2, 8, 5, 12), rnd(2, 8, 5, 12), 4, 2)], []


@case("concat_volume")
def concat_volume(rnd):
    l, r = rnd(2, 3, 5, 12), rnd(2, 3, 5, 12)
    return [S.build_concat_volume(l, r, 4), S.build_concat_volume(l, r, 4, zero_left=True)], []


@case("empty_volume")
def empty_volume(rnd):
    e = torch.empty((0, 8, 5, 12), device=DEV)
    att = torch.empty((0, 1, 4, 5, 12), device=DEV)
    return [S.build_gwc_volume(e, e, 4, 2), S.build_concat_volume(e, e, 4), S.build_concat_attention_volume(e, e, att, 4),
            S.disparity_regression(torch.empty((0, 4, 5, 12), device=DEV), 4)], []


@case("attn_volume.tensor", "attn_volume.lazy")
def attn_volume(rnd):
    l, r, att = rnd(2, 3, 5, 12), rnd(2, 3, 5, 12), rnd(2, 1, 4, 5, 12)
    lazy = S.build_concat_attention_volume(l, r, att, 4, lazy=True)
    return [S.build_concat_attention_volume(l, r, att, 4), lazy.p_att, lazy.tensor()], []


@case("disparity_regression")
def disparity_regression(rnd):
    p = torch.softmax(rnd(2, 6, 5, 7), 1)
    return [S.disparity_regression(p, 6), S.disparity_regression(p, 6, keepdim=True)], []


@case("upsample_softmax_regress")
def upsample_softmax_regress(rnd):
    cost = rnd(2, 1, 6, 5, 7)
    d1, u1 = S.upsample_softmax_regress(cost)
    d2, u2 = S.upsample_softmax_regress(cost[:, 0], want_uncertainty=False, align_corners=True)
    assert u2 is None
    return [d1, u1, d2], []


@case("softmax_regress")
def softmax_regress(rnd):
    return [S.softmax_regress(rnd(2, 1, 6, 5, 7))], []


@case("feature_gate")
def feature_gate(rnd):
    cv, logit = rnd(2, 4, 3, 5, 6), rnd(2, 4, 5, 6)
    out = S.feature_gate(cv, logit)
    return [out, S.feature_gate(cv.clone(), logit, inplace=True)], []


@case("refine_inputs")
def refine_inputs(rnd):
    b, c, h, w = 2, 3, 3, 25
    return [S.refine_inputs(rnd(b, c, h, w), rnd(b, c, h, w), rnd(b, 1, h, w).abs() * 10, rnd(c), rnd(c))], []


@case("patch_volume")
def patch_volume(rnd):
    g = 5
    dil = torch.tensor([1, 2, 2, 3, 1], dtype=torch.int32, device=DEV)
    return [S.patch_volume(rnd(2, g, 2, 18, 20), rnd(g, 9, scale=1 / 3), rnd(g, 9, scale=1 / 3), dil)], []


@case("window_attention")
def window_attention(rnd):
    c = 128
    return [S.window_attention(rnd(2, c, 4, 5, 7), _w(rnd, 3 * c, c, 1, 1, 1), rnd(3 * c, scale=0.1), _w(rnd, c, c, 1, 1, 1),
                               rnd(c, scale=0.1), heads=16)], []


# ------------------------------------------------------------------------------------------------ recording
class _Timer:
    """What KernelTimer.active has to be: launch() runs the call and keeps the five figures."""

    def __init__(self):
        self.rows = []

    def launch(self, tag, flops, nbytes, fn, issued=0.0, valu=0.0):
        fn()
        self.rows.append([tag, float(flops), float(nbytes), float(issued), float(valu)])


class _Spy:
    """The loaded library with the name of every launched entry (int result, stream last) appended to ``log``."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dv_") or fn.restype is not ctypes.c_int or not fn.argtypes or fn.argtypes[-1] is not ctypes.c_void_p:
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def sha(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    head = f"{t.dtype}{tuple(t.shape)}".encode()
    return hashlib.sha256(head + t.view(torch.uint8).numpy().tobytes() if t.numel() else head).hexdigest()


def images(plan, prefix="") -> dict:
    """SHA-256 of every tensor a plan holds (packed weights, folded scale / shift), the plans inside it included."""
    out = {}
    for key, v in sorted(vars(plan).items()):
        for i, item in enumerate(v if isinstance(v, tuple) else (v,)):
            name = f"{prefix}{key}" + (f"[{i}]" if isinstance(v, tuple) else "")
            if isinstance(item, torch.Tensor):
                out[name] = sha(item)
            elif type(item).__name__.endswith("Plan"):
                out.update(images(item, name + "."))
    return out


def run_case(name: str) -> dict:
    """Run one case under the recorders -> what the fixture keeps of it."""
    branches, fn = CASES[name]
    lib_mod = S._lib
    real, timer, entries = lib_mod.load(), _Timer(), []
    before = KernelTimer.active
    S.set_default_conv_precision("f32")
    lib_mod._lib, KernelTimer.active = _Spy(real, entries), timer
    try:
        with torch.no_grad():
            outs, plans = fn(_rnd(name))
        torch.cuda.synchronize()
    finally:
        lib_mod._lib, KernelTimer.active = real, before
        S.set_default_conv_precision(None)
    return {"branches": list(branches), "entries": entries, "timed": timer.rows, "outputs": [sha(t) for t in outs],
            "images": [images(p) for p in plans]}


def took(rec: dict, branch: str) -> bool:
    """Whether a recording shows the entry and the tag that ``branch`` stands for."""
    entry, tag = BRANCHES[branch]
    return (entry is None or entry in rec["entries"]) and (tag is None or any(re.match(tag, row[0]) for row in rec["timed"]))


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    recs = {name: run_case(name) for name in CASES}
    for name, rec in recs.items():
        for b in rec["branches"]:
            assert took(rec, b), (name, b, rec["entries"], [r[0] for r in rec["timed"]])
    missing = set(BRANCHES) - {b for rec in recs.values() for b in rec["branches"]}
    assert not missing, missing
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps({"cases": recs}, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out}: {len(recs)} cases, {sum(len(r['timed']) for r in recs.values())} timed launches")


if __name__ == "__main__":
    main()
