"""The pointer and bounds contract of the C ABI (include/diffuvolume_hip.h), entry point by entry point.

Every inference entry that launches a kernel and writes a caller-owned tensor is a row of ``TABLE``, and so are the training
entries that choose a path or refuse by alignment and the eight split-K weight-gradient entries, whose ``workspace`` is an
output operand of exactly the size their ``*_workspace_floats`` entry reports: every word of it written, none next to it
(the other training entries name their own offset-view test in tests/test_abi_arena_complete.py).  A row builds its
operands on the CPU, states the float64 reference as the existing test of that entry states it, and copies that test's
bar (``cite`` names the test).  Each row then runs, with EVERY operand inside a guard-banded arena (tests/arena.py):

  (a)  all operands 16-byte aligned;
  (b)  each pointer operand of the entry's alignment predicate displaced alone by one float;
  (o)  every OTHER tensor operand displaced alone by one float: an operand a predicate forgot looks exactly like these;
  (c)  all tensor operands displaced together by 1, 2 and 3 floats (float64 operands by as many doubles).

Packed weights stay aligned in (b) and (c); where the entry checks them, a displaced ``wpacked`` is a case of its own.  An
accepted call returns 0, leaves every guard word alone, writes every output element, lets no NaN of an input's guard
band reach a result, and meets the row's bar.  A documented refusal returns exactly the code of the source and leaves the
output arenas untouched (nothing was launched); an operand that makes (c) a refusal stays aligned in a second pass so
that the displaced forms of the other operands still run.
"""
import ctypes
import math

import pytest
import torch

import arena as A
from diffuvolume_amd import _lib
from diffuvolume_amd import submodule as S
from oracle import acv_oracle as O
from oracle import igev_oracle as IO
from oracle import pcw_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional

OK, ERR_UNSUPPORTED, ERR_ALIGN = 0, -3, -4


def G(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def act64(y, act):
    return {S.ACT_NONE: lambda t: t, S.ACT_RELU: torch.relu, S.ACT_MISH: lambda t: t * torch.tanh(F.softplus(t)),
            S.ACT_LEAKY: lambda t: F.leaky_relu(t, 0.01), S.ACT_SIGMOID: torch.sigmoid, S.ACT_TANH: torch.tanh}[act](y)


# ------------------------------------------------------------------ bars (each one copied from the test a row cites)
def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp(min=1e-30))


def bar_rel(limit):
    def check(name, got, ref):
        e = rel_err(got, ref)
        print(f"    {name}: rel_err {e:.2e} (bar {limit:.0e})")
        assert e < limit, (name, e, limit)
    return check


def bar_close(atol, rtol):
    def check(name, got, ref):
        print(f"    {name}: max abs err {float((got.double() - ref.double()).abs().max()):.2e} (atol {atol:.0e}, rtol {rtol:.0e})")
        torch.testing.assert_close(got.double(), ref.double(), atol=atol, rtol=rtol)
    return check


def bar_scaled(factor):
    """|got - ref| <= factor * max(1, max|ref|)."""
    def check(name, got, ref):
        e, lim = float((got.double() - ref.double()).abs().max()), factor * max(1.0, float(ref.abs().max()))
        print(f"    {name}: max abs err {e:.2e} (bar {lim:.2e})")
        assert e <= lim, (name, e, lim)
    return check


def bar_equal(name, got, ref):
    assert torch.equal(got, ref.to(got.dtype)), f"{name}: not bit-equal to the reference"


# ------------------------------------------------------------------ the harness
class Case:
    """inputs / inout: name -> CPU tensor; outs: name -> CPU tensor giving shape and dtype; ``call(lib, p, s)`` makes the
    ABI call with ``p(name)`` the operand's device pointer (None when the row has no such operand); ``ref``: name ->
    float64 reference of every output (and of the in/out operands a bar is wanted for); ``pack(lib)``: name -> CPU tensor
    of weights packed through the ABI (needs the GPU, so it is kept apart from the CPU part of the row)."""

    def __init__(self, inputs, outs, call, ref, bar, inout=None, pack=None, before=None, after=None):
        self.inputs, self.outs, self.call, self.ref, self.bar = inputs, outs, call, ref, bar
        self.inout, self.pack, self.before, self.after = inout or {}, pack, before, after
        self.packed = False


class Row:
    """pred: the pointer operands of the entry's alignment predicate (variant b); aligned: operands that never move;
    refuse: name -> (return code, byte alignment the entry demands); same_bits: pairs of variants whose outputs the
    source promises to be bit-equal."""

    def __init__(self, name, entry, build, cite, pred=(), aligned=(), refuse=None, variants="abc", same_bits=()):
        self.name, self.entry, self.build, self.cite = name, entry, build, cite
        self.pred, self.aligned, self.refuse, self.variants, self.same_bits = pred, set(aligned), refuse or {}, variants, same_bits

    def __repr__(self):
        return self.name


def pack_through_abi(lib, sizer, packer, w, *dims, words_per=1):
    """The entry's own packer on the GPU; returned on the CPU as int32 words so that it can be placed in an arena."""
    n = getattr(lib, sizer)(*dims)
    assert n > 0, (sizer, dims)
    nwords = n if words_per == 1 else (n + 3) // 4                     # *_packed_bytes: bytes -> words
    wd = w.contiguous().to(DEV)
    wp = torch.zeros(nwords, dtype=torch.int32, device=DEV)
    assert getattr(lib, packer)(wd.data_ptr(), wp.data_ptr(), *dims, _lib.stream_ptr()) == 0, packer
    torch.cuda.synchronize()
    return wp.cpu()


def ptr_array(p, names):
    return (ctypes.c_void_p * len(names))(*[p(n) for n in names])


def int_array(vals):
    return (ctypes.c_int * len(vals))(*vals)


_CASES = {}


def case_of(row):
    if row.name not in _CASES:
        _CASES[row.name] = row.build()
    c = _CASES[row.name]
    if c.pack is not None and not c.packed:
        c.inputs.update(c.pack(_lib.load()))
        c.packed = True
    return c


def variants_of(row, case):
    """[(label, {operand: offset in floats}, expected return code)]"""
    names = [n for n in list(case.inputs) + list(case.outs) + list(case.inout)]
    movable = [n for n in names if n not in row.aligned]

    def expected(off):
        for n, (code, align) in row.refuse.items():
            if n in names and (4 * off.get(n, 0)) % align:
                return code
        return OK

    out = [("a", {})]
    if "b" in row.variants:
        for n in row.pred:
            assert n in movable, f"{row.name}: predicate operand {n} is not an operand of the row"
            out.append((f"b:{n}", {n: 1}))
    for n in movable:
        if "b" not in row.variants or n not in row.pred:
            out.append((f"o:{n}", {n: 1}))
    for k in (1, 2, 3):
        off = {n: k for n in movable}
        out.append((f"c{k}", off))
        if expected(off) != OK:               # the operands the entry refuses stay put, the others still move
            keep = {n: k for n in movable if n not in row.refuse or (4 * k) % row.refuse[n][1] == 0}
            if keep:
                out.append((f"c{k}-accepted", keep))
    for n in row.refuse:                      # every documented refusal alone (wpacked among them)
        if n in names and not any(o == {n: 1} for _, o in out):
            out.append((f"refuse:{n}", {n: 1}))
    return [(label, off, expected(off)) for label, off in out]


def _stream():
    return _lib.stream_ptr() if DEV != "cpu" else 0


def _sync_or_stop(what):
    if DEV == "cpu":                   # tests/test_abi_arena_harness.py drives this harness with Python "kernels"
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a GPU fault: nothing more may start on this device
        pytest.exit(f"GPU fault in {what}: {e}", returncode=3)


def place_operands(row, case, label, off):
    """name -> Arena of every operand of ``case``, each displaced by ``off`` floats (tests/test_gpu_stream_contract.py places
    its operands through this too)."""
    ar = {}
    for n, t in case.inputs.items():
        ar[n] = A.place(t, off.get(n, 0), "in", DEV, name=f"{row.name}[{label}].{n}")
    for n, t in case.outs.items():
        ar[n] = A.place(t, off.get(n, 0), "out", DEV, name=f"{row.name}[{label}].{n}")
    for n, t in case.inout.items():
        ar[n] = A.place(t, off.get(n, 0), "inout", DEV, name=f"{row.name}[{label}].{n}")
    return ar


def run_variant(row, case, label, off, want):
    lib = _lib.load() if DEV != "cpu" else None
    ar = place_operands(row, case, label, off)
    p = lambda n: ar[n].data_ptr() if n in ar else None
    if case.before:
        case.before(lib)
    try:
        rc = case.call(lib, p, _stream())
        _sync_or_stop(f"{row.entry} [{row.name} {label}]")
    finally:
        if case.after:
            case.after(lib)
    assert rc == want, f"returned {rc}, the source gives {want} for this placement"
    for n in case.inputs:
        A.check_guards(ar[n])
    if want != OK:
        for n in case.outs:
            A.check_untouched(ar[n])
        for n, t in case.inout.items():
            A.check_guards(ar[n])
            assert torch.equal(ar[n].view.cpu(), t), f"{n}: a refused call changed an in/out operand"
        return None
    got = {}
    for n in list(case.outs) + list(case.inout):
        A.check_output(ar[n], case.ref.get(n))
        got[n] = ar[n].view.cpu()
        if n in case.ref:
            case.bar(n, got[n], case.ref[n])
    return got


REPORT = []


def run_row(row):
    case = case_of(row)
    failures, ran, refused, outputs = [], [], [], {}
    for label, off, want in variants_of(row, case):
        print(f"  {row.name} [{label}] expects {want}")
        try:
            outputs[label] = run_variant(row, case, label, off, want)
            (ran if want == OK else refused).append(label if want == OK else f"{label}={want}")
        except AssertionError as e:
            failures.append(f"[{label}] {type(e).__name__}: {e}")
    for x, y in row.same_bits:
        if outputs.get(x) is not None and outputs.get(y) is not None:
            for n in outputs[x]:
                if not torch.equal(outputs[x][n], outputs[y][n]):
                    failures.append(f"[{x} vs {y}] {n}: the two paths promise the same bits and differ")
    line = f"ARENA {row.entry} ({row.name}): ran {' '.join(ran)}" + (f"; refused {' '.join(refused)}" if refused else "")
    REPORT.append(line)
    print(line)
    if failures:
        pytest.fail(f"{row.entry} ({row.name}; bar of {row.cite}):\n  " + "\n  ".join(failures), pytrace=False)


# ------------------------------------------------------------------ rows: cost-volume builders
def _gwc(shape):
    def build():
        b, c, h, w, d, g = shape
        L, R = torch.randn(b, c, h, w, generator=G(3)), torch.randn(b, c, h, w, generator=G(4))
        ref = O.build_gwc_volume(L.double(), R.double(), d, g)
        base = bar_close(1e-6, 1e-6)

        def bar(name, got, r):
            base(name, got, r)
            for dd in range(1, min(d, w)):
                assert float(got[:, :, dd, :, :dd].abs().max()) == 0.0        # x < d stays exactly zero
        return Case({"ref": L, "tgt": R}, {"out": torch.empty(b, g, d, h, w)},
                    lambda lib, p, s: lib.dv_gwc_volume_f32(p("ref"), p("tgt"), p("out"), b, c, h, w, d, g, s), {"out": ref}, bar)
    return build


def _concat(shape, zero_left):
    def build():
        b, c, h, w, d = shape
        L, R = torch.randn(b, c, h, w, generator=G(5)), torch.randn(b, c, h, w, generator=G(6))
        ref = O.build_concat_volume(L.double(), R.double(), d, zero_left=zero_left)
        return Case({"ref": L, "tgt": R}, {"out": torch.empty(b, 2 * c, d, h, w)},
                    lambda lib, p, s: lib.dv_concat_volume_f32(p("ref"), p("tgt"), p("out"), b, c, h, w, d, int(zero_left), s),
                    {"out": ref}, bar_equal)
    return build


def _concat_att(shape, prob):
    def build():
        b, c, h, w, d = shape
        L, R = torch.randn(b, c, h, w, generator=G(7)), torch.randn(b, c, h, w, generator=G(8))
        att = torch.randn(b, 1, d, h, w, generator=G(9)) * 2
        ref = O.attention_concat_volume(att.double(), O.build_concat_volume(L.double(), R.double(), d))
        if prob:
            third = torch.softmax(att, dim=2)[:, 0].contiguous()
            call = lambda lib, p, s: lib.dv_concat_prob_volume_f32(p("ref"), p("tgt"), p("att"), p("out"), b, c, h, w, d, s)
        else:
            third = att
            call = lambda lib, p, s: lib.dv_concat_attn_volume_f32(p("ref"), p("tgt"), p("att"), p("out"), b, c, h, w, d, s)
        return Case({"ref": L, "tgt": R, "att": third}, {"out": torch.empty(b, 2 * c, d, h, w)}, call, {"out": ref},
                    bar_close(1e-6, 1e-5))
    return build


def _patch(shape, runs):
    def build():
        b, g, d, h, w = shape
        assert g == 40
        gen = G(81)
        x = torch.randn(*shape, generator=gen)
        conv = lambda c, dl: torch.nn.Conv3d(c, c, (1, 3, 3), 1, (0, dl, dl), dl, groups=c, bias=False).double()
        patch, l1, l2, l3 = conv(40, 1), conv(8, 1), conv(16, 2), conv(16, 3)
        for m in (patch, l1, l2, l3):
            m.weight.data = (torch.randn(m.weight.shape, generator=gen) * 0.4).double()
        with torch.no_grad():
            y = patch(x.double())
            ref = torch.cat((l1(y[:, :8]), l2(y[:, 8:24]), l3(y[:, 24:40])), dim=1)
        w1 = patch.weight.detach().reshape(40, 9).float()
        w2 = torch.cat([m.weight.detach().reshape(-1, 9) for m in (l1, l2, l3)]).float()
        dil = torch.tensor([1] * 8 + [2] * 16 + [3] * 16, dtype=torch.int32)
        if runs:
            g0, ng, dl = int_array([0, 8, 24]), int_array([8, 16, 16]), int_array([1, 2, 3])
            call = lambda lib, p, s: lib.dv_patch_volume_runs_f32(p("gwc"), p("w1"), p("w2"), p("dilation"), p("out"), b, g, d,
                                                                  h, w, 3, g0, ng, dl, s)
        else:
            call = lambda lib, p, s: lib.dv_patch_volume_f32(p("gwc"), p("w1"), p("w2"), p("dilation"), p("out"), b, g, d, h, w, s)
        return Case({"gwc": x, "w1": w1, "w2": w2, "dilation": dil}, {"out": torch.empty(*shape)}, call, {"out": ref},
                    bar_close(2e-5, 1e-5))
    return build


# ------------------------------------------------------------------ rows: the rank-1 first layer and its tables
def _pointwise(shape):
    def build():
        b, cin, cout, h, w = shape
        x = torch.randn(b, cin, h, w, generator=G(221))
        wt = torch.randn(cout, cin, generator=G(222)) * cin ** -0.5
        ref = F.conv2d(x.double(), wt.double().view(cout, cin, 1, 1))
        return Case({"in": x}, {"out": torch.empty(b, cout, h, w)},
                    lambda lib, p, s: lib.dv_pointwise_expand_f32(p("in"), p("wpacked"), p("out"), b, cin, h * w, cout, s),
                    {"out": ref}, bar_rel(2e-6),
                    pack=lambda lib: {"wpacked": pack_through_abi(lib, "dv_pointwise_expand_packed_floats",
                                                                  "dv_pointwise_expand_pack_weights_f32", wt, cin, cout)})
    return build


def _softmax_d():
    b, d, hw = 2, 12, 35
    att = torch.randn(b, d, hw, generator=G(11)) * 2
    return Case({"att": att}, {"p": torch.empty(b, d, hw)},
                lambda lib, p, s: lib.dv_softmax_d_f32(p("att"), p("p"), b, d, hw, s),
                {"p": torch.softmax(att.double(), dim=1)}, bar_rel(1e-6))


def _mul():
    n = 1003
    x, y = torch.randn(n, generator=G(12)), torch.rand(n, generator=G(13))
    return Case({"x": x, "y": y}, {"out": torch.empty(n)},
                lambda lib, p, s: lib.dv_mul_f32(p("x"), p("y"), p("out"), n, s), {"out": x.double() * y.double()}, bar_rel(1e-5))


def _rank1(shape):
    def build():
        b, c, cout, d, h, w = shape
        g = G(211)
        L, R = torch.randn(b, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g)
        att = torch.randn(b, 1, d, h, w, generator=g) * 2
        noise = torch.rand(b, d, h, w, generator=g)
        wt = torch.randn(cout, 2 * c, 3, 3, 3, generator=g) * (2.0 / (27 * cout)) ** 0.5
        scale, bias = torch.rand(cout, generator=g) * 0.4 + 0.8, torch.randn(cout, generator=g) * 0.1
        vol = O.attention_concat_volume(att.double(), O.build_concat_volume(L.double(), R.double(), d))
        y = F.conv3d(vol * noise.double().unsqueeze(1), wt.double(), None, 1, 1)
        ref = torch.relu(y * scale.double().view(1, -1, 1, 1, 1) + bias.double().view(1, -1, 1, 1, 1))
        # the layer's operands as Rank1FilterPlan hands them over: s = softmax(att) * noise and the two tap tables
        sfac = (torch.softmax(att, dim=2)[:, 0] * noise).contiguous()
        wl = wt[:, :c].permute(2, 3, 4, 0, 1).reshape(27 * cout, c, 1, 1)
        wr = wt[:, c:].permute(2, 3, 4, 0, 1).reshape(27 * cout, c, 1, 1)
        gl, gr = F.conv2d(L, wl).contiguous(), F.conv2d(R, wr).contiguous()
        return Case({"s": sfac, "gl": gl, "gr": gr, "ch_scale": scale, "ch_bias": bias}, {"out": torch.empty(b, cout, d, h, w)},
                    lambda lib, p, s: lib.dv_conv3d_rank1_filter_f32(p("s"), p("gl"), p("gr"), p("ch_scale"), p("ch_bias"),
                                                                     p("out"), b, d, h, w, cout, S.ACT_RELU, s),
                    {"out": ref}, bar_rel(1e-5))
    return build


def _noise_prepare(f64):
    def build():
        b, c, hw = 2, 12, 35
        x = torch.randn(b, c, hw, generator=G(14), dtype=torch.float64 if f64 else torch.float32) * 1.5
        shift = torch.randn(b, c, generator=G(15)) * 0.3
        ref = (torch.clamp(x.double() + shift.double().unsqueeze(-1), -1, 1) + 1) / 2
        if f64:
            return Case({"x_t": x, "shift": shift}, {"n01": torch.empty(b, c, hw, dtype=torch.float64), "n01_f32": torch.empty(b, c, hw)},
                        lambda lib, p, s: lib.dv_noise_prepare_f64(p("x_t"), p("shift"), p("n01"), p("n01_f32"), b, c, hw, s),
                        {"n01": ref, "n01_f32": ref}, bar_close(1e-6, 0))
        return Case({"x_t": x, "shift": shift}, {"n01": torch.empty(b, c, hw)},
                    lambda lib, p, s: lib.dv_noise_prepare_f32(p("x_t"), p("shift"), p("n01"), b, c, hw, s), {"n01": ref},
                    bar_close(1e-6, 0))
    return build


# ------------------------------------------------------------------ rows: 3-D convolutions
def _conv3d(kind, cin, cout, dims, k=3, stride=1, act=S.ACT_RELU, in_scale=False, residual=True, seed=7, xgain=1.0, hook=None):
    """kind: direct | wino | wino3 | s2pp | f16x3; hook = (test hook of the library, arguments for the call): pinned for the
    call and reset to its defaults (all zeros) afterwards."""
    def build():
        g = G(seed)
        b, d, h, w = dims
        x = torch.randn(b, cin, d, h, w, generator=g) * xgain
        wt = torch.randn(cout, cin, k, k, k, generator=g) * (2.0 / (k ** 3 * cin)) ** 0.5
        cs, cb = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        sc = torch.rand(b, d, h, w, generator=g) if in_scale else None
        xin = x.double() if sc is None else x.double() * sc.double().unsqueeze(1)
        y = F.conv3d(xin, wt.double(), None, stride, (k - 1) // 2)
        y = y * cs.double().view(1, -1, 1, 1, 1) + cb.double().view(1, -1, 1, 1, 1)
        res = torch.randn(y.shape, generator=g) if residual else None
        if res is not None:
            y = y + res.double()
        ref = act64(y, act)
        inputs = {"in": x, "ch_scale": cs, "ch_bias": cb}
        if sc is not None:
            inputs["in_scale"] = sc
        if res is not None:
            inputs["residual"] = res
        inout = {}
        if kind == "direct":
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv3d_packed_floats", "dv_conv3d_pack_weights_f32", wt, cin, cout, k)}
            call = lambda lib, p, s: lib.dv_conv3d_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("in_scale"), p("residual"),
                                                       p("out"), b, cin, d, h, w, cout, k, stride, act, s)
        elif kind == "wino":
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv3d_wino_packed_floats", "dv_conv3d_wino_pack_weights_f32", wt, cin, cout)}
            call = lambda lib, p, s: lib.dv_conv3d_wino_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("in_scale"),
                                                            p("residual"), p("out"), b, cin, d, h, w, cout, act, s)
        elif kind == "wino3":
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv3d_wino3_packed_floats", "dv_conv3d_wino3_pack_weights_f32", wt, cin, cout)}
            call = lambda lib, p, s: lib.dv_conv3d_wino3_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("residual"),
                                                             p("out"), b, cin, d, h, w, cout, act, s)
        elif kind == "s2pp":
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv3d_s2pp_packed_floats", "dv_conv3d_s2pp_pack_weights_f32", wt, cin, cout)}
            call = lambda lib, p, s: lib.dv_conv3d_s2pp_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("residual"),
                                                            p("out"), b, cin, d, h, w, cout, act, s)
        else:
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv3d_f16x3_packed_bytes", "dv_conv3d_f16x3_pack_weights", wt, cin, cout,
                                                            words_per=4)}
            inout = {"overflow_flag": torch.zeros(1, dtype=torch.int32)}
            call = lambda lib, p, s: lib.dv_conv3d_f16x3_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("in_scale"),
                                                             p("residual"), p("out"), p("overflow_flag"), b, cin, d, h, w, cout, act, s)
        refs = {"out": ref}
        if inout:
            refs["overflow_flag"] = torch.zeros(1, dtype=torch.float64)
        base = bar_rel(1e-5)

        def bar(name, got, r):
            if name == "overflow_flag":
                assert int(got.item()) == 0, "the split-fp16 range flag was raised"
            else:
                base(name, got, r)
        before = after = None
        if hook is not None:
            def before(lib):
                assert getattr(lib, hook[0])(*hook[1]) == 0

            def after(lib):
                getattr(lib, hook[0])(*([0] * len(hook[1])))
        return Case(inputs, {"out": torch.empty(ref.shape)}, call, refs, bar, inout=inout, pack=pack, before=before, after=after)
    return build


def _deconv3d(k, cin, cout, dims, act, impl=0, residual=True, seed=9):
    def build():
        g = G(seed)
        b, d, h, w = dims
        x = torch.randn(b, cin, d, h, w, generator=g)
        wt = torch.randn(cin, cout, k, k, k, generator=g) * (2.0 / (k ** 3 * cin)) ** 0.5
        cs, cb = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
        up = F.conv_transpose3d(x.double(), wt.double(), None, 2, 1, 1 if k == 3 else 0)
        y = up * cs.double().view(1, -1, 1, 1, 1) + cb.double().view(1, -1, 1, 1, 1)
        inputs = {"in": x, "ch_scale": cs, "ch_bias": cb}
        if residual:
            inputs["residual"] = torch.randn(y.shape, generator=g)
            y = y + inputs["residual"].double()
        ref = act64(y, act)
        names = ("dv_deconv3d_packed_floats", "dv_deconv3d_pack_weights_f32", "dv_deconv3d_k3s2_f32") if k == 3 else \
                ("dv_deconv3d_k4_packed_floats", "dv_deconv3d_k4_pack_weights_f32", "dv_deconv3d_k4s2_f32")
        call = lambda lib, p, s: getattr(lib, names[2])(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("residual"), p("out"),
                                                        b, cin, d, h, w, cout, act, s)

        def before(lib):
            assert lib.dv_deconv3d_set_impl(impl) == 0
            if impl == 2:
                assert lib.dv_deconv3d_pl_supported(cin, cout, d, h, w, 0) == 1
        return Case(inputs, {"out": torch.empty(ref.shape)}, call, {"out": ref}, bar_rel(1e-5),
                    pack=lambda lib: {"wpacked": pack_through_abi(lib, names[0], names[1], wt, cin, cout)},
                    before=before, after=lambda lib: lib.dv_deconv3d_set_impl(0))
    return build


def _redir(cin, cout, cskip, dims, act, impl, seed=51):
    def build():
        g = G(seed)
        b, d, h, w = dims
        x = torch.randn(b, cin, d, h, w, generator=g)
        skip = torch.randn(b, cskip, 2 * d, 2 * h, 2 * w, generator=g)
        wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
        wr = torch.randn(cout, cskip, generator=g) * (1.0 / cskip) ** 0.5
        cb = torch.randn(cout, generator=g) * 0.1
        y = F.conv_transpose3d(x.double(), wt.double(), None, 2, 1, 1) + F.conv3d(skip.double(), wr.double().view(cout, cskip, 1, 1, 1)) \
            + cb.double().view(1, -1, 1, 1, 1)
        ref = act64(y, act)

        def before(lib):
            assert lib.dv_deconv3d_set_impl(impl) == 0
            if impl == 2:
                assert lib.dv_deconv3d_pl_supported(cin, cout, d, h, w, cskip) == 1
        return Case({"in": x, "ch_bias": cb, "skip": skip, "redir_w": wr}, {"out": torch.empty(ref.shape)},
                    lambda lib, p, s: lib.dv_deconv3d_k3s2_redir_f32(p("in"), p("wpacked"), p("ch_bias"), p("skip"), p("redir_w"),
                                                                     p("out"), b, cin, d, h, w, cout, cskip, act, s),
                    {"out": ref}, bar_rel(1e-5),
                    pack=lambda lib: {"wpacked": pack_through_abi(lib, "dv_deconv3d_packed_floats", "dv_deconv3d_pack_weights_f32", wt, cin, cout)},
                    before=before, after=lambda lib: lib.dv_deconv3d_set_impl(0))
    return build


# ------------------------------------------------------------------ rows: 2-D convolutions
def _conv2d(kind, cins, cout, hw, b=1, k=3, dil=1, act=S.ACT_NONE, residual=False, mul=False, blend=False, bar=None, seed=31,
            cout2=0):
    """kind: plain | gated | cat | cat_ksplit | s2 | wino | wino_dil | wino_ksplit | wino_pair | wino_pair_ksplit | wino_s2b"""
    def build():
        g = G(seed)
        h, w = hw
        cin, ctot = sum(cins), cout + cout2
        xs = [torch.randn(b, c, h, w, generator=g) for c in cins]
        wt = torch.randn(ctot, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
        cs, cb = torch.rand(ctot, generator=g) + 0.5, torch.randn(ctot, generator=g) * 0.1
        stride = 2 if kind == "s2" else 1
        y = F.conv2d(torch.cat(xs, 1).double(), wt.double(), None, stride, dil if k == 3 else 0, dil if k == 3 else 1)
        y = y * cs.double().view(1, -1, 1, 1) + cb.double().view(1, -1, 1, 1)
        ho, wo = y.shape[2], y.shape[3]
        names = [f"in{i}" for i in range(len(xs))] if len(xs) > 1 or kind not in ("plain", "gated", "s2") else ["in"]
        inputs = dict(zip(names, xs))
        inputs.update({"ch_scale": cs, "ch_bias": cb})
        chans = int_array(list(cins))
        rnd = lambda c: torch.randn(b, c, ho, wo, generator=g)
        pair = kind in ("wino_pair", "wino_pair_ksplit")
        if pair:
            inputs.update({"residual1": rnd(cout), "residual2": rnd(cout2), "mul2": rnd(cout2)})
            y1 = act64(y[:, :cout] + inputs["residual1"].double(), act)
            y2 = act64(y[:, cout:] + inputs["residual2"].double(), act) * inputs["mul2"].double()
            refs = {"out1": y1, "out2": y2}
            outs = {"out1": torch.empty(y1.shape), "out2": torch.empty(y2.shape)}
        else:
            if residual:
                inputs["residual"] = rnd(cout)
                y = y + inputs["residual"].double()
            y = act64(y, act)
            if mul:
                inputs["mul"] = rnd(cout)
                y = y * inputs["mul"].double()
            if blend:
                inputs["blend_z"], inputs["blend_h"] = torch.rand(b, cout, ho, wo, generator=g), rnd(cout)
                y = inputs["blend_h"].double() + inputs["blend_z"].double() * (y - inputs["blend_h"].double())
            if kind == "wino_s2b":       # dv_space_to_batch2_f32's mapping of the result
                y = torch.stack([y[n, :, ry::2, rx::2] for n in range(b) for ry in (0, 1) for rx in (0, 1)])
            refs, outs = {"out": y}, {"out": torch.empty(y.shape)}
        wino = kind.startswith("wino")
        if wino:
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv2d_wino_packed_floats", "dv_conv2d_wino_pack_weights_f32", wt, cin, ctot)}
        else:
            pack = lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv2d_packed_floats", "dv_conv2d_pack_weights_f32", wt, cin, ctot, k, dil)}
        inout = {}
        ks = {"n": 0}
        if kind.endswith("ksplit"):
            lib0 = _lib.load()
            ks["n"] = lib0.dv_conv2d_wino_auto_kslices(cin, h, w, ctot, dil) if wino else lib0.dv_conv2d_auto_kslices(1, cin, h, w, ctot, k, dil)
            assert ks["n"] > 1, (kind, cins, hw, ks["n"])
            inout["scratch"] = torch.zeros(ks["n"] * b * ctot * h * w)
        epi = lambda p: (p("residual"), p("mul"), p("blend_z"), p("blend_h"))
        head = lambda p: (ptr_array(p, names), chans, len(names), p("wpacked"), p("ch_scale"), p("ch_bias"))
        calls = {
            "plain": lambda lib, p, s: lib.dv_conv2d_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("residual"), p("out"),
                                                         b, cin, h, w, cout, k, dil, act, s),
            "gated": lambda lib, p, s: lib.dv_conv2d_gated_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), *epi(p), p("out"),
                                                               b, cin, h, w, cout, k, dil, act, s),
            "s2": lambda lib, p, s: lib.dv_conv2d_s2_f32(p("in"), p("wpacked"), p("ch_scale"), p("ch_bias"), p("residual"), p("out"),
                                                         b, cin, h, w, cout, k, act, s),
            "cat": lambda lib, p, s: lib.dv_conv2d_cat_f32(*head(p), *epi(p), p("out"), b, h, w, cout, k, dil, act, s),
            "cat_ksplit": lambda lib, p, s: lib.dv_conv2d_cat_ksplit_f32(*head(p), *epi(p), p("out"), p("scratch"), ks["n"], b, h, w,
                                                                         cout, k, dil, act, s),
            "wino": lambda lib, p, s: lib.dv_conv2d_wino_cat_f32(*head(p), *epi(p), p("out"), b, h, w, cout, act, s),
            "wino_dil": lambda lib, p, s: lib.dv_conv2d_wino_dil_cat_f32(*head(p), *epi(p), p("out"), b, h, w, cout, dil, act, s),
            "wino_ksplit": lambda lib, p, s: lib.dv_conv2d_wino_cat_ksplit_f32(*head(p), *epi(p), p("out"), p("scratch"), ks["n"], b, h,
                                                                               w, cout, dil, act, s),
            "wino_pair": lambda lib, p, s: lib.dv_conv2d_wino_cat_pair_f32(*head(p), p("residual1"), p("mul1"), p("out1"), p("residual2"),
                                                                           p("mul2"), p("out2"), b, h, w, cout, cout2, act, s),
            "wino_pair_ksplit": lambda lib, p, s: lib.dv_conv2d_wino_cat_pair_ksplit_f32(
                *head(p), p("residual1"), p("mul1"), p("out1"), p("residual2"), p("mul2"), p("out2"), p("scratch"), ks["n"], b, h, w,
                cout, cout2, act, s),
            "wino_s2b": lambda lib, p, s: lib.dv_conv2d_wino_s2b_f32(*head(p), p("out"), b, h, w, cout, act, s),
        }
        return Case(inputs, outs, calls[kind], refs, bar or bar_rel(1e-5), inout=inout, pack=pack)
    return build


def _refine_inputs(shape):
    def build():
        b, c, h, w = shape
        g = G(77)
        fl, fr = torch.randn(b, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g)
        p3 = torch.rand(b, 1, h, w, generator=g) * 60 - 6
        du_a, du_b = torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
        frw = PO.warp(fr, p3)
        aff = du_a.view(1, c, 1, 1) * p3 + du_b.view(1, c, 1, 1)
        ref = torch.cat((fl - frw, fl, PO.mish(aff), p3, PO.correlation_pm(fl, frw, 24)), dim=1).double()
        return Case({"left": fl, "right": fr, "disp": p3, "du_a": du_a, "du_b": du_b}, {"out": torch.empty(ref.shape)},
                    lambda lib, p, s: lib.dv_refine_inputs_f32(p("left"), p("right"), p("disp"), p("du_a"), p("du_b"), p("out"),
                                                               b, c, h, w, 24, s), {"out": ref}, bar_close(2e-5, 1e-5))
    return build


def _space_to_batch():
    n, c, h, w = 3, 5, 8, 12
    x = torch.randn(n, c, h, w, generator=G(321))
    want = torch.stack([x[i, :, ry::2, rx::2] for i in range(n) for ry in (0, 1) for rx in (0, 1)])
    return Case({"in": x}, {"out": torch.empty(want.shape)},
                lambda lib, p, s: lib.dv_space_to_batch2_f32(p("in"), p("out"), n, c, h, w, s), {"out": want.double()}, bar_equal)


def _batch_to_space():
    b, c, h, w, levels = 2, 3, 8, 12, 2
    x = torch.randn(b, c, h, w, generator=G(322))
    sub = x
    for _ in range(levels):
        sub = torch.stack([sub[i, :, ry::2, rx::2] for i in range(sub.shape[0]) for ry in (0, 1) for rx in (0, 1)])
    return Case({"in": sub.contiguous()}, {"out": torch.empty(b, c, h, w)},
                lambda lib, p, s: lib.dv_batch_to_space_f32(p("in"), p("out"), b, c, h, w, levels, s), {"out": x.double()}, bar_equal)


# ------------------------------------------------------------------ rows: IGEV volume, lookup, update-block glue
def _feature_gate(shape):
    def build():
        g = G(95)
        cv = torch.randn(*shape, generator=g)
        logit = torch.randn(shape[0], shape[1], shape[3], shape[4], generator=g) * 3
        ref = torch.sigmoid(logit.double()).unsqueeze(2) * cv.double()
        b, c, d, h, w = shape
        return Case({"cv": cv, "logit": logit}, {"out": torch.empty(*shape)},
                    lambda lib, p, s: lib.dv_feature_gate_f32(p("cv"), p("logit"), p("out"), b, c, d, h, w, s), {"out": ref},
                    bar_close(1e-6, 1e-6))
    return build


def _window_attn(shape):
    def build():
        from diffuvolume_amd.acv_ddim import _WindowAttention
        from diffuvolume_amd.synth import synth_state_dict
        sd = {"a." + k: v for k, v in synth_state_dict(_WindowAttention(128, 16).state_dict(), seed=25).items()}
        x = torch.randn(*shape, generator=G(25))
        y64 = O.attention_block(x.double(), {k: v.double() for k, v in sd.items()}, "a")
        y32 = O.attention_block(x, sd, "a")
        scale = float(y64.abs().max())
        e_orc = float((y32.double() - y64).abs().max()) / scale

        def bar(name, got, ref):          # test_window_attention_vs_float64: at most 2x the fp32 oracle's own error + 1e-6
            e_hip = float((got.double() - ref).abs().max()) / scale
            print(f"    {name}: error / output scale {e_hip:.2e} (fp32 oracle {e_orc:.2e})")
            assert e_hip <= 2 * e_orc + 1e-6, (e_hip, e_orc)
        b, c, d, h, w = shape
        return Case({"x": x, "qkv_w": sd["a.qkv_3d.weight"].contiguous(), "qkv_b": sd["a.qkv_3d.bias"].contiguous(),
                     "proj_w": sd["a.final1x1.weight"].reshape(c, c).contiguous(), "proj_b": sd["a.final1x1.bias"].contiguous()},
                    {"out": torch.empty(*shape)},
                    lambda lib, p, s: lib.dv_window_attn3d_f32(p("x"), p("qkv_w"), p("qkv_b"), p("proj_w"), p("proj_b"), p("out"),
                                                               b, c, d, h, w, 16, s), {"out": y64}, bar)
    return build


def _allpairs(shape):
    def build():
        b, c, h, w1, w2 = shape
        g = G(63)
        f1, f2 = torch.randn(b, c, h, w1, generator=g), torch.randn(b, c, h, w2, generator=g)
        ref = IO.all_pairs_corr(f1.double(), f2.double()).reshape(b, h, w1, w2)
        ref1 = F.avg_pool2d(ref.reshape(b * h * w1, 1, 1, w2), [1, 2], stride=[1, 2]).reshape(b, h, w1, w2 // 2)
        lim = 2e-6 * float(ref.abs().max())

        def bar(name, got, r):
            e = float((got.double() - r).abs().max())
            print(f"    {name}: max abs err {e:.2e} (bar {lim:.2e})")
            assert e <= lim, (name, e, lim)
        return Case({"fmap1": f1, "fmap2": f2}, {"corr0": torch.empty(b, h, w1, w2), "corr1": torch.empty(b, h, w1, w2 // 2)},
                    lambda lib, p, s: lib.dv_allpairs_corr_f32(p("fmap1"), p("fmap2"), p("corr0"), p("corr1"), b, c, h, w1, w2, s),
                    {"corr0": ref, "corr1": ref1}, bar)
    return build


def _geo_lookup(d, w, fused):
    def build():
        b, c, h = 1, 8, 6
        gen = G(64 + d)
        geo = torch.randn(b, c, d, h, w, generator=gen)
        f1, f2 = torch.randn(b, 16, h, w, generator=gen), torch.randn(b, 16, h, w, generator=gen)
        disp = torch.rand(b, 1, h, w, generator=gen) * (d + 12) - 6                       # -6 .. d + 6
        disp[:, :, 0] = torch.arange(w, dtype=torch.float32) - 4                           # integers, also out of range
        disp[:, :, 1] = torch.arange(w, dtype=torch.float32) * 0.5 + 1e-6
        coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous()
        noisy = torch.rand(b, d, h, w, generator=gen)
        # (evaluated in float64; the oracle hands its result back rounded to float32)
        look = IO.geo_filter_lookup(geo.double(), f1.double(), f2.double(), disp.double(), coords.double(), noisy.double()).double()
        corr0 = torch.einsum("aijk,aijh->ajkh", f1, f2).contiguous()                      # what dv_allpairs_corr_f32 hands over
        corr1 = F.avg_pool2d(corr0, [1, 2], stride=[1, 2]).contiguous()
        inputs = {"geo": geo, "corr0": corr0, "corr1": corr1, "disp": disp, "coords": coords, "noisy": noisy}
        if not fused:
            return Case(inputs, {"out": torch.empty(look.shape)},
                        lambda lib, p, s: lib.dv_geo_filter_lookup_f32(p("geo"), p("corr0"), p("corr1"), p("disp"), p("coords"),
                                                                       p("noisy"), p("out"), b, c, d, h, w, w, 4, s),
                        {"out": look}, bar_close(3e-5, 1e-5))
        wt = torch.randn(64, 162, generator=gen) * 0.1
        inputs["bias"] = torch.randn(64, generator=gen) * 0.1
        ref = torch.relu(F.conv2d(look, wt.double().view(64, 162, 1, 1), inputs["bias"].double()))
        return Case(inputs, {"out": torch.empty(ref.shape)},
                    lambda lib, p, s: lib.dv_geo_filter_lookup_conv1x1_f32(p("geo"), p("corr0"), p("corr1"), p("disp"), p("coords"),
                                                                           p("noisy"), p("wpacked"), p("bias"), p("out"), b, c, d, h,
                                                                           w, w, 4, 64, S.ACT_RELU, s),
                    {"out": ref}, bar_scaled(2e-5),
                    pack=lambda lib: {"wpacked": pack_through_abi(lib, "dv_geo_lookup_conv1x1_packed_floats",
                                                                  "dv_geo_lookup_conv1x1_pack_weights_f32", wt, c)})
    return build


def _context_upsample(shape, softmax):
    def build():
        b, h, w = shape
        disp = torch.randn(b, 1, h, w, generator=G(3)).abs() * 4
        wts = torch.randn(b, 9, 4 * h, 4 * w, generator=G(4)) * (2.0 if softmax else 1.0)
        fn = lambda d, x: IO.context_upsample(d * 4.0, F.softmax(x, 1) if softmax else x)
        o64, o32 = fn(disp.double(), wts.double()), fn(disp, wts)
        nrm = lambda a, r: float((a.double().reshape(-1) - r.reshape(-1)).norm() / r.reshape(-1).norm().clamp_min(1e-30))
        lim = 2 * nrm(o32, o64) + 1e-6        # test_gradients_match_float64_autograd, "out"

        def bar(name, got, ref):
            e = nrm(got, ref)
            print(f"    {name}: relative L2 error {e:.2e} (bar {lim:.2e})")
            assert e <= lim, (e, lim)
        return Case({"disp_low": disp, "weights": wts}, {"out": torch.empty(b, 4 * h, 4 * w)},
                    lambda lib, p, s: lib.dv_context_upsample_f32(p("disp_low"), p("weights"), p("out"), b, h, w, 4.0, int(softmax), s),
                    {"out": o64.reshape(b, 4 * h, 4 * w)}, bar)
    return build


def _conv2d_1in(f16):
    def build():
        b, h, w, cout, k = 2, 7, 9, 64, 7
        g = G(151)
        d = torch.rand(b, 1, h, w, generator=g) * 40
        wt, bias = torch.randn(cout, 1, k, k, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1
        if f16:          # the autocast statement of test_gpu_igev_mixed's convd1: fp16 operands, fp32 accumulation, fp16 result
            r16 = lambda t: t.half().float()
            y = F.conv2d(r16(d).double(), r16(wt).double(), r16(bias).double(), 1, k // 2).float()
            ref = torch.relu(r16(y)).double()
            bar = bar_close(0.0, 2e-3)        # one fp16 ulp (2^-10 relative): the sum is rounded to fp16 once, after another order
        else:
            ref = F.relu(F.conv2d(d.double(), wt.double(), bias.double(), 1, k // 2))
            bar = bar_scaled(2e-6)
        fn = "dv_conv2d_1in_f16" if f16 else "dv_conv2d_1in_f32"
        return Case({"in": d, "w": wt, "bias": bias}, {"out": torch.empty(b, cout, h, w)},
                    lambda lib, p, s: getattr(lib, fn)(p("in"), p("w"), p("bias"), p("out"), b, h, w, cout, k, S.ACT_RELU, s),
                    {"out": ref}, bar)
    return build


def _resize(size):
    def build():
        b, c, h, w = 2, 3, 7, 9
        x = torch.randn(b, c, h, w, generator=G(152))
        ref = F.interpolate(x.double(), size, mode="bilinear", align_corners=True)
        return Case({"in": x}, {"out": torch.empty(b, c, *size)},
                    lambda lib, p, s: lib.dv_resize_bilinear_ac_f32(p("in"), p("out"), b * c, h, w, size[0], size[1], s), {"out": ref},
                    bar_close(1e-6, 1e-6))
    return build


def _avg_pool():
    b, c, h, w = 2, 3, 7, 9
    x = torch.randn(b, c, h, w, generator=G(153))
    ref = F.avg_pool2d(x.double(), 3, stride=2, padding=1)
    return Case({"in": x}, {"out": torch.empty(ref.shape)},
                lambda lib, p, s: lib.dv_avg_pool3s2_f32(p("in"), p("out"), b * c, h, w, s), {"out": ref}, bar_close(1e-6, 1e-6))


def _fewin(cin, cout, k, stride, h, w):
    def build():
        g = G(61)
        b = 2
        x = torch.randn(b, cin, h, w, generator=g)
        wt, bias = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k)) ** 0.5, torch.randn(cout, generator=g) * 0.1
        cs, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
        y = F.conv2d(x.double(), wt.double(), bias.double(), stride, k // 2)
        ref = torch.relu(y * cs.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        return Case({"in": x, "w": wt, "bias": bias, "ch_scale": cs, "ch_shift": sh}, {"out": torch.empty(ref.shape)},
                    lambda lib, p, s: lib.dv_conv2d_fewin_f32(p("in"), p("w"), p("bias"), p("ch_scale"), p("ch_shift"), p("out"), b, cin,
                                                              h, w, cout, k, stride, S.ACT_RELU, s), {"out": ref}, bar_rel(1e-5))
    return build


def _instance_norm():
    bc, h, w = 15, 21, 34
    x = torch.randn(3, 5, h, w, generator=G(62)) * 3 + 1
    ref = F.leaky_relu(F.instance_norm(x.double()), 0.01)

    def bar(name, got, r):
        e = float((got.double() - r).abs().max())
        print(f"    {name}: max abs err {e:.2e} (bar 1e-5)")
        assert e < 1e-5, e
    return Case({"in": x}, {"out": torch.empty(3, 5, h, w)},
                lambda lib, p, s: lib.dv_instance_norm_act_f32(p("in"), p("out"), bc, h * w, 1e-5, S.ACT_LEAKY, s), {"out": ref}, bar)


# ------------------------------------------------------------------ rows: regression tails, encoder, DDIM step, metrics
def _regress_tail(ac, uncertainty_only=False):
    def build():
        b, d, h, w = 1, 12, 3, 5
        cost = torch.randn(b, 1, d, h, w, generator=G(6)) * 5
        disp_ref, prob = O.upsample_softmax_regress(cost.double(), 4 * d, align_corners=ac)
        if uncertainty_only:
            other = (disp_ref + torch.randn(disp_ref.shape, generator=G(75), dtype=torch.float64) * 3).float()
            unc_ref = O.disparity_uncertainty(other.double(), prob)
            return Case({"cost": cost[:, 0].contiguous(), "disp": other}, {"unc": torch.empty(b, 4 * h, 4 * w)},
                        lambda lib, p, s: lib.dv_upsample_softmax_uncertainty_f32(p("cost"), p("disp"), p("unc"), b, d, h, w, int(ac), s),
                        {"unc": unc_ref}, bar_close(5e-4, 1e-5))
        return Case({"cost": cost[:, 0].contiguous()}, {"disp": torch.empty(b, 4 * h, 4 * w), "unc": torch.empty(b, 4 * h, 4 * w)},
                    lambda lib, p, s: lib.dv_upsample_softmax_regress_f32(p("cost"), p("disp"), p("unc"), b, d, h, w, int(ac), s),
                    {"disp": disp_ref, "unc": O.disparity_uncertainty(disp_ref, prob)}, bar_close(5e-4, 1e-5))
    return build


def _disparity_regression():
    b, d, h, w = 2, 12, 5, 7
    prob = torch.softmax(torch.randn(b, d, h, w, generator=G(16)) * 2, 1)
    return Case({"prob": prob}, {"disp": torch.empty(b, h, w)},
                lambda lib, p, s: lib.dv_disparity_regression_f32(p("prob"), p("disp"), b, d, h, w, s),
                {"disp": O.disparity_regression(prob.double(), d)}, bar_close(1e-5, 1e-5))


def _softmax_regress():
    b, d, h, w = 2, 48, 7, 9
    cost = torch.randn(b, d, h, w, generator=G(96)) * 5
    return Case({"cost": cost}, {"disp": torch.empty(b, h, w)},
                lambda lib, p, s: lib.dv_softmax_regress_f32(p("cost"), p("disp"), b, d, h, w, s),
                {"disp": O.disparity_regression(torch.softmax(cost.double(), 1), d)}, bar_close(2e-5, 1e-6))


def _quarter_disparity(b, h, w, nbins, seed):
    """Quarter-resolution disparities that stay 1e-3 away from every integer, so that floor() cannot come out differently
    in another precision, with both ends of the range present."""
    dq = torch.rand(b, h * w, generator=G(seed)) * (nbins - 1)
    frac = dq - dq.floor()
    dq = dq.floor() + frac.clamp(1e-3, 1 - 1e-3)
    dq[0, 0], dq[0, 1] = 0.25, nbins - 1 + 0.5          # the first and the forced last bin
    return dq


def _two_hot():
    b, nbins, h, w = 2, 12, 5, 7
    dq = _quarter_disparity(b, h, w, nbins, 17)
    ref = O.encode_two_hot(dq.view(b, 1, h, w), nbins).double().reshape(b, nbins, h * w) * 2 - 1
    return Case({"disp_q": dq}, {"x": torch.empty(b, nbins, h * w)},
                lambda lib, p, s: lib.dv_encode_two_hot_f32(p("disp_q"), p("x"), b, nbins, h * w, s), {"x": ref}, bar_equal)


def _masked_metrics():
    b, hw = 2, 301
    g = G(18)
    gt = torch.rand(b, hw, generator=g) * 100 - 5
    est = gt + torch.randn(b, hw, generator=g) * 2.5
    mask = torch.rand(b, hw, generator=g) > 0.3
    e, t = est.double(), gt.double()
    err = (t - e).abs()
    sums = torch.zeros(b, 8, dtype=torch.float64)
    for i in range(b):
        m = mask[i]
        sums[i] = torch.tensor([float(m.sum()), float((gt[i] > 0).sum()), float(err[i][m].sum()),
                                float(((err[i] > 3) & (err[i] / t[i].abs() > 0.05))[m].sum()), float((err[i] > 1)[m].sum()),
                                float((err[i] > 2)[m].sum()), float((err[i] > 3)[m].sum()), 0.0])
    # the mask is bytes: four to a word, padded to whole words so that it can live in an arena like the other operands
    m8 = torch.zeros(b * hw + (-b * hw) % 4, dtype=torch.uint8)
    m8[:b * hw] = mask.reshape(-1).to(torch.uint8)
    return Case({"est": est, "gt": gt, "mask": m8.view(torch.int32)}, {"sums": torch.empty(b, 8, dtype=torch.float64)},
                lambda lib, p, s: lib.dv_masked_metrics_f32(p("est"), p("gt"), p("mask"), p("sums"), b, hw, s), {"sums": sums},
                bar_close(1e-6 * hw, 0))


def _ddim_step(last):
    """The header's statement of one DDIM state update (acv_ddim.py:272-294, :318-362) in float64.  The kernel alone is held
    branch by branch, bit for bit and to float64 ulps, by test_gpu_ddim_kernels.py against the reference's own dtypes; this
    row is about the arena contract and keeps a float64 statement, whose bars come from the number formats:
    dq < 12 has a float32 ulp of 2^-20, the two-hot weight 2 * frac(dq) - 1 inherits at most 4 of them, and the bilinear
    /4 before it two roundings more: 1e-5 on x_start; pred_eps and x_next divide / scale that by coefficients <= 2: 2e-5.
    mask and ens are sums of a few float32 terms of size <= 1 / <= 50: 1e-6 and 1e-5."""
    def build():
        b, nbins, h, w = 2, 12, 4, 6
        g = G(19)
        H, W = 4 * h, 4 * w
        dq = _quarter_disparity(b, h, w, nbins, 20).view(b, 1, h, w)
        disp = (F.interpolate(dq, size=(H, W), mode="nearest") * 4).reshape(b, H, W).contiguous()   # its own down-sample gives dq back
        used = disp + torch.randn(b, H, W, generator=g) * 1.2
        unc = torch.rand(b, H, W, generator=g) * 5
        n01 = torch.rand(b, nbins, h, w, generator=g)
        eps = torch.randn(b, nbins, h, w, generator=g)
        fill = torch.rand(b, nbins, h, w, generator=g, dtype=torch.float64) * 2 - 1
        mask0 = (torch.rand(b, h, w, generator=g) > 0.6).float() * 0.5
        ens0 = torch.randn(b, H, W, generator=g)
        k = _lib.DvDdimCoef()
        k.sqrt_recip_alpha, k.sqrt_recipm1_alpha, k.sqrt_alpha_next, k.c, k.sigma = 1.6, 1.25, 0.8, 0.55, 0.25
        k.dif_thr, k.unc_thr, k.cof, k.last, k.clamp_max, k.ens_dif_thr = 1.0, 3.0, 0.3, int(last), float(4 * nbins - 1), 0.0
        down = lambda t: F.interpolate(t.unsqueeze(1), size=(h, w), mode="bilinear").squeeze(1)
        dq64 = down(disp.double().clamp(0, k.clamp_max)) / 4
        assert float((dq64 - dq64.round()).abs().min()) > 5e-4
        x_start = O.encode_two_hot(dq64.unsqueeze(1), nbins).double() * 2 - 1
        pred = (k.sqrt_recip_alpha * n01.double() - x_start) / k.sqrt_recipm1_alpha
        keep = down((((disp.double() - used.double()).abs() < k.dif_thr) & (unc.double() < k.unc_thr)).double())
        mask = (mask0.double() + keep).clamp(0, 1)
        x_next = torch.where(mask.unsqueeze(1) == 0, fill, x_start * k.sqrt_alpha_next + k.c * pred + k.sigma * eps.double())
        refs = {"x_start": x_start, "pred_eps": pred, "mask": mask, "ens": ens0.double() + 0.3 * disp.double()}
        outs = {"x_start": torch.empty(b, nbins, h, w), "pred_eps": torch.empty(b, nbins, h, w, dtype=torch.float64)}
        inputs = {"disp": disp, "unc": unc, "used": used, "n01_f32": n01}
        if not last:
            refs["x_next"] = x_next
            outs["x_next"] = torch.empty(b, nbins, h, w, dtype=torch.float64)
            inputs.update({"eps_f32": eps, "fill": fill})
        tol = {"x_start": 1e-5, "pred_eps": 2e-5, "x_next": 2e-5, "mask": 1e-6, "ens": 1e-5}

        def bar(name, got, ref):
            e = float((got.double() - ref).abs().max())
            print(f"    {name}: max abs err {e:.2e} (bar {tol[name]:.0e})")
            assert e <= tol[name], (name, e)
        return Case(inputs, outs,
                    lambda lib, p, s: lib.dv_ddim_step(p("disp"), p("unc"), p("used"), None, p("n01_f32"), None, p("eps_f32"), None,
                                                       p("fill"), p("mask"), p("x_start"), p("pred_eps"), p("x_next"), p("ens"), b,
                                                       nbins, h, w, ctypes.byref(k), s),
                    refs, bar, inout={"mask": mask0, "ens": ens0})
    return build


def _conv2d_f16(kind, cins, cout, hw, k=3, cout2=0, seed=97):
    """The fp16-autocast convolutions against `emulate` of test_gpu_conv2d_f16.py (operands rounded to fp16, float64 sum,
    every epilogue op rounded to fp16 again) and its `check`: inside the per-element bound the free accumulation order
    allows, at most 2 % of the outputs on the neighbouring fp16 value."""
    def build():
        from test_gpu_conv2d_f16 import check, emulate
        g = G(seed)
        b, (h, w) = 1, hw
        cin, ctot = sum(cins), cout + cout2
        r16 = lambda t: t.half().float()
        xs = [torch.randn(b, c, h, w, generator=g) for c in cins]
        wt = torch.randn(ctot, cin, k, k, generator=g) * (k * k * cin) ** -0.5
        bias = torch.randn(ctot, generator=g) * 0.1
        names = [f"in{i}" for i in range(len(xs))]
        inputs = dict(zip(names, xs))
        inputs["bias"] = bias
        chans = int_array(list(cins))
        rnd = lambda c, scale=1.0: r16(torch.randn(b, c, h, w, generator=g) * scale)
        if cout2 > 0:
            inputs.update({"residual1": rnd(cout, 0.5), "residual2": rnd(cout2, 0.5), "mul2": r16(torch.randn(b, cout2, h, w, generator=g).tanh())})
            emus = {"out1": emulate(xs, wt[:cout], bias[:cout], "sigmoid", residual=inputs["residual1"]),
                    "out2": emulate(xs, wt[cout:], bias[cout:], "sigmoid", residual=inputs["residual2"], mul=inputs["mul2"])}
        else:
            inputs.update({"residual": rnd(cout, 0.5), "blend_z": r16(torch.rand(b, cout, h, w, generator=g)),
                           "blend_h": r16(torch.randn(b, cout, h, w, generator=g).tanh())})
            emus = {"out": emulate(xs, wt, bias, "tanh", residual=inputs["residual"], blend=(inputs["blend_z"], inputs["blend_h"]))}
        refs = {n: e[0] for n, e in emus.items()}
        outs = {n: torch.empty(r.shape) for n, r in refs.items()}
        inout, ks = {}, {"n": 0}
        if kind.endswith("ksplit"):
            ks["n"] = _lib.load().dv_conv2d_f16_auto_kslices(cin, h, w, ctot, k)
            assert ks["n"] > 1, (cins, hw, ks["n"])
            inout["scratch"] = torch.zeros(ks["n"] * b * ctot * h * w)
        head = lambda p: (ptr_array(p, names), chans, len(names), p("wpacked"), p("bias"))
        calls = {
            "cat": lambda lib, p, s: lib.dv_conv2d_f16_cat(*head(p), p("residual"), p("mul"), p("blend_z"), p("blend_h"), p("out"), b, h,
                                                           w, cout, k, S.ACT_TANH, s),
            "cat_ksplit": lambda lib, p, s: lib.dv_conv2d_f16_cat_ksplit(*head(p), p("residual"), p("mul"), p("blend_z"), p("blend_h"),
                                                                         p("out"), p("scratch"), ks["n"], b, h, w, cout, k, S.ACT_TANH, s),
            "pair": lambda lib, p, s: lib.dv_conv2d_f16_cat_pair(*head(p), p("residual1"), p("mul1"), p("out1"), p("residual2"), p("mul2"),
                                                                 p("out2"), b, h, w, cout, cout2, S.ACT_SIGMOID, s),
            "pair_ksplit": lambda lib, p, s: lib.dv_conv2d_f16_cat_pair_ksplit(*head(p), p("residual1"), p("mul1"), p("out1"),
                                                                               p("residual2"), p("mul2"), p("out2"), p("scratch"), ks["n"],
                                                                               b, h, w, cout, cout2, S.ACT_SIGMOID, s),
        }
        return Case(inputs, outs, calls[kind], refs, lambda name, got, ref: check(got, emus[name]), inout=inout,
                    pack=lambda lib: {"wpacked": pack_through_abi(lib, "dv_conv2d_f16_packed_bytes", "dv_conv2d_f16_pack_weights", wt,
                                                                  cin, ctot, k, words_per=4)})
    return build


# ------------------------------------------------------------------ rows: training entries that choose a path by alignment
# (or refuse by it) and have no offset-view test of their own; references and bars are those of their own test modules
def _rel_l2_bar(f32, f64):
    """rel L2 against float64 <= 2 x that of the float32 torch expression + 1e-6 (tests/test_gpu_acv_train.py's convention)."""
    nrm = lambda a, r: float((a.double().reshape(-1) - r.double().reshape(-1)).norm() / r.double().reshape(-1).norm().clamp_min(1e-30))
    lims = {n: 2 * nrm(f32[n], f64[n]) + 1e-6 for n in f64}

    def bar(name, got, ref):
        e = nrm(got, ref)
        print(f"    {name}: relative L2 error {e:.2e} (bar {lims[name]:.2e})")
        assert e <= lims[name], (name, e, lims[name])
    return bar


def _feature_gate_bwd(shape):
    def build():
        from test_gpu_feature_gate_bwd import torch_grads
        gen = G(97)
        cv, g = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)
        logit = torch.randn(shape[0], shape[1], shape[3], shape[4], generator=gen) * 3
        r64, r32 = torch_grads(cv.double(), logit.double(), g.double()), torch_grads(cv, logit, g)
        b, c, d, h, w = shape
        nws = _lib.load().dv_feature_gate_bwd_workspace_floats(b, c, d, h, w)
        inout = {"workspace": torch.zeros(nws)} if nws else {}
        return Case({"cv": cv, "logit": logit, "g": g}, {"dcv": torch.empty(*shape), "dlogit": torch.empty(logit.shape)},
                    lambda lib, p, s: lib.dv_feature_gate_bwd_f32(p("cv"), p("logit"), p("g"), p("dcv"), p("dlogit"), p("workspace"),
                                                                  b, c, d, h, w, s),
                    {"dcv": r64[0], "dlogit": r64[1]}, _rel_l2_bar({"dcv": r32[0], "dlogit": r32[1]}, {"dcv": r64[0], "dlogit": r64[1]}),
                    inout=inout)
    return build


def _instance_norm_bwd(plane, act):
    def build():
        from test_gpu_igev_front_bwd import ACTS, in_torch
        x = torch.randn(2, 3, *plane, generator=G(61)) * 1.7 + 0.3
        cot = torch.randn(2, 3, *plane, generator=G(62))
        r64, r32 = in_torch(x, cot, act, torch.float64), in_torch(x, cot, act, torch.float32)
        hw = plane[0] * plane[1]
        return Case({"x": x, "g": cot}, {"dx": torch.empty(x.shape)},
                    lambda lib, p, s: lib.dv_instance_norm_act_bwd_f32(p("x"), p("g"), p("dx"), 6, hw, 1e-5, ACTS[act], s),
                    {"dx": r64["dx"]}, _rel_l2_bar({"dx": r32["dx"]}, {"dx": r64["dx"]}))
    return build


def _context_upsample_bwd(shape, softmax):
    def build():
        from test_gpu_context_upsample_bwd import inputs as cu_inputs, oracle_grads
        b, h, w = shape
        disp, wts, cot = cu_inputs(shape, softmax)
        _, d64, w64 = oracle_grads(disp, wts, cot, 4.0, softmax, torch.float64)
        _, d32, w32 = oracle_grads(disp, wts, cot, 4.0, softmax, torch.float32)
        return Case({"disp_low": disp, "weights": wts, "grad_out": cot},
                    {"d_weights": torch.empty(wts.shape), "d_disp": torch.empty(disp.shape)},
                    lambda lib, p, s: lib.dv_context_upsample_bwd_f32(p("disp_low"), p("weights"), p("grad_out"), p("d_weights"),
                                                                      p("d_disp"), p("cell_sums"), b, h, w, 4.0, int(softmax), s),
                    {"d_weights": w64, "d_disp": d64}, _rel_l2_bar({"d_weights": w32, "d_disp": d32}, {"d_weights": w64, "d_disp": d64}),
                    inout={"cell_sums": torch.zeros(b * 9 * h * w)})
    return build


# ------------------------------------------------------------------ rows: the split-K weight gradients of the training routes
# `workspace` is an OUTPUT of exactly *_workspace_floats(...) floats: the first kernel must write every word of it (the split
# sum reads them all back) and none next to it (production allocates exactly that many).  References and bars are those of
# the entries' own tests; a row's `claims` are the shape conditions it is there for, held from the size entry when it is built.
WGRAD_REQUIRED = {  # entry -> the conditions its rows must meet between them (tests/test_abi_arena_complete.py)
    "dv_conv3d_wgrad_f32": {"channel_tails", "channel_tiles", "plane_tails", "one_split", "ragged_splits"},
    "dv_deconv3d_k4s2_wgrad_f32": {"channel_tails", "plane_tails", "one_split", "ragged_splits"},
    "dv_conv2d_wgrad_f32": {"channel_tails", "channel_tiles", "plane_tails", "one_split", "ragged_splits"},
    "dv_conv2d_wgrad_cat_f32": {"channel_tails", "plane_tails", "one_split", "ragged_splits", "source_boundary", "k1", "k3"},
    "dv_conv2d_wgrad_cat_f16": {"channel_tails", "plane_tails", "one_split", "ragged_splits", "source_boundary", "k1", "k3"},
    "dv_conv2d_1in_wgrad_f32": {"channel_tails", "plane_tails"},       # no workspace, no splits: one block per (co, ky)
    "dv_deconv2d_k4s2_wgrad_f32": {"channel_tails", "plane_tails", "one_split", "ragged_splits"},
    "dv_conv2d_fewin_wgrad_f32": {"channel_tails", "plane_tails", "one_split", "ragged_splits"},
}
U24 = 2.0 ** -24


def wg_assert(claims, cout, cin, plane, brick, nbricks=1, splits=1, tile=0, bounds=(), k=0):
    """plane: the extents the bricks tile; tile: the block's channel tile where a second one is asked for; bounds: the first
    channels of the later sources of a concatenation."""
    facts = {
        "channel_tails": cout % 16 != 0 and cin % 16 != 0,
        "channel_tiles": tile > 0 and (cout > tile or cin > tile),
        "plane_tails": all(n % t != 0 for n, t in zip(plane, brick)),
        "one_split": splits == 1,
        "ragged_splits": splits >= 3 and nbricks % splits != 0,
        "source_boundary": any(o % 16 != 0 for o in bounds),
        "k1": k == 1,
        "k3": k == 3,
    }
    for c in claims:
        assert facts[c], f"the row no longer is a case of {c}: Cout {cout}, Cin {cin}, plane {tuple(plane)} in bricks of {brick}, " \
                         f"{nbricks} bricks over {splits} splits"


def bar_wgrad(mag, c):
    """Per element |dW - dW_f64| <= c * 2^-24 * sum |g x|: `mag` is that sum, c the depth_c / wgrad_c of the cited test."""
    def check(name, got, ref):
        err = (got.double() - ref).abs()
        print(f"    {name}: worst err / (u * mag) = {float((err / (mag * U24).clamp(min=1e-300)).max()):.1f} (c = {c})")
        assert torch.all(err <= c * U24 * mag), (name, c)
    return check


def wg_same_bits(operands, refused=()):
    """Variant (a) against every accepted displaced variant of a row without predicate operands: the sources promise that
    the bits depend on the shape only, so a path chosen by alignment would show here (labels as variants_of makes them)."""
    moved = [f"o:{n}" for n in operands if n not in refused]
    return tuple(("a", v) for v in moved + [f"c{k}" + ("-accepted" if refused else "") for k in (1, 2, 3)])


def _wg_conv3d(cin, cout, k, stride, b, dims, claims, seed=401):
    def build():
        from test_gpu_conv3d_wgrad import BRICK, depth_c, out_dims, ref_wgrad, split_plan
        gen = G(seed)
        out = out_dims(dims, k, stride)
        x, g = torch.randn(b, cin, *dims, generator=gen), torch.randn(b, cout, *out, generator=gen)
        nbricks, splits, _ = split_plan(b, cin, dims, cout, k, stride)
        wg_assert(claims, cout, cin, out, BRICK[(k, stride)], nbricks, splits, tile=32)
        nws = _lib.load().dv_conv3d_wgrad_workspace_floats(b, cin, *dims, cout, k, stride)
        assert nws == splits * cout * cin * k ** 3
        x64, g64 = x.double(), g.double()
        return Case({"x": x, "g": g}, {"dw": torch.empty(cout, cin, k, k, k), "workspace": torch.empty(nws)},
                    lambda lib, p, s: lib.dv_conv3d_wgrad_f32(p("x"), p("g"), p("dw"), p("workspace"), b, cin, *dims, cout, k, stride, s),
                    {"dw": ref_wgrad(x64, g64, k, stride)},
                    bar_wgrad(ref_wgrad(x64.abs(), g64.abs(), k, stride), depth_c(b, cin, dims, cout, k, stride)))
    build.claims = claims
    return build


def _wg_deconv3d_k4(ci, co, b, dims, claims, seed=402):
    def build():
        from test_gpu_deconv3d_k4_bwd import BRICK, f64_backward, split_plan, wgrad_c
        gen = G(seed)
        x, g = torch.randn(b, ci, *dims, generator=gen), torch.randn(b, co, *[2 * n for n in dims], generator=gen)
        nbricks, splits, _ = split_plan(ci, co, b, dims)
        wg_assert(claims, co, ci, dims, BRICK, nbricks, splits)
        nws = _lib.load().dv_deconv3d_k4s2_wgrad_workspace_floats(b, ci, *dims, co)
        assert nws == splits * ci * co * 64
        w0 = torch.zeros(ci, co, 4, 4, 4)                 # dW does not depend on the weights
        return Case({"x": x, "g": g}, {"dw": torch.empty(ci, co, 4, 4, 4), "workspace": torch.empty(nws)},
                    lambda lib, p, s: lib.dv_deconv3d_k4s2_wgrad_f32(p("x"), p("g"), p("dw"), p("workspace"), b, ci, *dims, co, s),
                    {"dw": f64_backward(x, w0, g)[1]}, bar_wgrad(f64_backward(x.abs(), w0, g.abs())[1], wgrad_c(ci, co, b, dims)))
    build.claims = claims
    return build


def _wg_conv2d(cin, cout, k, dil, b, h, w, claims, seed=403):
    def build():
        from test_gpu_conv2d_wgrad import brick, depth_c, ref_wgrad
        gen = G(seed)
        x, g = torch.randn(b, cin, h, w, generator=gen), torch.randn(b, cout, h, w, generator=gen)
        nws = _lib.load().dv_conv2d_wgrad_workspace_floats(b, cin, h, w, cout, k, dil)
        ty, tx = brick(k, dil)
        nbricks, splits = b * -(-h // ty) * -(-w // tx), nws // (cout * cin * k * k)
        assert nws > 0 and nws == splits * cout * cin * k * k
        wg_assert(claims, cout, cin, (h, w), (ty, tx), nbricks, splits, tile=32)
        x64, g64 = x.double(), g.double()
        return Case({"x": x, "g": g}, {"dw": torch.empty(cout, cin, k, k), "workspace": torch.empty(nws)},
                    lambda lib, p, s: lib.dv_conv2d_wgrad_f32(p("x"), p("g"), p("dw"), p("workspace"), b, cin, h, w, cout, k, dil, s),
                    {"dw": ref_wgrad(x64, g64, k, dil)}, bar_wgrad(ref_wgrad(x64.abs(), g64.abs(), k, dil), depth_c(b, cin, h, w, cout, k, dil)))
    build.claims = claims
    return build


def _wg_conv2d_cat(f16, chans, cout, k, b, h, w, claims, seed=404):
    def build():
        from test_gpu_conv2d_wgrad_cat import ref_wgrad
        if f16:          # the contract of the fp16 entry: the float64 gradient of the operands rounded to fp16
            from test_gpu_conv2d_wgrad_cat_f16 import TX, TY, depth_c, splits_of
            rnd, entry = (lambda t: t.half().double()), "dv_conv2d_wgrad_cat_f16"
        else:
            from test_gpu_conv2d_wgrad_cat import TX, TY, depth_c, splits_of
            rnd, entry = (lambda t: t.double()), "dv_conv2d_wgrad_cat_f32"
        gen = G(seed)
        cin = sum(chans)
        xs = [torch.randn(b, c, h, w, generator=gen) for c in chans]
        g = torch.randn(b, cout, h, w, generator=gen)
        splits = splits_of(chans, b, h, w, cout, k)                        # the size entry over numel(dW), checked to be whole
        nws = splits * cout * cin * k * k
        bounds = [sum(chans[:i]) for i in range(1, len(chans))]
        wg_assert(claims, cout, cin, (h, w), (TY, TX), b * -(-h // TY) * -(-w // TX), splits, bounds=bounds, k=k)
        names = [f"in{i}" for i in range(len(xs))]
        x64, g64 = torch.cat([rnd(t) for t in xs], dim=1), rnd(g)
        inputs = dict(zip(names, xs))
        inputs["g"] = g
        return Case(inputs, {"dw": torch.empty(cout, cin, k, k), "workspace": torch.empty(nws)},
                    lambda lib, p, s: getattr(lib, entry)(ptr_array(p, names), int_array(list(chans)), len(names), p("g"), p("dw"),
                                                          p("workspace"), b, h, w, cout, k, s),
                    {"dw": ref_wgrad(x64, g64, k)}, bar_wgrad(ref_wgrad(x64.abs(), g64.abs(), k), depth_c(chans, b, h, w, cout, k)))
    build.claims = claims
    return build


def _wg_conv2d_1in(cout, b, h, w, claims, seed=405):
    def build():
        k = 7
        gen = G(seed)
        x, g = torch.randn(b, 1, h, w, generator=gen), torch.randn(b, cout, h, w, generator=gen)
        wg_assert(claims, cout, 1, (b * h * w,), (256,))            # no bricks: the 256 threads stride over all B H W positions
        ref = torch.nn.grad.conv2d_weight(x.double(), (cout, 1, k, k), g.double(), padding=k // 2)
        mag = torch.nn.grad.conv2d_weight(x.double().abs(), (cout, 1, k, k), g.double().abs(), padding=k // 2)
        return Case({"x": x, "g": g}, {"dw": torch.empty(cout, 1, k, k)},
                    lambda lib, p, s: lib.dv_conv2d_1in_wgrad_f32(p("x"), p("g"), p("dw"), b, h, w, cout, k, s),
                    {"dw": ref}, bar_wgrad(mag, -(-b * h * w // 256) + 8))        # a chain of ceil(BHW / 256), then an 8-level tree
    build.claims = claims
    return build


def _wg_deconv2d_k4(ci, co, b, h, w, claims):
    """Bar of test_gradients_match_float64_autograd ("dw"): relative L2 <= 2 x that of float32 torch + 1e-6."""
    def build():
        from test_gpu_deconv2d_k4_bwd import inputs as k4_inputs, torch_grads
        x, wt, bias, cot = k4_inputs(ci, co, h, w, b)
        nws = _lib.load().dv_deconv2d_k4s2_wgrad_workspace_floats(b, ci, h, w, co)
        nbricks, splits = b * -(-h // 4) * -(-w // 16), nws // (ci * co * 16)        # bricks of 4 x 16 pixels of x
        assert nws > 0 and nws == splits * ci * co * 16
        wg_assert(claims, co, ci, (h, w), (4, 16), nbricks, splits)
        r64, r32 = torch_grads(x, wt, bias, cot, torch.float64)["dw"], torch_grads(x, wt, bias, cot, torch.float32)["dw"]
        return Case({"x": x, "g": cot}, {"dw": torch.empty(ci, co, 4, 4), "workspace": torch.empty(nws)},
                    lambda lib, p, s: lib.dv_deconv2d_k4s2_wgrad_f32(p("x"), p("g"), p("dw"), p("workspace"), b, ci, h, w, co, s),
                    {"dw": r64}, _rel_l2_bar({"dw": r32}, {"dw": r64}))
    build.claims = claims
    return build


def _wg_fewin(cin, k, stride, cout, b, h, w, claims):
    """Bar of test_fewin_weight_gradient ("dw"): relative L2 <= 2 x that of float32 torch + 1e-6."""
    def build():
        from test_gpu_igev_front_bwd import conv_inputs, conv_torch
        x, wt, bias, cot = conv_inputs(cin, cout, k, stride, h, w, b, 62)
        ho, wo = cot.shape[2:]
        nws = _lib.load().dv_conv2d_fewin_wgrad_workspace_floats(b, cin, h, w, cout, k, stride)
        nbricks, splits = b * -(-ho // 8) * -(-wo // 16), nws // (cout * cin * k * k)  # bricks of 8 x 16 output pixels
        assert nws > 0 and nws == splits * cout * cin * k * k
        wg_assert(claims, cout, cin, (ho, wo), (8, 16), nbricks, splits)
        r64 = conv_torch(x, wt, bias, cot, stride, torch.float64, False)["dw"]
        r32 = conv_torch(x, wt, bias, cot, stride, torch.float32, False)["dw"]
        return Case({"x": x, "g": cot}, {"dw": torch.empty(cout, cin, k, k), "workspace": torch.empty(nws)},
                    lambda lib, p, s: lib.dv_conv2d_fewin_wgrad_f32(p("x"), p("g"), p("dw"), p("workspace"), b, cin, h, w, cout, k,
                                                                    stride, s),
                    {"dw": r64}, _rel_l2_bar({"dw": r32}, {"dw": r64}))
    build.claims = claims
    return build


# ------------------------------------------------------------------ the table
WP = {"wpacked": (ERR_ALIGN, 16)}
R = Row
TABLE = [
    # cost-volume builders: the ragged plane of test_gwc_oracle / test_concat_oracle and a W % 4 == 0 one
    R("gwc_ragged", "dv_gwc_volume_f32", _gwc((1, 24, 3, 78, 12, 2)), "test_gwc_oracle", pred=("ref", "tgt", "out")),
    R("gwc_quads", "dv_gwc_volume_f32", _gwc((2, 24, 3, 80, 12, 2)), "test_gwc_oracle", pred=("ref", "tgt", "out")),
    R("concat_ragged", "dv_concat_volume_f32", _concat((1, 12, 3, 39, 6), False), "test_concat_oracle", pred=("ref", "tgt", "out")),
    R("concat_quads", "dv_concat_volume_f32", _concat((2, 12, 3, 40, 6), False), "test_concat_oracle", pred=("ref", "tgt", "out")),
    R("concat_quads_zero_left", "dv_concat_volume_f32", _concat((1, 12, 3, 40, 6), True), "test_concat_oracle", pred=("ref", "tgt", "out")),
    R("concat_attn_quads", "dv_concat_attn_volume_f32", _concat_att((1, 12, 3, 40, 6), False), "test_concat_attention",
      pred=("ref", "tgt", "att", "out")),
    R("concat_attn_ragged", "dv_concat_attn_volume_f32", _concat_att((1, 12, 3, 39, 6), False), "test_concat_attention",
      pred=("ref", "tgt", "att", "out")),
    R("concat_prob_quads", "dv_concat_prob_volume_f32", _concat_att((1, 12, 3, 40, 6), True), "test_concat_attention",
      pred=("ref", "tgt", "att", "out")),
    R("patch_quads", "dv_patch_volume_f32", _patch((2, 40, 2, 17, 12), False), "test_patch_volume_vs_pytorch_depthwise", pred=("gwc", "out")),
    R("patch_runs_quads", "dv_patch_volume_runs_f32", _patch((2, 40, 2, 17, 12), True), "test_patch_volume_vs_pytorch_depthwise",
      pred=("gwc", "out")),
    R("patch_runs_wide", "dv_patch_volume_runs_f32", _patch((1, 40, 1, 5, 140), True), "test_patch_volume_vs_pytorch_depthwise",
      pred=("gwc", "out")),
    R("patch_runs_ragged", "dv_patch_volume_runs_f32", _patch((1, 40, 2, 9, 50), True), "test_patch_volume_vs_pytorch_depthwise",
      pred=("gwc", "out")),
    # the rank-1 first layer
    R("pointwise_quads", "dv_pointwise_expand_f32", _pointwise((2, 8, 162, 4, 9)), "test_table_convolution_vs_torch", pred=("out",),
      aligned=("wpacked",), refuse=WP),
    R("pointwise_ragged", "dv_pointwise_expand_f32", _pointwise((1, 8, 162, 5, 7)), "test_table_convolution_vs_torch", pred=("out",),
      aligned=("wpacked",), refuse=WP),
    R("softmax_d", "dv_softmax_d_f32", _softmax_d, "test_rank1_filter_layer_vs_oracle_and_generic_conv", variants="ac"),
    R("mul", "dv_mul_f32", _mul, "test_rank1_filter_layer_vs_oracle_and_generic_conv", variants="ac"),
    R("rank1_quads", "dv_conv3d_rank1_filter_f32", _rank1((1, 8, 7, 12, 4, 12)), "test_rank1_filter_layer_vs_oracle_and_generic_conv",
      variants="ac"),
    R("rank1_ragged", "dv_conv3d_rank1_filter_f32", _rank1((1, 8, 6, 12, 4, 9)), "test_rank1_filter_layer_vs_oracle_and_generic_conv",
      variants="ac"),
    R("noise_prepare_f32", "dv_noise_prepare_f32", _noise_prepare(False), "test_aggregation_cost_parity", variants="ac"),
    R("noise_prepare_f64", "dv_noise_prepare_f64", _noise_prepare(True), "test_aggregation_cost_parity", variants="ac"),
    # 3-D convolutions: a full interior tile next to a ragged one, both branches of the epilogue's vector-store predicate
    R("conv3d_k3_fast", "dv_conv3d_f32", _conv3d("direct", 8, 32, (1, 4, 8, 32)), "test_conv_oracle", pred=("out", "residual"),
      aligned=("wpacked",), refuse=WP),
    R("conv3d_k3_partial", "dv_conv3d_f32", _conv3d("direct", 8, 32, (1, 5, 7, 36), in_scale=True), "test_conv_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_k3_ragged", "dv_conv3d_f32", _conv3d("direct", 6, 20, (1, 3, 5, 30), in_scale=True), "test_conv_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_k1", "dv_conv3d_f32", _conv3d("direct", 32, 32, (1, 4, 8, 16), k=1, act=S.ACT_NONE), "test_conv_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_k3s2", "dv_conv3d_f32", _conv3d("direct", 8, 16, (1, 8, 9, 16), stride=2), "test_conv_oracle", pred=("out", "residual"),
      aligned=("wpacked",), refuse=WP),
    R("conv3d_k3s2_ragged", "dv_conv3d_f32", _conv3d("direct", 8, 16, (1, 8, 9, 13), stride=2), "test_conv_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_head", "dv_conv3d_f32", _conv3d("direct", 5, 1, (1, 3, 5, 8), in_scale=True), "test_conv_single_channel_head_edges",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    # the z-marching form of the head (three planes per block) and both tilings of the direct stride-2 kernel, pinned by the
    # library's test hooks as test_conv_single_channel_head_z_march / test_stride2_tilings_give_the_same_bits pin them
    R("conv3d_head_z_march", "dv_conv3d_f32", _conv3d("direct", 7, 1, (1, 7, 9, 68), seed=29, hook=("dv_conv3d_set_c1z", (1, 3))),
      "test_conv_single_channel_head_z_march", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_k3s2_big_tiles", "dv_conv3d_f32", _conv3d("direct", 16, 64, (1, 4, 8, 64), stride=2, seed=191,
                                                       hook=("dv_conv3d_set_s2_tile", (1,))),
      "test_stride2_tilings_give_the_same_bits", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_k3s2_small_tiles", "dv_conv3d_f32", _conv3d("direct", 16, 64, (1, 6, 9, 37), stride=2, seed=191,
                                                         hook=("dv_conv3d_set_s2_tile", (2,))),
      "test_stride2_tilings_give_the_same_bits", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_f16x3", "dv_conv3d_f16x3_f32", _conv3d("f16x3", 8, 32, (1, 2, 4, 96), in_scale=True, seed=17, xgain=3.0),
      "test_conv_f16x3_oracle", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_f16x3_ragged", "dv_conv3d_f16x3_f32", _conv3d("f16x3", 32, 16, (1, 3, 9, 30), in_scale=True, seed=17, xgain=3.0),
      "test_conv_f16x3_oracle", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_wino", "dv_conv3d_wino_f32", _conv3d("wino", 8, 16, (1, 5, 6, 20), act=S.ACT_LEAKY, in_scale=True, seed=31),
      "test_conv_winograd_edges", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_wino_ragged", "dv_conv3d_wino_f32", _conv3d("wino", 5, 20, (2, 5, 7, 19), act=S.ACT_LEAKY, in_scale=True, seed=31),
      "test_conv_winograd_edges", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv3d_wino3", "dv_conv3d_wino3_f32", _conv3d("wino3", 8, 32, (1, 6, 8, 16), seed=97),
      "test_wino3_vs_float64_and_the_in_plane_kernel", pred=("out", "residual"), aligned=("wpacked",),
      refuse={"wpacked": (ERR_ALIGN, 16), "in": (ERR_ALIGN, 16)}),
    R("conv3d_wino3_64ch", "dv_conv3d_wino3_f32", _conv3d("wino3", 64, 64, (1, 3, 7, 12), seed=97),
      "test_wino3_vs_float64_and_the_in_plane_kernel", pred=("out", "residual"), aligned=("wpacked",),
      refuse={"wpacked": (ERR_ALIGN, 16), "in": (ERR_ALIGN, 16)}),
    R("conv3d_s2pp_one_quad", "dv_conv3d_s2pp_f32", _conv3d("s2pp", 4, 64, (1, 1, 1, 4), stride=2, seed=41), "test_s2pp_vs_torch_and_direct",
      pred=("out", "residual"), aligned=("wpacked",), refuse={"wpacked": (ERR_ALIGN, 16), "in": (ERR_ALIGN, 16)}),
    R("conv3d_s2pp", "dv_conv3d_s2pp_f32", _conv3d("s2pp", 5, 64, (1, 3, 5, 8), stride=2, seed=41), "test_s2pp_vs_torch_and_direct",
      pred=("out", "residual"), aligned=("wpacked",), refuse={"wpacked": (ERR_ALIGN, 16), "in": (ERR_ALIGN, 16)}),
    R("conv3d_s2pp_odd_wo", "dv_conv3d_s2pp_f32", _conv3d("s2pp", 8, 64, (1, 4, 9, 12), stride=2, seed=41), "test_s2pp_vs_torch_and_direct",
      pred=("out", "residual"), aligned=("wpacked",), refuse={"wpacked": (ERR_ALIGN, 16), "in": (ERR_ALIGN, 16)}),
    R("deconv3d_k3_one_tile", "dv_deconv3d_k3s2_f32", _deconv3d(3, 16, 32, (1, 2, 4, 32), S.ACT_RELU, impl=1), "test_deconv_oracle",
      pred=("in", "out", "residual"), aligned=("wpacked",), refuse=WP),
    R("deconv3d_k3_persistent", "dv_deconv3d_k3s2_f32", _deconv3d(3, 16, 32, (1, 2, 4, 32), S.ACT_RELU, impl=2),
      "test_persistent_vs_torch_and_one_tile", pred=("in", "out", "residual"), aligned=("wpacked",), refuse=WP),
    R("deconv3d_k3_default", "dv_deconv3d_k3s2_f32", _deconv3d(3, 16, 32, (1, 2, 4, 32), S.ACT_RELU, impl=0, residual=False),
      "test_persistent_vs_torch_and_one_tile", pred=("in", "out"), aligned=("wpacked",), refuse=WP),
    R("deconv3d_k3_ragged", "dv_deconv3d_k3s2_f32", _deconv3d(3, 16, 8, (1, 2, 3, 7), S.ACT_RELU), "test_deconv_oracle",
      pred=("in", "out", "residual"), aligned=("wpacked",), refuse=WP),
    R("deconv3d_k4", "dv_deconv3d_k4s2_f32", _deconv3d(4, 16, 8, (1, 4, 6, 32), S.ACT_LEAKY, seed=21), "test_deconv_k4_oracle",
      pred=("in", "out", "residual"), aligned=("wpacked",), refuse=WP),
    R("deconv3d_k4_ragged", "dv_deconv3d_k4s2_f32", _deconv3d(4, 32, 16, (2, 2, 5, 13), S.ACT_LEAKY, seed=21), "test_deconv_k4_oracle",
      pred=("in", "out", "residual"), aligned=("wpacked",), refuse=WP),
    R("redir_one_tile", "dv_deconv3d_k3s2_redir_f32", _redir(16, 32, 8, (1, 2, 4, 32), S.ACT_RELU, impl=1), "test_deconv_fused_redir",
      pred=("in", "out"), aligned=("wpacked",), refuse={"wpacked": (ERR_ALIGN, 16), "skip": (ERR_UNSUPPORTED, 16)}),
    R("redir_persistent", "dv_deconv3d_k3s2_redir_f32", _redir(16, 32, 8, (1, 2, 4, 32), S.ACT_RELU, impl=2),
      "test_persistent_vs_torch_and_one_tile", pred=("in", "out"), aligned=("wpacked",),
      refuse={"wpacked": (ERR_ALIGN, 16), "skip": (ERR_UNSUPPORTED, 16)}),
    R("redir_ragged", "dv_deconv3d_k3s2_redir_f32", _redir(64, 32, 32, (1, 2, 3, 18), S.ACT_MISH, impl=1), "test_deconv_fused_redir",
      pred=("in", "out"), aligned=("wpacked",), refuse={"wpacked": (ERR_ALIGN, 16), "skip": (ERR_UNSUPPORTED, 16)}),
    # 2-D convolutions
    R("conv2d_quads", "dv_conv2d_f32", _conv2d("plain", (32,), 1, (12, 80)), "test_conv2d_oracle", pred=("out",), aligned=("wpacked",),
      refuse=WP),
    R("conv2d_dilated_ragged", "dv_conv2d_f32", _conv2d("plain", (20,), 24, (10, 33), dil=3, act=S.ACT_RELU, residual=True),
      "test_conv2d_oracle", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv2d_dilated_quads", "dv_conv2d_f32", _conv2d("plain", (20,), 24, (10, 36), b=2, dil=3, act=S.ACT_MISH, residual=True),
      "test_conv2d_oracle", pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv2d_k1", "dv_conv2d_f32", _conv2d("plain", (24,), 40, (9, 68), k=1), "test_conv2d_oracle", pred=("out",), aligned=("wpacked",),
      refuse=WP),
    R("conv2d_d16", "dv_conv2d_f32", _conv2d("plain", (8,), 32, (20, 40), dil=16, residual=True), "test_conv2d_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv2d_gated", "dv_conv2d_gated_f32", _conv2d("gated", (40,), 32, (11, 72), b=2, act=S.ACT_TANH, residual=True, mul=True, blend=True,
                                                     bar=bar_close(4e-6, 1e-5), seed=111),
      "test_conv2d_gate_epilogues", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("conv2d_gated_ragged", "dv_conv2d_gated_f32", _conv2d("gated", (40,), 32, (11, 70), b=2, act=S.ACT_SIGMOID, residual=True, mul=True,
                                                            blend=True, bar=bar_close(4e-6, 1e-5), seed=111),
      "test_conv2d_gate_epilogues", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("conv2d_cat", "dv_conv2d_cat_f32", _conv2d("cat", (20, 6, 38), 32, (9, 72), b=2, act=S.ACT_RELU, bar=bar_close(2e-6, 1e-5), seed=151),
      "test_conv2d_over_virtual_concatenation", pred=("out",), aligned=("wpacked",), refuse=WP),
    R("conv2d_cat_ragged", "dv_conv2d_cat_f32", _conv2d("cat", (20, 6, 38), 32, (9, 70), b=2, act=S.ACT_RELU, residual=True, mul=True,
                                                        blend=True, seed=151),
      "test_conv2d_source_queue_edge_cases", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("conv2d_cat_ksplit", "dv_conv2d_cat_ksplit_f32", _conv2d("cat_ksplit", (64,), 32, (12, 40), act=S.ACT_RELU, residual=True, mul=True,
                                                               blend=True, seed=57),
      "test_conv2d_ksplit_small_launches", pred=("out", "residual", "mul", "blend_z", "blend_h", "scratch"), aligned=("wpacked",), refuse=WP),
    R("conv2d_cat_ksplit_ragged", "dv_conv2d_cat_ksplit_f32", _conv2d("cat_ksplit", (40, 24), 48, (9, 33), residual=True, mul=True,
                                                                      blend=True, seed=57),
      "test_conv2d_ksplit_small_launches", pred=("out", "residual", "mul", "blend_z", "blend_h", "scratch"), aligned=("wpacked",), refuse=WP),
    R("conv2d_s2", "dv_conv2d_s2_f32", _conv2d("s2", (64,), 128, (24, 64), residual=True, seed=61), "test_conv2d_stride2_oracle",
      pred=("out", "residual"), aligned=("wpacked",), refuse=WP),
    R("conv2d_s2_ragged", "dv_conv2d_s2_f32", _conv2d("s2", (32,), 64, (17, 70), act=S.ACT_RELU, seed=61), "test_conv2d_stride2_oracle",
      pred=("out",), aligned=("wpacked",), refuse=WP),
    R("conv2d_s2_k1", "dv_conv2d_s2_f32", _conv2d("s2", (32,), 64, (16, 130), k=1, seed=61), "test_conv2d_stride2_oracle", pred=("out",),
      aligned=("wpacked",), refuse=WP),
    R("wino2d", "dv_conv2d_wino_cat_f32", _conv2d("wino", (8,), 32, (16, 16), b=2, residual=True, mul=True, blend=True,
                                                  bar=bar_close(2e-5, 1e-5), seed=41),
      "test_conv2d_winograd", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_ragged", "dv_conv2d_wino_cat_f32", _conv2d("wino", (5, 7), 20, (9, 21), b=2, act=S.ACT_TANH, residual=True, mul=True,
                                                         blend=True, bar=bar_close(2e-5, 1e-5), seed=41),
      "test_conv2d_winograd", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_tiles", "dv_conv2d_wino_cat_f32", _conv2d("wino", (32, 16, 8, 8), 48, (24, 40), b=2, act=S.ACT_SIGMOID, residual=True,
                                                        mul=True, blend=True, bar=bar_close(2e-5, 1e-5), seed=41),
      "test_conv2d_winograd", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_dil", "dv_conv2d_wino_dil_cat_f32", _conv2d("wino_dil", (8,), 32, (16, 16), b=2, dil=2, residual=True, mul=True, blend=True,
                                                          bar=bar_close(2e-5, 1e-5), seed=43),
      "test_conv2d_winograd_dilated", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_dil_ragged", "dv_conv2d_wino_dil_cat_f32", _conv2d("wino_dil", (5, 7), 20, (19, 41), b=2, dil=3, act=S.ACT_TANH,
                                                                 residual=True, mul=True, blend=True, bar=bar_close(2e-5, 1e-5), seed=43),
      "test_conv2d_winograd_dilated", pred=("out", "residual", "mul", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_pair", "dv_conv2d_wino_cat_pair_f32", _conv2d("wino_pair", (16, 8), 32, (24, 40), b=2, act=S.ACT_SIGMOID, cout2=48, seed=31),
      "test_gru_gate_pair_launch_equals_the_two_convolutions", pred=("out1", "residual1"), aligned=("wpacked",),
      refuse={"wpacked": (ERR_ALIGN, 16), "residual2": (ERR_ALIGN, 16), "mul2": (ERR_ALIGN, 16), "out2": (ERR_ALIGN, 16)}),
    R("wino2d_pair_ragged", "dv_conv2d_wino_cat_pair_f32", _conv2d("wino_pair", (16, 8), 32, (23, 50), act=S.ACT_SIGMOID, cout2=48, seed=31),
      "test_gru_gate_pair_launch_equals_the_two_convolutions", pred=("out1", "residual1"), aligned=("wpacked",),
      refuse={"wpacked": (ERR_ALIGN, 16), "residual2": (ERR_ALIGN, 16), "mul2": (ERR_ALIGN, 16), "out2": (ERR_ALIGN, 16)}),
    R("wino2d_ksplit", "dv_conv2d_wino_cat_ksplit_f32", _conv2d("wino_ksplit", (256,), 128, (20, 36), act=S.ACT_TANH, residual=True,
                                                                blend=True, seed=91),
      "test_winograd_ksplit_small_launches", pred=("out", "residual", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_ksplit_ragged", "dv_conv2d_wino_cat_ksplit_f32", _conv2d("wino_ksplit", (130, 61, 3), 128, (24, 78), act=S.ACT_TANH,
                                                                       residual=True, blend=True, seed=91),
      "test_winograd_ksplit_small_launches", pred=("out", "residual", "blend_z", "blend_h"), aligned=("wpacked",), refuse=WP),
    R("wino2d_pair_ksplit", "dv_conv2d_wino_cat_pair_ksplit_f32", _conv2d("wino_pair_ksplit", (256,), 128, (20, 36), act=S.ACT_SIGMOID,
                                                                          cout2=128, seed=91),
      "test_winograd_ksplit_small_launches", pred=("out1", "residual1", "out2", "residual2", "mul2"), aligned=("wpacked",), refuse=WP),
    R("wino2d_s2b", "dv_conv2d_wino_s2b_f32", _conv2d("wino_s2b", (8,), 32, (16, 24), b=2, act=S.ACT_MISH, seed=321),
      "test_refinement_in_the_sub_image_domain", pred=("out",), aligned=("wpacked",), refuse=WP),
    R("wino2d_s2b_half_quads", "dv_conv2d_wino_s2b_f32", _conv2d("wino_s2b", (5, 7), 20, (10, 22), act=S.ACT_MISH, seed=321),
      "test_refinement_in_the_sub_image_domain", pred=("out",), aligned=("wpacked",), refuse=WP),
    R("refine_inputs", "dv_refine_inputs_f32", _refine_inputs((1, 20, 5, 40)), "test_refine_inputs_vs_oracle", variants="ac"),
    R("refine_inputs_ragged", "dv_refine_inputs_f32", _refine_inputs((2, 32, 7, 34)), "test_refine_inputs_vs_oracle", variants="ac"),
    R("space_to_batch2", "dv_space_to_batch2_f32", _space_to_batch, "test_refinement_in_the_sub_image_domain", pred=("out",),
      refuse={"in": (ERR_ALIGN, 8)}),
    R("batch_to_space", "dv_batch_to_space_f32", _batch_to_space, "test_refinement_in_the_sub_image_domain", variants="ac"),
    # IGEV
    R("feature_gate_quads", "dv_feature_gate_f32", _feature_gate((2, 8, 5, 6, 10)), "test_feature_gate", pred=("cv", "logit", "out")),
    R("feature_gate_ragged", "dv_feature_gate_f32", _feature_gate((1, 48, 3, 5, 7)), "test_feature_gate", pred=("cv", "logit", "out")),
    R("window_attn", "dv_window_attn3d_f32", _window_attn((1, 128, 8, 4, 8)), "test_window_attention_vs_float64", pred=("out",),
      aligned=("qkv_w", "proj_w"), refuse={"qkv_w": (ERR_ALIGN, 16), "proj_w": (ERR_ALIGN, 16)}),
    R("window_attn_padded", "dv_window_attn3d_f32", _window_attn((2, 128, 4, 6, 20)), "test_window_attention_vs_float64", pred=("out",),
      aligned=("qkv_w", "proj_w"), refuse={"qkv_w": (ERR_ALIGN, 16), "proj_w": (ERR_ALIGN, 16)}),
    R("window_attn_masked", "dv_window_attn3d_f32", _window_attn((2, 128, 4, 5, 7)), "test_window_attention_vs_float64", pred=("out",),
      aligned=("qkv_w", "proj_w"), refuse={"qkv_w": (ERR_ALIGN, 16), "proj_w": (ERR_ALIGN, 16)}),
    R("allpairs_corr", "dv_allpairs_corr_f32", _allpairs((1, 24, 3, 40, 40)), "test_igev_allpairs_corr_oracle", variants="ac"),
    R("allpairs_corr_ragged", "dv_allpairs_corr_f32", _allpairs((1, 7, 2, 17, 33)), "test_igev_allpairs_corr_oracle", variants="ac"),
    R("geo_lookup", "dv_geo_filter_lookup_f32", _geo_lookup(48, 40, False), "test_igev_geo_filter_lookup_window_edges", pred=("noisy",),
      same_bits=(("a", "b:noisy"),)),
    R("geo_lookup_odd_d", "dv_geo_filter_lookup_f32", _geo_lookup(13, 21, False), "test_igev_geo_filter_lookup_window_edges",
      pred=("noisy",), same_bits=(("a", "b:noisy"),)),
    R("geo_lookup_conv1x1", "dv_geo_filter_lookup_conv1x1_f32", _geo_lookup(48, 40, True),
      "test_igev_geo_lookup_fused_with_its_1x1_convolution", aligned=("wpacked",), variants="ac"),
    R("geo_lookup_conv1x1_odd_d", "dv_geo_filter_lookup_conv1x1_f32", _geo_lookup(13, 21, True),
      "test_igev_geo_lookup_fused_with_its_1x1_convolution", aligned=("wpacked",), variants="ac"),
    R("context_upsample_softmax", "dv_context_upsample_f32", _context_upsample((2, 5, 7), True), "test_gradients_match_float64_autograd",
      variants="ac", refuse={"weights": (ERR_ALIGN, 16), "out": (ERR_ALIGN, 16)}),
    R("context_upsample_plain", "dv_context_upsample_f32", _context_upsample((1, 2, 70), False), "test_gradients_match_float64_autograd",
      variants="ac", refuse={"weights": (ERR_ALIGN, 16), "out": (ERR_ALIGN, 16)}),
    R("conv2d_1in_f32", "dv_conv2d_1in_f32", _conv2d_1in(False), "test_update_glue_kernels_vs_torch", variants="ac"),
    R("conv2d_1in_f16", "dv_conv2d_1in_f16", _conv2d_1in(True), "test_update_block_call_vs_reference_autocast", variants="ac"),
    R("resize_quads", "dv_resize_bilinear_ac_f32", _resize((14, 20)), "test_update_glue_kernels_vs_torch", pred=("out",)),
    R("resize_ragged", "dv_resize_bilinear_ac_f32", _resize((13, 19)), "test_update_glue_kernels_vs_torch", pred=("out",)),
    R("avg_pool", "dv_avg_pool3s2_f32", _avg_pool, "test_update_glue_kernels_vs_torch", variants="ac"),
    R("fewin_stem", "dv_conv2d_fewin_f32", _fewin(3, 64, 7, 2, 37, 50), "test_front_kernels_vs_torch", variants="ac"),
    R("fewin_k5", "dv_conv2d_fewin_f32", _fewin(1, 16, 5, 1, 9, 20), "test_front_kernels_vs_torch", variants="ac"),
    R("instance_norm", "dv_instance_norm_act_f32", _instance_norm, "test_front_kernels_vs_torch", variants="ac"),
    R("f16_cat", "dv_conv2d_f16_cat", _conv2d_f16("cat", (20, 6, 38), 32, (48, 80)), "test_gate_chains", variants="ac", aligned=("wpacked",)),
    R("f16_cat_ksplit", "dv_conv2d_f16_cat_ksplit", _conv2d_f16("cat_ksplit", (128, 128), 128, (12, 40)), "test_ksplit_small_launches",
      variants="ac", aligned=("wpacked",)),
    R("f16_pair", "dv_conv2d_f16_cat_pair", _conv2d_f16("pair", (24, 40), 32, (48, 78), cout2=48), "test_gate_chains", variants="ac",
      aligned=("wpacked",)),
    R("f16_pair_ksplit", "dv_conv2d_f16_cat_pair_ksplit", _conv2d_f16("pair_ksplit", (128, 128), 128, (12, 40), cout2=128),
      "test_ksplit_small_launches", variants="ac", aligned=("wpacked",)),
    # regression tails, encoder, DDIM step, metrics
    R("regress_tail", "dv_upsample_softmax_regress_f32", _regress_tail(False), "test_regression_tail_extreme_costs", variants="ac"),
    R("regress_tail_ac", "dv_upsample_softmax_regress_f32", _regress_tail(True), "test_regression_tail_extreme_costs", variants="ac"),
    R("uncertainty_tail", "dv_upsample_softmax_uncertainty_f32", _regress_tail(True, True), "test_uncertainty_about_external_disparity",
      variants="ac"),
    R("disparity_regression", "dv_disparity_regression_f32", _disparity_regression, "test_disparity_regression", variants="ac"),
    R("softmax_regress", "dv_softmax_regress_f32", _softmax_regress, "test_softmax_regress", variants="ac"),
    R("two_hot", "dv_encode_two_hot_f32", _two_hot, "test_encoder_golden", variants="ac"),
    R("ddim_step", "dv_ddim_step", _ddim_step(False), "the number formats (see _ddim_step); test_gpu_ddim_kernels.py", variants="ac"),
    R("ddim_step_last", "dv_ddim_step", _ddim_step(True), "the number formats (see _ddim_step); test_gpu_ddim_kernels.py", variants="ac"),
    R("masked_metrics", "dv_masked_metrics_f32", _masked_metrics, "test_metrics_golden", variants="ac", aligned=("mask",)),
    # training entries with an alignment predicate (or refusal) and no offset-view test elsewhere
    R("feature_gate_bwd_ragged", "dv_feature_gate_bwd_f32", _feature_gate_bwd((2, 16, 6, 5, 7)), "test_gate_backward",
      pred=("cv", "logit", "g", "dcv", "dlogit", "workspace")),
    R("feature_gate_bwd_quads", "dv_feature_gate_bwd_f32", _feature_gate_bwd((1, 48, 3, 4, 8)), "test_gate_backward",
      pred=("cv", "logit", "g", "dcv", "dlogit")),
    R("feature_gate_bwd_split", "dv_feature_gate_bwd_f32", _feature_gate_bwd((1, 8, 48, 2, 4)), "test_gate_backward",
      pred=("cv", "logit", "g", "dcv", "dlogit", "workspace")),
    R("instance_norm_bwd_quads", "dv_instance_norm_act_bwd_f32", _instance_norm_bwd((16, 24), "leaky"), "test_instance_norm_act_backward",
      pred=("x", "g", "dx")),
    R("instance_norm_bwd_ragged", "dv_instance_norm_act_bwd_f32", _instance_norm_bwd((5, 7), "relu"), "test_instance_norm_act_backward",
      pred=("x", "g", "dx")),
    R("context_upsample_bwd", "dv_context_upsample_bwd_f32", _context_upsample_bwd((2, 5, 7), True), "test_gradients_match_float64_autograd",
      variants="ac", refuse={"weights": (ERR_ALIGN, 16), "grad_out": (ERR_ALIGN, 16), "d_weights": (ERR_ALIGN, 16)}),
]


def WG(name, entry, build, cite, operands=("x", "g", "dw", "workspace"), refuse=None):
    """A weight-gradient row: no alignment predicate, so every operand is displaced alone as an "other" one, and every
    accepted placement must give the bits of the aligned one."""
    return Row(name, entry, build, cite, refuse=refuse, same_bits=wg_same_bits(operands, refused=tuple(refuse or ())))


CAT3, CAT2 = ("in0", "in1", "in2", "g", "dw", "workspace"), ("in0", "in1", "g", "dw", "workspace")
TABLE += [
    # 3-D convolutions: k3 s1, k3 s2, k1; one brick; 36 bricks over 32 splits of 4 x 4 channel tiles
    WG("wgrad3d_k3s1", "dv_conv3d_wgrad_f32", _wg_conv3d(20, 40, 3, 1, 2, (3, 5, 18), ("channel_tails", "channel_tiles", "plane_tails")),
       "test_conv_weight_gradient"),
    WG("wgrad3d_k3s2", "dv_conv3d_wgrad_f32", _wg_conv3d(5, 33, 3, 2, 1, (5, 9, 19), ("channel_tails", "channel_tiles", "plane_tails")),
       "test_conv_weight_gradient"),
    WG("wgrad3d_k1", "dv_conv3d_wgrad_f32", _wg_conv3d(33, 17, 1, 1, 1, (3, 5, 17), ("channel_tails", "channel_tiles", "plane_tails")),
       "test_conv_weight_gradient"),
    WG("wgrad3d_one_brick", "dv_conv3d_wgrad_f32", _wg_conv3d(5, 7, 3, 1, 1, (2, 3, 9), ("channel_tails", "one_split")),
       "test_conv_weight_gradient"),
    WG("wgrad3d_ragged_splits", "dv_conv3d_wgrad_f32", _wg_conv3d(100, 100, 1, 1, 3, (5, 5, 17),
                                                                 ("channel_tails", "channel_tiles", "plane_tails", "ragged_splits")),
       "test_conv_weight_gradient"),
    # k4 transposed 3-D: two K waves share a brick; the three-tile block on one brick; 144 bricks over 128 splits
    WG("wgrad3d_k4", "dv_deconv3d_k4s2_wgrad_f32", _wg_deconv3d_k4(20, 9, 2, (3, 5, 9), ("channel_tails", "plane_tails")),
       "test_weight_gradient"),
    WG("wgrad3d_k4_three_tiles", "dv_deconv3d_k4s2_wgrad_f32", _wg_deconv3d_k4(48, 32, 1, (2, 3, 5), ("one_split",)), "test_weight_gradient"),
    WG("wgrad3d_k4_ragged_splits", "dv_deconv3d_k4s2_wgrad_f32", _wg_deconv3d_k4(20, 9, 3, (7, 15, 20),
                                                                                ("channel_tails", "plane_tails", "ragged_splits")),
       "test_weight_gradient"),
    # dilated 2-D: 4 x 32 bricks, the 2 x 32 bricks of dilation > 4, k1; one brick; 36 bricks over 32 splits
    WG("wgrad2d_k3", "dv_conv2d_wgrad_f32", _wg_conv2d(20, 40, 3, 1, 2, 9, 33, ("channel_tails", "channel_tiles", "plane_tails")),
       "test_weight_gradient"),
    WG("wgrad2d_k3_d5", "dv_conv2d_wgrad_f32", _wg_conv2d(5, 7, 3, 5, 1, 7, 37, ("channel_tails", "plane_tails")), "test_weight_gradient"),
    WG("wgrad2d_k1", "dv_conv2d_wgrad_f32", _wg_conv2d(33, 17, 1, 1, 1, 5, 35, ("channel_tails", "channel_tiles", "plane_tails")),
       "test_weight_gradient"),
    WG("wgrad2d_one_brick", "dv_conv2d_wgrad_f32", _wg_conv2d(5, 7, 3, 1, 1, 3, 20, ("channel_tails", "one_split")), "test_weight_gradient"),
    WG("wgrad2d_ragged_splits", "dv_conv2d_wgrad_f32", _wg_conv2d(100, 100, 1, 1, 3, 21, 33,
                                                                 ("channel_tails", "channel_tiles", "plane_tails", "ragged_splits")),
       "test_weight_gradient"),
    # over a virtual concatenation, fp32 and fp16 operands: source boundaries at channels 20 and 26 of two 64-wide tiles
    WG("wgrad_cat_k3", "dv_conv2d_wgrad_cat_f32", _wg_conv2d_cat(False, (20, 6, 39), 33, 3, 2, 5, 33,
                                                                 ("channel_tails", "plane_tails", "source_boundary", "k3")),
       "test_edge_shapes", operands=CAT3),
    WG("wgrad_cat_k1_ragged_splits", "dv_conv2d_wgrad_cat_f32", _wg_conv2d_cat(False, (5, 13, 3), 7, 1, 3, 9, 65,
                                                                               ("channel_tails", "plane_tails", "source_boundary", "k1",
                                                                                "ragged_splits")),
       "test_edge_shapes", operands=CAT3),
    WG("wgrad_cat_one_split", "dv_conv2d_wgrad_cat_f32", _wg_conv2d_cat(False, (5, 3), 7, 3, 1, 3, 20, ("channel_tails", "one_split", "k3")),
       "test_edge_shapes", operands=CAT2),
    WG("wgrad_cat_f16_k3", "dv_conv2d_wgrad_cat_f16", _wg_conv2d_cat(True, (20, 6, 39), 33, 3, 2, 5, 33,
                                                                     ("channel_tails", "plane_tails", "source_boundary", "k3")),
       "test_edge_shapes", operands=CAT3),
    WG("wgrad_cat_f16_k1_ragged_splits", "dv_conv2d_wgrad_cat_f16", _wg_conv2d_cat(True, (5, 13, 3), 7, 1, 3, 9, 65,
                                                                                   ("channel_tails", "plane_tails", "source_boundary",
                                                                                    "k1", "ragged_splits")),
       "test_edge_shapes", operands=CAT3),
    WG("wgrad_cat_f16_one_split", "dv_conv2d_wgrad_cat_f16", _wg_conv2d_cat(True, (5, 3), 7, 3, 1, 3, 20,
                                                                            ("channel_tails", "one_split", "k3")),
       "test_edge_shapes", operands=CAT2),
    WG("wgrad_1in", "dv_conv2d_1in_wgrad_f32", _wg_conv2d_1in(5, 3, 9, 33, ("channel_tails", "plane_tails")),
       "test_single_input_channel_weight_gradient", operands=("x", "g", "dw")),
    # k4 transposed 2-D: float4 stores into the workspace, so a workspace off a 16-byte boundary is refused and nothing runs
    WG("wgrad2d_k4", "dv_deconv2d_k4s2_wgrad_f32", _wg_deconv2d_k4(20, 9, 2, 5, 17, ("channel_tails", "plane_tails")),
       "test_gradients_match_float64_autograd", refuse={"workspace": (ERR_ALIGN, 16)}),
    WG("wgrad2d_k4_ragged_splits", "dv_deconv2d_k4s2_wgrad_f32", _wg_deconv2d_k4(32, 32, 3, 9, 3, ("plane_tails", "ragged_splits")),
       "test_gradients_match_float64_autograd", refuse={"workspace": (ERR_ALIGN, 16)}),
    WG("wgrad2d_k4_one_split", "dv_deconv2d_k4s2_wgrad_f32", _wg_deconv2d_k4(8, 3, 1, 5, 7, ("channel_tails", "plane_tails", "one_split")),
       "test_gradients_match_float64_autograd", refuse={"workspace": (ERR_ALIGN, 16)}),
    # few input channels: the 7 x 7 stride-2 stem, k3 over 9 bricks in 4 splits, k5 on one brick
    WG("wgrad_fewin_stem", "dv_conv2d_fewin_wgrad_f32", _wg_fewin(3, 7, 2, 20, 2, 17, 33, ("channel_tails", "plane_tails")),
       "test_fewin_weight_gradient"),
    WG("wgrad_fewin_k3_ragged_splits", "dv_conv2d_fewin_wgrad_f32", _wg_fewin(4, 3, 1, 5, 1, 17, 33,
                                                                             ("channel_tails", "plane_tails", "ragged_splits")),
       "test_fewin_weight_gradient"),
    WG("wgrad_fewin_k5_one_split", "dv_conv2d_fewin_wgrad_f32", _wg_fewin(1, 5, 2, 5, 1, 9, 20, ("channel_tails", "plane_tails", "one_split")),
       "test_fewin_weight_gradient"),
]
assert len({r.name for r in TABLE}) == len(TABLE)


@pytest.mark.parametrize("row", TABLE, ids=[r.name for r in TABLE])
def test_abi_arena(row):
    run_row(row)


# ------------------------------------------------------------------ the two Python-side fallbacks of Conv3dPlan
def _plan_case(cin, cout, stride, dims, seed):
    g = G(seed)
    x = torch.randn(dims[0], cin, *dims[1:], generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
    bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1,
          torch.rand(cout, generator=g) + 0.5)
    y = F.batch_norm(F.conv3d(x.double(), w.double(), None, stride, 1), bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(),
                     False, 0.0, 1e-5)
    plan = S.Conv3dPlan(w.to(DEV), tuple(t.to(DEV) for t in bn), stride=stride, act=S.ACT_RELU, precision="f32")
    return plan, x, torch.relu(y)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("layer", ["wino3_cin64", "s2pp"])
def test_conv3d_plan_falls_back_for_a_displaced_input(layer, offset):
    """Conv3dPlan routes a layer to the F(2x2x2) / polyphase kernel only when `x` is 16-byte aligned (both entries refuse
    anything else); a displaced `x` must reach the in-plane Winograd / direct stride-2 kernel and meet the same bar
    (test_conv_oracle: 1e-5 of the output scale), into a guard-banded output."""
    plan, x, ref = _plan_case(64, 64, 1, (1, 3, 7, 12), 97) if layer == "wino3_cin64" else _plan_case(8, 64, 2, (1, 4, 9, 12), 41)
    assert (plan.wino and S.Conv3dPlan.WINO3 and plan.cin >= S.Conv3dPlan.WINO3_MIN_CIN) if layer == "wino3_cin64" else plan.s2pp
    xin = A.place(x, offset, "in", DEV, name="x")
    out = A.place(torch.empty(ref.shape), offset, "out", DEV, name="out")
    got = plan(xin.view, out=out.view)
    _sync_or_stop(f"Conv3dPlan {layer}")
    assert got.data_ptr() == out.view.data_ptr()
    A.check_guards(xin)
    A.check_output(out, ref)
    e = rel_err(out.view.cpu(), ref)
    print(f"Conv3dPlan {layer} x displaced by {offset} floats: rel_err {e:.2e}")
    assert e < 1e-5
