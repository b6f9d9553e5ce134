"""The stream contract of the C ABI (include/diffuvolume_hip.h): every launch and memset of an entry goes to the `stream` it
is handed, and no entry blocks the host.

PyTorch's default stream is the null stream and its side streams are non-blocking, so on the default stream -- where the
rest of the suite runs -- an entry that sent one of its launches elsewhere, or waited for the device, looks exactly like a
correct one.  Here every row of the arena table (tests/test_gpu_abi_arena.py: the smallest edge shapes, a float64
reference, the bar of the entry's own test, ``call(lib, p, s)``) runs three times, all operands 16-byte aligned:

  1. TRUE run on the default stream (after one throw-away call that loads the code): meets the row's bar; bits kept,
     host time of the call kept.
  2. POISON run on the default stream: every floating-point input or in/out operand the row lets move holds zeros (a
     valid input of every entry; integer operands, masks, index tables and packed weights keep their true values).  Its
     output must FAIL the row's bar -- the detector has power for this row.
  3. GATED run on a non-blocking side stream S that the hardware was seen to run independently of the null stream
     (tests/streams.py: streams may share a hardware queue, and then a gate orders them).  The arenas hold the poison
     and the outputs the sentinel, all settled.
     On S: a gate (a kernel that only spins), the event ``gate_done``, the sentinel again into every output, device-to-
     device copies of the true operands, then the entry with S.  ``gate_done.query()`` is read as the call returns.
     The result must have intact guards, every output element written, meet the bar and equal the true run bit for bit,
     and the gate must still have been pending when the call returned.

A launch or memset that went to any other stream runs while the gate still spins: it reads poison or an unwritten
workspace, or writes what the sentinel fill behind the gate wipes out again; a call that waits for the device returns
after the gate.  The gate is calibrated once with events around the spin kernel and is at least 50 times the largest
host time of a warmed call over the table, and at least 10 ms.

The same three runs hold the 13 weight packers (their image in place of a bar), and stand-in "entries" written with torch
ops show that the harness catches each defect on this box -- which also shows that the side stream does not wait for
the null stream, what the whole method rests on.  The training entries that are no row of the table run through their
Python autograd wrappers (``WRAPPERS``), forward and backward under ``torch.cuda.stream(S)``.
tests/test_stream_contract_host.py holds the four groups complete.
"""
import time
from types import SimpleNamespace

import pytest
import torch

import arena as A
import streams
import test_gpu_abi_arena as T
from diffuvolume_amd import _lib
from test_gpu_abi_arena import TABLE, Case, Row

pytestmark = pytest.mark.gpu
DEV = T.DEV

# rows whose all-zero poison passes their bar take another finite, in-range poison: row name -> (word for the test id,
# lambda operand name, true tensor: poison tensor)
OTHER_POISON = {}

# dv_masked_metrics_f32 sums with floating atomics (double adds in any order): its bits may differ from run to run, so
# it is held to its bar on the side stream and left out of the bit comparison -- the only such entry.
NOT_BIT_EQUAL = {"dv_masked_metrics_f32"}

MIN_GATE_MS = 10.0
GATE_FACTOR = 50


class Ptr:
    """``p(name)``: the operand's device pointer, None when the row has none; ``p.ar``: the arenas (the stand-ins' view)."""

    def __init__(self, ar):
        self.ar = ar

    def __call__(self, n):
        return self.ar[n].data_ptr() if n in self.ar else None


def poisoned_names(row, case):
    return [n for n, t in list(case.inputs.items()) + list(case.inout.items())
            if t.is_floating_point() and n not in row.aligned]


def poisoned_operands(row, case):
    """The row's operands with every poisoned one replaced (what place_operands looks at, nothing else)."""
    make = OTHER_POISON[row.name][1] if row.name in OTHER_POISON else (lambda n, t: torch.zeros_like(t))
    names = poisoned_names(row, case)
    sub = lambda d: {n: (make(n, t) if n in names else t) for n, t in d.items()}
    return SimpleNamespace(inputs=sub(case.inputs), outs=case.outs, inout=sub(case.inout))


def bits_equal(x, y):
    return x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def call_on(row, case, ar, stream_ptr, after_call=None):
    """The row's call between its hooks, timed on the host; ``after_call`` runs as the call returns, before anything waits."""
    lib = _lib.load()
    if case.before:
        case.before(lib)
    try:
        t0 = time.perf_counter()
        rc = case.call(lib, Ptr(ar), stream_ptr)
        dt = time.perf_counter() - t0
        seen = after_call() if after_call else None
        T._sync_or_stop(f"{row.entry} [{row.name}]")
    finally:
        if case.after:
            case.after(lib)
    return rc, dt, seen


def verdict(row, case, ar, all_written=True):
    """Guards intact, every output element written, the row's bar met; the outputs on the CPU."""
    for n in case.inputs:
        A.check_guards(ar[n])
    got = {}
    for n in list(case.outs) + list(case.inout):
        if all_written:
            A.check_output(ar[n], case.ref.get(n))
        else:
            A.check_guards(ar[n])
        got[n] = ar[n].view.cpu()
        if n in case.ref:
            case.bar(n, got[n], case.ref[n])
    return got


def true_run(row, case, all_written=True):
    """Step 1: (outputs, host seconds of the warmed call)."""
    rc, _, _ = call_on(row, case, T.place_operands(row, case, "warm-up", {}), 0)
    assert rc == T.OK, f"{row.entry}: returned {rc}"
    ar = T.place_operands(row, case, "true", {})
    T._sync_or_stop("placing operands")
    rc, dt, _ = call_on(row, case, ar, 0)
    assert rc == T.OK, f"{row.entry}: returned {rc}"
    return verdict(row, case, ar, all_written), dt


def poison_run(row, case):
    """Step 2: the outputs of the call on poisoned operands."""
    names = poisoned_names(row, case)
    assert names, f"{row.name}: no operand to poison"
    ar = T.place_operands(row, poisoned_operands(row, case), "poison", {})
    T._sync_or_stop("placing operands")
    rc, _, _ = call_on(row, case, ar, 0)
    assert rc == T.OK, f"{row.entry}: returned {rc} on the poison"
    return {n: ar[n].view.cpu() for n in list(case.outs) + list(case.inout)}


def fails_the_bar(case, got):
    failed = []
    for n in got:
        if n in case.ref:
            try:
                case.bar(n, got[n], case.ref[n])
            except AssertionError:
                failed.append(n)
    return failed


def gated_run(row, case, gate, all_written=True):
    """Step 3: the outputs of the call on S behind the gate; raises if the entry blocked the host."""
    names = poisoned_names(row, case)
    ar = T.place_operands(row, poisoned_operands(row, case), "gated", {})
    true = {n: {**case.inputs, **case.inout}[n].contiguous().to(DEV) for n in names}
    side = gate.side
    gate_start, gate_done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    T._sync_or_stop("placing operands")
    with torch.cuda.stream(side):
        gate_start.record()
        torch.cuda._sleep(gate.cycles)
        gate_done.record()
        for n in case.outs:                                    # whatever ran ahead of the gate wrote into this
            ar[n].payload_words().fill_(A.SENTINEL)
        for n in names:
            ar[n].view.copy_(true[n])
    rc, dt, pending = call_on(row, case, ar, side.cuda_stream, after_call=lambda: not gate_done.query())
    assert rc == T.OK, f"{row.entry}: returned {rc} on the side stream"
    got = verdict(row, case, ar, all_written)
    assert pending, (f"{row.entry} blocked the host: the gate ({gate.ms:.1f} ms asked for, {gate_start.elapsed_time(gate_done):.1f} ms "
                     f"measured) was over when the call returned after {dt * 1e3:.3f} ms on the host")
    return got


# ------------------------------------------------------------------ the gate
@pytest.fixture(scope="module")
def session():
    """Step 1 of every row (an AssertionError is kept for the row's own test), then the one gate of the session."""
    true = {}
    for row in TABLE:
        try:
            true[row.name] = true_run(row, T.case_of(row))
        except AssertionError as e:
            true[row.name] = e
    times = {n: v[1] for n, v in true.items() if not isinstance(v, AssertionError)}
    assert times, "no row of the table ran"
    worst = max(times, key=times.get)
    ms = max(MIN_GATE_MS, GATE_FACTOR * times[worst] * 1e3)
    cycles = streams.calibrate_gate(ms)
    gate = SimpleNamespace(ms=ms, cycles=cycles, side=streams.pick_streams(1, cycles)[0])
    print(f"STREAM largest host time of a warmed call over the table: {times[worst] * 1e3:.3f} ms ({worst}); "
          f"gate {ms:.1f} ms = {gate.cycles} cycles of the spin kernel")
    return SimpleNamespace(true=true, gate=gate, worst_ms=times[worst] * 1e3)


def test_gate_length(session):
    """The chosen gate is what the method asks for, and what RUNS is at least that (it is calibrated with a margin)."""
    g = session.gate
    print(f"STREAM largest warmed host call {session.worst_ms:.3f} ms, gate {g.ms:.1f} ms")
    assert g.ms >= MIN_GATE_MS and g.ms >= GATE_FACTOR * session.worst_ms
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(g.cycles)
    e1.record()
    T._sync_or_stop("the gate")
    took = e0.elapsed_time(e1)
    print(f"STREAM the gate ran {took:.1f} ms")
    assert took >= MIN_GATE_MS and took >= GATE_FACTOR * session.worst_ms, (took, session.worst_ms)


def stream_id(row):
    return row.name + (f"-poison_{OTHER_POISON[row.name][0]}" if row.name in OTHER_POISON else "")


@pytest.mark.parametrize("row", TABLE, ids=[stream_id(r) for r in TABLE])
def test_entry_keeps_to_its_stream(row, session):
    case = T.case_of(row)
    first = session.true[row.name]
    if isinstance(first, AssertionError):
        raise first
    true_out, dt = first
    print(f"  {row.name}: host time of the warmed call {dt * 1e3:.3f} ms")
    failed = fails_the_bar(case, poison_run(row, case))
    assert failed, (f"{row.name}: the poison run passes the row's bar, so a launch that read the poison would not show; "
                    "give the row another finite, in-range poison in OTHER_POISON")
    got = gated_run(row, case, session.gate)
    if row.entry not in NOT_BIT_EQUAL:
        for n in got:
            assert bits_equal(got[n], true_out[n]), f"{row.entry}: {n} on the side stream differs from the default-stream run"


# ------------------------------------------------------------------ the harness catches what it is there for
def _standin(body):
    """A two-launch "entry" y = 2 x + 1 through a workspace, in torch ops on the arenas: ``body(x, tmp, y, s)`` with ``s`` the
    stream it was handed."""
    x = torch.randn(3, 37, generator=T.G(5))

    def call(lib, p, s):
        body(p.ar["x"].view, p.ar["tmp"].view, p.ar["y"].view, torch.cuda.ExternalStream(s) if s else torch.cuda.default_stream())
        return 0
    case = Case({"x": x}, {"tmp": torch.empty(3, 37), "y": torch.empty(3, 37)}, call, {"y": 2 * x.double() + 1}, T.bar_close(1e-6, 1e-6))
    return Row("standin", "standin", None, "this file"), case


def _good(x, tmp, y, s):
    with torch.cuda.stream(s):
        torch.mul(x, 2, out=tmp)
        torch.add(tmp, 1, out=y)


def _ignores_its_stream(x, tmp, y, s):
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.mul(x, 2, out=tmp)
        torch.add(tmp, 1, out=y)


def _second_launch_elsewhere(x, tmp, y, s):
    with torch.cuda.stream(s):
        torch.mul(x, 2, out=tmp)
    with torch.cuda.stream(torch.cuda.default_stream()):
        torch.add(tmp, 1, out=y)


def _blocks_the_host(x, tmp, y, s):
    _good(x, tmp, y, s)
    s.synchronize()


def _three_runs(row, case, gate):
    true_out, _ = true_run(row, case)
    assert fails_the_bar(case, poison_run(row, case))
    got = gated_run(row, case, gate)
    for n in got:
        assert bits_equal(got[n], true_out[n]), n


def test_harness_passes_a_correct_entry(session):
    _three_runs(*_standin(_good), session.gate)


@pytest.mark.parametrize("body, symptom", [(_ignores_its_stream, "NEVER WRITTEN"), (_second_launch_elsewhere, "NEVER WRITTEN"),
                                           (_blocks_the_host, "blocked the host")],
                         ids=["ignores_its_stream", "second_launch_on_the_default_stream", "synchronises_inside"])
def test_harness_catches(body, symptom, session):
    """Each defect the method is there for, in a stand-in that calls no library code.  The first two also show that a side
    stream of this box does not wait for the null stream: if it did, their work would queue up behind the gate and pass."""
    with pytest.raises(AssertionError, match=symptom):
        _three_runs(*_standin(body), session.gate)


# ------------------------------------------------------------------ the weight packers
# (size entry, packer, dims, weight shape): the sizes of the arena rows that consume the image
PACKERS = [
    ("dv_pointwise_expand_packed_floats", "dv_pointwise_expand_pack_weights_f32", (8, 162), (162, 8)),
    ("dv_conv3d_packed_floats", "dv_conv3d_pack_weights_f32", (8, 32, 3), (32, 8, 3, 3, 3)),
    ("dv_conv3d_f16x3_packed_bytes", "dv_conv3d_f16x3_pack_weights", (8, 32), (32, 8, 3, 3, 3)),
    ("dv_conv3d_wino_packed_floats", "dv_conv3d_wino_pack_weights_f32", (8, 16), (16, 8, 3, 3, 3)),
    ("dv_conv3d_wino3_packed_floats", "dv_conv3d_wino3_pack_weights_f32", (8, 32), (32, 8, 3, 3, 3)),
    ("dv_conv3d_s2pp_packed_floats", "dv_conv3d_s2pp_pack_weights_f32", (5, 64), (64, 5, 3, 3, 3)),
    ("dv_deconv3d_packed_floats", "dv_deconv3d_pack_weights_f32", (16, 32), (16, 32, 3, 3, 3)),
    ("dv_deconv3d_k4_packed_floats", "dv_deconv3d_k4_pack_weights_f32", (16, 8), (16, 8, 4, 4, 4)),
    ("dv_conv2d_packed_floats", "dv_conv2d_pack_weights_f32", (20, 24, 3, 3), (24, 20, 3, 3)),
    ("dv_conv2d_wino_packed_floats", "dv_conv2d_wino_pack_weights_f32", (8, 32), (32, 8, 3, 3)),
    ("dv_conv2d_f16_packed_bytes", "dv_conv2d_f16_pack_weights", (64, 32, 3), (32, 64, 3, 3)),
    ("dv_geo_lookup_conv1x1_packed_floats", "dv_geo_lookup_conv1x1_pack_weights_f32", (8,), (64, 162)),
    ("dv_deconv3d_k4s2_dgrad_packed_floats", "dv_deconv3d_k4s2_dgrad_pack_weights_f32", (20, 9), (20, 9, 4, 4, 4)),
]


@pytest.mark.parametrize("sizer, packer, dims, wshape", PACKERS, ids=[p[1] for p in PACKERS])
def test_packer_keeps_to_its_stream(sizer, packer, dims, wshape, session):
    """The weight arrives behind the gate and the pack runs on S: the image equals the default-stream image bit for bit,
    differs from the image of a zero weight, and the call does not block.  (An image may have padding no kernel reads or
    writes, so "every element written" is not asked of it; guards are.)"""
    lib = _lib.load()
    n = getattr(lib, sizer)(*dims)
    assert n > 0, (sizer, dims)
    nwords = (n + 3) // 4 if sizer.endswith("_bytes") else n
    w = torch.randn(*wshape, generator=T.G(71))
    case = Case({"w": w}, {"image": torch.empty(nwords, dtype=torch.int32)},
                lambda lib, p, s: getattr(lib, packer)(p("w"), p("image"), *dims, s), {}, None)
    row = Row(packer, packer, None, "this file")
    true_out, dt = true_run(row, case, all_written=False)
    print(f"  {packer}: host time of the warmed call {dt * 1e3:.3f} ms")
    assert not bits_equal(poison_run(row, case)["image"], true_out["image"]), "the image of a zero weight equals the true image"
    got = gated_run(row, case, session.gate, all_written=False)
    assert bits_equal(got["image"], true_out["image"]), f"{packer}: the image packed on the side stream differs"


# ------------------------------------------------------------------ training entries behind their autograd wrappers
class Wrapped:
    """``entries``: the exports the wrapper's forward and backward launch; ``make()`` -> inputs (name -> CPU tensor),
    ``grad`` (the inputs differentiated), ``run(t)`` on device tensors -> output(s), ``params`` (module parameters: like
    packed weights they hold their true values from the start, and their gradients are compared too)."""

    def __init__(self, name, entries, make):
        self.name, self.entries, self.make = name, tuple(entries), make


def _rnd(seed):
    g = T.G(seed)
    return lambda *s, gain=1.0: torch.randn(*s, generator=g) * gain


def _w_gwc():
    from diffuvolume_amd import train_volume
    b, c, h, w, d, g = 1, 24, 2, 7, 9, 8                                  # test_gpu_volume_train.GWC_SHAPES: odd W
    r = _rnd(301)
    return SimpleNamespace(inputs={"ref": r(b, c, h, w), "tgt": r(b, c, h, w)}, grad=("ref", "tgt"),
                           run=lambda t: train_volume.build_gwc_volume_train(t["ref"], t["tgt"], d, g))


def _w_concat():
    from diffuvolume_amd import train_volume
    b, c, h, w, d = 2, 6, 3, 11, 5                                        # CONCAT_SHAPES, mode "scale"
    r = _rnd(302)
    return SimpleNamespace(inputs={"ref": r(b, c, h, w), "tgt": r(b, c, h, w), "scale": r(b, d, h, w)}, grad=("ref", "tgt", "scale"),
                           run=lambda t: train_volume.build_concat_volume_train(t["ref"], t["tgt"], d, False, t["scale"]))


def _w_warp_corr():
    from diffuvolume_amd import train_refine
    b, c, h, w = 2, 3, 3, 25                                              # test_gpu_refine_train "wrap_overlaps_tile"
    r = _rnd(303)
    disp = torch.rand(b, 1, h, w, generator=T.G(304)) * 30
    return SimpleNamespace(inputs={"left": r(b, c, h, w), "right": r(b, c, h, w), "disp": disp}, grad=("left", "right", "disp"),
                           run=lambda t: train_refine.warp_corr_train(t["left"], t["right"], t["disp"]))


def _w_bn3d():
    from diffuvolume_amd import train_norm
    shape = (2, 3, 1, 1, 5)                                               # test_gpu_norm_train "sub_wave"
    r = _rnd(305)
    inputs = {"x": r(*shape), "weight": r(3) + 1, "bias": r(3), "running_mean": r(3), "running_var": r(3).abs() + 0.5, "skip": r(*shape)}

    def run(t):
        y = train_norm.batch_norm_act_train(t["x"], t["weight"], t["bias"], t["running_mean"], t["running_var"], act="mish",
                                            skip=t["skip"])
        return y, t["running_mean"], t["running_var"]
    return SimpleNamespace(inputs=inputs, grad=("x", "weight", "bias", "skip"), run=run)


def _w_patch():
    from diffuvolume_amd import train_patch
    shape = (2, 40, 2, 17, 12)                                            # test_gpu_patch_train "row_tiles"
    dil = (1,) * 8 + (2,) * 16 + (3,) * 16
    r = _rnd(306)
    return SimpleNamespace(inputs={"gwc": r(*shape), "w1": r(40, 9, gain=0.4), "w2": r(40, 9, gain=0.4)}, grad=("gwc", "w1", "w2"),
                           run=lambda t: train_patch.patch_volume_train(t["gwc"], t["w1"], t["w2"], dil))


def _w_attn():
    from diffuvolume_amd import train_attn
    c = 128                                                               # test_gpu_attn_train "one_window"
    r = _rnd(307)
    inputs = {"x": r(1, c, 4, 4, 4), "qkv_w": r(3 * c, c, gain=c ** -0.5), "qkv_b": r(3 * c, gain=0.1),
              "proj_w": r(c, c, gain=c ** -0.5), "proj_b": r(c, gain=0.1)}
    return SimpleNamespace(inputs=inputs, grad=tuple(inputs),
                           run=lambda t: train_attn.window_attention_train(t["x"], t["qkv_w"], t["qkv_b"], t["proj_w"], t["proj_b"], 16))


def _w_resize():
    from diffuvolume_amd import train_net2d
    return SimpleNamespace(inputs={"x": _rnd(308)(1, 7, 3, 5)}, grad=("x",),   # test_gpu_resize_bwd "ratio", BC = 7
                           run=lambda t: train_net2d.resize_bilinear_train(t["x"], (7, 9)))


def _w_dwconv():
    from diffuvolume_amd import train2d
    r = _rnd(309)                                                         # test_gpu_dwconv: (7, 9), 5 channels, stride 2
    return SimpleNamespace(inputs={"x": r(2, 5, 7, 9), "weight": r(5, 1, 3, 3, gain=0.3)}, grad=("x", "weight"),
                           run=lambda t: train2d.dwconv2d(t["x"], t["weight"], 2))


def _w_loss():
    from diffuvolume_amd import train_loss
    shape, k = (1, 3, 5), 4                                               # test_gpu_loss_train "tail", K = 4
    r = _rnd(310)
    inputs = {f"pred{i}": r(*shape, gain=3.0) + 20 for i in range(k)}
    inputs.update(gt=r(*shape, gain=3.0) + 20, mask=torch.rand(*shape, generator=T.G(311)) > 0.3)
    weights = [0.5, 0.5, 0.7, 1.0]
    return SimpleNamespace(inputs=inputs, grad=tuple(f"pred{i}" for i in range(k)),
                           run=lambda t: train_loss.masked_loss_train([t[f"pred{i}"] for i in range(k)], t["gt"], t["mask"], weights))


def _w_tail():
    from diffuvolume_amd import train_tail
    return SimpleNamespace(inputs={"cost": _rnd(312)(2, 5, 3, 4, gain=3.0)}, grad=("cost",),   # test_gpu_regress_train (2, 5, 3, 4)
                           run=lambda t: train_tail.upsample_softmax_regress_train(t["cost"], False))


def _w_geo_lookup():
    from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
    b, c, d, h, w, w2 = 1, 3, 13, 3, 21, 21                               # test_gpu_geo_lookup_bwd.SHAPES, kind "uniform"
    r = _rnd(313)
    disp = (torch.rand(b * h * w, generator=T.G(314)) * (d + 10) - 5).view(b, 1, h, w)
    coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous()
    inputs = {"geo": r(b, c, d, h, w), "fmap1": r(b, 6, h, w), "fmap2": r(b, 6, h, w2), "disp": disp, "coords": coords,
              "noisy": r(b, d, h, w)}
    return SimpleNamespace(inputs=inputs, grad=("geo", "fmap1", "fmap2"),
                           run=lambda t: Combined_Geo_Encoding_Volume(t["fmap1"], t["fmap2"], t["geo"])(t["disp"], t["coords"], t["noisy"]))


def _w_deconv3d_k4():
    from diffuvolume_amd import train3d
    r = _rnd(315)                                                         # test_gpu_deconv3d_k4_bwd.SHAPES: odd W
    return SimpleNamespace(inputs={"x": r(1, 32, 3, 4, 7), "weight": r(32, 16, 4, 4, 4, gain=(64 * 32) ** -0.5)}, grad=("x", "weight"),
                           run=lambda t: train3d.conv_transpose3d_k4(t["x"], t["weight"]))


def _w_gru(f16):
    def make():
        from diffuvolume_amd.synth import synth_state_dict
        from diffuvolume_amd.update import ConvGRU
        hid, cin, h, w = 32, 24, 5, 9                                     # a tail in H * W, two x sources
        gru = ConvGRU(hid, cin)
        gru.load_state_dict(synth_state_dict(gru.state_dict(), seed=3))
        gru = gru.to(DEV).train().set_train_precision("f16" if f16 else "f32")
        r = _rnd(316)
        inputs = {"h": torch.tanh(r(1, hid, h, w)), "cz": r(1, hid, h, w), "cr": r(1, hid, h, w), "cq": r(1, hid, h, w),
                  "x0": r(1, 16, h, w), "x1": r(1, 8, h, w)}
        return SimpleNamespace(inputs=inputs, grad=tuple(inputs), params=list(gru.parameters()),
                               run=lambda t: gru(t["h"], t["cz"], t["cr"], t["cq"], t["x0"], t["x1"]))
    return make


WRAPPERS = [
    Wrapped("train_volume.gwc", ["dv_gwc_volume_bwd_f32"], _w_gwc),
    Wrapped("train_volume.concat", ["dv_concat_volume_bwd_f32"], _w_concat),
    Wrapped("train_refine.warp_corr", ["dv_warp_corr_f32", "dv_warp_corr_bwd_f32"], _w_warp_corr),
    Wrapped("train_norm.batch_norm_act", ["dv_bn3d_stats_f32", "dv_bn3d_apply_act_f32", "dv_bn3d_act_bwd_f32"], _w_bn3d),
    Wrapped("train_patch.patch_volume", ["dv_patch_volume_bwd_f32"], _w_patch),
    Wrapped("train_attn.window_attention", ["dv_window_attn3d_bwd_f32"], _w_attn),
    Wrapped("train_net2d.resize_bilinear", ["dv_resize_bilinear_ac_bwd_f32"], _w_resize),
    Wrapped("train2d.dwconv2d", ["dv_dwconv3x3_f32", "dv_dwconv3x3_bwd_f32"], _w_dwconv),
    Wrapped("train_loss.masked_loss", ["dv_masked_loss_fwd_f32", "dv_masked_loss_bwd_f32"], _w_loss),
    Wrapped("train_tail.regress", ["dv_upsample_softmax_regress_bwd_f32"], _w_tail),
    Wrapped("geometry_ddim.lookup", ["dv_allpairs_corr_bwd_f32", "dv_geo_filter_lookup_bwd_f32"], _w_geo_lookup),
    Wrapped("train3d.conv_transpose3d_k4", ["dv_deconv3d_k4s2_dgrad_f32"], _w_deconv3d_k4),
    Wrapped("update.ConvGRU_f32", ["dv_gru_reset_mul_f32", "dv_gru_blend_f32", "dv_gru_gates_bwd_blend_f32",
                                   "dv_gru_gates_bwd_reset_f32"], _w_gru(False)),
    Wrapped("update.ConvGRU_f16", ["dv_gru_reset_mul_f16", "dv_gru_blend_f16"], _w_gru(True)),
]


def _forward_backward(case, t, cots):
    """Forward and backward on the current stream -> [outputs..., input gradients..., parameter gradients...] (device).
    ``cots``: the cotangents of the differentiable outputs, in order; None = ones-shaped probes are not wanted: the caller
    only asks for the outputs' shapes (first element of the result) and no backward runs."""
    params = getattr(case, "params", [])
    for n in case.grad:
        t[n].requires_grad_(True)
    for p in params:
        p.grad = None
    outs = case.run(t)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    diff = [o for o in outs if o.requires_grad]
    assert diff, "no differentiable output"
    if cots is None:
        return [tuple(o.shape) for o in diff]
    assert len(cots) == len(diff)
    torch.autograd.backward(diff, list(cots))
    grads = [t[n].grad for n in case.grad] + [p.grad for p in params]
    assert all(g is not None for g in grads), "an input that should have a gradient has none"
    return [o.detach() for o in outs] + grads


def _device_inputs(case, zeros):
    return {n: (torch.zeros(v.shape, dtype=v.dtype, device=DEV) if zeros and v.is_floating_point() else v.to(DEV))
            for n, v in case.inputs.items()}


def _record_launches(monkeypatch):
    """The entry names that go through ``_lib.launch`` / ``_lib.timed_launch`` from now on."""
    seen = set()
    launch, timed_launch = _lib.launch, _lib.timed_launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **kw: (seen.add(name), launch(name, *a, **kw))[1])
    monkeypatch.setattr(_lib, "timed_launch", lambda tag, flops, nbytes, name, *a, **kw:
                        (seen.add(name), timed_launch(tag, flops, nbytes, name, *a, **kw))[1])
    return seen


@pytest.mark.parametrize("wrapped", WRAPPERS, ids=[w.name for w in WRAPPERS])
def test_wrapper_keeps_to_the_current_stream(wrapped, session, monkeypatch):
    """Forward and backward under ``torch.cuda.stream(S)``.  The inputs AND the cotangents are zeros, made on the default
    stream and settled, and are filled by ``copy_`` on S behind the gate: every output and gradient equals the
    default-stream run bit for bit, every one of them differs from it in the run on the zeros (so each launch, the
    ones that read nothing but a cotangent included, has power), and every entry the wrapper is listed for is seen
    to be launched.  (No asynchrony assertion: the wrappers may read a result by design.)"""
    for knob in ("CONV3D", "CONV2D", "LOOKUP", "TAIL", "VOLUME", "REFINE", "NORM", "PATCH", "ATTN", "NET2D", "LOSS"):
        monkeypatch.setenv("DV_TRAIN_" + knob, "hip")
    case = wrapped.make()
    true_in = _device_inputs(case, zeros=False)
    shapes = _forward_backward(case, _device_inputs(case, zeros=False), None)
    true_cots = [torch.randn(sh, generator=T.G(900 + i)).to(DEV) for i, sh in enumerate(shapes)]
    zero_cots = lambda: [torch.zeros_like(c) for c in true_cots]
    T._sync_or_stop("the inputs")
    want = [x.cpu() for x in _forward_backward(case, _device_inputs(case, zeros=False), true_cots)]
    T._sync_or_stop(f"{wrapped.name} on the default stream")
    zero = [x.cpu() for x in _forward_backward(case, _device_inputs(case, zeros=True), zero_cots())]
    T._sync_or_stop(f"{wrapped.name} on zeros")
    same = [i for i, (a, b) in enumerate(zip(zero, want)) if bits_equal(a, b)]
    assert not same, f"{wrapped.name}: results {same} of the run on zeros equal the true run: no power for what writes them"
    t, cots = _device_inputs(case, zeros=True), zero_cots()
    side = session.gate.side
    T._sync_or_stop("the zero inputs")
    launched = _record_launches(monkeypatch)
    with torch.cuda.stream(side):
        torch.cuda._sleep(session.gate.cycles)
        for n, v in t.items():
            v.copy_(true_in[n])
        for z, c in zip(cots, true_cots):
            z.copy_(c)
        got = _forward_backward(case, t, cots)
    T._sync_or_stop(f"{wrapped.name} on the side stream")
    assert set(wrapped.entries) <= launched, f"{wrapped.name} never launched {sorted(set(wrapped.entries) - launched)}"
    got = [x.cpu() for x in got]
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert bits_equal(a, b), f"{wrapped.name}: result {i} on the side stream differs from the default-stream run"
