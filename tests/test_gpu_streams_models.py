"""The three models across streams and threads.

The reference drives the models through ``nn.DataParallel``, one Python thread per replica, and a serving caller runs
each request under a stream of its own.  ``_lib.launch`` hands PyTorch's current stream to every entry, so a model follows
its caller's stream; what a stream cannot order for another one is what the package BUILDS once and keeps -- packed
weights, folded BatchNorm, the per-layer plans of IGEV's front, the time-MLP shifts of the DDIM loop.  ``PlanCache``
carries the guarantee (diffuvolume_amd/plans.py): what ``plans()`` / ``prepare()`` return has been waited for on the
stream that built it.

Every comparison is bit for bit against the same forward on the default stream; the noise comes from a ``NoiseTape``.
Gates and independent side streams: tests/streams.py.
"""
import threading
import types
from contextlib import contextmanager

import pytest
import torch
from torch import nn

import streams
from conftest import load_golden
from diffuvolume_amd.plans import PlanCache
from diffuvolume_amd.synth import NoiseTape, StubMobileNetV2, synth_state_dict, synth_stereo_batch
from test_igev_model import ARGS as IGEV_ARGS, golden_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE_MS = 10.0
FORWARDS = 4                        # per thread
JOIN_SECONDS = 300

LOCAL = threading.local()           # .tape: the NoiseTape of the forward this thread is running


# ------------------------------------------------------------------ the three models at their smallest test sizes
def _acv():
    import diffuvolume_amd as dv
    m = dv.ACVNet_DDIM(192, False, False)                                 # tests/test_gpu_dropin.py
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=1, logit_gain=8.0), strict=True)
    return m.to(DEV).eval()


def _pcw():
    from diffuvolume_amd.pwcnet_ddim import PWCNet_ddim
    g = load_golden("pcw_forward_eval")                                   # tests/test_gpu_pcw.py::test_forward_golden
    scale = {str(k): float(v) for k, v in zip(g["scale_keys"].tolist(), g["scale_vals"].tolist())}
    m = PWCNet_ddim(192, True)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=2, logit_gain=8.0, scale=scale), strict=True)
    return m.to(DEV).eval()


def _igev():
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    m = IGEVStereo_ddim(types.SimpleNamespace(**IGEV_ARGS), feature=Feature(StubMobileNetV2()), sampling_timesteps=2)
    m.load_state_dict(synth_state_dict(m.state_dict(), seed=3, scale={"update_block.disp_head.conv2.weight": 0.05,
                                                                      "update_block.disp_head.conv2.bias": 0.0}), strict=True)
    return m.to(DEV).eval()                                               # tests/test_igev_model.py


def _stereo_halves():
    b = synth_stereo_batch(2, 64, 128, seed=3, shifts=(8, 20))
    return [tuple(b[k][i:i + 1].contiguous() for k in ("left", "right", "used", "disp")) for i in range(2)]


def _call_acv(m, ins):
    return m(*ins, None)[0]


def _call_pcw(m, ins):
    return m(*ins, None)[0][0]


def _call_igev(m, ins):
    return m(*ins, iters=3, test_mode=True, noise=LOCAL.tape)[0]


MODELS = {"acv": (_acv, _stereo_halves, _call_acv), "pcw": (_pcw, _stereo_halves, _call_pcw),
          "igev": (_igev, lambda: [golden_inputs(11), golden_inputs(12)], _call_igev)}


@contextmanager
def taped(*models):
    """ACV and PCW draw inside ``forward``: their ``ddim_sample`` takes this thread's tape (IGEV's forward takes ``noise``)."""
    patched = [m for m in models if type(m).__name__ != "IGEVStereo_ddim"]
    for m in patched:
        m.ddim_sample = (lambda m: lambda *a, **kw: type(m).ddim_sample(m, *a, noise=LOCAL.tape, **kw))(m)
    try:
        yield
    finally:
        for m in patched:
            del m.ddim_sample


def forward(name, model, ins, tape):
    LOCAL.tape = tape
    return MODELS[name][2](model, ins)


def settle(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a GPU fault: nothing more may start on this device
        pytest.exit(f"GPU fault in {what}: {e}", returncode=3)


def on_device(ins):
    return tuple(t.to(DEV) for t in ins)


def replica_of(model):
    """What nn.parallel.replicate makes of a module tree on its own device, without the broadcast: every module through
    ``_replicate_for_data_parallel`` (a PlanCache replica drops its plans and remembers its source), children re-linked,
    the parameters as plain tensor attributes -- here the source's own storage instead of a broadcast copy."""
    mods = list(model.modules())
    index = {id(m): i for i, m in enumerate(mods)}
    reps = [m._replicate_for_data_parallel() for m in mods]
    for m, r in zip(mods, reps):
        for key, child in m._modules.items():
            if child is not None:
                r._modules[key] = reps[index[id(child)]]
        for key, p in m._parameters.items():
            if p is None:
                r._parameters[key] = None
            else:
                setattr(r, key, p.detach())
    return reps[0]


@pytest.fixture(scope="module")
def gate():
    cycles = streams.calibrate_gate(GATE_MS)
    a, b = streams.pick_streams(2, cycles)
    return types.SimpleNamespace(cycles=cycles, a=a, b=b)


@pytest.fixture(scope="module")
def serial():
    """name -> (per-thread inputs on the device, [thread][forward] outputs of the serial default-stream run on a model of
    its own): computed once, shared, never modified."""
    out = {}

    def get(name):
        if name not in out:
            model = MODELS[name][0]()
            ins = [on_device(x) for x in MODELS[name][1]()]
            with taped(model):
                refs = []
                for k in range(2):
                    tape = NoiseTape(40 + k)
                    refs.append([forward(name, model, ins[k], tape).clone() for _ in range(FORWARDS)])
            settle(f"{name} on the default stream")
            assert all(bool(torch.isfinite(t).all()) for r in refs for t in r)
            assert not torch.equal(refs[0][0], refs[1][0])
            out[name] = (ins, refs)
        return out[name]
    return get


def forward_behind_a_gate(call, ins, side, cycles):
    """``call(inputs)`` under ``torch.cuda.stream(side)`` on inputs that are zeros, made on the default stream and settled,
    and are filled with ``ins`` by copies on ``side`` behind a gate: whatever ``call`` sends to another stream reads the
    zeros (or what its predecessors on ``side`` have not written yet).  Returns (result, the late inputs): the caller
    holds on to the inputs until it has settled -- they were allocated on the default stream, and the allocator would
    hand their memory to the next default-stream tensor while ``side`` still waits behind its gate."""
    late = tuple(torch.zeros_like(t) for t in ins)
    settle("the inputs")
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        for z, t in zip(late, ins):
            z.copy_(t)
        return call(late), late


# ------------------------------------------------------------------ a model on a side stream
@pytest.mark.parametrize("name, mode", [("acv", ""), ("pcw", ""), ("igev", "overlap"), ("igev", "no_overlap"), ("igev", "graph")],
                         ids=["acv", "pcw", "igev-overlap", "igev-no_overlap", "igev-graph"])
def test_model_on_a_side_stream(name, mode, gate, serial, monkeypatch):
    """``forward`` (eval) under ``torch.cuda.stream(S)`` on inputs that arrive on S behind a gate: a launch, a memset or
    a torch op of the forward that went to another stream would read them too early.  Everything the model builds once
    and keeps is built and settled by a throw-away forward BEFORE the gate (a build waits for its stream, which would
    drain the gate), and every compared forward has a gate and re-zeroed inputs of its own.  (A draw of the NoiseTape is
    a blocking copy from the host: from the first draw on the gate is drained; the front, the volume and the encoder
    of every model are launched before it.)  ``test_the_gate_catches_an_op_off_its_stream`` shows the power."""
    from diffuvolume_amd.igev_stereo_ddim import IGEVDiffusionLoop
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    ins, refs = serial(name)
    model = MODELS[name][0]()
    replays = []
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), replay(self))[1])
    old = BasicMultiUpdateBlock.OVERLAP, IGEVDiffusionLoop.use_graph
    try:
        if name == "igev":
            BasicMultiUpdateBlock.OVERLAP, IGEVDiffusionLoop.use_graph = mode != "no_overlap", mode == "graph"
        with taped(model):
            forward(name, model, ins[1], NoiseTape(7))                      # builds and settles plans and first-use caches
            settle(f"{name}: the throw-away forward")
            del replays[:]
            tape = NoiseTape(40)
            got = []
            for _ in range(2):
                out, keep = forward_behind_a_gate(lambda late: forward(name, model, late, tape).clone(), ins[0], gate.a, gate.cycles)
                settle(f"{name} on a side stream")
                got.append(out)
    finally:
        BasicMultiUpdateBlock.OVERLAP, IGEVDiffusionLoop.use_graph = old
    assert bool(replays) == (mode == "graph"), f"{len(replays)} graph replays in mode {mode!r}"
    for j, t in enumerate(got):
        assert torch.equal(t, refs[0][j]), f"{name} [{mode}] forward {j} on a side stream differs from the default-stream run"


class _TwoOps(nn.Module):
    """A stand-in model: y = 2 x + 1 in two ops through a buffer; ``leak`` sends the second one to the default stream."""

    def __init__(self, n, leak):
        super().__init__()
        self.leak = leak
        self.register_buffer("tmp", torch.full((n,), -1.0))

    def forward(self, x):
        torch.mul(x, 2.0, out=self.tmp)
        with torch.cuda.stream(torch.cuda.default_stream() if self.leak else torch.cuda.current_stream()):
            return self.tmp + 1.0


@pytest.mark.parametrize("leak", [False, True], ids=["keeps_to_its_stream", "one_op_on_the_default_stream"])
def test_the_gate_catches_an_op_off_its_stream(leak, gate):
    """The power of ``forward_behind_a_gate``: a module that sends one op to the default stream is caught, a correct one passes."""
    n = 1 << 16
    x = torch.randn(n, generator=torch.Generator().manual_seed(8))
    m = _TwoOps(n, leak).to(DEV)
    got, keep = forward_behind_a_gate(lambda late: m(*late), (x.to(DEV),), gate.a, gate.cycles)
    settle("the stand-in model")
    assert torch.equal(got.cpu(), 2.0 * x + 1.0) == (not leak)


# ------------------------------------------------------------------ plans built on A serve B
def prepare_all(model):
    return [m.prepare() for m in model.modules() if isinstance(m, PlanCache)]


@pytest.mark.parametrize("name, how", [("acv", "prepare"), ("pcw", "prepare"), ("acv", "first_forward"), ("pcw", "first_forward"),
                                       ("igev", "first_forward")])
def test_plans_built_on_one_stream_serve_another(name, how, gate, serial):
    """A fresh model builds on stream A behind a gate what it keeps; with no explicit wait a forward then runs on stream B,
    which the hardware runs independently of A (tests/streams.py).  "prepare": ``prepare()`` of the model and its
    plan-holding submodules.  "first_forward": a whole forward on A (other inputs, its own tape), which also builds what
    ``prepare()`` does not -- the plans ``_RefinePlan`` makes on first use, the loop's time-MLP shifts, the per-layer
    plans of IGEV's front (no PlanCache slot holds them, which is why IGEV has this form only)."""
    ins, refs = serial(name)
    model = MODELS[name][0]()
    with taped(model):
        if how == "prepare":
            with torch.cuda.stream(gate.a):
                torch.cuda._sleep(gate.cycles)
                prepare_all(model)
            first = keep = None
        else:
            first, keep = forward_behind_a_gate(lambda late: forward(name, model, late, NoiseTape(41)).clone(), ins[1], gate.a, gate.cycles)
        with torch.cuda.stream(gate.b):
            got = forward(name, model, ins[0], NoiseTape(40)).clone()
    settle(f"{name}: built on stream A, used on stream B")
    assert torch.equal(got, refs[0][0])
    assert first is None or torch.equal(first, refs[1][0])


def test_a_replica_finds_plans_parked_from_another_stream(gate, serial):
    """nn.DataParallel re-creates its replicas on every forward: the second replica finds the plans the first one built --
    on another stream -- parked on the source."""
    ins, refs = serial("acv")
    model = MODELS["acv"][0]()
    first = replica_of(model)
    with torch.cuda.stream(gate.a):
        torch.cuda._sleep(gate.cycles)
        built = prepare_all(first)
    second = replica_of(model)
    assert second._plans is None
    with taped(second), torch.cuda.stream(gate.b):
        got = forward("acv", second, ins[0], NoiseTape(40)).clone()
    settle("a replica on stream B with plans parked from stream A")
    assert second._plans is built[0], "the second replica built plans of its own"
    assert torch.equal(got, refs[0][0])


class _ScaledWeight(PlanCache, nn.Module):
    """A stand-in with a float-only plan: ``_build_plans`` is one torch op on the current stream."""

    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(5)))

    def _build_plans(self, slot):
        return torch.mul(self.weight.detach(), 2.0)


@pytest.mark.parametrize("through", ["_build_plans", "plans"])
def test_the_gate_catches_an_unordered_plan_build(through, gate):
    """The detector's power, on a plan that holds no index table: built DIRECTLY behind the gate on A and consumed on B the
    result is not there yet -- caught --; through ``plans()`` it is."""
    n = 1 << 20
    m = _ScaledWeight(n).to(DEV)
    x = torch.randn(n, generator=torch.Generator().manual_seed(6))
    want = x + 2.0 * m.weight.detach().cpu()
    xd = x.to(DEV)
    with torch.cuda.stream(gate.a):                       # the block the build will be handed holds something else
        torch.full((n,), -1.0, device=DEV)
    settle("the stand-in's setup")
    with torch.cuda.stream(gate.a):
        torch.cuda._sleep(gate.cycles)
        p = m._build_plans(None) if through == "_build_plans" else m.plans()
    with torch.cuda.stream(gate.b):
        got = xd + p
    settle("the stand-in")
    same = torch.equal(got.cpu(), want)
    assert same == (through == "plans"), ("an unordered build went unnoticed: the gate has no power" if same else
                                          "plans() handed out a plan its building stream had not finished")


# ------------------------------------------------------------------ two threads, two streams
@pytest.mark.parametrize("sharing", ["one_model", "two_replicas"])
@pytest.mark.parametrize("name", ["acv", "igev"])
def test_two_threads_two_streams(name, sharing, gate, serial):
    """Two threads, a stream each, released together; each runs its own inputs and its own NoiseTape through a FRESH model
    (so the plans are built while both run) that the two share, or through a replica each of one source."""
    ins, refs = serial(name)
    source = MODELS[name][0]()
    models = [source, source] if sharing == "one_model" else [replica_of(source), replica_of(source)]
    barrier, errors, outs = threading.Barrier(2), [], [None, None]

    def work(k):
        try:
            with torch.cuda.stream((gate.a, gate.b)[k]):
                tape = NoiseTape(40 + k)
                barrier.wait(timeout=JOIN_SECONDS)
                outs[k] = [forward(name, models[k], ins[k], tape).clone() for _ in range(FORWARDS)]
                torch.cuda.current_stream().synchronize()
        except BaseException as e:                        # re-raised in the test
            errors.append((k, e))
            barrier.abort()

    threads = [threading.Thread(target=work, args=(k,), name=f"stream-{k}") for k in range(2)]
    with taped(*set(models)):
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_SECONDS)
        alive = [t.name for t in threads if t.is_alive()]
        assert not alive, f"still running after {JOIN_SECONDS} s: {alive}"
    settle(f"{name}, two threads, {sharing}")
    if errors:
        raise errors[0][1]
    for k in range(2):
        for j in range(FORWARDS):
            assert torch.equal(outs[k][j], refs[k][j]), f"{name} ({sharing}): thread {k}, forward {j} differs from the serial run"
