"""SceneFlow ACVNet_DDIM on the HIP path against the IMPORTED REFERENCE's own outputs, at the contract's RAW bars, on the
conditioned network of oracle/calibrate.py (BatchNorm buffers = statistics of the data; fixtures written by
oracle/make_golden_acv_conditioned.py).  On this network the fp32 oracle is within 1e-3 px of its float64 evaluation on
every pixel of every step (tests/test_oracle_acv_conditioned.py), so two correct fp32 evaluations must agree within the
bar: |d disp| <= 1e-3 px on 99.9 % of the pixels, |d EPE| < 1e-4.  This is the statement of the contract for the
headline path; tests/test_gpu_parity.py keeps the looser figures of the unconditioned network as regression ceilings.

Every fixture runs under both routings of the 3x3x3 stride-1 layers: the shipped one (the F(2x2x2,3x3x3) kernel of
csrc/conv3d_wino3.hip from 64 input channels on) and the in-plane F(2x2,3x3) kernel everywhere."""
import pytest
import torch

from conftest import load_golden
from diffuvolume_amd import _lib
from diffuvolume_amd import submodule as S
from diffuvolume_amd.synth import NoiseTape
from oracle import acv_oracle as O
from oracle import calibrate as C
from oracle import loop_parity as LP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = ["acv_conditioned_16x32", "acv_conditioned_24x32_b2"]
ROUTINGS = ["shipped", "in_plane"]
# F(2x2x2) launches per DDIM step under the shipped routing: conv2 (64 -> 64) and conv4 (128 -> 128) of the hourglasses
# dres2 and dres3.  dres0's first layer (64 -> 32) carries the noise filter as its input prologue, which that kernel does
# not take: it runs on the in-plane kernel for a plain volume (csrc/rank1_filter.hip for a factor handle) either way.
WINO3_PER_STEP = 4

_RUNS = {}


def dev(t):
    return t.to(DEV)


def _epe(disp, used):
    return float((disp.cpu() - used).abs().mean())


def _setup(name):
    """Fixture, conditioned weights, the model on the device, the input volume and the fp32 oracle's trajectory (cached:
    both routings of a fixture share them)."""
    if name not in _RUNS:
        from diffuvolume_amd import ACVNet_DDIM
        g = load_golden(name)
        sd = C.conditioned_acv_state_dict(g)
        m = ACVNet_DDIM(192, False, False)
        m.load_state_dict(sd, strict=True)
        x = C.conditioned_acv_inputs(g["batch"], g["h"], g["w"], g["seed"])
        orc = O.ACVDiffusionOracle(sd)
        final_o, stack_o, trace = LP.oracle_trajectory(orc, x["vol"], g["used"], g["x_T"], g["tape_seed"])
        _, _, d64, _ = O.ACVDiffusionOracle(C.f64_state_dict(sd)).model_predictions(x["vol"].double(), g["x_T"], g["t"])
        _RUNS.clear()
        _RUNS[name] = dict(g=g, sd=sd, model=m.to(DEV).eval(), vol=x["vol"], final_o=final_o, stack_o=stack_o,
                           trace=trace, d64=d64)
    return _RUNS[name]


@pytest.fixture(params=ROUTINGS)
def routing(request, monkeypatch):
    """Sets the routing and counts the calls into the F(2x2x2) kernel's entry point."""
    lib = _lib.load()
    real, calls = lib.dv_conv3d_wino3_f32, {"n": 0}

    def counting(*args):
        calls["n"] += 1
        return real(*args)

    monkeypatch.setattr(lib, "dv_conv3d_wino3_f32", counting)
    keep = (S.Conv3dPlan.WINO3, S.Conv3dPlan.WINO3_MIN_CIN)
    S.Conv3dPlan.WINO3 = request.param == "shipped"
    try:
        yield request.param, calls
    finally:
        S.Conv3dPlan.WINO3, S.Conv3dPlan.WINO3_MIN_CIN = keep


def _expect_launches(route, calls, steps):
    want = WINO3_PER_STEP * steps if route == "shipped" else 0
    assert calls["n"] == want, (route, calls["n"], want)
    calls["n"] = 0


@pytest.mark.parametrize("name", FIXTURES)
def test_conditioned_network_against_the_reference(name, routing):
    """(1) Step 1 against the reference's model_predictions: at most max(1e-3, 1/npx) of the pixels beyond 1e-3 px, mean
    below 1e-4 px, |d EPE| (against `used`) below 1e-4, uncertainty within 1e-3 on average, and EVERY pixel within
    1e-3 px of the float64 oracle.  (2) The 5-step loop against the oracle at raw bars, teacher forced and decision
    forced (oracle/loop_parity.py), and -- when no renewal decision comes out differently -- every step of the stack and
    the ensemble against the reference's own ddim_sample at raw bars.  The F(2x2x2) kernel is counted: exactly
    WINO3_PER_STEP launches per step under the shipped routing, none in-plane."""
    route, calls = routing
    r = _setup(name)
    g, m, vol, used = r["g"], r["model"], r["vol"], r["g"]["used"]
    npx = g["disp"].numel()
    bar = max(LP.BAR_FRAC, 1.0 / npx)
    vol_d, used_d = dev(vol), dev(used)
    calls["n"] = 0

    # (1) step 1
    pn, xs, disp, handle = m.model_predictions(vol_d, dev(g["x_T"]), dev(g["t"]))
    torch.cuda.synchronize()
    _expect_launches(route, calls, 1)
    disp = disp.cpu()
    d = (disp - g["disp"]).abs()
    n_off = int((d > LP.BAR_PX).sum())
    e64 = (disp.double() - r["d64"]).abs()
    print(f"{name} [{route}] step 1 vs reference: {n_off} of {npx} pixels beyond 1e-3 px, mean {float(d.mean()):.2e}, "
          f"max {float(d.max()):.2e} px; vs float64 max {float(e64.max()):.2e} px")
    assert n_off / npx <= bar and float(d.mean()) < 1e-4, (n_off, float(d.mean()), float(d.max()))
    assert abs(_epe(disp, used) - _epe(g["disp"], used)) < LP.BAR_EPE
    assert float((handle.uncertainty.cpu() - g["unc"]).abs().mean()) < 1e-3
    assert float(e64.max()) < LP.BAR_PX, float(e64.max())

    # (2) the loop: free run against the reference's stack
    stack = [used]

    def keep(i, st):
        if st["when"] == "out":
            stack.append(st["disp"].cpu().clone())

    final, _ = m.ddim_sample(vol_d, used_d, dev(g["x_T"]), noise=NoiseTape(g["tape_seed"]), trace=keep)
    torch.cuda.synchronize()
    nsteps = len(r["trace"])
    _expect_launches(route, calls, nsteps)
    final = final.cpu()
    tf = LP.teacher_forced(m, r["trace"], vol_d, used_d, used, used)
    df = LP.decision_forced(m, r["trace"], vol_d, used_d, g["x_T"], used)
    fr = LP.free_run(m, r["trace"], r["stack_o"], r["final_o"], vol_d, used_d, g["x_T"], used, g["tape_seed"])
    calls["n"] = 0
    for s in tf + df:
        assert s["frac_gt_1e-3"] <= bar and s["epe_delta"] < LP.BAR_EPE, s
    flips = sum(s["flips_mask_zero"] for s in fr["steps"])
    offending = [int(((stack[i] - g["stack"][i]).abs() > LP.BAR_PX).sum()) for i in range(1, nsteps + 1)]
    print(f"{name} [{route}] loop: pixels beyond 1e-3 px vs the reference per step {offending}, renewal flips {flips}; "
          f"teacher forced {[s['frac_gt_1e-3'] for s in tf]}, decision forced {[s['frac_gt_1e-3'] for s in df]}")
    if flips == 0:
        for s in fr["steps"]:
            assert s["frac_gt_1e-3"] <= bar and s["epe_delta"] < LP.BAR_EPE, ("free run", s)
        for i in range(1, nsteps + 1):
            di = (stack[i] - g["stack"][i]).abs()
            assert float((di > LP.BAR_PX).float().mean()) <= bar, (i, float(di.mean()), float(di.max()))
            assert abs(_epe(stack[i], used) - _epe(g["stack"][i], used)) < LP.BAR_EPE, i
        dfin = (final - g["final"]).abs()
        assert float((dfin > LP.BAR_PX).float().mean()) <= bar, (float(dfin.mean()), float(dfin.max()))
        assert abs(_epe(final, used) - _epe(g["final"], used)) < LP.BAR_EPE


def test_batch_items_alone_give_the_same_bits(routing):
    """The B = 2 fixture: each item run alone (model_predictions and the 5-step loop, its slice of the batch's draws)
    gives the bits of its slice of the batch run."""
    route, calls = routing
    r = _setup("acv_conditioned_24x32_b2")
    g, m = r["g"], r["model"]
    vol_d, used_d, x_d, t_d = dev(r["vol"]), dev(g["used"]), dev(g["x_T"]), dev(g["t"])
    b = vol_d.shape[0]
    _, _, disp_b, h_b = m.model_predictions(vol_d, x_d, t_d)
    unc_b = h_b.uncertainty.clone()
    tape_b = NoiseTape(g["tape_seed"])
    final_b, stack_b = m.ddim_sample(vol_d, used_d, x_d, noise=tape_b)
    for i in range(b):
        sl = slice(i, i + 1)
        _, _, disp_i, h_i = m.model_predictions(vol_d[sl].contiguous(), x_d[sl].contiguous(), t_d[sl].contiguous())
        assert torch.equal(disp_i, disp_b[sl]) and torch.equal(h_i.uncertainty, unc_b[sl]), i
        tape = NoiseTape(g["tape_seed"])

        def draw(kind, shape, dtype):                   # the batch's draws, sliced to this item
            return tape(kind, (b,) + tuple(shape[1:]), dtype)[sl]

        final_i, stack_i = m.ddim_sample(vol_d[sl].contiguous(), used_d[sl].contiguous(), x_d[sl].contiguous(), noise=draw)
        assert torch.equal(final_i, final_b[sl]) and torch.equal(stack_i, stack_b[:, sl]), i
    torch.cuda.synchronize()
    want = WINO3_PER_STEP * (1 + 5) * (1 + b) if route == "shipped" else 0
    assert calls["n"] == want, (route, calls["n"], want)
