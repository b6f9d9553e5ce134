"""The kernels of csrc/ddim.hip alone, branch by branch, against tests/ddim_statement.py: one DDIM state update of the
reference (SceneFlow/models/acv_ddim.py:272-294, :318-362; KITTI15/core/igev_stereo_ddim.py:265-272, :316-327) in plain
torch with the reference's dtypes, on the CPU.  The trajectory tests carry bars of 1e-3 px; a float32 rounding point kept in
the wrong place moves x_next by 1e-7.  Here x_start and mask are held bit for bit (every multiplication on their way is by
0.5 or 2, so contraction cannot move them), pred_eps, x_next and ens to the derived ulp bars of ddim_statement.py, which
test_ddim_statement_host.py shows a float64-everywhere update misses 1e7 times over.

The inputs are an edge map (ddim_statement.edge_inputs): every quarter-resolution pixel is one case -- an integer position
and the float32 just below it, the forced last bin, both clamps, 0..4 pixels kept, |disp - used| and unc exactly on their
thresholds -- crossed with mask0 in {0, 0.5, 1} and IGEV's coords0.  Every output starts as NaN and must end written."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ddim_statement as S
from diffuvolume_amd import _lib, ddim
from oracle import acv_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = lambda seed: torch.Generator().manual_seed(seed)

SHAPES = [(2, 12, 5, 7), (2, 48, 9, 15), (1, 2, 1, 1)]      # 70 of 128 threads; two blocks and a tail; the smallest accepted
STATES = [torch.float32, torch.float64]                    # the first step; every later one
FORMS = {"acv": dict(eta=1.0, dif_thr=1.0, unc_thr=3.0, ens_dif_thr=0.0),
         "igev": dict(eta=1.0, dif_thr=5.0, unc_thr=float("inf"), ens_dif_thr=3.0)}
DV_ERR_NULL, DV_ERR_SHAPE = -1, -2
OUTPUTS = ("x_start", "pred_eps", "x_next")
POINTERS = ("disp", "unc", "used", "coords0", "n01_f32", "n01_f64", "eps_f32", "eps_f64", "fill", "mask", "x_start",
            "pred_eps", "x_next", "ens")


@pytest.fixture(scope="module")
def tables():
    return ddim.Tables(torch.cumprod(1 - ddim.cosine_beta_schedule(1000), 0))


def coef(tables, form, nbins, time, time_next, cof=0.3):
    return ddim.step_coef(tables, time, time_next, cof, clamp_max=float(nbins - 1 if form == "igev" else 4 * nbins - 1),
                          **FORMS[form])


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def nans(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def inputs(form, shape, state, seed=0, last=False):
    """The edge map of this form and the state tensors of one step, on the CPU."""
    b, nbins, h, w = shape
    e = S.edge_inputs(b, nbins, h, w, form == "igev", seed)
    g = G(77 + seed)
    n01 = torch.rand(b, nbins, h, w, generator=g, dtype=state)
    n01.view(-1)[0], n01.view(-1)[-1] = 0.0, 1.0                      # both ends of the filter's range
    inp = {k: e[k] for k in ("disp", "unc", "used", "coords0", "mask0")}
    inp.update(n01=n01, eps=None if last else torch.randn(b, nbins, h, w, generator=g, dtype=state),
               fill=None if last else torch.rand(b, nbins, h, w, generator=g, dtype=torch.float64) * 2 - 1,
               ens0=torch.randn(b, 4 * h, 4 * w, generator=g) * 20)
    return inp


def raw_step(dev, k, b, nbins, h, w):
    """dv_ddim_step on a dict of device tensors (None: NULL), one per pointer of its signature."""
    rc = _lib.load().dv_ddim_step(*[_lib.ptr(dev.get(name)) for name in POINTERS], b, nbins, h, w, ctypes.byref(k),
                                  _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def device_args(inp, k, shape, want_pred=True):
    b, nbins, h, w = shape
    up = lambda t: None if t is None else t.to(DEV).contiguous()
    n01, eps = inp["n01"], inp["eps"]
    dev = {name: up(inp[name]) for name in ("disp", "unc", "used", "coords0", "fill")}
    dev["mask"], dev["ens"] = up(inp["mask0"].clone()), up(None if inp["ens0"] is None else inp["ens0"].clone())   # in / out
    for name, t in (("n01", n01), ("eps", eps)):
        dev[name + "_f32"] = up(t) if t is not None and t.dtype == torch.float32 else None
        dev[name + "_f64"] = up(t) if t is not None and t.dtype == torch.float64 else None
    dev["x_start"] = nans((b, nbins, h, w), torch.float32)
    dev["pred_eps"] = nans((b, nbins, h, w), torch.float64) if want_pred else None
    dev["x_next"] = None if k.last else nans((b, nbins, h, w), torch.float64)
    return dev


def run_step(inp, k, shape, want_pred=True):
    dev = device_args(inp, k, shape, want_pred)
    with torch.cuda.device(DEV):
        assert raw_step(dev, k, *shape) == 0
    return {name: None if dev[name] is None else dev[name].cpu() for name in OUTPUTS + ("mask", "ens")}


def check(inp, k, shape, got, what):
    """Every output of one call against the statement; prints the worst ratio of error to bar per output."""
    nbins = shape[1]
    xs, pn, mask, xn, ens = S.ddim_step_statement(inp["disp"], inp["unc"], inp["used"], inp["coords0"], inp["n01"], inp["eps"],
                                                  inp["fill"], inp["mask0"], inp["ens0"], k, nbins)
    for name in OUTPUTS + ("mask", "ens"):
        assert got[name] is None or bool(torch.isfinite(got[name]).all()), f"{what}: {name} not all written"
    flips = int((got["x_start"] != xs).any(dim=1).sum())
    assert same_bits(got["x_start"], xs), f"{what}: x_start differs at {flips} of {xs[:, 0].numel()} pixels"
    assert same_bits(got["mask"], mask), f"{what}: mask"
    ratios = {}

    def hold(name, value, ref, bar, where=None):
        r = (value.double() - ref.double()).abs() / bar
        r = r if where is None else r[where]
        ratios[name] = float(r.max()) if r.numel() else 0.0

    if got["pred_eps"] is not None:
        assert got["pred_eps"].dtype == pn.dtype == torch.float64
        hold("pred_eps", got["pred_eps"], pn, S.pred_eps_bar(k, inp["n01"]))
    if got["x_next"] is not None:
        assert got["x_next"].dtype == xn.dtype == torch.float64
        filled = (mask == 0).unsqueeze(1).expand_as(xn)
        assert same_bits(got["x_next"][filled], inp["fill"][filled]), f"{what}: x_next where mask == 0"
        hold("x_next", got["x_next"], xn, S.x_next_bar(k, xs, pn, inp["n01"], inp["eps"]), ~filled)
    if got["ens"] is not None:
        hold("ens", got["ens"], ens, S.ens_bar(k, S.output_rule(inp["disp"], inp["used"], k), ens).clamp(min=1e-300))
    print(f"    {what}: error / bar " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, f"{what}: {name} is {r:.3f} of its bar"
    return mask


@pytest.mark.parametrize("state", STATES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", ["acv", "igev"])
def test_step_against_the_statement(tables, form, shape, state):
    """ACV / PCW: unc, no coords0, no output rule.  IGEV: coords0, unc NULL, unc_thr inf, clamp_max nbins - 1, output rule
    dif < 3 with a pixel exactly on 3.  The coefficients of the first and of a middle pair of a 5-step loop."""
    seen = set()
    for time, time_next in (ddim.time_pairs(1000, 5)[0], ddim.time_pairs(1000, 5)[2]):
        k = coef(tables, form, shape[1], time, time_next)
        inp = inputs(form, shape, state)
        assert (inp["unc"] is None) == (form == "igev") == (inp["coords0"] is not None)
        mask = check(inp, k, shape, run_step(inp, k, shape), f"{form} {shape} {state} t={time}")
        seen |= set(mask.unique().tolist())
    if shape[2] * shape[3] > 1:
        assert {0.0, 0.25} <= seen                          # some pixels take `fill`, some are kept by one pixel of four


@pytest.mark.parametrize("state", STATES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", ["acv", "igev"])
def test_last_step_with_pred_eps(tables, form, shape, state):
    """The `model_predictions` form: last = 1, used = disp, a zero mask, pred_eps wanted, x_next and ens NULL."""
    k = coef(tables, form, shape[1], 999, -1, cof=0.0)
    inp = inputs(form, shape, state, seed=1, last=True)
    inp.update(used=inp["disp"], mask0=torch.zeros_like(inp["mask0"]), ens0=None)
    got = run_step(inp, k, shape)
    assert k.last == 1 and got["x_next"] is None and got["ens"] is None and got["pred_eps"] is not None
    check(inp, k, shape, got, f"last+pred_eps {form} {shape} {state}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", ["acv", "igev"])
def test_last_step_without_pred_eps(tables, form, shape):
    """last = 1, pred_eps NULL and both n01 pointers NULL: x_start, mask and ens alone."""
    k = coef(tables, form, shape[1], 199, -1)
    inp = inputs(form, shape, torch.float64, seed=2, last=True)
    inp["n01"] = None
    got = run_step(inp, k, shape, want_pred=False)
    assert got["pred_eps"] is None and got["x_next"] is None
    check(inp, k, shape, got, f"last {form} {shape}")


@pytest.mark.parametrize("state", STATES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_zero_weight_leaves_the_ensemble(tables, shape, state):
    time, time_next = ddim.time_pairs(1000, 5)[2]
    k = coef(tables, "acv", shape[1], time, time_next, cof=0.0)
    inp = inputs("acv", shape, state, seed=3)
    got = run_step(inp, k, shape)
    assert same_bits(got["ens"], inp["ens0"])
    got["ens"] = None
    check(inp, k, shape, got, f"cof=0 {shape} {state}")


@pytest.mark.parametrize("state", STATES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_no_ensemble(tables, shape, state):
    time, time_next = ddim.time_pairs(1000, 5)[0]
    k = coef(tables, "igev", shape[1], time, time_next)
    inp = inputs("igev", shape, state, seed=4)
    inp["ens0"] = None
    check(inp, k, shape, run_step(inp, k, shape), f"ens=NULL {shape} {state}")


def test_outer_pixels_reach_the_ensemble_only(tables):
    """The twelve outer pixels of each 4x4 cell: not in x_start, mask or x_next, all of them in ens."""
    shape = SHAPES[0]
    b, nbins, h, w = shape
    time, time_next = ddim.time_pairs(1000, 5)[2]
    k = coef(tables, "acv", nbins, time, time_next)
    inp = inputs("acv", shape, torch.float64, seed=5)
    first = run_step(inp, k, shape)
    centre = torch.zeros(b, 4 * h, 4 * w, dtype=torch.bool)
    for dy in (1, 2):
        for dx in (1, 2):
            centre[:, dy::4, dx::4] = True
    g = G(6)
    other = dict(inp)
    for name, scale in (("disp", 60.0), ("used", 60.0), ("unc", 5.0)):
        other[name] = torch.where(centre, inp[name], torch.rand(b, 4 * h, 4 * w, generator=g) * scale - 5)
    second = run_step(other, k, shape)
    for name in ("x_start", "pred_eps", "mask", "x_next"):
        assert same_bits(first[name], second[name]), name
    assert float((first["ens"] != second["ens"])[~centre].float().mean()) > 0.99
    assert same_bits(first["ens"][centre], second["ens"][centre])
    check(other, k, shape, second, "outer pixels")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", ["acv", "igev"])
def test_x_start_and_mask_are_atens_on_the_device(tables, form, shape):
    """The kernel's `down4` is "evaluated in PyTorch's order": x_start and mask bit for bit what ATen's own bilinear kernel
    on the GPU, floor, scatter and the last-bin `where` give -- what the reference computes."""
    b, nbins, h, w = shape
    k = coef(tables, form, nbins, 199, -1)
    inp = inputs(form, shape, torch.float32, seed=7, last=True)
    got = run_step(inp, k, shape)
    with torch.cuda.device(DEV):
        disp, used, mask0 = inp["disp"].to(DEV), inp["used"].to(DEV), inp["mask0"].to(DEV)
        dn = F.interpolate(disp.clamp(0, k.clamp_max)[:, None], size=(h, w), mode="bilinear") / 4
        if form == "igev":
            dn = torch.clamp(inp["coords0"].to(DEV)[:, None] + dn, 0, nbins - 1)
        x_start = torch.clamp(S.two_hot(dn, nbins) * 2 - 1., -1, 1)
        keep = torch.abs(disp - used) < k.dif_thr
        if form == "acv":
            keep = keep & (inp["unc"].to(DEV) < k.unc_thr)
        mask = torch.clamp(mask0 + F.interpolate(keep.float()[:, None], size=(h, w), mode="bilinear")[:, 0], 0, 1)
        mine = S.quarter_position(inp["disp"], inp["coords0"], k.clamp_max, nbins)
        flips = int((dn.cpu().floor() != mine.floor()).sum())
    moved = int((dn.cpu() != mine).sum())
    print(f"    ATen on the device, {form} {shape}: {moved} positions differ, {flips} floor decisions flip")
    assert same_bits(got["x_start"], x_start), f"{flips} floor decisions flip, {moved} of {dn.numel()} positions differ"
    assert same_bits(got["mask"], mask)


# ---- dv_noise_prepare_f32 / f64 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("state", STATES, ids=["f32", "f64"])
def test_noise_prepare(state):
    """Bit-equal to ((x + shift).clamp(-1, 1) + 1) / 2 in the state's dtype, n01_f32 to its float32; x + shift exactly on -1
    and +1, one float of the state's dtype inside and outside each, and far beyond both.  Six full blocks and a tail."""
    b, c, hw = 2, 5, 173
    g = G(8)
    shift = torch.randn(b, c, generator=g)
    shift[0] = torch.tensor([0.0, 0.25, -0.5, 0.75, -1.0])            # batch 0: the sums below are exact
    x = torch.randn(b, c, 1, hw, generator=g, dtype=state) * 0.8
    one = torch.ones(c, dtype=state)
    s0 = shift[0].to(state)
    edges = [-one, one, torch.nextafter(-one, one), torch.nextafter(-one, -2 * one), torch.nextafter(one, -one),
             torch.nextafter(one, 2 * one), -1.5 * one, 1.5 * one, -40 * one, 40 * one]
    for i, e in enumerate(edges):
        x[0, :, 0, i] = e - s0
        exact = x[0, :, 0, i] + s0 == e                                # the neighbours of +-1: with a zero shift at least
        assert bool(exact[0]) and (bool(exact.all()) or 2 <= i <= 5)
    ref = S.noise_prepare_statement(x, shift)
    assert ref.dtype == state and float(ref.min()) == 0.0 and float(ref.max()) == 1.0
    assert 0 < float(ref[0, 0, 0, 2]) < 1e-7                           # one float inside -1 is not clamped
    lib = _lib.load()
    with torch.cuda.device(DEV):
        xd, sd = x.to(DEV), shift.to(DEV)
        n01 = nans(x.shape, state)
        if state == torch.float32:
            rc = lib.dv_noise_prepare_f32(xd.data_ptr(), sd.data_ptr(), n01.data_ptr(), b, c, hw, _lib.stream_ptr())
        else:
            n01f = nans(x.shape, torch.float32)
            rc = lib.dv_noise_prepare_f64(xd.data_ptr(), sd.data_ptr(), n01.data_ptr(), n01f.data_ptr(), b, c, hw,
                                          _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert same_bits(n01, ref)
        if state == torch.float64:
            assert same_bits(n01f, ref.float())
        # the launcher: the same bits, and for a float32 state one tensor in both roles
        a, a32 = ddim.noise_prepare(None, xd, None, shift=sd)
        torch.cuda.synchronize()
        assert same_bits(a, ref) and same_bits(a32, ref.float()) and (a32 is a) == (state == torch.float32)


# ---- dv_encode_two_hot_f32 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", [2, 12, 48])
def test_encode_two_hot(nbins):
    """Bit-equal to the oracle's two-hot * 2 - 1 on every integer of [0, nbins), its two float32 neighbours and
    nbins - 0.5.  Outside [0, nbins) the oracle raises (scatter index out of range) and the kernel writes quietly what
    its arithmetic gives: pinned here as finite, in [-1, 1], and all -1 from nbins upwards."""
    ints = torch.arange(nbins, dtype=torch.float32)
    inside = torch.cat([ints, torch.nextafter(ints, ints + 1), torch.nextafter(ints[1:], ints[1:] - 1),
                        torch.tensor([nbins - 0.5]), torch.nextafter(torch.tensor([float(nbins)]), torch.tensor([0.0]))])
    inside = torch.stack([inside, inside.flip(0)]).view(2, 1, 1, -1)
    ref = O.encode_two_hot(inside, nbins) * 2 - 1
    with torch.cuda.device(DEV):
        got = ddim.encode_two_hot(inside.to(DEV), nbins)
        torch.cuda.synchronize()
    assert same_bits(got, ref)
    top = torch.tensor(float(nbins))
    outside = torch.tensor([[-1e-45, -0.5, -1.0, -1.5, -100.0, -1e6],
                            [float(top), float(torch.nextafter(top, 2 * top)), nbins + 0.5, nbins + 1.0, 2.0 * nbins, 1e6]])
    with pytest.raises(RuntimeError):
        O.encode_two_hot(outside.view(2, 1, 1, -1), nbins)
    with torch.cuda.device(DEV):
        x = nans((2, nbins, 1, outside.shape[1]), torch.float32)
        rc = _lib.load().dv_encode_two_hot_f32(outside.to(DEV).data_ptr(), x.data_ptr(), 2, nbins, outside.shape[1],
                                               _lib.stream_ptr())
        torch.cuda.synchronize()
    x = x.cpu()
    assert rc == 0 and bool(torch.isfinite(x).all()) and float(x.min()) >= -1 and float(x.max()) <= 1
    assert bool((x[1] == -1).all())


# ---- refusals -----------------------------------------------------------------------------------------------------

def _both_n01(dev, dims):
    dev["n01_f64"] = dev["n01_f32"].double()


def _drop(*names):
    def change(dev, dims):
        for name in names:
            dev[name] = None
    return change


def _dim(name, value):
    def change(dev, dims):
        dims[name] = value
    return change


REFUSALS = {"both n01": (_both_n01, DV_ERR_NULL), "no n01": (_drop("n01_f32", "n01_f64"), DV_ERR_NULL),
            "no eps": (_drop("eps_f32", "eps_f64"), DV_ERR_NULL), "no fill": (_drop("fill"), DV_ERR_NULL),
            "no x_next": (_drop("x_next"), DV_ERR_NULL), "nbins 1": (_dim("nbins", 1), DV_ERR_SHAPE),
            "B 0": (_dim("b", 0), DV_ERR_SHAPE)}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(tables, case):
    """A call the entry refuses returns the code of the check that refused it and launches nothing: every output still
    holds its NaN, mask and ens their input."""
    shape = SHAPES[0]
    time, time_next = ddim.time_pairs(1000, 5)[0]
    k = coef(tables, "acv", shape[1], time, time_next)
    assert k.last == 0
    inp = inputs("acv", shape, torch.float32, seed=9)
    change, code = REFUSALS[case]
    with torch.cuda.device(DEV):
        dev = device_args(inp, k, shape)
        dims = dict(zip("b nbins h w".split(), shape))
        change(dev, dims)
        assert raw_step(dev, k, dims["b"], dims["nbins"], dims["h"], dims["w"]) == code
    for name in OUTPUTS:
        assert dev[name] is None or bool(torch.isnan(dev[name]).all()), name
    assert same_bits(dev["mask"], inp["mask0"]) and same_bits(dev["ens"], inp["ens0"])


def test_ddim_update_refuses_a_float16_eps(tables):
    shape = SHAPES[0]
    time, time_next = ddim.time_pairs(1000, 5)[0]
    k = coef(tables, "acv", shape[1], time, time_next)
    inp = inputs("acv", shape, torch.float32, seed=10)
    with torch.cuda.device(DEV):
        d = {name: t.to(DEV) for name, t in inp.items() if t is not None}
        mask, ens = d["mask0"].clone(), d["ens0"].clone()
        with pytest.raises(_lib.DiffuVolumeError, match="dv_ddim_step"):
            ddim.ddim_update(d["disp"], d["used"], d["n01"], d["eps"].half(), d["fill"], mask, ens, k, unc=d["unc"])
        torch.cuda.synchronize()
    assert same_bits(mask, inp["mask0"]) and same_bits(ens, inp["ens0"])


# ---- three chained steps through the Python launchers -------------------------------------------------------------

@pytest.mark.parametrize("form", ["acv", "igev"])
def test_three_chained_steps(tables, form):
    """ddim.noise_prepare and ddim.ddim_update over a 3-step loop with fixed random tensors in the network's place: the
    state enters float32 and is float64 from the second step on, eps drawn in the state's dtype.  Each step teacher-forced
    (from the statement's state) at the bars of the single step; the free run's last float64 state at three times the
    x_next bar, its last x_start bit for bit."""
    shape = b, nbins, h, w = SHAPES[1]
    g = G(11)
    shift = torch.randn(b, nbins, generator=g) * 0.3
    state = torch.randn(b, nbins, h, w, generator=g)                                   # x_T, float32
    mask, ens = torch.zeros(b, h, w), S.edge_inputs(b, nbins, h, w, form == "igev", 20)["used"] * 0.5
    free = {"state": state.to(DEV), "mask": mask.clone().to(DEV), "ens": ens.clone().to(DEV)}
    pairs = ddim.time_pairs(1000, 3)
    with torch.cuda.device(DEV):
        sd = shift.to(DEV)
        for i, (time, time_next) in enumerate(pairs):
            k = coef(tables, form, nbins, time, time_next, cof=(0.2, 0.0, 0.3)[i])
            assert state.dtype == (torch.float32 if i == 0 else torch.float64) and k.last == int(i == 2)
            e = S.edge_inputs(b, nbins, h, w, form == "igev", 21 + i)
            eps = None if k.last else torch.randn(b, nbins, h, w, generator=g, dtype=state.dtype)
            fill = None if k.last else torch.rand(b, nbins, h, w, generator=g, dtype=torch.float64) * 2 - 1
            n01 = S.noise_prepare_statement(state, shift)
            inp = dict(disp=e["disp"], unc=e["unc"], used=e["used"], coords0=e["coords0"], n01=n01, eps=eps, fill=fill,
                       mask0=mask, ens0=ens)
            up = lambda t: None if t is None else t.to(DEV)
            net = {name: up(e[name]) for name in ("disp", "unc", "used", "coords0")}

            def step(state_d, mask_d, ens_d):
                a, a32 = ddim.noise_prepare(None, state_d, None, shift=sd)
                assert a.dtype == state_d.dtype and a32.dtype == torch.float32
                xs, xn, pn = ddim.ddim_update(net["disp"], net["used"], a, up(eps), up(fill), mask_d, ens_d, k,
                                              unc=net["unc"], coords0=net["coords0"], want_pred_noise=True)
                torch.cuda.synchronize()
                return a, a32, xs, xn, pn

            # teacher-forced
            mask_d, ens_d = mask.clone().to(DEV), ens.clone().to(DEV)
            a, a32, xs, xn, pn = step(state.to(DEV), mask_d, ens_d)
            assert same_bits(a, n01) and same_bits(a32, n01.float())
            got = {"x_start": xs.cpu(), "pred_eps": pn.cpu(), "x_next": None if xn is None else xn.cpu(), "mask": mask_d.cpu(),
                   "ens": ens_d.cpu()}
            assert (xn is None) == bool(k.last)
            check(inp, k, shape, got, f"chained {form} step {i} ({state.dtype})")
            xs_s, pn_s, mask, xn_s, ens = S.ddim_step_statement(e["disp"], e["unc"], e["used"], e["coords0"], n01, eps, fill,
                                                                mask, ens, k, nbins)
            # free run
            _, _, fxs, fxn, _ = step(free["state"], free["mask"], free["ens"])
            assert same_bits(free["mask"], mask) and same_bits(fxs, xs_s)
            if not k.last:
                assert fxn.dtype == torch.float64
                filled = (mask == 0).unsqueeze(1).expand_as(xn_s)
                r = ((fxn.cpu() - xn_s).abs() / (3 * S.x_next_bar(k, xs_s, pn_s, n01, eps)))[~filled]
                print(f"    chained {form} step {i}: free-run state error / (3 x bar) {float(r.max()):.3f}")
                assert same_bits(fxn.cpu()[filled], fill[filled])
                assert float(r.max()) <= 1.0
                free["state"], state = fxn, xn_s
