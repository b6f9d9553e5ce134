"""The backward of IGEV's geometry lookup on the MI355X (dv_geo_filter_lookup_bwd_f32, and through it
dv_allpairs_corr_bwd_f32) against float64 autograd of oracle.igev_oracle.geo_filter_lookup.

Bar, per gradient (dgeo, dfmap1, dfmap2), as relative L2 against the float64 gradient:
    rel(hip, f64) <= 2 * err32 + 1e-6
with err32 the relative L2 error of the SAME oracle expression run in float32 on the CPU (2x: HIP reorders the same
float32 sums).  The cotangent is float32-representable and the loss a plain sum, so the oracle's closing `.float()` rounds
nothing on the way back.  Integer and out-of-range disparities are asserted like every other case: the gradients are
continuous in the disparity.

Shapes (B, C, D, h, w, W2): IGEV's C and D with a partial last block and wave; an odd D (not a multiple of 4) with fewer
pixels than a wave; D below the 24-entry window with W2 != W1; an odd W2 with a row longer than a wave.  Four kinds of
disparity each: uniform in [-5, D+5), integers in [-3, D+3), a smooth ramp, lanes alternating between 0 and D-1.

Measured on the MI355X (worst over the 16 cases): dgeo 1.08e-6 against a bar of 3.17e-6 (err32 1.08e-6), dfmap1 9.5e-7
against 2.90e-6 (err32 9.5e-7), dfmap2 1.05e-6 against 3.09e-6 (err32 1.05e-6): the HIP gradients carry the float32
oracle's error, which is that of the sample positions."""
import pytest
import torch

from diffuvolume_amd import _lib
from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
from diffuvolume_amd.synth import _gen
from oracle.igev_oracle import geo_filter_lookup

pytestmark = pytest.mark.gpu
SHAPES = [(2, 8, 48, 5, 37, 37), (1, 3, 13, 3, 21, 21), (1, 8, 14, 2, 9, 12), (1, 2, 48, 1, 70, 35)]
KINDS = ("uniform", "integer", "ramp", "alternate")
FEAT = 6
NAMES = ("geo", "fmap1", "fmap2")


def make_inputs(shape, kind):
    """CPU float32 tensors: geo, fmap1, fmap2, disp, coords, noisy, cot."""
    b, c, d, h, w, w2 = shape
    seed = 1000 + 10 * SHAPES.index(shape) + KINDS.index(kind)
    rnd = lambda key, *s: torch.randn(*s, generator=_gen(seed, key))
    n = b * h * w
    if kind == "uniform":
        disp = torch.rand(n, generator=_gen(seed, "disp")) * (d + 10) - 5
    elif kind == "integer":
        disp = torch.randint(-3, d + 3, (n,), generator=_gen(seed, "disp")).float()
    elif kind == "ramp":
        disp = torch.linspace(0.25, d - 1.25, n)
    else:
        disp = torch.where(torch.arange(n) % 2 == 0, torch.zeros(n), torch.full((n,), float(d - 1)))
    coords = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(b, 1, h, w).contiguous()
    return dict(geo=rnd("geo", b, c, d, h, w), fmap1=rnd("f1", b, FEAT, h, w), fmap2=rnd("f2", b, FEAT, h, w2),
                disp=disp.view(b, 1, h, w), coords=coords, noisy=rnd("noisy", b, d, h, w),
                cot=rnd("cot", b, 2 * (9 * c + 9), h, w))


def oracle_grads(x, dtype):
    leaves = [x[n].detach().clone().to(dtype).requires_grad_(True) for n in NAMES]
    out = geo_filter_lookup(leaves[0], leaves[1], leaves[2], x["disp"].to(dtype), x["coords"].to(dtype), x["noisy"].to(dtype))
    (out * x["cot"]).sum().backward()
    return {n: t.grad.double() for n, t in zip(NAMES, leaves)}


_REF = {}


def reference(shape, kind):
    """(inputs, float64 gradients, err32 per gradient), computed once per case and shared, never modified."""
    if (shape, kind) not in _REF:
        x = make_inputs(shape, kind)
        g64, g32 = oracle_grads(x, torch.float64), oracle_grads(x, torch.float32)
        _REF[shape, kind] = (x, g64, {n: rel(g32[n], g64[n]) for n in NAMES})
    return _REF[shape, kind]


def rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def hip_step(x, need=(True, True, True)):
    """Forward + backward through the product's training route -> (out, {name: grad or None})."""
    leaves = {n: x[n].detach().cuda().requires_grad_(r) for n, r in zip(NAMES, need)}
    vol = Combined_Geo_Encoding_Volume(leaves["fmap1"], leaves["fmap2"], leaves["geo"])
    out = vol(x["disp"].cuda(), x["coords"].cuda(), x["noisy"].cuda())
    (out * x["cot"].cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {n: t.grad for n, t in leaves.items()}


def abi_bwd(go, disp, coords, noisy, dims, want_geo=True, want_corr=True):
    """dv_geo_filter_lookup_bwd_f32 straight through the C ABI, outputs pre-filled with NaN."""
    b, c, d, h, w, w2 = dims
    dgeo = torch.full((b, c, d, h, w), float("nan"), device="cuda")
    dcorr = torch.full((b, h, w, w2), float("nan"), device="cuda")
    code = _lib.load().dv_geo_filter_lookup_bwd_f32(go.data_ptr(), disp.data_ptr(), coords.data_ptr(), noisy.data_ptr(),
                                                    dgeo.data_ptr() if want_geo else None,
                                                    dcorr.data_ptr() if want_corr else None, b, c, d, h, w, w2, 4,
                                                    _lib.stream_ptr())
    torch.cuda.synchronize()
    assert code == 0, code
    return dgeo, dcorr


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_match_float64_autograd(shape, kind):
    x, g64, err32 = reference(shape, kind)
    _, grads = hip_step(x)
    bad = []
    for n in NAMES:
        e, bar = rel(grads[n], g64[n]), 2 * err32[n] + 1e-6
        print(f"PARITY lookup bwd {shape} {kind} d{n}: {e:.3e}  err32 {err32[n]:.3e}  bar {bar:.2e}")
        assert torch.isfinite(grads[n]).all()
        if not e <= bar:
            bad.append((n, e, bar))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_abi_writes_every_element_once_and_reproducibly(shape):
    """Outputs pre-filled with NaN come back fully written; a NULL output leaves the other one's bits alone; an offset
    (4-byte aligned) view of the noise gives the same bits; two launches give the same bits; dgeo through autograd is
    the kernel's output."""
    x, _, _ = reference(shape, "uniform")
    go, disp, coords, noisy = (x[k].cuda() for k in ("cot", "disp", "coords", "noisy"))
    dgeo, dcorr = abi_bwd(go, disp, coords, noisy, shape)
    assert not torch.isnan(dgeo).any() and not torch.isnan(dcorr).any()
    dgeo2, dcorr2 = abi_bwd(go, disp, coords, noisy, shape)
    assert same_bits(dgeo, dgeo2) and same_bits(dcorr, dcorr2)
    only_geo, untouched = abi_bwd(go, disp, coords, noisy, shape, want_corr=False)
    assert same_bits(only_geo, dgeo) and torch.isnan(untouched).all()
    untouched, only_corr = abi_bwd(go, disp, coords, noisy, shape, want_geo=False)
    assert same_bits(only_corr, dcorr) and torch.isnan(untouched).all()
    shifted = torch.empty(noisy.numel() + 1, device="cuda")[1:].view_as(noisy).copy_(noisy)
    assert shifted.data_ptr() % 16 == 4
    dgeo3, dcorr3 = abi_bwd(go, disp, coords, shifted, shape)
    assert same_bits(dgeo3, dgeo) and same_bits(dcorr3, dcorr)
    _, grads = hip_step(x, need=(True, False, False))
    assert same_bits(grads["geo"], dgeo)


def test_batch_of_two_equals_two_batches_of_one():
    shape = SHAPES[0]
    x, _, _ = reference(shape, "uniform")
    go, disp, coords, noisy = (x[k].cuda() for k in ("cot", "disp", "coords", "noisy"))
    dgeo, dcorr = abi_bwd(go, disp, coords, noisy, shape)
    for i in range(2):
        part = abi_bwd(go[i:i + 1].contiguous(), disp[i:i + 1].contiguous(), coords[i:i + 1].contiguous(),
                       noisy[i:i + 1].contiguous(), (1, *shape[1:]))
        assert same_bits(part[0], dgeo[i:i + 1]) and same_bits(part[1], dcorr[i:i + 1])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_one_sided_requires_grad_and_forward_bits(shape):
    x, _, _ = reference(shape, "ramp")
    out, full = hip_step(x)
    with torch.no_grad():
        plain = Combined_Geo_Encoding_Volume(x["fmap1"].cuda(), x["fmap2"].cuda(), x["geo"].cuda())(
            x["disp"].cuda(), x["coords"].cuda(), x["noisy"].cuda())
    assert same_bits(out, plain)                                            # the forward is the inference launch
    for need in ((True, False, False), (False, True, True), (False, True, False), (False, False, True)):
        out1, grads = hip_step(x, need=need)
        assert same_bits(out1, plain)
        for n, r in zip(NAMES, need):
            assert (grads[n] is not None) == r, (need, n)
            if r:
                assert same_bits(grads[n], full[n]), (need, n)


def test_bad_arguments_return_the_abi_error_codes():
    lib = _lib.load()
    shape = SHAPES[1]
    b, c, d, h, w, w2 = shape
    x, _, _ = reference(shape, "uniform")
    go, disp, coords, noisy = (x[k].cuda() for k in ("cot", "disp", "coords", "noisy"))
    dgeo = torch.zeros(b, c, d, h, w, device="cuda")
    p = lambda t: t.data_ptr()
    call = lambda *a: lib.dv_geo_filter_lookup_bwd_f32(*a, _lib.stream_ptr())
    assert call(None, p(disp), p(coords), p(noisy), p(dgeo), None, b, c, d, h, w, w2, 4) == -1
    assert call(p(go), p(disp), p(coords), None, p(dgeo), None, b, c, d, h, w, w2, 4) == -1
    assert call(p(go), p(disp), p(coords), p(noisy), None, None, b, c, d, h, w, w2, 4) == -1       # nothing asked for
    assert call(p(go), p(disp), p(coords), p(noisy), p(dgeo), None, 0, c, d, h, w, w2, 4) == -2
    assert call(p(go), p(disp), p(coords), p(noisy), p(dgeo), None, b, c, 3, h, w, w2, 4) == -2
    assert call(p(go), p(disp), p(coords), p(noisy), p(dgeo), None, b, c, d, h, w, w2, 3) == -3
    torch.cuda.synchronize()
    assert float(dgeo.abs().max()) == 0.0                                   # nothing was launched
