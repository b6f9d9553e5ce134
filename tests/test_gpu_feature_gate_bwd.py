"""dv_feature_gate_bwd_f32 (csrc/feature_gate.hip) and train3d.feature_gate_train against float64.

Bar (the convention of tests/test_gpu_acv_train.py): relative L2 against float64 <= 2 x that of the float32 torch
expression on the CPU, + 1e-6 -- for dcv and dlogit separately."""
import functools

import pytest
import torch

from diffuvolume_amd import _lib, train3d
from diffuvolume_amd.submodule import feature_gate
from diffuvolume_amd.synth import _gen

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 6, 5, 7),         # H*W = 35: scalar path (D split in two)
          (1, 48, 3, 4, 8),         # vector path, no split
          (1, 8, 48, 2, 4)]         # tiny plane, long d sum: D split over blocks, partials added in split order


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def torch_grads(cv, logit, g):
    cv, logit = cv.clone().requires_grad_(), logit.clone().requires_grad_()
    (torch.sigmoid(logit).unsqueeze(2) * cv).backward(g)
    return cv.grad, logit.grad


@functools.lru_cache(maxsize=None)
def case(shape):
    gen = _gen(97, str(shape))
    cv, g = torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)
    logit = torch.randn(shape[0], shape[1], shape[3], shape[4], generator=gen) * 3
    ref = torch_grads(cv.double(), logit.double(), g.double())
    f32 = torch_grads(cv, logit, g)
    return cv, logit, g, ref, f32


@pytest.mark.parametrize("shape", SHAPES)
def test_gate_backward(shape):
    cv, logit, g, ref, f32 = case(shape)
    out = train3d.feature_gate_grads(cv.cuda(), logit.cuda(), g.cuda())
    for name, o, r, t in zip(("dcv", "dlogit"), out, ref, f32):
        e, bar = rel(o, r), 2 * rel(t, r) + 1e-6
        print(f"{shape} {name}: hip {e:.2e}, torch fp32 {rel(t, r):.2e}, bar {bar:.2e}")
        assert e <= bar, name


def test_split_is_exercised():
    ws = _lib.load().dv_feature_gate_bwd_workspace_floats
    assert ws(1, 48, 3, 4, 8) == 0                               # no split: the thread finishes dlogit itself
    assert ws(1, 8, 48, 2, 4) % (8 * 8) == 0 and ws(1, 8, 48, 2, 4) // (8 * 8) > 1
    assert ws(2, 16, 6, 5, 7) // (32 * 35) == 2


@pytest.mark.parametrize("shape", SHAPES)
def test_two_launches_same_bits(shape):
    cv, logit, g = (t.cuda() for t in case(shape)[:3])
    a, b = train3d.feature_gate_grads(cv, logit, g), train3d.feature_gate_grads(cv, logit, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", SHAPES)
def test_function_forward_is_the_inference_gate(shape, monkeypatch):
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    cv, logit, g, ref, _ = case(shape)
    cvd, ld = cv.cuda().requires_grad_(), logit.cuda().requires_grad_()
    y = train3d.feature_gate_train(cvd, ld)
    assert y.data_ptr() != cvd.data_ptr()                                   # out of place
    assert torch.equal(y.detach(), feature_gate(cv.cuda(), logit.cuda()))   # bit for bit dv_feature_gate_f32
    y.backward(g.cuda())
    direct = train3d.feature_gate_grads(cv.cuda(), logit.cuda(), g.cuda())
    assert torch.equal(cvd.grad, direct[0]) and torch.equal(ld.grad, direct[1])
    monkeypatch.setenv("DV_TRAIN_CONV3D", "torch")
    yt = train3d.feature_gate_train(cv.cuda(), logit.cuda())
    torch.testing.assert_close(yt, y.detach(), rtol=1e-5, atol=1e-6)


def test_bad_arguments_and_cpu_tensors():
    lib = _lib.load()
    t = torch.zeros(1024, device="cuda")
    p, s = t.data_ptr(), _lib.stream_ptr()
    for bad in range(5):
        args = [p] * 6
        args[bad] = None
        assert lib.dv_feature_gate_bwd_f32(*args, 1, 2, 3, 4, 4, s) == -1
    assert lib.dv_feature_gate_bwd_f32(p, p, p, p, p, None, 1, 8, 48, 2, 4, s) == -1     # a split needs the workspace
    assert lib.dv_feature_gate_bwd_f32(p, p, p, p, p, p, 1, 2, 0, 4, 4, s) == -2
    assert lib.dv_feature_gate_bwd_workspace_floats(1, 2, 3, 0, 4) == 0
    with pytest.raises(_lib.DiffuVolumeError):
        train3d.feature_gate_train(torch.zeros(1, 2, 3, 4, 4), torch.zeros(1, 2, 4, 4))
