"""Host side of diffuvolume_amd/plans.py without a GPU: the pointer / channel arrays of a virtual concatenation, what the
shared checks refuse (exception types and messages as the plans raised them before the checks were written once), and that
submodule.py re-exports the plans' names as the same objects."""
import ast
import ctypes
from pathlib import Path

import pytest
import torch

from diffuvolume_amd import DiffuVolumeError, plans as P, submodule as S

ROOT = Path(__file__).resolve().parent.parent


class _CudaLike(torch.Tensor):
    """A CPU tensor that claims to be on the GPU: the checks run up to the launch they guard."""
    @property
    def is_cuda(self):
        return True


def t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_CudaLike)


def bare(cls, **attrs):
    """A plan without its weight images (building them needs the GPU): the refusals come before any launch."""
    plan = object.__new__(cls)
    plan.__dict__.update(attrs)
    return plan


def test_cat_args_pointers_and_channels():
    parts = [torch.zeros(2, c, 3, 5) for c in (3, 1, 7)]
    ptrs, chans, n = P.cat_args(parts)
    assert n == 3 and list(chans) == [3, 1, 7] and list(ptrs) == [x.data_ptr() for x in parts]
    assert isinstance(ptrs, ctypes.Array) and ptrs._type_ is ctypes.c_void_p and chans._type_ is ctypes.c_int
    ptrs, chans, n = P.cat_args(parts[:1])
    assert n == 1 and list(chans) == [3] and ptrs[0] == parts[0].data_ptr()


CAT = "virtual concatenation: 1..4 tensors with equal batch and spatial size"


@pytest.mark.parametrize("x,exc,msg", [
    ([t(1, 2, 4, 4)] * 5, RuntimeError, CAT),
    ([], RuntimeError, CAT),
    ([t(1, 4, 4, 4), t(2, 4, 4, 4)], RuntimeError, CAT),
    ([t(1, 4, 4, 4), t(1, 4, 4, 5)], RuntimeError, CAT),
    ([t(1, 4, 4, 4), t(1, 3, 4, 4)], RuntimeError, "expected 8 input channels, got 7"),
    (t(1, 7, 4, 4), RuntimeError, "expected 8 input channels, got 7"),
    ([torch.zeros(1, 8, 4, 4)], DiffuVolumeError, "x is on cpu"),
    ([None], TypeError, "x must be a tensor"),
    (t(1, 8, 4, 4, dtype=torch.float64), TypeError, "x must be float32, got torch.float64"),
])
def test_virtual_concatenation_refusals(x, exc, msg):
    plans = (bare(P.Conv2dPlan, cin=8, cout=4, k=3, dilation=1, stride=1, act=0, wino_packed=None),
             bare(P.Conv2dF16Plan, cin=8, c1=4, c2=0, k=3, act=0))
    for call in (lambda: P.cat_parts(x, 8), lambda: plans[0](x), lambda: plans[1](x)):
        with pytest.raises(exc) as e:
            call()
        assert type(e.value) is exc and msg in str(e.value)


def test_cat_parts_returns_the_checked_sources():
    a, b = t(2, 3, 4, 5), t(2, 5, 4, 5)
    assert [x.data_ptr() for x in P.cat_parts([a, b], 8)] == [a.data_ptr(), b.data_ptr()]
    assert len(P.cat_parts(a, 3)) == 1
    nc = t(2, 4, 5, 3).permute(0, 3, 1, 2)                     # a view: the sources come back contiguous
    assert not nc.is_contiguous() and P.cat_parts(nc, 3)[0].is_contiguous()


def test_pair_plan_falls_back_to_its_single_plans():
    """More than four sources, or a launch too small for the Winograd kernel: the two single plans (which raise what
    they raise); a launch the pair kernel takes is checked like every virtual concatenation."""
    pair = bare(P.Conv2dPairPlan, cin=8, c1=32, c2=32, act=0, packed=t(1), single=(lambda x, **k: "s0", lambda x, **k: "s1"))
    assert pair([t(1, 2, 64, 128)] * 5) == ("s0", "s1")
    assert pair(t(1, 8, 4, 4)) == ("s0", "s1")
    assert bare(P.Conv2dPairPlan, packed=None, single=pair.single)(t(1, 8, 64, 128)) == ("s0", "s1")
    with pytest.raises(RuntimeError, match="expected 8 input channels, got 7"):
        pair([t(1, 4, 64, 128), t(1, 3, 64, 128)])
    with pytest.raises(RuntimeError, match="virtual concatenation"):
        pair([t(1, 4, 64, 128), t(1, 4, 64, 127)])
    with pytest.raises(RuntimeError, match="residual shape mismatch"):
        pair(t(1, 8, 64, 128), residual=(t(1, 32, 64, 127), None))


def test_same_shape():
    like = t(1, 4, 4, 4)
    assert P.same_shape(None, like, "residual") is None
    ok = t(1, 4, 4, 4)
    assert P.same_shape(ok, like, "residual").data_ptr() == ok.data_ptr()
    assert P.same_shape(ok, (1, 4, 4, 4), "skip").data_ptr() == ok.data_ptr()
    for name in ("residual", "mul", "blend z", "blend h", "skip"):
        with pytest.raises(RuntimeError) as e:
            P.same_shape(t(1, 4, 4, 5), like, name)
        assert type(e.value) is RuntimeError and str(e.value) == f"{name} shape mismatch"
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        P.same_shape(torch.zeros(1, 4, 4, 4), like, "residual")
    with pytest.raises(TypeError, match="mul must be float32"):
        P.same_shape(t(1, 4, 4, 4, dtype=torch.float16), like, "mul")


def test_epilogue_operands_of_the_plans():
    x = t(1, 8, 4, 4)
    c2 = bare(P.Conv2dPlan, cin=8, cout=4, k=3, dilation=1, stride=1, act=0, wino_packed=None)
    bad, ok = t(1, 4, 4, 5), t(1, 4, 4, 4)
    for kw, msg in ((dict(residual=bad), "residual"), (dict(mul=bad), "mul"), (dict(blend=(bad, ok)), "blend z"),
                    (dict(blend=(ok, bad)), "blend h")):
        with pytest.raises(RuntimeError, match=f"{msg} shape mismatch"):
            c2(x, **kw)
    s2 = bare(P.Conv2dPlan, cin=8, cout=4, k=3, dilation=1, stride=2, act=0, wino_packed=None)
    with pytest.raises(RuntimeError, match="virtual concatenation is stride-1 only"):
        s2([x])
    with pytest.raises(RuntimeError, match="gate operands are stride-1 only"):
        s2(x, mul=t(1, 4, 2, 2))
    with pytest.raises(RuntimeError, match="residual shape mismatch"):
        s2(x, residual=ok)
    with pytest.raises(DiffuVolumeError, match="s2b_out"):
        c2(x, s2b_out=True)
    f16 = bare(P.Conv2dF16Plan, cin=8, c1=4, c2=0, k=3, act=0)
    with pytest.raises(RuntimeError, match="blend h shape mismatch"):
        f16(x, blend=(ok, bad))
    c3 = bare(P.Conv3dPlan, cin=8, cout=4, k=3, stride=1, act=0)
    with pytest.raises(RuntimeError, match="residual shape mismatch"):
        c3(t(1, 8, 2, 4, 4), residual=t(1, 4, 2, 4, 5))
    with pytest.raises(RuntimeError, match="expected 8 input channels, got 7"):
        c3(t(1, 7, 2, 4, 4))
    with pytest.raises(RuntimeError, match=r"in_scale must be \[B,D,H,W\]"):
        c3(t(1, 8, 2, 4, 4), in_scale=t(1, 2, 4, 5))
    d3 = bare(P.Deconv3dPlan, cin=8, cout=4, k=3, act=0, redir_w=t(4, 2), cskip=2)
    with pytest.raises(RuntimeError, match="skip shape mismatch"):
        d3(t(1, 8, 2, 4, 4), skip=t(1, 2, 4, 8, 9))
    with pytest.raises(RuntimeError, match="residual shape mismatch"):
        d3(t(1, 8, 2, 4, 4), residual=t(1, 4, 4, 8, 9))
    with pytest.raises(RuntimeError, match="excludes residual="):
        d3(t(1, 8, 2, 4, 4), skip=t(1, 2, 4, 8, 8), residual=t(1, 4, 4, 8, 8))


def test_dev_f32_is_check_f32_plus_the_inference_refusal():
    with pytest.raises(TypeError, match="x must be a tensor"):
        P._dev_f32(None, "x")
    with pytest.raises(DiffuVolumeError, match="x is on cpu.*no CPU fallback"):
        P._dev_f32(torch.zeros(2), "x")
    with pytest.raises(TypeError, match="x must be float32, got torch.int32"):
        P._dev_f32(t(2, dtype=torch.int32), "x")
    with pytest.raises(NotImplementedError, match="inference-only"):
        P._dev_f32(t(2).requires_grad_(True), "x")
    with torch.no_grad():
        assert P._dev_f32(t(2).requires_grad_(True), "x") is not None
    view = t(4, 3).t()
    assert not view.is_contiguous() and P._dev_f32(view, "x").is_contiguous()


def _imported_from_submodule():
    """Every name some module of the package, a test or a tool imports from diffuvolume_amd.submodule."""
    names = set()
    for folder in ("diffuvolume_amd", "tests", "tools"):
        for path in (ROOT / folder).glob("*.py"):
            for node in ast.walk(ast.parse(path.read_text())):
                if isinstance(node, ast.ImportFrom) and node.module is not None and \
                        (node.module == "diffuvolume_amd.submodule" or (node.level == 1 and node.module == "submodule")):
                    names.update(a.name for a in node.names)
    return names


def test_submodule_reexports_the_same_objects():
    moved = {"Conv3dPlan", "Conv2dPlan", "Conv2dPairPlan", "Conv2dF16Plan", "Deconv3dPlan", "Deconv2dK4S2Plan",
             "PointwiseExpandPlan", "Rank1FilterPlan", "PlanCache", "weight_key", "_fold_bn", "_dev_f32", "AttentionConcatVolume",
             "volume_factors", "set_default_conv_precision", "default_conv_precision", "split_overflow_flag",
             "check_split_overflow", "ACT_NONE", "ACT_RELU", "ACT_MISH", "ACT_LEAKY", "ACT_SIGMOID", "ACT_TANH"}
    for name in moved:
        assert getattr(S, name) is getattr(P, name), name
    for name in set(S.__all__) | _imported_from_submodule():
        assert hasattr(S, name), name
        if hasattr(P, name):
            assert getattr(S, name) is getattr(P, name), name
    assert moved >= {n for n in S.__all__ if hasattr(P, n)}
    assert _imported_from_submodule() - moved <= {n for n in dir(S) if getattr(getattr(S, n), "__module__", None) == S.__name__}


def test_switches_set_through_submodule_reach_the_plans(monkeypatch):
    monkeypatch.setattr(S.Conv3dPlan, "WINO3", False)
    assert P.Conv3dPlan.WINO3 is False
    monkeypatch.setattr(S.Conv2dPlan, "WINO_MIN_BLOCKS", 0)
    assert P.Conv2dPlan.WINO_MIN_BLOCKS == 0
    monkeypatch.delenv("DV_CONV_PRECISION", raising=False)
    try:
        S.set_default_conv_precision("f32_direct")
        assert P.default_conv_precision() == S.default_conv_precision() == "f32_direct"
    finally:
        S.set_default_conv_precision(None)
    assert P.default_conv_precision() == "f32"
    with pytest.raises(ValueError):
        S.set_default_conv_precision("bf16")
