"""The table driver of tests/test_gpu_abi_arena.py (variants, refusals, reporting) on the CPU: a Python "entry point" that
takes raw pointers like the C ABI and commits one fault at a time -- each in ONE placement only, the way a wrong alignment
predicate or a wrong scalar body would -- must fail its row with the variant and the reason named; the correct one passes."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_abi_arena as T

N = 40


def _f32(ptr, n):
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n,))


def _entry(fault):
    """out = 2 * x + 1 over N floats; `wpacked` must be 16-byte aligned (-4); a 'vector path' when `out` is aligned."""
    def call(lib, p, stream):
        x, out, wp = p("x"), p("out"), p("wpacked")
        if wp % 16 and fault != "ignores_wpacked":
            if fault == "refusal_writes":
                _f32(out, 1)[0] = 0.0
            return -3 if fault == "wrong_code" else -4
        vec = out % 16 == 0
        o = _f32(out, N)
        n = N - 1 if (fault == "skips_last" and not vec) else N
        o[:n] = 2 * _f32(x, n) + 1
        if fault == "tail_store" and out % 16 == 8:             # a pair store that runs over the end at 8-byte offsets only
            _f32(out, N + 1)[N] = 0.0
        if fault == "scalar_body_wrong" and not vec:
            o[N - 1] += 1e-3
        if fault == "reads_past_input" and x % 16:              # multiply-by-mask instead of a select
            with np.errstate(invalid="ignore"):
                o[N - 1] += 0.0 * _f32(x, N + 1)[N]
        return 0
    return call


def _row(fault):
    def build():
        x = torch.randn(N, generator=T.G(1))
        return T.Case({"x": x, "wpacked": torch.arange(8, dtype=torch.int32)}, {"out": torch.empty(N)}, _entry(fault),
                      {"out": x.double() * 2 + 1}, T.bar_close(1e-6, 1e-6))
    return T.Row(f"fake_{fault}", "fake_entry", build, "test_fake", pred=("out",), aligned=("wpacked",), refuse=T.WP)


@pytest.fixture(autouse=True)
def _on_the_cpu(monkeypatch):
    monkeypatch.setattr(T, "DEV", "cpu")


def test_a_correct_entry_passes_every_variant():
    before = len(T.REPORT)
    T.run_row(_row("none"))
    assert T.REPORT[before:] == ["ARENA fake_entry (fake_none): ran a b:out o:x c1 c2 c3; refused refuse:wpacked=-4"]


@pytest.mark.parametrize("fault,message", [
    ("tail_store", r"\[c2\] ArenaError: .*PAST THE END"),
    ("skips_last", r"\[b:out\] ArenaError: .*NEVER WRITTEN"),
    ("scalar_body_wrong", r"\[b:out\] AssertionError"),
    ("reads_past_input", r"\[o:x\] ArenaError: .*NaN in the output"),
    ("ignores_wpacked", r"\[refuse:wpacked\] AssertionError: returned 0, the source gives -4"),
    ("wrong_code", r"\[refuse:wpacked\] AssertionError: returned -3, the source gives -4"),
    ("refusal_writes", r"\[refuse:wpacked\] ArenaError: .*refused call wrote 1 word"),
])
def test_a_faulty_entry_fails_its_row(fault, message):
    with pytest.raises(pytest.fail.Exception, match=message) as e:
        T.run_row(_row(fault))
    text = str(e.value)
    assert "fake_entry" in text and "bar of test_fake" in text
    if fault == "tail_store":                                   # only the 8-byte placement is at fault, and only it is blamed
        assert "[a]" not in text and "[c1]" not in text and "[c3]" not in text and "[b:out]" not in text
