"""tests/arena.py on the CPU: fake "kernels" that each commit one of the errors the guard-banded arenas exist to catch
must be reported with the right message, and a correct one must pass -- the proof that tests/test_gpu_abi_arena.py can fail."""
import pytest
import torch

import arena as A


def _flat(a):
    """The raw float32 words of an arena, the way a kernel with a bad index sees them."""
    return a.buf.view(torch.float32)


def _good(x, out):
    out.view.copy_(x.view * 2 + 1)


def _writes_one_past_the_end(x, out):
    _good(x, out)
    _flat(out)[out.lo + out.nwords - 1 + 1] = 7.0


def _writes_the_word_before(x, out):
    _good(x, out)
    _flat(out)[out.lo - 1] = 7.0


def _skips_an_interior_element(x, out):
    keep = _flat(out)[out.lo + 17].clone()
    _good(x, out)
    _flat(out)[out.lo + 17] = keep


def _adds_zero_times_a_guard_value(x, out):
    _good(x, out)
    out.view.view(-1)[5] += 0 * _flat(x)[x.lo - 1]          # the "multiply by mask" form of a bounds check


KERNELS = [(_good, None), (_writes_one_past_the_end, "PAST THE END"), (_writes_the_word_before, "BEFORE the payload"),
           (_skips_an_interior_element, "NEVER WRITTEN"), (_adds_zero_times_a_guard_value, "NaN in the output")]


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("kernel,message", KERNELS, ids=[k.__name__.strip("_") for k, _ in KERNELS])
def test_planted_faults_are_reported(kernel, message, offset):
    x = torch.randn(3, 5, 8)
    xin = A.place(x, offset, "in", name="x")
    out = A.place(torch.empty(3, 5, 8), offset, "out", name="out")
    kernel(xin, out)
    ref = x.double() * 2 + 1
    if message is None:
        A.check_output(out, ref)
        assert torch.equal(out.view, ref.float())
    else:
        with pytest.raises(A.ArenaError, match=message):
            A.check_output(out, ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
@pytest.mark.parametrize("offset", [0, 1, 2, 3, 5])
def test_layout(dtype, offset):
    t = (torch.arange(24).reshape(2, 3, 4) + 1).to(dtype)
    a = A.place(t, offset, "in")
    words = t.element_size() // 4
    assert a.view.data_ptr() % 16 == 4 * ((offset * words) % 4)
    assert a.lo == A.GUARD + offset * words and a.lo >= 64 and A.GUARD % 4 == 0
    assert a.buf.numel() == 2 * A.GUARD + offset * words + t.numel() * words
    assert torch.equal(a.view, t)
    assert bool((a.buf[:a.lo] == A.INPUT_NAN).all()) and bool((a.buf[a.lo + a.nwords:] == A.INPUT_NAN).all())
    A.check_guards(a)
    if dtype != torch.int32:                                  # the surroundings of an input are NaN in the operand's type
        assert bool(torch.isnan(a.buf[:a.lo - a.lo % words].view(dtype)).all())
    o = A.place(t, offset, "out")
    assert bool((o.buf == A.SENTINEL).all())
    if dtype != torch.int32:
        assert bool(torch.isnan(o.view).all())
    A.check_untouched(o)


def test_refused_call_must_leave_the_arena_alone():
    o = A.place(torch.empty(4, 4), 1, "out", name="out")
    o.view[2, 2] = 0.0
    with pytest.raises(A.ArenaError, match="refused call wrote 1 word"):
        A.check_untouched(o)


def test_float64_output_and_inout():
    o = A.place(torch.empty(6, dtype=torch.float64), 1, "out", name="x_next")
    o.view.copy_(torch.arange(6, dtype=torch.float64))
    o.view[3] = float("nan")                                   # a NaN the reference has too is not a leak
    ref = torch.arange(6, dtype=torch.float64)
    ref[3] = float("nan")
    A.check_output(o, ref)
    with pytest.raises(A.ArenaError, match="NaN in the output"):
        A.check_output(o, torch.arange(6, dtype=torch.float64))
    o2 = A.place(torch.empty(6, dtype=torch.float64), 0, "out", name="x_next")
    o2.view[:5] = 1.0
    with pytest.raises(A.ArenaError, match="NEVER WRITTEN"):
        A.check_output(o2)
    io = A.place(torch.ones(5), 2, "inout", name="mask")      # in/out operands: guards only
    A.check_output(io, torch.ones(5))
    io.buf.view(torch.float32)[io.lo + 5] = 0.0
    with pytest.raises(A.ArenaError, match="PAST THE END"):
        A.check_output(io, torch.ones(5))
