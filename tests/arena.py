"""Guard-banded arenas for tests of the C ABI's pointer and bounds contract.

A tensor handed to a kernel normally starts on a fresh allocator block: it is 512-byte aligned, and a store one element
past its end (or an element that is never stored) lands in memory no comparison looks at.  ``place`` puts an operand into
the middle of one flat buffer instead,

    [ guard | offset_floats pad | payload | guard ]

so that its base pointer has a chosen misalignment (``data_ptr() % 16 == 4 * (offset_floats % 4)``) and every word around
it is known.  Inputs are surrounded by NaN: a read outside the payload that reaches a result poisons it.  Outputs are
filled -- payload included -- with one quiet-NaN bit pattern, and ``check_output`` compares bit patterns afterwards:

  * every guard / pad word still holds the sentinel   (nothing was written outside the payload),
  * no payload word still holds it                   (every element was written),
  * the payload has no NaN the reference has not     (no guard value leaked into a result).

The sentinel 0x7FF8A5A5 (around inputs: 0x7FF85A5A) is a quiet NaN as a float32 and, repeated, as a float64; no arithmetic
produces it from numbers (the default NaN of the hardware and of PyTorch is 0x7FC00000 / 0xFFC00000).  float64 and int32
operands are placed in the same kind of buffer; a float64 payload is displaced by whole doubles (8 bytes per unit of
``offset_floats``).
"""
from __future__ import annotations

import torch

GUARD = 64                      # floats on each side: a multiple of 4, so the guards do not change the alignment
SENTINEL = 0x7FF8A5A5           # int32 view of the fill word of an output / in-out arena
INPUT_NAN = 0x7FF85A5A          # ... of an input arena: another quiet NaN, because hardware propagates a NaN operand's
                                # bits -- a leaked input guard must not read as "never written"

KINDS = ("in", "out", "inout")


class ArenaError(AssertionError):
    pass


class Arena:
    """One placed operand: ``view`` is the tensor to hand to the kernel, ``buf`` the int32 words around and under it."""

    def __init__(self, buf, lo, nwords, view, kind, name):
        self.buf, self.lo, self.nwords, self.view, self.kind, self.name = buf, lo, nwords, view, kind, name

    def data_ptr(self) -> int:
        return self.view.data_ptr()

    def payload_words(self):
        return self.buf[self.lo:self.lo + self.nwords]


def place(t: torch.Tensor, offset_floats: int = 0, kind: str = "in", device="cpu", name: str = "operand") -> Arena:
    """Copy the CPU tensor ``t`` into a guard-banded buffer on ``device``.  kind "in": payload = t, NaN around it;
    "out": sentinel everywhere (t gives shape and dtype only); "inout": payload = t, checked like an output's guards."""
    assert kind in KINDS, kind
    assert GUARD >= 64 and GUARD % 4 == 0
    assert offset_floats >= 0
    t = t.contiguous()
    wpe = t.element_size() // 4                       # words per element
    assert t.element_size() % 4 == 0, "operands are made of 32-bit words"
    pad = offset_floats * wpe                         # float64: whole doubles, so the payload stays element-aligned
    nwords = t.numel() * wpe
    total = GUARD + pad + nwords + GUARD
    buf = torch.full((total,), INPUT_NAN if kind == "in" else SENTINEL, dtype=torch.int32, device=device)
    assert buf.data_ptr() % 16 == 0, "the arena itself must start 16-byte aligned"
    lo = GUARD + pad
    view = buf[lo:lo + nwords].view(t.dtype).view(t.shape)
    if kind != "out":
        view.copy_(t)
    assert view.data_ptr() % 16 == 4 * (pad % 4), (view.data_ptr() % 16, offset_floats)
    assert view.is_contiguous()
    return Arena(buf, lo, nwords, view, kind, name)


def _where(mask, base, limit=8):
    idx = torch.nonzero(mask).flatten()[:limit].cpu().tolist()
    return [i + base for i in idx], int(mask.sum())


def check_guards(a: Arena) -> None:
    """Every word outside the payload still holds its fill word."""
    fill = INPUT_NAN if a.kind == "in" else SENTINEL
    before = a.buf[:a.lo] != fill
    after = a.buf[a.lo + a.nwords:] != fill
    if bool(before.any()):
        where, n = _where(before, -a.lo)
        raise ArenaError(f"{a.name}: {n} word(s) written BEFORE the payload, at word offsets {where} from its start")
    if bool(after.any()):
        where, n = _where(after, a.nwords)
        raise ArenaError(f"{a.name}: {n} word(s) written PAST THE END of the payload, at word offsets {where} from its "
                         f"start (payload is {a.nwords} words)")


def check_untouched(a: Arena) -> None:
    """A refused call launched nothing: the whole arena, payload included, still holds the sentinel."""
    assert a.kind == "out"
    bad = a.buf != SENTINEL
    if bool(bad.any()):
        where, n = _where(bad, -a.lo)
        raise ArenaError(f"{a.name}: a refused call wrote {n} word(s), at word offsets {where} from the payload's start")


def check_output(a: Arena, ref: torch.Tensor = None) -> None:
    """The three bounds properties of an output arena (see the module docstring); ``ref`` is the float64 reference, only
    looked at for the NaN it may legitimately hold."""
    check_guards(a)
    if a.kind == "out":
        words = a.payload_words()
        if a.view.element_size() == 8:                 # a double is unwritten when both of its words are
            stale = (words[0::2] == SENTINEL) & (words[1::2] == SENTINEL)
        else:
            stale = words == SENTINEL
        if bool(stale.any()):
            where, n = _where(stale, 0)
            raise ArenaError(f"{a.name}: {n} element(s) NEVER WRITTEN, at flat indices {where} of shape {tuple(a.view.shape)}")
    if a.view.is_floating_point():
        nan = torch.isnan(a.view)
        if ref is not None:
            nan = nan & ~torch.isnan(ref.to(nan.device)).reshape(nan.shape)
        if bool(nan.any()):
            where, n = _where(nan.flatten(), 0)
            raise ArenaError(f"{a.name}: {n} NaN in the output that the reference does not have, at flat indices {where} "
                             f"of shape {tuple(a.view.shape)} (a value read outside an input's payload reached a result)")
