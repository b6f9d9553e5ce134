"""Gates and side streams for the tests that hold the package to its stream contract.

A *gate* is a kernel that only spins (``torch.cuda._sleep``), enqueued on a stream ahead of the work under test: whatever
was sent to that stream waits for it, whatever was sent elsewhere does not, and the difference shows in the values.  Its
length comes from events around the spin kernel, never from a clock constant.

That only has power between two streams the hardware runs independently.  A process has a few hardware queues and the
runtime maps its streams onto them, so two streams -- the null stream among them -- may share a queue, and then the
second one's work queues up behind the first one's gate as if it had been ordered.  ``pick_streams`` therefore probes:
it hands out side streams for which a small kernel on the null stream, and on each stream picked before, was seen to
finish while a gate on the candidate was still spinning, and the other way round.
"""
import torch

PROBES = 16                         # candidates tried per stream asked for


def _settle():
    torch.cuda.synchronize()


MARGIN = 1.25                       # the spin kernel's clock is not the events' clock: ask for a quarter more


def calibrate_gate(ms: float) -> int:
    """Cycles of the spin kernel for at least ``ms`` milliseconds (``MARGIN`` times ``ms`` by the calibration run)."""
    torch.cuda._sleep(1_000_000)                               # loads the kernel
    probe = 20_000_000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    _settle()
    took = e0.elapsed_time(e1)
    assert took > 0.1, f"the spin kernel of {probe} cycles took {took} ms: it cannot serve as a gate"
    return int(probe / took * ms * MARGIN)


def runs_ahead(gated, other, cycles: int) -> bool:
    """True when a small kernel on ``other`` finishes while a gate of ``cycles`` on ``gated`` is still spinning."""
    word = torch.zeros(64, device="cuda")
    gate_done, other_done = torch.cuda.Event(), torch.cuda.Event()
    _settle()
    with torch.cuda.stream(gated):
        torch.cuda._sleep(cycles)
        gate_done.record()
    with torch.cuda.stream(other):
        word.add_(1.0)
        other_done.record()
    while not (other_done.query() or gate_done.query()):       # ends with the gate at the latest
        pass
    ahead = other_done.query() and not gate_done.query()
    _settle()
    return ahead


def independent(a, b, cycles: int) -> bool:
    return runs_ahead(a, b, cycles) and runs_ahead(b, a, cycles)


def pick_streams(n: int, cycles: int):
    """``n`` side streams that run independently of the null stream and of each other (see the module docstring)."""
    picked = []
    null = torch.cuda.default_stream()
    for i in range(PROBES * n):
        if len(picked) == n:
            break
        s = torch.cuda.Stream()
        ok = all(independent(s, o, cycles) for o in [null] + picked)
        print(f"STREAM candidate {i} ({s.cuda_stream:#x}): {'independent' if ok else 'shares a queue with a stream it must not wait for'}")
        if ok:
            picked.append(s)
    assert len(picked) == n, (f"found {len(picked)} of {n} side streams that run independently of the null stream and of each "
                              "other: a gate has no power on this box")
    return picked
