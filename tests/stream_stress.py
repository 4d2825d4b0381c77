"""Tools that hold one stream back while another runs, for tests/test_stream_handover_gpu.py.  On an idle GPU a missing
wait between two streams changes nothing: the producer finished long ago.  Here a stream is DELAYED by ordinary queued
work, so whatever has to wait for it either waits or reads what is not there yet.

delay(stream, ms): a chain of large bf16 torch.mm calls on buffers of this module's own.  Its length comes from one
event-timed matmul, measured when the module is first used on a device.  No spin kernel, no torch.cuda._sleep (its
behaviour on ROCm is not something this project has measured), no stream memory operations, no host callbacks: a delay
is work like any other, and shares the CUs with whatever runs beside it.

Canary: proof that the second stream really began while the first was still held.  A one-element device tensor, zero and
synchronised before the run; the delayed stream writes 1 to it right after its delay; the other stream copies it first
thing, before its own work.  After the final synchronise the copy must read 0.  A run whose canary reads 1 proved nothing:
`until_open` repeats the attempt on fresh cold state with the delay doubled, three doublings at the most, then fails.

window_ms: how long to hold a stream.  20 x the event-timed solo run time of the work that has to fit inside the window,
with a floor of 20 ms.  The factor is there because that work shares the CUs with the delay's matmuls and nobody has
measured by how much that slows it; the canary is the real guard, the factor only makes the first attempt usually do.

slow_side / slow_call / without: context managers that place delays, or take a wait away, without touching the package.
No fixtures here and nothing for a conftest: a plain helper module, like tests/backbone_trace.py.
"""
import contextlib
import math

import pytest
import torch

_DIM = 8192             # one [8192, 8192] x [8192, 8192] bf16 product: about a millisecond of every CU
_STATE = {}             # device -> (a, b, out, milliseconds per product)


def _state(dev):
    st = _STATE.get(dev)
    if st is None:
        g = torch.Generator(device=dev).manual_seed(5)
        a = torch.randn(_DIM, _DIM, device=dev, generator=g).to(torch.bfloat16)
        b = torch.randn(_DIM, _DIM, device=dev, generator=g).to(torch.bfloat16)
        out = torch.empty(_DIM, _DIM, device=dev, dtype=torch.bfloat16)
        for _ in range(2):                      # library set-up and kernel load stay out of the timed product
            torch.mm(a, b, out=out)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.mm(a, b, out=out)
        e1.record()
        torch.cuda.synchronize(dev)
        st = _STATE[dev] = (a, b, out, max(e0.elapsed_time(e1), 0.05))
        print(f"stream_stress: one {_DIM}^3 bf16 product = {st[3]:.3f} ms")
    return st


def delay(stream, ms):
    """Queue about `ms` milliseconds of matmuls on `stream` (on top of what it already holds).  -> the products queued."""
    a, b, out, per = _state(stream.device)
    count = max(1, math.ceil(ms / per))
    with torch.cuda.stream(stream):
        for _ in range(count):
            torch.mm(a, b, out=out)
    return count


def solo_ms(run, dev, repeats=3):
    """Event-timed run time of run() on the current stream with nothing beside it: the least of `repeats`, after one warm call."""
    run()
    torch.cuda.synchronize(dev)
    best = float("inf")
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize(dev)
        best = min(best, e0.elapsed_time(e1))
    return best


def window_ms(run, dev, what=""):
    solo = solo_ms(run, dev)
    ms = max(20.0, 20.0 * solo)
    print(f"stream_stress: {what} solo {solo:.3f} ms -> delay {ms:.1f} ms")
    return ms


class Canary:
    def __init__(self, dev):
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seen = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

    def write(self, stream):
        """On the delayed stream, right after its delay."""
        with torch.cuda.stream(stream):
            self.flag.fill_(1)

    def read(self, stream):
        """On the other stream, before (or, where the test says so, after) its own work."""
        with torch.cuda.stream(stream):
            self.seen.copy_(self.flag)

    def open(self):
        """After the final synchronise: True if the reading stream got there while the delayed one was still held."""
        seen = int(self.seen.item())
        assert seen in (0, 1), "the canary was never read"
        return seen == 0


def until_open(attempt, ms, what, doublings=3):
    """attempt(ms) -> (result, Canary), run on fresh cold state and synchronised.  -> the result of the first attempt
    whose canary shows an open window; fails the test if the window stays shut after `doublings` doublings of the delay."""
    for i in range(doublings + 1):
        used = ms * 2 ** i
        result, canary = attempt(used)
        if canary.open():
            print(f"stream_stress: {what}: window open (canary 0) with a delay of {used:.1f} ms, attempt {i + 1}")
            return result
        print(f"stream_stress: {what}: canary read 1 with a delay of {used:.1f} ms: this run proved nothing")
    pytest.fail(f"{what}: the second stream never began while the first was held (delays up to {used:.1f} ms)")


def two_lanes(dev, ms, first, second):
    """The cold two-lane protocol.  Lane A: delay, canary write, first().  Lane B: canary read, second().  One synchronise
    at the end; both streams are fresh and everything the package keyed by them is dropped again.
    -> ((result of first, result of second), Canary)"""
    from vpr_amd import ops
    lane_a, lane_b = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    canary = Canary(dev)
    delay(lane_a, ms)
    canary.write(lane_a)
    with torch.cuda.stream(lane_a):
        ra = first()
    canary.read(lane_b)
    with torch.cuda.stream(lane_b):
        rb = second()
    torch.cuda.synchronize(dev)
    for s in (lane_a, lane_b):
        ops.drop_stream_caches(s.cuda_stream)
    return (ra, rb), canary


@contextlib.contextmanager
def slow_side(ms):
    """Slow side: every fork of _streams._TorchEvents / _RawEvents is followed by a delay on the side stream, right after its
    wait for the main stream."""
    from vpr_amd import _streams
    saved = [(cls, cls.fork) for cls in (_streams._TorchEvents, _streams._RawEvents)]

    def wrap(fork):
        def slow_fork(self, main, side):
            fork(self, main, side)
            delay(side, ms)
        return slow_fork

    for cls, fork in saved:
        cls.fork = wrap(fork)
    try:
        yield
    finally:
        for cls, fork in saved:
            cls.fork = fork


@contextlib.contextmanager
def slow_call(owner, name, ms, stream=None, only=None):
    """Every call of owner.name is preceded by a delay on `stream` (default: the stream that is current at the call).
    Slow main: slow_call(ops, "attention_qkv_split_bf16", ms) holds the main stream before each attention of the backbone,
    which reaches the function through the module attribute.  only(*args): delay only the calls it accepts."""
    fn = getattr(owner, name)

    def slow(*args, **kwargs):
        if only is None or only(*args, **kwargs):
            delay(stream if stream is not None else torch.cuda.current_stream(), ms)
        return fn(*args, **kwargs)

    setattr(owner, name, slow)
    try:
        yield
    finally:
        setattr(owner, name, fn)


@contextlib.contextmanager
def without(owner, name, replacement):
    """A harness self-check's mutation: owner.name replaced (a join by a no-op, a fork by one that does not wait), undone at
    exit and followed by a device synchronise, so that nothing queued under the mutation outlives it."""
    fn = getattr(owner, name)
    setattr(owner, name, replacement)
    try:
        yield
    finally:
        setattr(owner, name, fn)
        torch.cuda.synchronize()
