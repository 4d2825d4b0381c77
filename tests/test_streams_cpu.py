"""_streams on a machine without a GPU: torch.cuda.Stream and the HIP runtime are fakes that record what they are asked.
The registries (same key -> same object, a drop removes exactly one main stream's entries and closes what has native
handles), the native handles (allocated with today's flags, freed exactly once), the fork / mark / join call sequences
pinned to what the backbone's side chain has always enqueued, and the cls-tail hook carrying the patch count."""
import contextlib
import types

import pytest
import torch

from vpr_amd import _streams, modules, ops
from vpr_amd.backbone import SplitTokens

DEV = torch.device("cuda", 0)


class FakeStream:
    made = []

    def __init__(self, device=None, priority=0):
        self.device, self.priority, self.cuda_stream = device, priority, 0x1000 + len(FakeStream.made)
        FakeStream.made.append(self)


class FakeHip:
    """Records every runtime call as (name, plain-int arguments...); handles are 0x100, 0x101, ..."""

    def __init__(self):
        self.calls, self._next = [], 0x100

    def _new(self, ref):
        ref._obj.value = self._next
        self._next += 1
        return ref._obj.value

    def hipExtMallocWithFlags(self, ref, nbytes, flags):
        self.calls.append(("malloc", self._new(ref), nbytes, flags))
        return 0

    def hipEventCreateWithFlags(self, ref, flags):
        self.calls.append(("create", self._new(ref), flags))
        return 0

    def hipFree(self, p):
        self.calls.append(("free", p.value))
        return 0

    def hipEventDestroy(self, e):
        self.calls.append(("destroy", e.value))
        return 0

    def hipStreamWriteValue32(self, stream, p, value, flags):
        self.calls.append(("write", p.value, stream, value, flags))
        return 0

    def hipStreamWaitValue32(self, stream, p, value, flags, mask):
        self.calls.append(("wait", p.value, stream, value, flags, mask))
        return 0

    def hipEventRecord(self, e, stream):
        self.calls.append(("record", e.value, stream))
        return 0

    def hipStreamWaitEvent(self, stream, e, flags):
        self.calls.append(("wait_event", e.value, stream, flags))
        return 0

    def named(self, *names):
        return [c for c in self.calls if c[0] in names]


@pytest.fixture
def fake(monkeypatch):
    hip = FakeHip()
    FakeStream.made = []
    monkeypatch.setattr(_streams, "hip", lambda: hip)
    monkeypatch.setattr(torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    yield hip
    for raw in (0xA, 0xB):
        ops.drop_stream_caches(raw)


def _keys(raw):
    return [k for c in ops._STREAM_KEYED for k in c._entries if k[1] == raw]


# ------------------------------------------------------------------------------------------------------- 1. registry
def test_registry_returns_one_object_per_key_and_a_drop_forgets_exactly_one_main_stream(fake):
    a = _streams.side_stream(DEV, 0xA, "cls", priority=-1)
    assert _streams.side_stream(DEV, 0xA, "cls", priority=-1) is a and len(FakeStream.made) == 1
    assert (a.device, a.priority) == (DEV, -1)                              # the priority reached the constructor
    b, c = _streams.side_stream(DEV, 0xB, "cls"), _streams.side_stream(DEV, 0xA, "salad")
    assert b is not a and c is not a and b is not c and (b.priority, c.priority) == (0, 0)
    light, sig = _streams.fork_join(DEV, 0xA, "light"), _streams.fork_join(DEV, 0xA, "signals")
    other = _streams.fork_join(DEV, 0xB, "light")
    assert _streams.fork_join(DEV, 0xA, "light") is light and _streams.fork_join(DEV, 0xA, "signals") is sig
    assert other is not light and isinstance(light, _streams._RawEvents) and isinstance(sig, _streams._StreamSignals)
    ev = _streams.fork_join(DEV, 0xA, "events")                             # "events": a fresh object per forward, never kept
    assert isinstance(ev, _streams._TorchEvents) and _streams.fork_join(DEV, 0xA, "events") is not ev
    ws = ops._WORKSPACES.get((0, 0xA, "test"), torch.zeros, (4,))
    assert len(_keys(0xA)) == 5 and len(_keys(0xB)) == 2
    closed = []
    for s in (light, sig, other):
        real = s.close
        s.close = lambda s=s, real=real: (closed.append(s), real())
    ops.drop_stream_caches(0xA)
    assert _keys(0xA) == [] and len(_keys(0xB)) == 2
    assert closed == [light, sig] or closed == [sig, light]                 # each dropped sync object closed once, the other kept
    assert _streams.side_stream(DEV, 0xB, "cls") is b and _streams.fork_join(DEV, 0xB, "light") is other
    assert _streams.side_stream(DEV, 0xA, "cls") is not a
    del ws


# ------------------------------------------------------------------------------------------------- 2. native handles
def test_native_handles_are_allocated_with_todays_flags_and_freed_exactly_once(fake, monkeypatch):
    sig = _streams._StreamSignals(DEV)
    assert fake.calls == [("malloc", 0x100, 8, 0x2), ("malloc", 0x101, 8, 0x2)]        # two words, hipMallocSignalMemory
    ring = _streams._RawEvents(DEV)
    created = fake.named("create")
    assert len(created) == _streams._RawEvents.RING == 128
    assert all(c[2] == 0x2 | 0x20000000 for c in created)                  # DisableTiming | DisableSystemFence
    handles = [c[1] for c in created]
    sig.close()
    ring.close()
    assert sorted(c[1] for c in fake.named("free")) == [0x100, 0x101]
    assert sorted(c[1] for c in fake.named("destroy")) == sorted(handles) and len(set(handles)) == 128
    n = len(fake.calls)
    sig.close(), ring.close()                                               # idempotent
    sig.__del__(), ring.__del__()
    del sig, ring
    assert len(fake.calls) == n
    # at interpreter shutdown the finaliser leaves the runtime alone
    sig2, ring2 = _streams._StreamSignals(DEV), _streams._RawEvents(DEV)
    n = len(fake.calls)
    with monkeypatch.context() as m:
        m.setattr(_streams.sys, "is_finalizing", lambda: True)
        sig2.__del__(), ring2.__del__()
    with monkeypatch.context() as m:                                        # later still, the module's globals are None
        m.setattr(_streams, "sys", None)
        sig2.__del__(), ring2.__del__()
    assert len(fake.calls) == n
    del sig2, ring2                                                        # collected while running: released
    assert len(fake.named("free")) == 4 and len(fake.named("destroy")) == 256


# ---------------------------------------------------------------------------------------------- 3. protocol sequence
def test_stream_signals_enqueue_write_then_wait_with_a_32_bit_counter(fake):
    main, side = types.SimpleNamespace(cuda_stream=0xA), types.SimpleNamespace(cuda_stream=0x5)
    sig = _streams._StreamSignals(DEV)
    w0, w1 = 0x100, 0x101
    del fake.calls[:]
    sig.fork(main, side)
    assert fake.calls == [("write", w0, 0xA, 1, 0), ("wait", w0, 0x5, 1, 0x1, 0xFFFFFFFF)]      # c incremented first; WaitValueEq
    tick = sig.mark(side)
    assert tick == 1 and fake.calls[2:] == [("write", w1, 0x5, 1, 0)]
    sig.fork(main, side)                                                    # the next block forks before this one is joined
    sig.join(main, tick)
    assert fake.calls[3:] == [("write", w0, 0xA, 2, 0), ("wait", w0, 0x5, 2, 0x1, 0xFFFFFFFF),
                              ("wait", w1, 0xA, 1, 0x1, 0xFFFFFFFF)]        # join waits for the tick it was given
    sig.count = 2 ** 32 - 2
    del fake.calls[:]
    sig.fork(main, side)
    t = sig.mark(side)
    sig.join(main, t)
    sig.fork(main, side)
    t = sig.mark(side)
    sig.join(main, t)
    assert [c[3] for c in fake.calls] == [2 ** 32 - 1] * 4 + [0] * 4        # masked to 32 bits: 2^32 - 1 is followed by 0
    assert sig.count == 2 ** 32
    sig.close()


def test_raw_events_walk_the_ring_and_every_wait_names_the_record_before_it(fake):
    main, side = types.SimpleNamespace(cuda_stream=0xA), types.SimpleNamespace(cuda_stream=0x5)
    ring = _streams._RawEvents(DEV)
    base, RING = 0x100, _streams._RawEvents.RING
    del fake.calls[:]
    ring.fork(main, side)
    e = ring.mark(side)
    ring.join(main, e)
    assert fake.calls == [("record", base, 0xA), ("wait_event", base, 0x5, 0),
                          ("record", base + 1, 0x5), ("wait_event", base + 1, 0xA, 0)]
    del fake.calls[:]
    for _ in range(RING):                                                   # 2 slots per block: wraps twice
        ring.fork(main, side)
        ring.join(main, ring.mark(side))
    records = fake.named("record")
    assert [c[1] - base for c in records] == [(2 + i) % RING for i in range(2 * RING)]
    for i, c in enumerate(fake.calls):
        if c[0] == "wait_event":
            prev = fake.calls[i - 1]
            assert prev[0] == "record" and prev[1] == c[1] and prev[2] != c[2]       # the event just recorded, on the other stream
    ring.close()


# -------------------------------------------------------------------------------------------------------- 4. the hook
def test_features_installs_a_hook_that_carries_the_patch_count_to_the_token_stage(monkeypatch):
    ext = modules.DinoV2Salad("vit_small")
    seen, staged = [], []
    cls_rows, n = torch.zeros(2, 384, dtype=torch.bfloat16), 100

    def backbone_forward(x, split=False):
        seen.append(ext.backbone.cls_tail_hook)
        ext.backbone.cls_tail_hook(cls_rows, 0xA, n)                        # what _blocks_side_chain does on its side stream
        return SplitTokens(torch.zeros(2, n, 384, dtype=torch.bfloat16), cls_rows, True)

    monkeypatch.setattr(ext.backbone, "forward", backbone_forward)
    monkeypatch.setattr(ext.aggregator, "pack", lambda: "packed")
    monkeypatch.setattr(ops, "salad_stage_token", lambda *a: staged.append(a))
    monkeypatch.setattr(type(ext.aggregator), "forward", lambda self, t, want_bf16=False: t)
    out = ext.features(torch.zeros(2, 3, 140, 140))
    assert seen == [ext.aggregator.token_stage] and ext.backbone.cls_tail_hook is None
    assert len(staged) == 1 and staged[0][0] is cls_rows and staged[0][1:] == ("packed", n, 0xA)
    assert out.token_ready is True
    ext.token_on_cls_stream = False
    monkeypatch.setattr(ext.backbone, "forward", lambda x, split=False: seen.append(ext.backbone.cls_tail_hook) or out)
    ext.features(torch.zeros(2, 3, 140, 140))
    assert seen[-1] is None and len(staged) == 1
