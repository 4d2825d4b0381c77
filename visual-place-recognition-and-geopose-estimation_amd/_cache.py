"""The one cache behind everything the host layer keeps in device memory between calls: workspaces, packed weights,
batch-size-keyed backbone constants.

A HIP graph addresses what it was captured on by raw pointer.  So a value handed out while the current stream is
capturing becomes PINNED: for the life of the process it is never freed and never replaced under its key, whatever the
capacity, however its source tensors change.  The one exception is an explicit `drop()`: the caller states that the
graphs are gone (with their private stream).  Needs no GPU and nothing beyond torch; no locks (callers hold the GIL
and a key carries its stream where two streams must not share).

A value is BUILT by asynchronous device work on whatever stream makes the first call, and a later caller on another
stream gets it on a host-side hit: nothing on the device orders that caller after the build.  So every value carries a
`Handover`: the stream it was built on and an event recorded right after the build.  The first hit from any other
stream makes that stream wait for the event and marks the value's tensors as used by it (so that an eviction cannot
hand their memory back to the builder's allocator pool while the borrower's queued kernels still read them); every later
hit from that stream, and every hit from the builder's own, costs one host-side comparison.  The stream probe and the
three device actions come from outside (`StreamProbes`; ops.cache() supplies them, tests/test_cache_cpu.py fakes them).
"""
from __future__ import annotations

from typing import Callable, Hashable, NamedTuple, Optional, Sequence

import torch


def tensor_key(*tensors: torch.Tensor) -> tuple:
    """Identity part of a cache key: storage address, version counter (in-place writes bump it), shape and device of
    each tensor.  An address can be recycled once its tensor is freed, so pass the same tensors as `sources` of the
    entry: while it is cached they stay allocated and no other tensor can appear under their key."""
    return tuple((t.data_ptr(), t._version, t.shape, t.device) for t in tensors)


class StreamProbes(NamedTuple):
    """What a Handover asks of the device layer.  current() -> a hashable name of the current stream, None where there
    is none (no GPU in use: nothing is recorded, nothing is ever waited for); record() -> an event recorded on the current
    stream; wait(event): the current stream waits for it; keep(value): the current stream is noted as a user of the
    value's device memory."""
    current: Callable[[], Optional[Hashable]]
    record: Callable[[], object]
    wait: Callable[[object], None]
    keep: Callable[[object], None]


class Handover:
    """Made right after a value was built: remembers the building stream and an event recorded on it.  Built under graph
    capture it remembers nothing: what is built during capture belongs to the graph."""
    __slots__ = ("_probes", "_capturing", "stream", "event", "lent")

    def __init__(self, probes: StreamProbes, capturing: Callable[[], bool]):
        self._probes, self._capturing = probes, capturing
        self.stream = None if capturing() else probes.current()
        self.event = probes.record() if self.stream is not None else None
        self.lent: set = set()          # the other streams that already wait for `event`

    def __deepcopy__(self, memo) -> "Handover":
        """A copy of the owner (copy.deepcopy of a module) holds copies of the values, made by the copier on its own
        stream: the copy's hand-over remembers nothing (and an event is no copyable thing)."""
        new = Handover.__new__(Handover)
        new._probes, new._capturing, new.stream, new.event, new.lent = self._probes, self._capturing, None, None, set()
        return new

    def lend(self, value) -> None:
        """Called at every hand-out of `value`.  From the builder's stream, or from one that was lent to before: a
        comparison.  From another stream, once: wait + keep.  Under capture nothing is waited for (_streams.Captured
        synchronises the device before it captures) and nothing is remembered."""
        if self.stream is None:
            return
        cur = self._probes.current()
        if cur == self.stream or cur in self.lent or cur is None or self._capturing():
            return
        self._probes.wait(self.event)
        self._probes.keep(value)
        self.lent.add(cur)


class Cache:
    def __init__(self, capturing: Callable[[], bool], capacity: Optional[int] = None, probes: Optional[StreamProbes] = None):
        """capturing: the capture probe (ops.capturing).  capacity: most UNPINNED entries kept, oldest evicted first
        (None: unbounded); pinned entries do not count and can still be hit.  probes: the stream probes of the hand-over
        between streams (None: values are handed out as they are)."""
        self._capturing, self.capacity, self._probes = capturing, capacity, probes
        self._entries: dict = {}        # key -> [value, pinned, sources, need, Handover | None]; dicts keep insertion order = age
        self._outgrown: list = []       # (key, value) of pinned values that a larger `need` replaced under their key

    def get(self, key: Hashable, build: Callable, args: tuple = (), sources: Sequence = (), need: int = 0):
        """The value cached under `key`, or build(*args), stored.  sources: what the key was derived from (kept alive
        with the entry).  need: a size the value must cover; an entry built for a smaller one is rebuilt (it grows)
        and, if pinned, the old value is kept allocated beside the new one."""
        ent = self._entries.get(key)
        if ent is None or ent[3] < need:
            if ent is None:
                self._evict(1)
            elif ent[1]:
                self._outgrown.append((key, ent[0]))
            ent = self._entries[key] = [build(*args), False, sources, need, None]
            if self._probes is not None:
                ent[4] = Handover(self._probes, self._capturing)
        elif ent[4] is not None:
            ent[4].lend(ent[0])
        if not ent[1] and self._capturing():
            ent[1] = True
        return ent[0]

    def _evict(self, room: int) -> None:
        if self.capacity is not None:
            unpinned = [k for k, e in self._entries.items() if not e[1]]
            for k in unpinned[:max(0, len(unpinned) + room - self.capacity)]:
                del self._entries[k]

    def drop(self, predicate: Callable[[Hashable], bool]) -> None:
        """Forget every entry, pinned or not, whose key satisfies `predicate`, and close() the values that have one (_streams)."""
        for k in [k for k in self._entries if predicate(k)]:
            close = getattr(self._entries.pop(k)[0], "close", None)
            if close is not None:
                close()
        self._outgrown = [(k, v) for k, v in self._outgrown if not predicate(k)]

    def __contains__(self, key: Hashable) -> bool:
        return key in self._entries

    def __len__(self) -> int:
        return len(self._entries)
