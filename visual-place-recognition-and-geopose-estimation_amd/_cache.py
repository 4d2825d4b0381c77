"""The one cache behind everything the host layer keeps in device memory between calls: workspaces, packed weights,
batch-size-keyed backbone constants.

A HIP graph addresses what it was captured on by raw pointer.  So a value handed out while the current stream is
capturing becomes PINNED: for the life of the process it is never freed and never replaced under its key, whatever the
capacity, however its source tensors change.  The one exception is an explicit `drop()`: the caller states that the
graphs are gone (with their private stream).  Needs no GPU and nothing beyond torch; no locks (callers hold the GIL
and a key carries its stream where two streams must not share).
"""
from __future__ import annotations

from typing import Callable, Hashable, Optional, Sequence

import torch


def tensor_key(*tensors: torch.Tensor) -> tuple:
    """Identity part of a cache key: storage address, version counter (in-place writes bump it), shape and device of
    each tensor.  An address can be recycled once its tensor is freed, so pass the same tensors as `sources` of the
    entry: while it is cached they stay allocated and no other tensor can appear under their key."""
    return tuple((t.data_ptr(), t._version, t.shape, t.device) for t in tensors)


class Cache:
    def __init__(self, capturing: Callable[[], bool], capacity: Optional[int] = None):
        """capturing: the capture probe (ops.capturing).  capacity: most UNPINNED entries kept, oldest evicted first
        (None: unbounded); pinned entries do not count and can still be hit."""
        self._capturing, self.capacity = capturing, capacity
        self._entries: dict = {}        # key -> [value, pinned, sources, need]; dicts keep insertion order = age
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
            ent = self._entries[key] = [build(*args), False, sources, need]
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
