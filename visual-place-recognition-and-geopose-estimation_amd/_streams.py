"""The one owner of what the host layer keeps per stream besides device buffers: helper streams, the fork / join objects
with native HIP handles, and the warm-up + capture protocol of a HIP graph.

Helper streams and fork / join objects live in two `_cache.Cache` registries keyed (device index, raw handle of the MAIN
stream, ...) like every other stream-keyed cache, listed in `ops._STREAM_KEYED`: `ops.drop_stream_caches(raw)` forgets them
with that stream's workspaces and runs `close()` on what holds native handles.
"""
from __future__ import annotations

import ctypes
import functools
import os
import sys
from typing import Callable, Optional

import torch

from . import ops

_P, _U, _U32 = ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint32
_PROTOTYPES = {"hipExtMallocWithFlags": [ctypes.POINTER(_P), ctypes.c_size_t, _U], "hipFree": [_P],
               "hipStreamWriteValue32": [_P, _P, _U32, _U], "hipStreamWaitValue32": [_P, _P, _U32, _U, _U32],
               "hipEventCreateWithFlags": [ctypes.POINTER(_P), _U], "hipEventRecord": [_P, _P],
               "hipStreamWaitEvent": [_P, _P, _U], "hipEventDestroy": [_P]}


@functools.lru_cache(None)
def hip() -> ctypes.CDLL:
    """The HIP runtime torch itself uses, opened once, with the prototypes of the calls made here."""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    for name, argtypes in _PROTOTYPES.items():
        getattr(lib, name).argtypes = argtypes
    return lib


class _Closing:
    def __del__(self):      # close() at collection, but not at interpreter shutdown (the HIP runtime may be gone by then)
        if sys is not None and not sys.is_finalizing():     # (late in shutdown this module's globals are already None)
            self.close()


class _Native(_Closing):
    """Native handles in `_handles`, each released exactly once through the runtime call named `_free`."""
    def close(self) -> None:
        while self._handles:
            getattr(self._hip, self._free)(self._handles.pop())


class _StreamSignals(_Native):
    """Fork / join between two HIP streams through stream memory operations (hipStreamWriteValue32 on the producer stream,
    hipStreamWaitValue32 on the consumer stream, one 32-bit word of signal memory per direction, values from a counter that
    only grows) instead of hipEventRecord + hipStreamWaitEvent.  Round-3 experiment, OFF by default: an event operation costs
    the launch stream ~7 us of queue time whether or not anything has to be waited for (scripts/step_gaps.py: 14 us per block
    of the ViT), and in a two-GEMM probe the memory operations are cheaper (scripts/stream_sync_probe.py: 21 -> 13.5 us per
    fork + join pair) — but in the real step they are slower: 11.7-11.9 vs 11.31 ms per step (bench.py --side-sync signals, two
    runs each, one box).  A wait is only ever enqueued AFTER its write has been enqueued, so no stream can be left waiting
    for a value that never comes.  close() is hipFree, which synchronizes the device: no step ever takes that path."""
    _free = "hipFree"

    def __init__(self, device: torch.device):
        self._handles, self.count = [], 0
        self._hip = hip()
        with torch.cuda.device(device):
            for _ in range(2):
                p = ctypes.c_void_p()
                if self._hip.hipExtMallocWithFlags(ctypes.byref(p), 8, 0x2) != 0:          # hipMallocSignalMemory
                    raise RuntimeError("hipExtMallocWithFlags(hipMallocSignalMemory) failed")
                self._handles.append(p)

    def signal(self, word: int, stream: torch.cuda.Stream, value: int) -> None:
        if self._hip.hipStreamWriteValue32(stream.cuda_stream, self._handles[word], value & 0xFFFFFFFF, 0) != 0:
            raise RuntimeError("hipStreamWriteValue32 failed")

    def wait(self, word: int, stream: torch.cuda.Stream, value: int) -> None:
        # hipStreamWaitValueEq: the words only ever hold the value of the latest signal, and a wait for value v is enqueued
        # before the signal for v + 1 can be (program order of the loop), so equality is exact even across the 2^32 wrap
        if self._hip.hipStreamWaitValue32(stream.cuda_stream, self._handles[word], value & 0xFFFFFFFF, 0x1, 0xFFFFFFFF) != 0:
            raise RuntimeError("hipStreamWaitValue32 failed")

    # the three-call protocol DinoV2._blocks_side_chain uses (same as _TorchEvents / _RawEvents)
    def fork(self, main: torch.cuda.Stream, side: torch.cuda.Stream) -> None:
        self.count += 1
        self.signal(0, main, self.count)
        self.wait(0, side, self.count)

    def mark(self, side: torch.cuda.Stream) -> int:
        self.signal(1, side, self.count)
        return self.count

    def join(self, main: torch.cuda.Stream, tick: int) -> None:
        self.wait(1, main, tick)


class _TorchEvents:
    """Fork / join by torch.cuda.Event (hipEventDisableTiming; the record carries a system-scope release)."""

    def fork(self, main: torch.cuda.Stream, side: torch.cuda.Stream) -> None:
        e = torch.cuda.Event()
        e.record(main)
        side.wait_event(e)

    def mark(self, side: torch.cuda.Stream) -> "torch.cuda.Event":
        e = torch.cuda.Event()
        e.record(side)
        return e

    def join(self, main: torch.cuda.Stream, e: "torch.cuda.Event") -> None:
        main.wait_event(e)


class _RawEvents(_Native):
    """Fork / join by HIP events created with hipEventDisableTiming | hipEventDisableSystemFence (torch.cuda.Event cannot pass
    the second flag): the record then carries no system-scope cache writeback / invalidate — both streams are queues of
    the same device, device scope is all the hand-over needs.  A ring of events: a wait refers to the record that was
    latest when the wait was enqueued, so re-recording an event later never disturbs a wait already in a queue."""
    RING, _free = 128, "hipEventDestroy"

    def __init__(self, device: torch.device, flags: int = 0x2 | 0x20000000):
        self._handles, self._next = [], 0
        self._hip = hip()
        with torch.cuda.device(device):
            for _ in range(self.RING):
                e = ctypes.c_void_p()
                st = self._hip.hipEventCreateWithFlags(ctypes.byref(e), flags)
                if st != 0:
                    raise RuntimeError(f"hipEventCreateWithFlags(0x{flags:x}) failed: hipError {st}")
                self._handles.append(e)

    def _record(self, stream: torch.cuda.Stream):
        e = self._handles[self._next]
        self._next = (self._next + 1) % self.RING
        if self._hip.hipEventRecord(e, stream.cuda_stream) != 0:
            raise RuntimeError("hipEventRecord failed")
        return e

    def _wait(self, stream: torch.cuda.Stream, e) -> None:
        if self._hip.hipStreamWaitEvent(stream.cuda_stream, e, 0) != 0:
            raise RuntimeError("hipStreamWaitEvent failed")

    def fork(self, main: torch.cuda.Stream, side: torch.cuda.Stream) -> None:
        self._wait(side, self._record(main))

    def mark(self, side: torch.cuda.Stream):
        return self._record(side)

    def join(self, main: torch.cuda.Stream, e) -> None:
        self._wait(main, e)


_SIDES, _SYNCS = ops.cache(), ops.cache()   # (device index, main raw handle, role | mode) -> Stream | _RawEvents / _StreamSignals
ops._STREAM_KEYED += [_SIDES, _SYNCS]


def _index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def side_stream(device: torch.device, main_raw: int, role: str, priority: Optional[int] = None) -> torch.cuda.Stream:
    """Helper stream `role` ("cls" backbone cls rows, "salad" token MLP, "head" pose head) of the main stream `main_raw`."""
    return _SIDES.get((_index(device), main_raw, role), torch.cuda.Stream, (device, priority or 0))


def fork_join(device: torch.device, main_raw: int, mode: str):
    """DinoV2.side_sync `mode`: a fresh _TorchEvents, or the _RawEvents / _StreamSignals kept for this main stream."""
    if mode == "events":
        return _TorchEvents()
    return _SYNCS.get((_index(device), main_raw, mode), _StreamSignals if mode == "signals" else _RawEvents, (device,))


class Captured(_Closing):
    """run() as a HIP graph: a private stream that waits for the current one, `warmup` runs on it (module load, allocator,
    the stream-keyed workspaces), join, device synchronize, then the capture of run() on that SAME stream, so the graph
    addresses the buffers the warm-up made.  `out` is what the captured run() returned: the graph's static outputs."""

    def __init__(self, run: Callable[[], object], device: torch.device, warmup: int = 2):
        cur = torch.cuda.current_stream(device)
        self.stream = torch.cuda.Stream(device=device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):
                run()
        cur.wait_stream(self.stream)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):      # if this raises, collection of the half-made object closes it
            self.out = run()

    def close(self) -> None:
        """Destroy the graph and forget everything the package keyed by its private stream (ops.drop_stream_caches)."""
        self.graph = self.out = None
        if getattr(self, "stream", None) is not None:
            ops.drop_stream_caches(self.stream.cuda_stream)
            self.stream = None
