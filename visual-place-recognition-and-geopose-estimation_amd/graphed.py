"""Replay a model forward from a HIP graph, one graph per input shape.

The evaluation / gallery-building loops are host-bound once the GPU path is in place: a ViT-L/14 + SALAD forward is
~300 kernel launches = 4-6 ms of Python under the GIL per batch, the same lock the image-decode threads
(`loader.ImageBatchLoader`) need.  Captured once per input shape, the forward is ONE graph launch (0.1 ms of host time,
same GPU time as the eager in-stream forward: `scripts/graph_backbone.py`).

Capture rules the wrapped function must obey (the HIP paths of this package do): no host sync, no `.item()`/`.cpu()`,
workspaces from `ops.workspace`.  Warm-up and capture follow the package's one protocol, `_streams.Captured`: both run on
the SAME private stream (one per graph), so the stream-keyed buffers the warm-up allocated are the ones the graph
addresses.  The DINOv2 backbone's cls-row side stream is switched off inside the captured forward: fork / join branches
replay slower than the eager side stream (16.2 vs 10.9 ms) while the linear chain replays at the eager in-stream time
(11.3 ms); results are bit-identical either way (`test_cls_side_chain_is_bit_identical_to_in_stream_path`,
`test_graphed_forward_equals_eager`).

A captured graph addresses its operands by raw pointer, including what the package caches between calls.  All of that lives
in `_cache.Cache`, which pins every entry handed out during a capture: never evicted, never freed when its value is rebuilt
(a workspace that has to grow), so graphs of several input shapes and eager calls can be interleaved freely.  Only `close()`
— or collection of the wrapper — forgets them, through `ops.drop_stream_caches()`: everything keyed by the private stream,
i.e. its workspaces, raw-token buffers, and the helper streams and fork / join objects (`_streams`) made for work on it.

Weights are addressed the same way: after changing parameters (a state-dict load, `fold_layerscale()`, `pack()`), build
a new GraphedForward.

The returned tensors are the graph's static output buffers: valid until the next call with the same input shape —
consume (or clone) them before that, on the stream the call was made on.
"""
from __future__ import annotations

from typing import Callable, Dict, Tuple

import torch

from . import _streams


def _backbones(obj) -> list:
    """DinoV2 backbones reachable from a module (their cls side chain is disabled while a graph is captured)."""
    return [m for m in obj.modules() if hasattr(m, "cls_side_chain")] if isinstance(obj, torch.nn.Module) else []


class GraphedForward:
    def __init__(self, fn: Callable[[torch.Tensor], object], module: torch.nn.Module = None, warmup: int = 2):
        """fn(x) -> tensor or (nested) tuple of tensors.  `module` (optional): where to look for DINOv2 backbones whose
        side stream has to be off during capture (defaults to fn if it is a module)."""
        self.fn, self.warmup = fn, max(1, warmup)
        self._backbones = _backbones(module if module is not None else fn)
        self._graphs: Dict[Tuple, Tuple] = {}      # (shape, dtype, device index) -> (_streams.Captured, static input)
        self.fallback_reason = None          # set when a capture failed: the wrapper then runs the eager forward for good

    def close(self) -> None:
        """Destroy the graphs and forget what the package keyed by their private streams (_streams.Captured.close)."""
        for cap, _ in self._graphs.values():
            cap.close()
        self._graphs.clear()

    def _run(self, x):
        saved = [b.cls_side_chain for b in self._backbones]
        for b in self._backbones:
            b.cls_side_chain = False
        try:
            with torch.no_grad():
                return self.fn(x)
        finally:
            for b, s in zip(self._backbones, saved):
                b.cls_side_chain = s

    def __call__(self, x: torch.Tensor):
        if not x.is_cuda or self.fallback_reason is not None:
            return self._run(x)
        key = (tuple(x.shape), x.dtype, x.device.index)
        entry = self._graphs.get(key)
        if entry is None:
            static_in = x.clone()
            try:
                cap = _streams.Captured(lambda: self._run(static_in), x.device, self.warmup)
            except Exception as e:                             # noqa: BLE001  a forward that cannot be captured (host sync, ...)
                self.fallback_reason = f"{type(e).__name__}: {e}"
                torch.cuda.synchronize(x.device)
                return self._run(x)
            entry = self._graphs[key] = (cap, static_in)
        cap, static_in = entry
        static_in.copy_(x)
        cap.graph.replay()
        return cap.out

    def graphs(self) -> int:
        return len(self._graphs)
