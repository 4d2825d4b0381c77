"""Tensor-level wrappers over the C ABI (include/vpr_amd.h).

Each function takes torch tensors that already live on the GPU, launches the HIP kernels on
torch's current stream and returns torch tensors; PyTorch is used for device memory and streams
only.  Any non-zero status raises RuntimeError — there is no eager/CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._cache import Cache, Handover, StreamProbes, tensor_key


def _raw_stream(device_index: int = -1) -> int:
    """Current HIP stream handle of a device (torch.cuda.current_stream() costs ~8 us of Python per call; this is
    the C entry point underneath it, ~0.3 us — there are ~300 launches per pipeline step)."""
    if device_index < 0:
        device_index = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(device_index)


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(_raw_stream())


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _need(t: torch.Tensor, dtype: torch.dtype, name: str, ndim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"{name}: expected {ndim} dims, got {t.dim()}")


def capturing() -> bool:
    """True while the current stream records into a HIP graph: whatever a cache hands out now is baked into the graph
    as a raw address and must stay allocated for as long as the graph may be replayed."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _current_stream_name() -> Optional[Tuple[int, int]]:
    """(device index, raw handle) of the current stream; None while this process has not touched a GPU."""
    if not torch.cuda.is_initialized():
        return None
    idx = torch.cuda.current_device()
    return idx, torch._C._cuda_getCurrentRawStream(idx)


def _current_stream_object() -> "torch.Stream":
    """torch.cuda.current_stream() through the C entry point underneath it (like _raw_stream: none of the Python device
    bookkeeping, and nothing a test that substitutes torch.cuda.Stream / torch.cuda.device can get in the way of)."""
    sid, idx, kind = torch._C._cuda_getCurrentStream(torch.cuda.current_device())
    return torch._C._CudaStreamBase(stream_id=sid, device_index=idx, device_type=kind)


def _record_event() -> "torch.cuda.Event":
    e = torch.cuda.Event()
    e.record(_current_stream_object())
    return e


def _wait_event(event: "torch.cuda.Event") -> None:
    event.wait(_current_stream_object())


def _keep_for_current_stream(value) -> None:
    """Tensor.record_stream on every GPU tensor in `value` (a tensor, or tuples / lists of them): when the last reference
    goes, the allocator reuses the memory only after what the current stream has queued by then."""
    if isinstance(value, torch.Tensor):
        if value.is_cuda:
            value.record_stream(_current_stream_object())
    elif isinstance(value, (tuple, list)):
        for v in value:
            _keep_for_current_stream(v)


# The hand-over of a cached value from the stream that built it to any other (_cache.Handover): one event wait and one
# record_stream at the first hit from that stream, host-side comparisons ever after.
_PROBES = StreamProbes(_current_stream_name, _record_event, _wait_event, _keep_for_current_stream)


def handover() -> Handover:
    """A _cache.Handover for a device value built just now on the current stream and kept outside any cache (folded
    LayerScale weights, FusedGeoPoseHead's packed matrices): call .lend(value) wherever the value is used."""
    return Handover(_PROBES, lambda: capturing())


def cache(capacity: Optional[int] = None) -> Cache:
    """A _cache.Cache that asks this module's capturing() (looked up per call: a test can substitute it) and orders
    every value it hands to a stream other than the one that built it (_PROBES)."""
    return Cache(lambda: capturing(), capacity, _PROBES)


def _call(name: str, *args) -> None:
    """Call the entry point `name` of the library and raise, under that same name, on a non-zero status."""
    st = getattr(_lib.lib(), name)(*args)
    if st:
        _lib.check(st, name)


# Caches keyed (device index, raw stream handle, ...): two streams driving the library concurrently (e.g. two batches in
# flight) never share scratch memory, and drop_stream_caches() forgets a stream that is gone.
_WORKSPACES = cache()
_ZERO_ROWS = cache(8)
_STREAM_KEYED = [_WORKSPACES, _ZERO_ROWS]       # the one list: _streams adds its helper-stream and fork / join registries


def _alloc_bytes(nbytes: int, device: torch.device, zero: bool) -> torch.Tensor:
    return (torch.zeros if zero else torch.empty)(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _alloc_zero_rows(M: int, C: int, device: torch.device) -> torch.Tensor:
    return torch.zeros((M, C), dtype=torch.bfloat16, device=device)


def workspace(name: str, nbytes: int, device: torch.device, stream_key: Optional[int] = None, zero: bool = False) -> torch.Tensor:
    """Cached byte buffer per (device, stream, name); grows, never shrinks.  One entry of the package's graph-safe cache
    (_cache.Cache): a buffer handed out during graph capture is never freed (a later, larger request gets a new one; the
    old one stays allocated beside it) until drop_stream_caches() forgets its stream.
    stream_key: raw handle of the stream that OWNS the buffer when the caller is working for it from a helper stream.
    zero: a new buffer is zero-filled (kernels with arrival counters at the head of their workspace need zeros on first use
    and leave zeros behind: vpr_pose_head_fused)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, _raw_stream(idx) if stream_key is None else stream_key, name)
    return _WORKSPACES.get(key, _alloc_bytes, (nbytes, device, zero), need=nbytes)


def zero_rows_bf16(M: int, C: int, device: torch.device) -> torch.Tensor:
    """Cached [M, C] bf16 matrix per (device, current stream, shape), zero when created: the backbone's raw-token buffer,
    whose cls rows nothing ever writes."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return _ZERO_ROWS.get((idx, _raw_stream(idx), M, C), _alloc_zero_rows, (M, C, device))


def drop_stream_caches(raw_stream: int) -> None:
    """Forget every entry keyed by this stream handle (workspaces, raw-token buffers, its helper streams and fork / join objects:
    _streams), pinned ones included (_streams.Captured.close(): the private stream is gone, with the graphs that addressed them)."""
    for c in _STREAM_KEYED:
        c.drop(lambda k: k[1] == raw_stream)


# ------------------------------------------------------------------------------------------ SALAD
@dataclass
class SaladWeights:
    """Kernel-format SALAD weights (bf16 [out,in] matrices, f32 biases), all on one GPU.

    w1_sc = cat(score.0.weight, cluster_features.0.weight) [2*hidden, C]; see include/vpr_amd.h.
    """
    w1_sc: torch.Tensor
    b1_sc: torch.Tensor
    w2_s: torch.Tensor
    b2_s: torch.Tensor
    w2_c: torch.Tensor
    b2_c: torch.Tensor
    w1_t: torch.Tensor
    b1_t: torch.Tensor
    w2_t: torch.Tensor
    b2_t: torch.Tensor
    dustbin: float = 1.0

    matrix_dtype = torch.bfloat16       # class-level (no annotation: not a field)
    _workspace = ("salad", "vpr_salad_workspace_bytes", True)      # workspace name, its size query, zero-filled when new

    def validate(self) -> Tuple[int, int, int, int, int]:
        for n in ("w1_sc", "w2_s", "w2_c", "w1_t", "w2_t"):
            _need(getattr(self, n), self.matrix_dtype, n, 2)
        for n in ("b1_sc", "b2_s", "b2_c", "b1_t", "b2_t"):
            _need(getattr(self, n), torch.float32, n, 1)
        hidden2, C = self.w1_sc.shape
        hidden = hidden2 // 2
        m, l, t = self.w2_s.shape[0], self.w2_c.shape[0], self.w2_t.shape[0]
        ok = (self.w2_s.shape[1] == hidden and self.w2_c.shape[1] == hidden and
              tuple(self.w1_t.shape) == (hidden, C) and self.w2_t.shape[1] == hidden and
              self.b1_sc.numel() == 2 * hidden and self.b2_s.numel() == m and
              self.b2_c.numel() == l and self.b1_t.numel() == hidden and self.b2_t.numel() == t)
        if not ok:
            raise RuntimeError("SaladWeights: inconsistent shapes")
        return C, hidden, m, l, t

    def c_struct(self) -> _lib.SaladWeightsC:
        fs, fc = _salad_w2_fragments(self)
        ptrs = [getattr(self, n).data_ptr() for n, _ in _lib.SaladWeightsC._fields_[:10]]
        return _lib.SaladWeightsC(*ptrs, fs.data_ptr() if fs is not None else None, fc.data_ptr() if fc is not None else None)


_SALAD_FRAGS = cache(16)
salad_use_fragments = True      # False: hand the C ABI null *_frag pointers (the kernel then reads W2 row-major; tests / A/B)


def _pack_w2_fragments(src: torch.Tensor) -> torch.Tensor:
    frag = torch.empty_like(src)
    _call("vpr_salad_pack_w2_fragments", _ptr(src), src.shape[0], src.shape[1], _ptr(frag), _stream())
    return frag


def _salad_w2_fragments(w: "SaladWeights"):
    """(w2_s, w2_c) in MFMA fragment order (vpr_salad_pack_w2_fragments), packed once per (storage, version) like the pose
    head's planes."""
    out = []
    if not salad_use_fragments:
        return None, None
    for src in (w.w2_s, w.w2_c):
        n_out, hidden = src.shape
        if src.dtype != torch.bfloat16 or not src.is_cuda or n_out % 16 or hidden % 256:
            out.append(None)
            continue
        out.append(_SALAD_FRAGS.get(tensor_key(src), _pack_w2_fragments, (src,), (src,)))
    return out[0], out[1]


def _tokens(tokens, dtype: torch.dtype, what: str):
    """[B, 1+n, C] (cls first) or a (patch [B,n,C], cls [B,C]) pair, of `dtype` -> (patch pointer, patch image stride, cls
    pointer, cls stride, B, n, C, device); strides in elements."""
    if isinstance(tokens, torch.Tensor):
        _need(tokens, dtype, "tokens", 3)
        B, tpi, C = tokens.shape
        p = tokens.data_ptr()
        return ctypes.c_void_p(p + tokens.element_size() * C), tpi * C, ctypes.c_void_p(p), tpi * C, B, tpi - 1, C, tokens.device
    patch, cls = tokens
    _need(patch, dtype, "patch", 3)
    _need(cls, dtype, "cls", 2)
    B, n, C = patch.shape
    if tuple(cls.shape) != (B, C):
        raise RuntimeError(f"{what}: cls must be [B, C] = {(B, C)}, got {tuple(cls.shape)}")
    return _ptr(patch), n * C, _ptr(cls), C, B, n, C, patch.device


def _salad_setup(w: SaladWeights, B: int, n: int, device: torch.device, Ct: Optional[int] = None, want_bf16: Optional[bool] = None,
                 out: Optional[torch.Tensor] = None, owner_raw_stream: Optional[int] = None):
    """What every aggregation entry needs: validated weights (with Ct given, checked against the token width), the
    workspace (of stream `owner_raw_stream`, default the current one) and, unless want_bf16 is None, the outputs.
    -> ((C, hidden, m, l, t), workspace, descriptor f32 [B, t+l*m] (`out` if given), bf16 copy or None)."""
    C, hidden, m, l, t = dims = w.validate()
    if Ct is not None and Ct != C:
        raise RuntimeError(f"tokens have C={Ct}, weights expect {C}")
    name, size_query, zero = w._workspace
    ws = workspace(name, getattr(_lib.lib(), size_query)(B, n, C, m, l, t, hidden), device, owner_raw_stream, zero)
    if want_bf16 is None:
        return dims, ws, None, None
    if out is None:
        out = torch.empty((B, t + l * m), dtype=torch.float32, device=device)
    else:
        _need(out, torch.float32, "out", 2)
        if tuple(out.shape) != (B, t + l * m):
            raise RuntimeError(f"out must be [B, t+l*m] = {(B, t + l * m)}, got {tuple(out.shape)}")
    out16 = torch.empty((B, t + l * m), dtype=torch.bfloat16, device=device) if want_bf16 else None
    return dims, ws, out, out16


def salad_aggregate(tokens: torch.Tensor, w: SaladWeights, sinkhorn_iters: int = 3,
                    want_bf16: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """tokens [B, 1+n, C] bf16 (cls first) -> (descriptor f32 [B, t+l*m], bf16 copy or None)."""
    _need(tokens, torch.bfloat16, "tokens", 3)
    B, tpi, Ct = tokens.shape
    (C, hidden, m, l, t), ws, out, out16 = _salad_setup(w, B, tpi - 1, tokens.device, Ct, want_bf16)
    cw = w.c_struct()
    _call("vpr_salad_aggregate", _ptr(tokens), B, tpi, C, ctypes.byref(cw), float(w.dustbin), m, l, t, hidden,
          int(sinkhorn_iters), _ptr(out), _ptr(out16), _ptr(ws), ws.numel(), _stream())
    return out, out16


def salad_stage_token(cls: torch.Tensor, w: SaladWeights, n: int, owner_raw_stream: int) -> None:
    """Stage T of the aggregation on its own (vpr_salad_stage_token): token MLP of the B cls rows on the CURRENT stream,
    result left in the SALAD workspace that belongs to stream `owner_raw_stream` (the stream that will run
    salad_aggregate_split(..., token_done=True) for the same batch, ordered after this call by the caller).  The DINOv2
    backbone calls it from its cls-row side stream, where the cls tokens are final ~0.3 ms before the patch tokens."""
    _need(cls, torch.bfloat16, "cls", 2)
    B, Ct = cls.shape
    (C, hidden, m, l, t), ws, _, _ = _salad_setup(w, B, n, cls.device, owner_raw_stream=owner_raw_stream)
    if Ct != C:
        raise RuntimeError(f"cls {tuple(cls.shape)} does not match weights with C={C}")
    cw = w.c_struct()
    _call("vpr_salad_stage_token", _ptr(cls), C, B, n, C, ctypes.byref(cw), m, l, t, hidden, _ptr(ws), ws.numel(), _stream())


def salad_aggregate_split(patch: torch.Tensor, cls: torch.Tensor, w: SaladWeights, sinkhorn_iters: int = 3,
                          want_bf16: bool = True, overlap: Optional[bool] = None,
                          token_done: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """patch [B, n, C] bf16 + cls [B, C] bf16 -> (descriptor f32 [B, t+l*m], bf16 copy or None).
    token_done: salad_stage_token already ran for these cls rows (and is ordered before this call): stages M and A only.
    overlap=True: the aggregation runs as its three stages with the token MLP (64 cls rows: two 4 us weight streams) on a
    side stream beside the all-CU score / cluster GEMM, joined before the Sinkhorn stage — same kernels, same workspace,
    bit-identical result to the one-call form.  Off by default: one fork + join between two HIP streams costs ~25 us here;
    the pipeline hides the token MLP for free by running it on the backbone's cls-row stream (salad_stage_token)."""
    _need(patch, torch.bfloat16, "patch", 3)
    _need(cls, torch.bfloat16, "cls", 2)
    B, n, Ct = patch.shape
    (C, hidden, m, l, t), ws, out, out16 = _salad_setup(w, B, n, patch.device, want_bf16=want_bf16)
    if Ct != C or tuple(cls.shape) != (B, C):
        raise RuntimeError(f"patch {tuple(patch.shape)} / cls {tuple(cls.shape)} do not match weights with C={C}")
    cw = w.c_struct()
    mlps = (_ptr(patch), n * C, B, n, C, ctypes.byref(cw), m, l, t, hidden, _ptr(ws), ws.numel())
    aggregate = (B, n, C, float(w.dustbin), m, l, t, hidden, int(sinkhorn_iters), _ptr(out), _ptr(out16), _ptr(ws), ws.numel())
    if token_done:
        raw = _stream()
        _call("vpr_salad_stage_mlps", *mlps, raw)
        _call("vpr_salad_stage_aggregate", *aggregate, raw)
        return out, out16
    if overlap is None:
        overlap = False     # measured (scripts/salad_ab.py): the fork + join of a side stream costs more than the 10 us it hides
    if not overlap:
        _call("vpr_salad_aggregate_split", _ptr(patch), _ptr(cls), B, n, C, ctypes.byref(cw), float(w.dustbin), m, l, t,
              hidden, int(sinkhorn_iters), _ptr(out), _ptr(out16), _ptr(ws), ws.numel(), _stream())
        return out, out16
    main = torch.cuda.current_stream(patch.device)
    main_raw = ctypes.c_void_p(main.cuda_stream)
    from . import _streams
    side = _streams.side_stream(patch.device, main_raw.value, "salad")
    side.wait_stream(main)                                   # cls (and the workspace's previous consumer) are ready
    _call("vpr_salad_stage_token", _ptr(cls), C, B, n, C, ctypes.byref(cw), m, l, t, hidden, _ptr(ws), ws.numel(),
          ctypes.c_void_p(side.cuda_stream))
    _call("vpr_salad_stage_mlps", *mlps, main_raw)
    main.wait_stream(side)
    _call("vpr_salad_stage_aggregate", *aggregate, main_raw)
    return out, out16


def _salad_whole(entry: str, dtype: torch.dtype, tokens, w: SaladWeights, iters: int, want_bf16: bool,
                 out: Optional[torch.Tensor] = None, extra=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The whole aggregation through `entry`, one of the C calls that address either token layout in place: `tokens` of
    `dtype` as _tokens() takes them.  extra(B, n, hidden) -> (arguments between sinkhorn_iters and the outputs, arguments
    between the outputs and the workspace): what vpr_salad_aggregate_train adds to the common parameter list."""
    patch_ptr, patch_stride, cls_ptr, cls_stride, B, n, Ct, device = _tokens(tokens, dtype, entry[len("vpr_"):])
    (C, hidden, m, l, t), ws, out, out16 = _salad_setup(w, B, n, device, Ct, want_bf16, out)
    before, after = extra(B, n, hidden) if extra is not None else ((), ())
    cw = w.c_struct()
    _call(entry, patch_ptr, patch_stride, cls_ptr, cls_stride, B, n, C, ctypes.byref(cw), float(w.dustbin), m, l, t, hidden,
          int(iters), *before, _ptr(out), _ptr(out16), *after, _ptr(ws), ws.numel(), _stream())
    return out, out16


def salad_aggregate_train(tokens, w: SaladWeights, dropout_p: float, seed: int, pass_index: int, image_base: int = 0,
                          sinkhorn_iters: int = 3, want_bf16: bool = True, mask_out: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The aggregation in training mode: Dropout(dropout_p) active in the score / cluster MLPs, as the hub model runs while
    dinov2salad_finetuning.py:115 has it in train() (vpr_salad_aggregate_train).  `tokens` = [B, 1+n, C] bf16 (cls first) or a
    (patch [B,n,C], cls [B,C]) bf16 pair.  The mask is a pure function of (seed, pass_index, image_base + b, token, unit): a
    dataset aggregated in any chunking gives the same bits.  seed: unsigned 64-bit; pass_index: unsigned 32-bit.
    mask_out (uint8 [B*n, 2*hidden], optional) receives the mask, 1 = kept.  dropout_p = 0 gives the bits of
    salad_aggregate_split.  out (f32 [B, t+l*m], contiguous, optional): where the descriptor goes (e.g. rows of a
    fine-tuning buffer).  -> (descriptor f32 [B, t+l*m], bf16 copy or None)."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"salad_aggregate_train: seed must be an unsigned 64-bit integer, got {seed!r}")
    if not 0 <= int(pass_index) < 1 << 32:
        raise ValueError(f"salad_aggregate_train: pass_index must be an unsigned 32-bit integer, got {pass_index!r}")

    def train_args(B: int, n: int, hidden: int):
        if mask_out is not None:
            _need(mask_out, torch.uint8, "mask_out", 2)
            if tuple(mask_out.shape) != (B * n, 2 * hidden):
                raise RuntimeError(f"mask_out must be [B*n, 2*hidden] = {(B * n, 2 * hidden)}, got {tuple(mask_out.shape)}")
        return (float(dropout_p), int(seed), int(pass_index), int(image_base)), (_ptr(mask_out),)

    return _salad_whole("vpr_salad_aggregate_train", torch.bfloat16, tokens, w, sinkhorn_iters, want_bf16, out, train_args)


class SaladStageViews(NamedTuple):
    S: torch.Tensor                  # [slabs, B*n, m] f32: partial-sum slabs of the cluster scores (slab 0 carries b2_s)
    F: torch.Tensor                  # [slabs, B*n, l] f32: the same for the cluster features
    g: torch.Tensor                  # [B, t] f32: token features
    H: Optional[torch.Tensor]        # [B*n, 2*hidden] bf16 hidden activations — unfused route (slabs == 1) only, else None


def salad_stage_views(ws: torch.Tensor, B: int, n: int, w: SaladWeights) -> SaladStageViews:
    """Views of what stages T and M left in the SALAD workspace `ws` (ops.workspace("salad", ...) of the stream that ran
    them) for a batch of B images x n patch tokens (tests).  The layout comes from vpr_salad_stage_outputs
    (include/vpr_amd_salad_stages.h), which asks the library's own plan: nothing about it is restated here.  The route
    (slabs) is the one the A/B switches select NOW, so ask before changing them."""
    C, hidden, m, l, t = w.validate()
    S, F, g, H = (ctypes.c_void_p(0) for _ in range(4))
    slabs, rows = ctypes.c_int(0), ctypes.c_longlong(0)
    _call("vpr_salad_stage_outputs", _ptr(ws), ws.numel(), B, n, C, m, l, t, hidden, ctypes.byref(S), ctypes.byref(F),
          ctypes.byref(g), ctypes.byref(H), ctypes.byref(slabs), ctypes.byref(rows))

    def view(p: ctypes.c_void_p, dtype: torch.dtype, *shape: int) -> torch.Tensor:
        off, count = p.value - ws.data_ptr(), 1
        for s in shape:
            count *= s
        return ws[off: off + count * dtype.itemsize].view(dtype).view(*shape)

    ns, r = slabs.value, rows.value
    return SaladStageViews(view(S, torch.float32, ns, r, m), view(F, torch.float32, ns, r, l), view(g, torch.float32, B, t),
                           view(H, torch.bfloat16, r, 2 * hidden) if ns == 1 else None)


@dataclass
class SaladWeightsF32(SaladWeights):
    """The same ten tensors, all f32 (vpr_salad_weights_f32): operands of the f32-accurate aggregation."""
    matrix_dtype = torch.float32
    _workspace = ("salad_f32", "vpr_salad_f32_workspace_bytes", False)

    def c_struct(self) -> _lib.SaladWeightsF32C:
        return _lib.SaladWeightsF32C(*[getattr(self, n).data_ptr() for n, _ in _lib.SaladWeightsF32C._fields_])


def salad_aggregate_f32(tokens, w: SaladWeightsF32, sinkhorn_iters: int = 3,
                        want_bf16: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The aggregation at the reference's precision: `tokens` = [B, 1+n, C] f32 (cls first) or a (patch [B,n,C], cls [B,C])
    pair of f32 tensors, f32 weights -> (descriptor f32 [B, t+l*m], bf16 copy or None).  vpr_salad_aggregate_f32."""
    return _salad_whole("vpr_salad_aggregate_f32", torch.float32, tokens, w, sinkhorn_iters, want_bf16)


class SaladF32StageViews(NamedTuple):
    H: torch.Tensor                  # [B*n, 2*hidden] f32 hidden activations: score head, then cluster head
    Ht: torch.Tensor                 # [B, hidden] f32 hidden activations of the token MLP
    S: torch.Tensor                  # [B*n, m] f32 cluster scores (b2_s included)
    F: torch.Tensor                  # [B*n, l] f32 cluster features
    g: torch.Tensor                  # [B, t] f32 token features
    A1: torch.Tensor                 # [B*n, 6, C] bf16 planes of the patch tokens, activation order (q h m m h h)
    cls3: torch.Tensor               # [B, 6, C] bf16 planes of the cls rows, activation order
    W1: torch.Tensor                 # [2*hidden, 6, C] bf16 planes of w1_sc, weight order (h q m h m h)
    H2: torch.Tensor                 # [B*n, 2, 6, hidden] bf16 planes of H: head (score, cluster), segment, column
    W1t: torch.Tensor                # [hidden, 6, C], weight order
    W2s: torch.Tensor                # [m, 6, hidden]
    W2c: torch.Tensor                # [l, 6, hidden]
    W2t: torch.Tensor                # [t, 6, hidden]
    Ht2: torch.Tensor                # [B, 6, hidden] bf16 planes of Ht, activation order


def salad_f32_stage_views(ws: torch.Tensor, B: int, n: int, w: "SaladWeightsF32") -> SaladF32StageViews:
    """Views of what the f32-accurate aggregation (salad_aggregate_f32, _f32_n, _f32_hires) left in its workspace `ws`
    (ops.workspace("salad_f32", ...) of the stream that ran it) for a batch of B images x n patch tokens (tests).  The layout
    comes from vpr_salad_f32_stage_outputs (include/vpr_amd_salad_f32_stages.h), which asks the library's own plan: nothing
    about it is restated here but the shapes the header states."""
    C, hidden, m, l, t = w.validate()
    names = SaladF32StageViews._fields
    ptrs = {k: ctypes.c_void_p(0) for k in names}
    _call("vpr_salad_f32_stage_outputs", _ptr(ws), ws.numel(), B, n, C, m, l, t, hidden, *[ctypes.byref(ptrs[k]) for k in names])

    def view(p: ctypes.c_void_p, dtype: torch.dtype, *shape: int) -> torch.Tensor:
        off, count = p.value - ws.data_ptr(), 1
        for s in shape:
            count *= s
        return ws[off: off + count * dtype.itemsize].view(dtype).view(*shape)

    r, f, b = B * n, torch.float32, torch.bfloat16
    shapes = dict(H=(f, r, 2 * hidden), Ht=(f, B, hidden), S=(f, r, m), F=(f, r, l), g=(f, B, t), A1=(b, r, 6, C), cls3=(b, B, 6, C),
                  W1=(b, 2 * hidden, 6, C), H2=(b, r, 2, 6, hidden), W1t=(b, hidden, 6, C), W2s=(b, m, 6, hidden),
                  W2c=(b, l, 6, hidden), W2t=(b, t, 6, hidden), Ht2=(b, B, 6, hidden))
    return SaladF32StageViews(*[view(ptrs[k], *shapes[k]) for k in names])


def _salad_stage_a(entry: str, scores: torch.Tensor, feats: torch.Tensor, tokfeat: torch.Tensor, dustbin: float, iters: int,
                   want_bf16: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Stage A alone through `entry` (vpr_salad_sinkhorn_aggregate or its run-time-n form: the same parameter list)."""
    _need(scores, torch.float32, "scores", 3)
    _need(feats, torch.float32, "feats", 3)
    _need(tokfeat, torch.float32, "tokfeat", 2)
    B, n, m = scores.shape
    l, t = feats.shape[2], tokfeat.shape[1]
    if feats.shape[:2] != (B, n) or tokfeat.shape[0] != B:
        raise RuntimeError(f"{entry[len('vpr_'):]}: inconsistent shapes")
    out = torch.empty((B, t + l * m), dtype=torch.float32, device=scores.device)
    out16 = torch.empty_like(out, dtype=torch.bfloat16) if want_bf16 else None
    _call(entry, _ptr(scores), _ptr(feats), _ptr(tokfeat), B, n, m, l, t, float(dustbin), int(iters), _ptr(out), _ptr(out16), _stream())
    return out, out16


def salad_sinkhorn_aggregate(scores: torch.Tensor, feats: torch.Tensor, tokfeat: torch.Tensor,
                             dustbin: float, sinkhorn_iters: int = 3,
                             want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """scores [B,n,m] f32, feats [B,n,l] f32, tokfeat [B,t] f32 -> descriptor (Sinkhorn stage only)."""
    return _salad_stage_a("vpr_salad_sinkhorn_aggregate", scores, feats, tokfeat, dustbin, sinkhorn_iters, want_bf16)


# ---- any patch-token count 65 .. 576 (include/vpr_amd_salad_anyres.h); the functions above keep their n = 256 domain ----
def salad_sinkhorn_aggregate_n(scores: torch.Tensor, feats: torch.Tensor, tokfeat: torch.Tensor,
                               dustbin: float, iters: int = 3,
                               want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """salad_sinkhorn_aggregate for any n in 65 .. 576: scores [B,n,m] f32, feats [B,n,l] f32, tokfeat [B,t] f32 -> descriptor
    (and its bf16 copy).  Always the run-time-n kernel, n = 256 included.  vpr_salad_sinkhorn_aggregate_n."""
    return _salad_stage_a("vpr_salad_sinkhorn_aggregate_n", scores, feats, tokfeat, dustbin, iters, want_bf16)


def salad_aggregate_n(tokens, w: SaladWeights, iters: int = 3,
                      want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The aggregation for any patch-token count n in 65 .. 576: `tokens` = [B, 1+n, C] bf16 (cls first) or a (patch [B,n,C],
    cls [B,C]) bf16 pair, addressed in place -> (descriptor f32 [B, t+l*m], bf16 copy or None).  n == 256 gives the bits of
    salad_aggregate_split.  vpr_salad_aggregate_n."""
    return _salad_whole("vpr_salad_aggregate_n", torch.bfloat16, tokens, w, iters, want_bf16)


def salad_aggregate_f32_n(tokens, w: SaladWeightsF32, iters: int = 3,
                          want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """salad_aggregate_f32 for any n in 65 .. 576 (f32 tokens, hub layout or pair; f32 weights); n == 256 gives its bits.
    vpr_salad_aggregate_f32_n."""
    return _salad_whole("vpr_salad_aggregate_f32_n", torch.float32, tokens, w, iters, want_bf16)


# ---- 65 .. 1369 patch tokens, i.e. up to 518 px (include/vpr_amd_salad_hires.h); the functions above keep their domains ----
def salad_sinkhorn_aggregate_hires(scores: torch.Tensor, feats: torch.Tensor, tokfeat: torch.Tensor,
                                   dustbin: float, iters: int = 3,
                                   want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """salad_sinkhorn_aggregate for any n in 65 .. 1369: scores [B,n,m] f32, feats [B,n,l] f32, tokfeat [B,t] f32 -> descriptor
    (and its bf16 copy).  Always the high-resolution kernel, which recomputes K from the scores on every pass instead of
    keeping it in LDS, n <= 576 included.  vpr_salad_sinkhorn_aggregate_hires."""
    return _salad_stage_a("vpr_salad_sinkhorn_aggregate_hires", scores, feats, tokfeat, dustbin, iters, want_bf16)


def salad_aggregate_hires(tokens, w: SaladWeights, iters: int = 3,
                          want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The aggregation for any patch-token count n in 65 .. 1369 (448 px = 1024, 518 px = 1369): `tokens` = [B, 1+n, C] bf16
    (cls first) or a (patch [B,n,C], cls [B,C]) bf16 pair, addressed in place -> (descriptor f32 [B, t+l*m], bf16 copy or
    None).  n == 256 gives the bits of salad_aggregate_split, any other n <= 576 those of salad_aggregate_n.
    vpr_salad_aggregate_hires."""
    return _salad_whole("vpr_salad_aggregate_hires", torch.bfloat16, tokens, w, iters, want_bf16)


def salad_aggregate_f32_hires(tokens, w: SaladWeightsF32, iters: int = 3,
                              want_bf16: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """salad_aggregate_f32 for any n in 65 .. 1369 (f32 tokens, hub layout or pair; f32 weights); n == 256 gives its bits,
    any other n <= 576 those of salad_aggregate_f32_n.  vpr_salad_aggregate_f32_hires."""
    return _salad_whole("vpr_salad_aggregate_f32_hires", torch.float32, tokens, w, iters, want_bf16)


def _need_rows(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    """A 2-D GPU matrix whose rows may be padded (stride(1) == 1, any stride(0)): the leading dimension goes to C."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() != 2 or (t.stride(1) != 1 and t.shape[1] > 1):
        raise RuntimeError(f"{name}: expected a 2-D tensor with unit column stride")


def _gemm_fields(a, w, bias, relu, out_dtype, out, a_group_rows, a_group_stride, m):
    """The vpr_gemm_problem fields of one GEMM (allocating `out` if it is None).  Only what the library cannot see is
    checked here (dtypes, shapes, that row-group addressing stays inside a's storage); strides, alignment and the
    tile constraints are the library's to judge, and its status is passed through."""
    _need_rows(a, torch.bfloat16, "a")
    _need_rows(w, torch.bfloat16, "w")
    if bias is not None:
        _need(bias, torch.float32, "bias", 1)
    K = a.shape[1]
    M = a.shape[0] if m is None else int(m)
    N = w.shape[0]
    if w.shape[1] != K or (bias is not None and bias.numel() != N):
        raise RuntimeError("gemm_nt_bf16: inconsistent shapes")
    if a_group_rows > 0 and M > 0:
        # A row r lives at a + (r // a_group_rows) * a_group_stride + (r % a_group_rows) * lda: it must stay in a's storage
        def row(r):
            return r // a_group_rows * a_group_stride + r % a_group_rows * a.stride(0)
        last = max(row(r) for r in (M - 1, (M - 1) // a_group_rows * a_group_rows - 1) if r >= 0) + K
        if a_group_stride < 0 or a.storage_offset() + last > a.untyped_storage().nbytes() // a.element_size():
            raise RuntimeError("gemm_nt_bf16: row groups reach past the storage of a")
    elif m is not None and m != a.shape[0]:
        raise RuntimeError("gemm_nt_bf16: m= is for row-group addressing")
    if out is None:
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("gemm_nt_bf16: out_dtype must be float32 or bfloat16")
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    else:
        if out.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("gemm_nt_bf16: out must be float32 or bfloat16")
        _need_rows(out, out.dtype, "out")
        if tuple(out.shape) != (M, N):
            raise RuntimeError(f"gemm_nt_bf16: out must be [{M}, {N}], got {tuple(out.shape)}")
    fields = (_ptr(a), a.stride(0), int(a_group_rows), int(a_group_stride), _ptr(w), w.stride(0), _ptr(bias), int(relu),
              _ptr(out), out.stride(0), int(out.dtype == torch.bfloat16), M, N, K)
    return fields, out


def gemm_nt_bf16(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False,
                 out_dtype: torch.dtype = torch.float32, tile256: bool = False, *, out: Optional[torch.Tensor] = None,
                 a_group_rows: int = 0, a_group_stride: int = 0, m: Optional[int] = None) -> torch.Tensor:
    """act(a @ w.T + bias): a [M,K] bf16, w [N,K] bf16 -> [M,N] f32 or bf16 (MFMA, f32 accumulate).

    a / w may have padded rows (their stride(0) is passed as lda / ldw).  out: an [M,N] f32 / bf16 matrix to write into,
    e.g. a row or column slice of a wider buffer (its stride(0) is ldc; its dtype overrides out_dtype).  With
    a_group_rows > 0, row r of A lives at a + (r // a_group_rows) * a_group_stride + (r % a_group_rows) * a.stride(0)
    (elements) and m gives the row count M (default a.shape[0])."""
    fields, out = _gemm_fields(a, w, bias, relu, out_dtype, out, a_group_rows, a_group_stride, m)
    _call("vpr_gemm256_nt_bf16" if tile256 else "vpr_gemm_nt_bf16", *fields, _stream())
    return out


def gemm_nt_group_bf16(problems) -> list:
    """1 to 3 GEMMs in ONE launch of the grouped kernel (vpr_gemm_nt_group_bf16).  problems: dicts with the arguments
    of gemm_nt_bf16 (keys a, w, and optionally bias, relu, out_dtype, out, a_group_rows, a_group_stride, m).
    Returns the outputs in order."""
    problems = list(problems)
    arr = (_lib.GemmProblemC * max(1, len(problems)))()
    outs = []
    for i, p in enumerate(problems):
        fields, out = _gemm_fields(p["a"], p["w"], p.get("bias"), p.get("relu", False), p.get("out_dtype", torch.float32),
                                   p.get("out"), p.get("a_group_rows", 0), p.get("a_group_stride", 0), p.get("m"))
        arr[i] = _lib.GemmProblemC(*[f.value if isinstance(f, ctypes.c_void_p) else f for f in fields])
        outs.append(out)
    _call("vpr_gemm_nt_group_bf16", arr, len(problems), _stream())
    return outs


# -------------------------------------------------------------------------------------------- kNN
def knn_workspace(B: int, N: int, D: int, k: int, device: torch.device) -> torch.Tensor:
    nbytes = _lib.lib().vpr_knn_workspace_bytes(B, N, D, k)
    if nbytes == 0:
        raise RuntimeError(f"vpr_knn: unsupported shape B={B} N={N} D={D} k={k} (need D % 64 == 0, 1 <= k <= 64)")
    return workspace("knn", nbytes, device)


NORM_BOUND_BF16 = 1.002     # L2-normalised rows rounded to bf16 (the unchecked C entry points assume the same)
NORM_BOUND_FP8 = 1.0625     # ... quantised to e4m3 with a per-row scale


def _check_args(B: int, device, status: Optional[torch.Tensor], uncertified: Optional[torch.Tensor]) -> None:
    if status is not None:
        _need(status, torch.int32, "status", 1)
        if status.numel() != B:
            raise RuntimeError("status: one int32 per query")
    if uncertified is not None:
        _need(uncertified, torch.int32, "uncertified", 1)


def knn_topk(q: torch.Tensor, gallery: torch.Tensor, k: int, index_base: int = 0,
             ws: Optional[torch.Tensor] = None, *, norm_bound: float = NORM_BOUND_BF16,
             status: Optional[torch.Tensor] = None, uncertified: Optional[torch.Tensor] = None,
             exact_fallback: bool = False, score_events: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B,D] bf16, gallery [N,D] bf16 -> (scores f32 [B,k] descending, indices int32 [B,k]).
    score_events: a list -> the call runs as its two stages (vpr_knn_topk_scores_stage / _select_stage: same kernels,
    same result) and appends a (start, end) pair of timing events around the score stage.
    The kernels certify each query's answer as the exact top-k (include/vpr_amd.h, "Checked forms"):
    `status` (int32 [B]) receives 0 / 1 (certified) or 2 (not certified), `uncertified` (int32 [1]) counts the 2s
    without a host sync; `norm_bound` = upper bound of the gallery row norms.  exact_fallback=True reads the status
    back (one sync) and re-runs the flagged queries exhaustively, so the result is exact unconditionally — for rows of
    at most 17408 bytes (D <= 8704 bf16, 17408 e4m3), the exhaustive kernel's limit.  Wider rows: if the checked search
    flags a query, the call raises the exhaustive entry point's error (VPR_ERR_UNSUPPORTED) after the search has run;
    a caller's `status` then still reads 2 for the flagged queries (never 3) and 0 / 1 for the others, whose rows a
    call without exact_fallback returns exact; with no query flagged the call succeeds at any width.
    e4m3 scales must be finite and > 0 (include/vpr_amd.h)."""
    _need(q, torch.bfloat16, "q", 2)
    _need(gallery, torch.bfloat16, "gallery", 2)
    if gallery.shape[1] != q.shape[1]:
        raise RuntimeError("knn_topk: q and gallery disagree on D")
    return _knn_topk(q, None, gallery, None, k, index_base, ws, norm_bound, status, uncertified, exact_fallback, score_events)


def _knn_topk(q, q_scale, gallery, gallery_scale, k, index_base, ws, norm_bound, status, uncertified, exact_fallback,
              score_events) -> Tuple[torch.Tensor, torch.Tensor]:
    """The body of knn_topk (scales None: vpr_knn_topk_checked) and knn_topk_fp8 (vpr_knn_topk_fp8_checked) on checked
    operands."""
    B, D = q.shape
    N = gallery.shape[0]
    if ws is None:
        ws = knn_workspace(B, N, D, k, q.device)
    if exact_fallback and status is None:
        status = torch.empty((B,), dtype=torch.int32, device=q.device)
    _check_args(B, q.device, status, uncertified)
    vals = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=q.device)
    if score_events is not None:
        _topk_two_stage(q, q_scale, gallery, gallery_scale, B, N, D, k, index_base, vals, idx, ws, norm_bound, status,
                        uncertified, score_events)
    else:
        if q_scale is None:
            name, operands = "vpr_knn_topk_checked", (_ptr(q), _ptr(gallery))
        else:
            name, operands = "vpr_knn_topk_fp8_checked", (_ptr(q), _ptr(q_scale), _ptr(gallery), _ptr(gallery_scale))
        _call(name, *operands, B, N, D, int(k), int(index_base), _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(),
              float(norm_bound), _ptr(status), _ptr(uncertified), _stream())
    if exact_fallback:
        _exhaustive_fixup(q, q_scale, gallery, gallery_scale, k, index_base, status, vals, idx)
    return vals, idx


def _topk_two_stage(q, q_scale, gallery, gallery_scale, B, N, D, k, index_base, vals, idx, ws, norm_bound, status,
                    uncertified, score_events) -> None:
    fp8 = q_scale is not None
    args = (_ptr(q), _ptr(q_scale) if fp8 else None, _ptr(gallery), _ptr(gallery_scale) if fp8 else None, int(fp8),
            B, N, D, int(k))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _call("vpr_knn_topk_scores_stage", *args, _ptr(ws), ws.numel(), _stream())
    e1.record()
    score_events.append((e0, e1))
    _call("vpr_knn_topk_select_stage", *args, int(index_base), _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(),
          float(norm_bound), _ptr(status), _ptr(uncertified), _stream())


def knn_topk_exhaustive(q: torch.Tensor, gallery: torch.Tensor, k: int, index_base: int = 0,
                        q_scale: Optional[torch.Tensor] = None, gallery_scale: Optional[torch.Tensor] = None,
                        ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every score computed exactly (f64), then the same selection: exact by construction, slow (fallback for the
    queries the certification flags).  bf16 operands, or uint8 e4m3 operands with both per-row scales."""
    fp8 = q.dtype == torch.uint8
    _need(q, torch.uint8 if fp8 else torch.bfloat16, "q", 2)
    _need(gallery, q.dtype, "gallery", 2)
    if fp8:
        _need(q_scale, torch.float32, "q_scale", 1)
        _need(gallery_scale, torch.float32, "gallery_scale", 1)
    B, D = q.shape
    N = gallery.shape[0]
    if gallery.shape[1] != D:
        raise RuntimeError("knn_topk_exhaustive: q and gallery disagree on D")
    if ws is None:
        ws = knn_workspace(B, N, D, k, q.device)
    vals = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=q.device)
    _call("vpr_knn_topk_exhaustive", _ptr(q), _ptr(q_scale) if fp8 else None, _ptr(gallery),
          _ptr(gallery_scale) if fp8 else None, int(fp8), B, N, D, int(k),
          int(index_base), _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(), _stream())
    return vals, idx


def _exhaustive_fixup(q, q_scale, gallery, gallery_scale, k, index_base, status, vals, idx) -> int:
    """Host side of exact_fallback: one D2H read of `status`, exhaustive re-run of the queries marked 2."""
    bad = torch.nonzero(status == 2).flatten()           # syncs
    if bad.numel() == 0:
        return 0
    qb = q[bad].contiguous()
    v2, i2 = knn_topk_exhaustive(qb, gallery, k, index_base, q_scale[bad].contiguous() if q_scale is not None else None,
                                 gallery_scale)
    vals[bad], idx[bad] = v2, i2
    status[bad] = 3                                       # 3 = exact through the exhaustive path
    return int(bad.numel())


def quantize_fp8_rows(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [rows, D] f32 -> (e4m3 bytes [rows, D] uint8, per-row scale [rows] f32); value = scale * fp8."""
    _need(x, torch.float32, "x", 2)
    rows, D = x.shape
    q = torch.empty((rows, D), dtype=torch.uint8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _call("vpr_quantize_fp8_rows", _ptr(x), rows, D, _ptr(q), _ptr(scale), _stream())
    return q, scale


def knn_topk_fp8(q: torch.Tensor, q_scale: torch.Tensor, gallery: torch.Tensor, gallery_scale: torch.Tensor,
                 k: int, index_base: int = 0, ws: Optional[torch.Tensor] = None, *, norm_bound: float = NORM_BOUND_FP8,
                 status: Optional[torch.Tensor] = None, uncertified: Optional[torch.Tensor] = None,
                 exact_fallback: bool = False, score_events: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp8 (e4m3 bytes + per-row f32 scale) variant of knn_topk; D % 128 == 0.  norm_bound bounds the norms of the
    DEQUANTISED gallery rows."""
    _need(q, torch.uint8, "q", 2)
    _need(gallery, torch.uint8, "gallery", 2)
    _need(q_scale, torch.float32, "q_scale", 1)
    _need(gallery_scale, torch.float32, "gallery_scale", 1)
    if gallery.shape[1] != q.shape[1] or q_scale.numel() != q.shape[0] or gallery_scale.numel() != gallery.shape[0]:
        raise RuntimeError("knn_topk_fp8: inconsistent shapes")
    return _knn_topk(q, q_scale, gallery, gallery_scale, k, index_base, ws, norm_bound, status, uncertified, exact_fallback,
                     score_events)


def knn_scores(q: torch.Tensor, gallery: torch.Tensor, ws: torch.Tensor) -> None:
    """Stage 1 only (the HBM-bound score kernel); results stay in `ws`."""
    _need(q, torch.bfloat16, "q", 2)
    _need(gallery, torch.bfloat16, "gallery", 2)
    B, D = q.shape
    _call("vpr_knn_scores", _ptr(q), _ptr(gallery), B, gallery.shape[0], D, _ptr(ws), ws.numel(), _stream())


def knn_select(q: torch.Tensor, gallery: torch.Tensor, k: int, ws: torch.Tensor,
               index_base: int = 0, *, norm_bound: float = NORM_BOUND_BF16, status: Optional[torch.Tensor] = None,
               uncertified: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stage 2+3 (candidate selection, exact rescoring, ordering, certification) on scores already in `ws`."""
    B, D = q.shape
    _check_args(B, q.device, status, uncertified)
    vals = torch.empty((B, k), dtype=torch.float32, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=q.device)
    _call("vpr_knn_select_checked", _ptr(q), _ptr(gallery), B, gallery.shape[0], D, int(k), int(index_base),
          _ptr(vals), _ptr(idx), _ptr(ws), ws.numel(), float(norm_bound), _ptr(status), _ptr(uncertified), _stream())
    return vals, idx


def knn_scores_view(ws: torch.Tensor, B: int, N: int, D: int, k: int) -> torch.Tensor:
    """View of the score matrix S[B, N] inside a kNN workspace (tests)."""
    ld = ctypes.c_int(0)
    p = _lib.lib().vpr_knn_scores_ptr(_ptr(ws), B, N, D, k, ctypes.byref(ld))
    if not p:
        raise RuntimeError("vpr_knn_scores_ptr: unsupported shape")
    off = p - ws.data_ptr()
    flat = ws[off: off + B * ld.value * 4].view(torch.float32)
    return flat.view(B, ld.value)[:, :N]


def topk_merge(vals: torch.Tensor, idxs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """vals/idxs [shards, B, k] (per-shard top-k with global indices) -> merged [B, k]."""
    _need(vals, torch.float32, "vals", 3)
    _need(idxs, torch.int32, "idxs", 3)
    if vals.shape != idxs.shape:
        raise RuntimeError("topk_merge: vals and idxs shapes differ")
    R, B, k = vals.shape
    ov = torch.empty((B, k), dtype=torch.float32, device=vals.device)
    oi = torch.empty((B, k), dtype=torch.int32, device=vals.device)
    _call("vpr_topk_merge", _ptr(vals), _ptr(idxs), R, B, k, _ptr(ov), _ptr(oi), _stream())
    return ov, oi


_POSE_MODES = {"top1": _lib.POSE_TOP1, "weighted": _lib.POSE_WEIGHTED}


def retrieval_pose(vals: torch.Tensor, idx: torch.Tensor, labels_dev: torch.Tensor, mode: str = "top1",
                   temperature: float = 0.01, q_targets: Optional[torch.Tensor] = None, tau: float = 0.0,
                   scaler=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Geopose and first-hit ranks of the merged top-k, on the device (include/vpr_amd_retrieval.h).
    vals f32 / idx int32 [B, k] (k <= 64), labels_dev f64 [N, 4] = (lat, lon, angle_deg, Region_ID) (gallery.device_labels),
    q_targets f64 [B, 3] = each query's (lat, lon, Region_ID) or None, scaler = four host numbers (mean_lat, mean_lon,
    scale_lat, scale_lon) or None.  Returns (pose64 f64 [B, 3] = lat, lon, angle_deg; pose4 f32 [B, 4] = standardised
    lat / lon, sin, cos; hit_tau int32 [B]; hit_region int32 [B]); the hits are -1 without q_targets."""
    _need(vals, torch.float32, "vals", 2)
    _need(idx, torch.int32, "idx", 2)
    _need(labels_dev, torch.float64, "labels_dev", 2)
    if vals.shape != idx.shape:
        raise RuntimeError("retrieval_pose: vals and idx shapes differ")
    if labels_dev.shape[1] != 4:
        raise RuntimeError("retrieval_pose: labels_dev must be [N, 4] = (lat, lon, angle_deg, Region_ID)")
    if mode not in _POSE_MODES:
        raise RuntimeError("retrieval_pose: mode must be 'top1' or 'weighted'")
    B, k = vals.shape
    if q_targets is not None:
        _need(q_targets, torch.float64, "q_targets", 2)
        if q_targets.shape != (B, 3):
            raise RuntimeError("retrieval_pose: q_targets must be [B, 3] = (lat, lon, Region_ID)")
    sc = None
    if scaler is not None:
        scaler = [float(x) for x in scaler]
        if len(scaler) != 4:
            raise RuntimeError("retrieval_pose: scaler must be (mean_lat, mean_lon, scale_lat, scale_lon)")
        sc = (ctypes.c_double * 4)(*scaler)                           # read during the call: a temporary is enough
    dev = vals.device
    pose64 = torch.empty((B, 3), dtype=torch.float64, device=dev)
    pose4 = torch.empty((B, 4), dtype=torch.float32, device=dev)
    hit_tau = torch.empty((B,), dtype=torch.int32, device=dev)
    hit_region = torch.empty((B,), dtype=torch.int32, device=dev)
    _call("vpr_retrieval_pose", _ptr(vals), _ptr(idx), B, k, _ptr(labels_dev), labels_dev.shape[0], _POSE_MODES[mode],
          float(temperature), _ptr(q_targets), float(tau), sc, _ptr(pose64), _ptr(pose4), _ptr(hit_tau), _ptr(hit_region),
          _stream())
    return pose64, pose4, hit_tau, hit_region


def _expand_check(what: str, q, vals, idx, n_use: int, alpha: float, q_weight: float) -> None:
    _need(q, torch.bfloat16, "q", 2)
    _need(vals, torch.float32, "vals", 2)
    _need(idx, torch.int32, "idx", 2)
    if vals.shape != idx.shape:
        raise RuntimeError(f"{what}: vals and idx shapes differ")
    if vals.shape[0] != q.shape[0]:
        raise RuntimeError(f"{what}: q and vals disagree on B")
    if not 1 <= int(n_use) <= vals.shape[1]:
        raise RuntimeError(f"{what}: n_use must be in 1..k (k = {vals.shape[1]})")
    if not alpha >= 0.0 or not q_weight >= 0.0:
        raise RuntimeError(f"{what}: alpha and q_weight must be >= 0")


def query_expand(q: torch.Tensor, vals: torch.Tensor, idx: torch.Tensor, rows: torch.Tensor,
                 scales: Optional[torch.Tensor] = None, index_base: int = 0, n_use: Optional[int] = None, alpha: float = 3.0,
                 q_weight: float = 1.0, add_query: bool = True, *, finish: bool = False,
                 partial: Optional[torch.Tensor] = None):
    """One shard's contribution to the expanded queries (include/vpr_amd_expand.h): q bf16 [B, D], vals f32 / idx int32 [B, k]
    (k <= 128) from a search, rows = the shard, bf16 [n_local, D] or uint8 e4m3 bytes with per-row f32 `scales`, owning global
    rows index_base ...  Returns partial f32 [B, D] = add_query * q_weight * q + sum over the local neighbours j < n_use of
    vals^alpha * row (n_use None: all k).
    finish=True (a gallery of one shard): the same call normalises; returns (out_f32 [B, D] unit rows, out_bf16 [B, D]).
    partial: the f32 [B, D] buffer to write; None: with finish=True a cached scratch buffer of the current stream (pinned
    while a graph is captured, like every workspace), else a new tensor."""
    n_use = vals.shape[1] if n_use is None and isinstance(vals, torch.Tensor) and vals.dim() == 2 else n_use
    _expand_check("query_expand", q, vals, idx, n_use, alpha, q_weight)
    fp8 = isinstance(rows, torch.Tensor) and rows.dtype == torch.uint8
    _need(rows, torch.uint8 if fp8 else torch.bfloat16, "rows", 2)
    if fp8 != (scales is not None):
        raise RuntimeError("query_expand: uint8 (e4m3) rows come with per-row scales, bf16 rows without")
    if fp8:
        _need(scales, torch.float32, "scales", 1)
        if scales.numel() != rows.shape[0]:
            raise RuntimeError("query_expand: scales: one per row")
    B, D = q.shape
    if rows.shape[1] != D:
        raise RuntimeError("query_expand: q and rows disagree on D")
    dev = q.device
    if partial is None:
        partial = (workspace("query_expand", B * D * 4, dev)[:B * D * 4].view(torch.float32).view(B, D) if finish
                   else torch.empty((B, D), dtype=torch.float32, device=dev))
    else:
        _need(partial, torch.float32, "partial", 2)
        if partial.shape != (B, D):
            raise RuntimeError("query_expand: partial must be [B, D]")
    out_f32 = torch.empty((B, D), dtype=torch.float32, device=dev) if finish else None
    out_bf16 = torch.empty((B, D), dtype=torch.bfloat16, device=dev) if finish else None
    _call("vpr_query_expand", _ptr(q), _ptr(vals), _ptr(idx), B, D, vals.shape[1], _ptr(rows), _ptr(scales), rows.shape[0],
          int(index_base), int(n_use), float(alpha), float(q_weight), int(bool(add_query)), _ptr(partial), _ptr(out_f32),
          _ptr(out_bf16), _stream())
    return (out_f32, out_bf16) if finish else partial


def query_expand_finish(partials: torch.Tensor, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Shard partials f32 [R, B, D] (R <= 64, summed in shard order) + the searched queries q bf16 [B, D] -> (out_f32 [B, D]
    unit rows, out_bf16 [B, D] = its bf16 rounding); a query whose sum is zero or not finite comes back as q."""
    _need(partials, torch.float32, "partials", 3)
    _need(q, torch.bfloat16, "q", 2)
    R, B, D = partials.shape
    if q.shape != (B, D):
        raise RuntimeError("query_expand_finish: partials [R, B, D] and q [B, D] disagree")
    out_f32 = torch.empty((B, D), dtype=torch.float32, device=q.device)
    out_bf16 = torch.empty((B, D), dtype=torch.bfloat16, device=q.device)
    _call("vpr_query_expand_finish", _ptr(partials), R, _ptr(q), B, D, _ptr(out_f32), _ptr(out_bf16), _stream())
    return out_f32, out_bf16


def _rerank_check(what: str, q, idx, rows, k) -> int:
    for t, name in ((q, "q"), (rows, "rows")):                  # bf16, or f32 taken as it is
        _need(t, torch.float32 if isinstance(t, torch.Tensor) and t.dtype == torch.float32 else torch.bfloat16, name, 2)
    _need(idx, torch.int32, "idx", 2)
    if idx.shape[0] != q.shape[0]:
        raise RuntimeError(f"{what}: q and idx disagree on B")
    if rows.shape[1] != q.shape[1]:
        raise RuntimeError(f"{what}: q and rows disagree on D")
    if idx.device != q.device or rows.device != q.device:
        raise RuntimeError(f"{what}: q, idx and rows must live on one device")
    kc = idx.shape[1]
    if not 1 <= kc <= _lib.RERANK_MAX_KC:
        raise RuntimeError(f"{what}: idx must hold 1..{_lib.RERANK_MAX_KC} candidates per query, got {kc}")
    k = kc if k is None else int(k)
    if not 1 <= k <= kc:
        raise RuntimeError(f"{what}: k must be in 1..kc (kc = {kc})")
    return k


def rerank_rows(q: torch.Tensor, idx: torch.Tensor, rows: torch.Tensor, index_base: int = 0, k: Optional[int] = None,
                ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Two-tier retrieval (include/vpr_amd_rerank.h): q [B, D] bf16 or f32, idx int32 [B, kc] (kc <= 128) the candidates of a
    coarse search as global rows, rows = this shard's FINE rows [n_local, D] bf16 or f32, owning global rows index_base ...
    Returns (vals f32 [B, k], idx int32 [B, k]): the k best (None: all kc) of the candidates this shard owns by the f32 dot
    product with their fine row, (score desc, index asc); everything else — the -1 padding, rows of other shards — is never
    dereferenced and comes back as (-inf, -1) at the tail.  The output is a list vpr_topk_merge / retrieval_pose take.
    ws: a byte buffer of vpr_rerank_workspace_bytes(B, kc); None: the current stream's cached one (pinned while a graph is
    captured, like every workspace)."""
    k = _rerank_check("rerank_rows", q, idx, rows, k)
    B, D = q.shape
    kc = idx.shape[1]
    dev = q.device
    need = _lib.lib().vpr_rerank_workspace_bytes(B, kc)
    if ws is None:
        ws = workspace("rerank_rows", need, dev)
    else:
        _need(ws, torch.uint8, "ws", 1)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    out = torch.empty((B, k), dtype=torch.int32, device=dev)
    if B == 0:
        return vals, out
    _call("vpr_rerank_rows", _ptr(q), int(q.dtype == torch.float32), _ptr(idx), B, D, kc, _ptr(rows),
          int(rows.dtype == torch.float32), rows.shape[0], int(index_base), k, _ptr(vals), _ptr(out), _ptr(ws), ws.numel(),
          _stream())
    return vals, out


def _local_check(what: str, q_local, idx, g_local, k, dtype=torch.bfloat16, l_step: int = 32, max_n: int = _lib.LOCAL_MAX_N) -> int:
    """The argument checks of both element types: bf16 features of a width that is a multiple of 32, e4m3 bytes of 64; max_n
    = the patch limit of the form (256, or 1369 for the _hires calls)."""
    for t, name in ((q_local, "q_local"), (g_local, "g_local")):
        _need(t, dtype, name, 3)
    _need(idx, torch.int32, "idx", 2)
    if idx.shape[0] != q_local.shape[0]:
        raise RuntimeError(f"{what}: q_local and idx disagree on B")
    if g_local.shape[2] != q_local.shape[2]:
        raise RuntimeError(f"{what}: q_local and g_local disagree on l")
    if idx.device != q_local.device or g_local.device != q_local.device:
        raise RuntimeError(f"{what}: q_local, idx and g_local must live on one device")
    for t, name in ((q_local, "q_local"), (g_local, "g_local")):
        if not 1 <= t.shape[1] <= max_n:
            raise RuntimeError(f"{what}: {name} must hold 1..{max_n} patches per image, got {t.shape[1]}")
    l = q_local.shape[2]
    if l % l_step or not l_step <= l <= _lib.LOCAL_MAX_L:
        raise RuntimeError(f"{what}: the feature width must be a multiple of {l_step} in {l_step}..{_lib.LOCAL_MAX_L}, got {l}")
    kc = idx.shape[1]
    if not 1 <= kc <= _lib.LOCAL_MAX_KC:
        raise RuntimeError(f"{what}: idx must hold 1..{_lib.LOCAL_MAX_KC} candidates per query, got {kc}")
    k = kc if k is None else int(k)
    if not 1 <= k <= kc:
        raise RuntimeError(f"{what}: k must be in 1..kc (kc = {kc})")
    return k


class LocalRerankDebug(NamedTuple):
    """The optional outputs of vpr_local_rerank, candidate order: pair_score f32 / pair_matches int32 [B, kc] ((-inf, 0) for a
    candidate the shard does not own), row_nn int32 [B, kc, n_q] / col_nn int32 [B, kc, n_g] (-1: none, or not owned)."""
    pair_score: torch.Tensor
    pair_matches: torch.Tensor
    row_nn: torch.Tensor
    col_nn: torch.Tensor


def _local_rerank_call(what: str, entry: str, ws_entry: str, dtype, l_step: int, q_local, idx, g_local, index_base, k, min_sim,
                       ws, debug, max_n: int = _lib.LOCAL_MAX_N):
    """local_rerank / local_rerank_fp8 and their _hires forms: the checks, the workspace, the outputs and the one library call."""
    k = _local_check(what, q_local, idx, g_local, k, dtype, l_step, max_n)
    min_sim = float(min_sim)
    if min_sim != min_sim:
        raise RuntimeError(f"{what}: min_sim must be a number")
    B, n_q, l = q_local.shape
    n_local, n_g = g_local.shape[:2]
    kc = idx.shape[1]
    dev = q_local.device
    need = getattr(_lib.lib(), ws_entry)(B, kc)
    if ws is None:
        ws = workspace(what, need, dev)
    else:
        _need(ws, torch.uint8, "ws", 1)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    out = torch.empty((B, k), dtype=torch.int32, device=dev)
    matches = torch.empty((B, k), dtype=torch.int32, device=dev)
    dbg = None
    if debug:
        dbg = LocalRerankDebug(torch.empty((B, kc), dtype=torch.float32, device=dev), torch.empty((B, kc), dtype=torch.int32, device=dev),
                               torch.empty((B, kc, n_q), dtype=torch.int32, device=dev),
                               torch.empty((B, kc, n_g), dtype=torch.int32, device=dev))
    if B:
        _call(entry, _ptr(q_local), n_q, _ptr(idx), B, kc, _ptr(g_local), n_g, l, n_local, int(index_base), min_sim,
              k, _ptr(vals), _ptr(out), _ptr(matches), *[_ptr(t) for t in (dbg or (None,) * 4)], _ptr(ws), ws.numel(), _stream())
    return (vals, out, matches, dbg) if debug else (vals, out, matches)


def local_rerank(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, index_base: int = 0, k: Optional[int] = None,
                 min_sim: float = 0.0, ws: Optional[torch.Tensor] = None, debug: bool = False):
    """Local-feature re-ranking (include/vpr_amd_local.h): q_local bf16 [B, n_q, l], idx int32 [B, kc] (kc <= 128) the candidates
    of a search as global rows, g_local = this shard's local features bf16 [n_local, n_g, l], owning global rows index_base ...
    Returns (vals f32 [B, k], idx int32 [B, k], matches int32 [B, k]): the k best (None: all kc) of the candidates this shard
    owns by the sum of the similarities of their mutual-nearest-neighbour patch pairs of similarity >= min_sim, (score desc,
    index asc); everything else is never dereferenced and comes back as (-inf, -1, 0) at the tail.  debug=True: a fourth
    element, LocalRerankDebug.  ws: a byte buffer of vpr_local_workspace_bytes(B, kc); None: the current stream's cached one."""
    return _local_rerank_call("local_rerank", "vpr_local_rerank", "vpr_local_workspace_bytes", torch.bfloat16, 32, q_local, idx,
                              g_local, index_base, k, min_sim, ws, debug)


def quantize_patch_fp8(x: torch.Tensor) -> torch.Tensor:
    """Patch features to their e4m3 store (include/vpr_amd_patch_fp8.h): x f32 or bf16 of any shape -> uint8 of that shape, the
    OCP e4m3fn byte of x * 2^8 per element, one round-to-nearest-even from the f32 value; beyond +-448 / 256 saturates, NaN and
    +-Inf become the NaN byte 0x7F."""
    if isinstance(x, torch.Tensor) and x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"x: expected dtype torch.float32 or torch.bfloat16, got {x.dtype}")
    _need(x, x.dtype if isinstance(x, torch.Tensor) else torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        _call("vpr_patch_quantize_fp8", _ptr(x), int(x.dtype == torch.bfloat16), x.numel(), _ptr(out), _stream())
    return out


def local_rerank_fp8(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, index_base: int = 0,
                     k: Optional[int] = None, min_sim: float = 0.0, ws: Optional[torch.Tensor] = None, debug: bool = False):
    """local_rerank on e4m3 patch features (include/vpr_amd_patch_fp8.h): q_local uint8 [B, n_q, l] and g_local uint8
    [n_local, n_g, l] as quantize_patch_fp8 writes them, l a multiple of 64; the similarity is 2^-16 times the dot product of
    the byte values, everything else — arguments, outputs, debug=, ws — is local_rerank's."""
    return _local_rerank_call("local_rerank_fp8", "vpr_patch_rerank_fp8", "vpr_patch_workspace_bytes_fp8", torch.uint8,
                              _lib.PATCH_FP8_MIN_L, q_local, idx, g_local, index_base, k, min_sim, ws, debug)


def local_rerank_hires(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, index_base: int = 0,
                       k: Optional[int] = None, min_sim: float = 0.0, ws: Optional[torch.Tensor] = None, debug: bool = False):
    """local_rerank for 1..1369 patches on either side (include/vpr_amd_local_hires.h; 322 to 518 px images): arguments,
    outputs, debug= and ws= are local_rerank's.  The score of more than 256 candidate patches is summed in blocks of 256
    columns; at 256 patches and below every output equals local_rerank's bit for bit."""
    return _local_rerank_call("local_rerank_hires", "vpr_hires_local_rerank", "vpr_hires_local_workspace_bytes", torch.bfloat16, 32,
                              q_local, idx, g_local, index_base, k, min_sim, ws, debug, _lib.LOCAL_HIRES_MAX_N)


def local_rerank_fp8_hires(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, index_base: int = 0,
                           k: Optional[int] = None, min_sim: float = 0.0, ws: Optional[torch.Tensor] = None, debug: bool = False):
    """local_rerank_fp8 for 1..1369 patches on either side (include/vpr_amd_local_hires.h): everything else is
    local_rerank_fp8's; at 256 patches and below every output equals it bit for bit."""
    return _local_rerank_call("local_rerank_fp8_hires", "vpr_hires_patch_rerank_fp8", "vpr_hires_local_workspace_bytes", torch.uint8,
                              _lib.PATCH_FP8_MIN_L, q_local, idx, g_local, index_base, k, min_sim, ws, debug, _lib.LOCAL_HIRES_MAX_N)


# ---- spatial verification of the patch matches (include/vpr_amd_spatial.h) ----
def _spatial_grid_check(what: str, n_q: int, gw_q, n_g: int, gw_g, tol) -> Tuple[int, int, int]:
    """The grid rules of include/vpr_amd_spatial.h: each gw divides its n, 0 <= tol <= 8, at most 5329 shift bins."""
    gw_q, gw_g, tol = int(gw_q), int(gw_g), int(tol)
    for n, gw, name in ((n_q, gw_q, "gw_q"), (n_g, gw_g, "gw_g")):
        if not 1 <= gw <= n or n % gw:
            raise RuntimeError(f"{what}: {name} must be a grid width in 1..{n} that divides the {n} patches of an image, got {gw}")
    if not 0 <= tol <= _lib.SPATIAL_MAX_TOL:
        raise RuntimeError(f"{what}: tol must be in 0..{_lib.SPATIAL_MAX_TOL}, got {tol}")
    bins = (gw_q + gw_g - 1) * (n_q // gw_q + n_g // gw_g - 1)
    if bins > _lib.SPATIAL_MAX_BINS:
        raise RuntimeError(f"{what}: the two grids span {bins} shift bins, more than {_lib.SPATIAL_MAX_BINS}")
    return gw_q, gw_g, tol


class SpatialVerify(NamedTuple):
    """The outputs of vpr_spatial_verify per pair: score f32 [P], inliers / matches int32 [P], shift int32 [P, 2] = (dx, dy) of
    the dominant bin ((INT32_MIN, INT32_MIN) without a match), inlier_mask uint8 [P, n_g] or None."""
    score: torch.Tensor
    inliers: torch.Tensor
    matches: torch.Tensor
    shift: torch.Tensor
    inlier_mask: Optional[torch.Tensor]


def spatial_verify(partner: torch.Tensor, sim: torch.Tensor, n_q: int, gw_q: int, gw_g: int, tol: int = 1,
                   want_mask: bool = False) -> SpatialVerify:
    """The verification stage on its own (include/vpr_amd_spatial.h): partner int32 [P, n_g] (the query patch matched to
    candidate column j; anything outside 0..n_q-1 is no match) and sim f32 [P, n_g]; the query grid is gw_q wide with n_q
    patches, the candidate's gw_g wide.  Matches vote for their shift, the dominant shift's (2 tol + 1)^2 window decides the
    inliers, the score is the f32 sum of their similarities in the order of include/vpr_amd_local_hires.h."""
    _need(partner, torch.int32, "partner", 2)
    _need(sim, torch.float32, "sim", 2)
    if partner.shape != sim.shape or partner.device != sim.device:
        raise RuntimeError("spatial_verify: partner and sim must have one shape and live on one device")
    P, n_g = partner.shape
    n_q = int(n_q)
    for n, name in ((n_q, "n_q"), (n_g, "n_g")):
        if not 1 <= n <= _lib.LOCAL_HIRES_MAX_N:
            raise RuntimeError(f"spatial_verify: {name} must be in 1..{_lib.LOCAL_HIRES_MAX_N}, got {n}")
    gw_q, gw_g, tol = _spatial_grid_check("spatial_verify", n_q, gw_q, n_g, gw_g, tol)
    dev = partner.device
    out = SpatialVerify(torch.empty(P, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                        torch.empty(P, dtype=torch.int32, device=dev), torch.empty((P, 2), dtype=torch.int32, device=dev),
                        torch.empty((P, n_g), dtype=torch.uint8, device=dev) if want_mask else None)
    if P:
        _call("vpr_spatial_verify", _ptr(partner), _ptr(sim), P, n_q, gw_q, n_g, gw_g, tol, *[_ptr(t) for t in out], _stream())
    return out


class SpatialRerankDebug(NamedTuple):
    """The optional outputs of vpr_spatial_local_rerank, candidate order: pair_score f32 / pair_inliers / pair_matches int32
    [B, kc], pair_shift int32 [B, kc, 2] ((-inf, 0, 0, (INT32_MIN, INT32_MIN)) for a candidate the shard does not own), row_nn
    int32 [B, kc, n_q] / col_nn int32 [B, kc, n_g] (-1: none, or not owned)."""
    pair_score: torch.Tensor
    pair_inliers: torch.Tensor
    pair_matches: torch.Tensor
    pair_shift: torch.Tensor
    row_nn: torch.Tensor
    col_nn: torch.Tensor


def local_rerank_spatial(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, gw_q: int, gw_g: int, tol: int = 1,
                         index_base: int = 0, k: Optional[int] = None, min_sim: float = 0.0, ws: Optional[torch.Tensor] = None,
                         debug: bool = False):
    """Local re-ranking with spatial verification (include/vpr_amd_spatial.h): local_rerank_hires' arguments, with bf16
    features or the uint8 e4m3 store of quantize_patch_fp8 (both sides alike), the widths gw_q / gw_g of the two patch grids
    (raster order, as SaladAggregator.local_features emits them: img_size // 14) and the window half-width tol.  Returns (vals
    f32 [B, k], idx int32 [B, k], inliers int32 [B, k]): a candidate's score is the sum over the mutual-NN matches that lie
    within tol bins of the pair's dominant grid shift; inliers is their number.  debug=True: a fourth element,
    SpatialRerankDebug.  ws: a byte buffer of vpr_spatial_workspace_bytes(B, kc, n_g); None: the current stream's cached one."""
    what = "local_rerank_spatial"
    if not isinstance(q_local, torch.Tensor) or q_local.dtype not in (torch.bfloat16, torch.uint8):
        raise RuntimeError(f"{what}: q_local must be bf16 features or their uint8 e4m3 store")
    fp8 = q_local.dtype == torch.uint8
    k = _local_check(what, q_local, idx, g_local, k, q_local.dtype, _lib.PATCH_FP8_MIN_L if fp8 else 32, _lib.LOCAL_HIRES_MAX_N)
    min_sim = float(min_sim)
    if min_sim != min_sim:
        raise RuntimeError(f"{what}: min_sim must be a number")
    B, n_q, l = q_local.shape
    n_local, n_g = g_local.shape[:2]
    gw_q, gw_g, tol = _spatial_grid_check(what, n_q, gw_q, n_g, gw_g, tol)
    kc = idx.shape[1]
    dev = q_local.device
    need = _lib.lib().vpr_spatial_workspace_bytes(B, kc, n_g)
    if ws is None:
        ws = workspace(what, need, dev)
    else:
        _need(ws, torch.uint8, "ws", 1)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    out = torch.empty((B, k), dtype=torch.int32, device=dev)
    inliers = torch.empty((B, k), dtype=torch.int32, device=dev)
    dbg = None
    if debug:
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        dbg = SpatialRerankDebug(torch.empty((B, kc), dtype=torch.float32, device=dev), i32(B, kc), i32(B, kc), i32(B, kc, 2),
                                 i32(B, kc, n_q), i32(B, kc, n_g))
    if B:
        _call("vpr_spatial_local_rerank", _ptr(q_local), n_q, _ptr(idx), B, kc, _ptr(g_local), n_g, l, n_local, int(index_base),
              min_sim, k, _ptr(vals), _ptr(out), _ptr(inliers), *[_ptr(t) for t in (dbg or (None,) * 6)], int(fp8), gw_q, gw_g, tol,
              _ptr(ws), ws.numel(), _stream())
    return (vals, out, inliers, dbg) if debug else (vals, out, inliers)


# ---- verification under a similarity transform (include/vpr_amd_similarity.h) ----
def _similarity_grid_check(what: str, n_q: int, gw_q, n_g: int, gw_g, tol) -> Tuple[int, int, int]:
    """The grid rules of include/vpr_amd_similarity.h: each gw divides its n, 0 <= tol <= 8, every grid side at most 37."""
    gw_q, gw_g, tol = int(gw_q), int(gw_g), int(tol)
    for n, gw, name in ((n_q, gw_q, "gw_q"), (n_g, gw_g, "gw_g")):
        if not 1 <= gw <= n or n % gw:
            raise RuntimeError(f"{what}: {name} must be a grid width in 1..{n} that divides the {n} patches of an image, got {gw}")
    if not 0 <= tol <= _lib.SIM_MAX_TOL:
        raise RuntimeError(f"{what}: tol must be in 0..{_lib.SIM_MAX_TOL}, got {tol}")
    for n, gw, name in ((n_q, gw_q, "query"), (n_g, gw_g, "candidate")):
        if max(gw, n // gw) > _lib.SIM_MAX_SIDE:
            raise RuntimeError(f"{what}: the {name} grid is {gw} x {n // gw}; a grid side is at most {_lib.SIM_MAX_SIDE}")
    return gw_q, gw_g, tol


class SimilarityVerify(NamedTuple):
    """The outputs of vpr_similarity_verify per pair: score f32 [P], inliers / matches int32 [P], model int32 [P, 6] = (h, the
    column of m_s, the column of m_t, re, im, |dg|^2) of the winning hypothesis (six times INT32_MIN without a model),
    inlier_mask uint8 [P, n_g] or None."""
    score: torch.Tensor
    inliers: torch.Tensor
    matches: torch.Tensor
    model: torch.Tensor
    inlier_mask: Optional[torch.Tensor]


def similarity_model_scale_rotation(model_row) -> Optional[Tuple[float, float]]:
    """A model row (h, column of m_s, column of m_t, re, im, |dg|^2) on the host -> (scale, rotation in degrees) of the
    transform that takes candidate positions to query positions: |re + i im| / |dg|^2 and atan2(im, re).  None for the row of
    a pair without a model (INT32_MIN throughout)."""
    _, _, _, re_, im, n2g = (int(v) for v in model_row)
    if n2g <= 0:
        return None
    return math.hypot(re_, im) / n2g, math.degrees(math.atan2(im, re_))


def similarity_verify(partner: torch.Tensor, sim: torch.Tensor, n_q: int, gw_q: int, gw_g: int, tol: int = 1,
                      want_mask: bool = False) -> SimilarityVerify:
    """The verification stage on its own (include/vpr_amd_similarity.h): partner int32 [P, n_g] (the query patch matched to
    candidate column j; anything outside 0..n_q-1 is no match) and sim f32 [P, n_g]; the query grid is gw_q wide with n_q
    patches, the candidate's gw_g wide.  256 two-match hypotheses of scale (1/2..2), rotation (+-45 degrees) and shift; the
    matches within tol patches of the best one's prediction are the inliers, the score is the f32 sum of their similarities in
    the order of include/vpr_amd_local_hires.h."""
    _need(partner, torch.int32, "partner", 2)
    _need(sim, torch.float32, "sim", 2)
    if partner.shape != sim.shape or partner.device != sim.device:
        raise RuntimeError("similarity_verify: partner and sim must have one shape and live on one device")
    P, n_g = partner.shape
    n_q = int(n_q)
    for n, name in ((n_q, "n_q"), (n_g, "n_g")):
        if not 1 <= n <= _lib.SIM_MAX_N:
            raise RuntimeError(f"similarity_verify: {name} must be in 1..{_lib.SIM_MAX_N}, got {n}")
    gw_q, gw_g, tol = _similarity_grid_check("similarity_verify", n_q, gw_q, n_g, gw_g, tol)
    dev = partner.device
    out = SimilarityVerify(torch.empty(P, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                           torch.empty(P, dtype=torch.int32, device=dev), torch.empty((P, 6), dtype=torch.int32, device=dev),
                           torch.empty((P, n_g), dtype=torch.uint8, device=dev) if want_mask else None)
    if P:
        _call("vpr_similarity_verify", _ptr(partner), _ptr(sim), P, n_q, gw_q, n_g, gw_g, tol, *[_ptr(t) for t in out], _stream())
    return out


class SimilarityRerankDebug(NamedTuple):
    """The optional outputs of vpr_similarity_local_rerank, candidate order: pair_score f32 / pair_inliers / pair_matches int32
    [B, kc], pair_model int32 [B, kc, 6] ((-inf, 0, 0, six times INT32_MIN) for a candidate the shard does not own;
    similarity_model_scale_rotation reads a row), row_nn int32 [B, kc, n_q] / col_nn int32 [B, kc, n_g] (-1: none, or not owned)."""
    pair_score: torch.Tensor
    pair_inliers: torch.Tensor
    pair_matches: torch.Tensor
    pair_model: torch.Tensor
    row_nn: torch.Tensor
    col_nn: torch.Tensor


def local_rerank_similarity(q_local: torch.Tensor, idx: torch.Tensor, g_local: torch.Tensor, gw_q: int, gw_g: int, tol: int = 1,
                            index_base: int = 0, k: Optional[int] = None, min_sim: float = 0.0, ws: Optional[torch.Tensor] = None,
                            debug: bool = False):
    """Local re-ranking verified under a similarity transform (include/vpr_amd_similarity.h): local_rerank_spatial's arguments.
    Returns (vals f32 [B, k], idx int32 [B, k], inliers int32 [B, k]): a candidate's score is the sum over the mutual-NN matches
    that lie within tol patches of where the pair's best scale-rotation-shift hypothesis puts them; inliers is their number.
    debug=True: a fourth element, SimilarityRerankDebug.  ws: a byte buffer of vpr_similarity_workspace_bytes(B, kc, n_g);
    None: the current stream's cached one."""
    what = "local_rerank_similarity"
    if not isinstance(q_local, torch.Tensor) or q_local.dtype not in (torch.bfloat16, torch.uint8):
        raise RuntimeError(f"{what}: q_local must be bf16 features or their uint8 e4m3 store")
    fp8 = q_local.dtype == torch.uint8
    k = _local_check(what, q_local, idx, g_local, k, q_local.dtype, _lib.PATCH_FP8_MIN_L if fp8 else 32, _lib.LOCAL_HIRES_MAX_N)
    min_sim = float(min_sim)
    if min_sim != min_sim:
        raise RuntimeError(f"{what}: min_sim must be a number")
    B, n_q, l = q_local.shape
    n_local, n_g = g_local.shape[:2]
    gw_q, gw_g, tol = _similarity_grid_check(what, n_q, gw_q, n_g, gw_g, tol)
    kc = idx.shape[1]
    dev = q_local.device
    need = _lib.lib().vpr_similarity_workspace_bytes(B, kc, n_g)
    if ws is None:
        ws = workspace(what, need, dev)
    else:
        _need(ws, torch.uint8, "ws", 1)
    vals = torch.empty((B, k), dtype=torch.float32, device=dev)
    out = torch.empty((B, k), dtype=torch.int32, device=dev)
    inliers = torch.empty((B, k), dtype=torch.int32, device=dev)
    dbg = None
    if debug:
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        dbg = SimilarityRerankDebug(torch.empty((B, kc), dtype=torch.float32, device=dev), i32(B, kc), i32(B, kc), i32(B, kc, 6),
                                    i32(B, kc, n_q), i32(B, kc, n_g))
    if B:
        _call("vpr_similarity_local_rerank", _ptr(q_local), n_q, _ptr(idx), B, kc, _ptr(g_local), n_g, l, n_local, int(index_base),
              min_sim, k, _ptr(vals), _ptr(out), _ptr(inliers), *[_ptr(t) for t in (dbg or (None,) * 6)], int(fp8), gw_q, gw_g, tol,
              _ptr(ws), ws.numel(), _stream())
    return (vals, out, inliers, dbg) if debug else (vals, out, inliers)


PROJECT_CHUNK_ROWS = 65536      # rows per vpr_project_rows call: bounds the workspace for million-row inputs


def project_rows(x: torch.Tensor, P: torch.Tensor, c: torch.Tensor, normalize: bool = True, want_f32: bool = False,
                 want_bf16: bool = True, out=None):
    """Descriptor projection (include/vpr_amd_project.h): x bf16 [rows, D] (unit column stride; a row stride >= D that is a
    multiple of 8 is taken as it is), P bf16 [d, D], c f32 [d] -> z = x P^T + c, L2-normalised per row when `normalize`
    (a row whose norm is 0 or not finite becomes +0).  Returns (out_f32 [rows, d] or None, out_bf16 [rows, d] or None); the
    bf16 output is the RNE rounding of the f32 one.
    out: None, or a pair (out_f32, out_bf16) of contiguous [rows, d] tensors (either None) to write instead of new ones.
    The workspace is a cached buffer of the current stream (pinned while a graph is captured, like every workspace);
    inputs taller than PROJECT_CHUNK_ROWS go through several calls."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("x: expected a GPU tensor (the HIP path has no CPU fallback)")
    if x.dtype != torch.bfloat16:
        raise RuntimeError(f"x: expected dtype {torch.bfloat16}, got {x.dtype}")
    if x.dim() != 2:
        raise RuntimeError(f"x: expected 2 dims, got {x.dim()}")
    _need(P, torch.bfloat16, "P", 2)
    _need(c, torch.float32, "c", 1)
    rows, D = x.shape
    d = P.shape[0]
    if P.shape[1] != D:
        raise RuntimeError("project_rows: x and P disagree on D")
    if c.shape[0] != d:
        raise RuntimeError("project_rows: P and c disagree on d")
    if P.device != x.device or c.device != x.device:
        raise RuntimeError("project_rows: x, P and c must live on one device")
    if rows > 1 and (x.stride(1) != 1 or x.stride(0) < D or x.stride(0) % 8):
        raise RuntimeError("x: expected unit column stride and a row stride >= D that is a multiple of 8")
    if rows <= 1 and not x.is_contiguous():
        raise RuntimeError("x: expected a contiguous tensor")
    x_stride = x.stride(0) if rows > 1 else D
    dev = x.device
    if out is not None:
        out_f32, out_bf16 = out
        for t, dt, name in ((out_f32, torch.float32, "out_f32"), (out_bf16, torch.bfloat16, "out_bf16")):
            if t is not None:
                _need(t, dt, name, 2)
                if t.shape != (rows, d):
                    raise RuntimeError(f"project_rows: {name} must be [rows, d]")
    else:
        out_f32 = torch.empty((rows, d), dtype=torch.float32, device=dev) if want_f32 else None
        out_bf16 = torch.empty((rows, d), dtype=torch.bfloat16, device=dev) if want_bf16 else None
    if out_f32 is None and out_bf16 is None:
        raise RuntimeError("project_rows: at least one of the f32 and bf16 outputs is needed")
    L = _lib.lib()
    for lo in range(0, rows, PROJECT_CHUNK_ROWS):
        n = min(PROJECT_CHUNK_ROWS, rows - lo)
        nbytes = L.vpr_project_workspace_bytes(n, D, d)
        ws = workspace("project_rows", nbytes, dev)
        _call("vpr_project_rows", ctypes.c_void_p(x.data_ptr() + 2 * lo * x_stride), x_stride, n, D, _ptr(P), _ptr(c), d,
              int(bool(normalize)), _ptr(None if out_f32 is None else out_f32[lo:lo + n]),
              _ptr(None if out_bf16 is None else out_bf16[lo:lo + n]), _ptr(ws), ws.numel(), _stream())
    return out_f32, out_bf16


def project_route(rows: int, D: int, d: int) -> int:
    """vpr_project_route: 0 = split-K streaming, 1 = tiled; raises for shapes vpr_project_rows refuses."""
    r = _lib.lib().vpr_project_route(int(rows), int(D), int(d))
    if r < 0:
        _lib.check(r, "vpr_project_route")
    return r


# ------------------------------------------------------------------------------------------ heads
_POSE_PLANES = cache(12)


def check_sincos_offset(what: str, sincos_offset: int, n_out: int) -> None:
    """The rule of include/vpr_amd.h: a non-negative sincos_offset names the output pair [offset, offset + 1]."""
    if sincos_offset >= 0 and sincos_offset + 2 > n_out:
        raise RuntimeError(f"{what}: sincos_offset {sincos_offset} needs sincos_offset + 2 <= n_out = {n_out}")


def _pack_w1_planes(W1: torch.Tensor, frag: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    hi = torch.empty(W1.shape, dtype=torch.bfloat16, device=W1.device)
    lo = torch.empty(W1.shape, dtype=torch.bfloat16, device=W1.device)
    if frag:
        _call("vpr_pose_head_pack_w1_frag", _ptr(W1), W1.shape[0], W1.shape[1], _ptr(hi), _ptr(lo), _stream())
    else:
        _call("vpr_pose_head_pack_w1", _ptr(W1), W1.numel(), _ptr(hi), _ptr(lo), _stream())
    return hi, lo


def _pose_w1_planes(W1: torch.Tensor, frag: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hi, lo) bf16 planes of a first-layer weight, packed once per (storage, version) by vpr_pose_head_pack_w1 (row-major)
    or vpr_pose_head_pack_w1_frag (MFMA fragment order, for the single-launch kernel).
    The entry keeps a reference to W1: while it is cached its storage cannot be freed and handed to another weight
    of the same shape (a recycled address with version 0 would otherwise hit the stale planes)."""
    return _POSE_PLANES.get((tensor_key(W1), bool(frag)), _pack_w1_planes, (W1, frag), (W1,))


def pose_head(x: torch.Tensor, W1: Optional[torch.Tensor], b1: Optional[torch.Tensor], W2: torch.Tensor,
              b2: torch.Tensor, sincos_offset: int = -1, split: bool = True, fused: bool = False) -> torch.Tensor:
    """W2 relu(W1 x + b1) + b2 in f32 (W1 None -> single Linear); optional unit-normalised pair.
    split: first layer as four bf16 MFMAs on (hi, lo) planes of x and W1 (f32 accuracy, ~3x faster than the
    exact-f32 MFMA path, which split=False keeps).  fused=True (with split): vpr_pose_head_fused — fragment-order weight
    planes and, with VPR_POSE_VARIANT=1, ONE launch whose split-K slabs are finished by arrival counters.  Measured
    (scripts/pose_ab.py, B = 64, D = 8448, hidden 1024): one launch 31.8 us, fragment planes + epilogue launch 22.6 us,
    row-major planes + epilogue launch (vpr_pose_head_split, the default) 21.8 us — the serial finisher tail of the
    counter form costs more than the second launch it removes.  All forms are bitwise reproducible."""
    _need(x, torch.float32, "x", 2)
    _need(W2, torch.float32, "W2", 2)
    _need(b2, torch.float32, "b2", 1)
    B, D = x.shape
    n_out = W2.shape[0]
    hidden = 0
    if W1 is not None:
        _need(W1, torch.float32, "W1", 2)
        _need(b1, torch.float32, "b1", 1)
        hidden = W1.shape[0]
        if W1.shape[1] != D or b1.numel() != hidden or W2.shape[1] != hidden:
            raise RuntimeError("pose_head: inconsistent MLP shapes")
    elif W2.shape[1] != D:
        raise RuntimeError("pose_head: W2 must be [n_out, D] for the linear head")
    if b2.numel() != n_out:
        raise RuntimeError("pose_head: b2 size")
    check_sincos_offset("pose_head", int(sincos_offset), n_out)
    L = _lib.lib()
    out = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    fused_bytes = L.vpr_pose_head_fused_workspace_bytes(B, D, hidden) if (hidden > 0 and split and fused) else 0
    if fused_bytes > 0:
        hi, lo = _pose_w1_planes(W1, frag=True)
        ws = workspace("pose_fused", fused_bytes, x.device, zero=True)
        _call("vpr_pose_head_fused", _ptr(x), _ptr(hi), _ptr(lo), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(out), B, D, hidden,
              n_out, int(sincos_offset), _ptr(ws), ws.numel(), _stream())
        return out
    if hidden > 0 and split and D % 32 == 0 and hidden % 16 == 0:
        hi, lo = _pose_w1_planes(W1)
        ws = workspace("pose", L.vpr_pose_head_split_workspace_bytes(B, D, hidden), x.device)
        _call("vpr_pose_head_split", _ptr(x), _ptr(hi), _ptr(lo), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(out), B, D, hidden,
              n_out, int(sincos_offset), _ptr(ws), ws.numel(), _stream())
        return out
    ws = workspace("pose", L.vpr_pose_head_workspace_bytes(B, D, hidden, n_out), x.device)
    _call("vpr_pose_head", _ptr(x), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(out), B, D, hidden, n_out,
          int(sincos_offset), _ptr(ws), ws.numel(), _stream())
    return out


def head_train_state(W1: torch.Tensor, W2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Zeroed AdamW moment buffers (m, v) for vpr_head_train_step, laid out [W1 | b1 | W2 | b2]."""
    hidden, D = W1.shape
    n = _lib.lib().vpr_head_train_state_floats(D, hidden, W2.shape[0])
    return (torch.zeros(n, dtype=torch.float32, device=W1.device), torch.zeros(n, dtype=torch.float32, device=W1.device))


def head_train_state_views(buf: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor):
    """The four per-parameter views (W1, b1, W2, b2 shaped) of one moment buffer."""
    hidden, D = W1.shape
    n_out = W2.shape[0]
    o1 = hidden * D
    o2 = o1 + hidden
    o3 = o2 + n_out * hidden
    return buf[:o1].view(hidden, D), buf[o1:o2], buf[o2:o3].view(n_out, hidden), buf[o3:o3 + n_out]


def _loss_kind(loss: str) -> int:
    """VPR_LOSS_MSE / VPR_LOSS_HUBER of include/vpr_amd.h."""
    if loss not in ("mse", "huber"):
        raise RuntimeError(f"head_train: loss must be 'mse' (nn.MSELoss) or 'huber' (nn.HuberLoss), got {loss!r}")
    return 1 if loss == "huber" else 0


def _head_train_check(X, Y, W1, b1, W2, b2, m, v):
    _need_rows(X, torch.float32, "X")           # rows may be padded: stride(0) goes to C as x_stride / y_stride
    _need_rows(Y, torch.float32, "Y")
    _need(W1, torch.float32, "W1", 2)
    _need(b1, torch.float32, "b1", 1)
    _need(W2, torch.float32, "W2", 2)
    _need(b2, torch.float32, "b2", 1)
    _need(m, torch.float32, "m", 1)
    _need(v, torch.float32, "v", 1)
    hidden, D = W1.shape
    n_out = W2.shape[0]
    if X.shape[1] != D or Y.shape[0] != X.shape[0] or Y.shape[1] != n_out or b1.numel() != hidden or W2.shape[1] != hidden \
            or b2.numel() != n_out:
        raise RuntimeError("head_train: inconsistent shapes")
    if m.numel() != _lib.lib().vpr_head_train_state_floats(D, hidden, n_out) or v.numel() != m.numel():
        raise RuntimeError("head_train: moment buffers must hold vpr_head_train_state_floats() floats (ops.head_train_state)")
    return D, hidden, n_out


def _dropout_args(dropout_p: float, dropout_seed: int):
    """(p, seed) of the *_dropout entry points: 0 <= p < 1, seed a uint64 (include/vpr_amd.h: the mask specification)."""
    p = float(dropout_p)
    if not (0.0 <= p < 1.0):
        raise RuntimeError(f"head_train: dropout_p must satisfy 0 <= p < 1 (nn.Dropout in training mode), got {dropout_p!r}")
    seed = int(dropout_seed)
    if not (0 <= seed < 1 << 64):
        raise RuntimeError(f"head_train: dropout_seed must be an unsigned 64-bit integer, got {dropout_seed!r}")
    return p, seed


def head_train_epoch(X: torch.Tensor, Y: torch.Tensor, order: torch.Tensor, batch_size: int, W1: torch.Tensor, b1: torch.Tensor,
                     W2: torch.Tensor, b2: torch.Tensor, m: torch.Tensor, v: torch.Tensor, first_step: int, lr: float = 1e-5,
                     betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, loss: str = "mse",
                     huber_delta: float = 1.0, dropout_p: float = 0.0, dropout_seed: int = 0) -> torch.Tensor:
    """One pass over the rows listed in `order` (int32, device) in batches of `batch_size` (vpr_head_train_epoch: the whole
    launch sequence enqueued by ONE library call).  Returns the batch losses [ceil(n / batch_size)] (device tensor; nothing
    waits for the GPU).  The caller guarantees 0 <= order < X.shape[0]: the kernels gather rows by these indices unchecked.
    X and Y may have padded rows (unit column stride, X.stride(0) % 4 == 0), as for head_train_step.
    dropout_p > 0: nn.Dropout(dropout_p) in training mode after the ReLU, masks drawn from (dropout_seed, step, position in
    the batch, hidden unit) as include/vpr_amd.h specifies (vpr_head_train_epoch_dropout)."""
    D, hidden, n_out = _head_train_check(X, Y, W1, b1, W2, b2, m, v)
    p_drop, seed = _dropout_args(dropout_p, dropout_seed)
    _need(order, torch.int32, "order", 1)
    n = order.numel()
    if n < 1 or batch_size < 1:
        raise RuntimeError("head_train_epoch: empty pass")
    L = _lib.lib()
    nbytes = L.vpr_head_train_workspace_bytes(min(batch_size, n), D, hidden, n_out)
    if nbytes == 0:
        raise RuntimeError(f"head_train_epoch: unsupported shape B={min(batch_size, n)} D={D} hidden={hidden} n_out={n_out} "
                           "(need 1 <= B <= 64, D % 16 == 0, hidden % 32 == 0, n_out <= 8)")
    ws = workspace("head_train", nbytes, X.device)
    losses = torch.empty((n + batch_size - 1) // batch_size, dtype=torch.float32, device=X.device)
    args = (_ptr(X), X.stride(0), _ptr(order), n, int(batch_size), _ptr(Y), Y.stride(0), D, hidden, n_out,
            _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(m), _ptr(v), int(first_step), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _loss_kind(loss), float(huber_delta), _ptr(losses))
    if p_drop == 0.0:
        _call("vpr_head_train_epoch", *args, _ptr(ws), ws.numel(), _stream())
    else:
        _call("vpr_head_train_epoch_dropout", *args, p_drop, seed, _ptr(ws), ws.numel(), _stream())
    for t in (W1, b1, W2, b2, m, v):
        torch.autograd.graph.increment_version(t)
    return losses


def head_train_step(X: torch.Tensor, Y: torch.Tensor, idx: Optional[torch.Tensor], W1: torch.Tensor, b1: torch.Tensor,
                    W2: torch.Tensor, b2: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float = 1e-5,
                    betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                    loss_out: Optional[torch.Tensor] = None, loss: str = "mse", huber_delta: float = 1.0,
                    dropout_p: float = 0.0, dropout_seed: int = 0, mask_out: Optional[torch.Tensor] = None) -> None:
    """One batch of head-only fine-tuning on cached descriptors (vpr_head_train_step): forward, MSELoss, backward and
    AdamW update of Linear(D,hidden)-ReLU-Linear(hidden,n_out), in place on W1 / b1 / W2 / b2 / m / v.
    X [rows, D] f32, Y [rows, n_out] f32, unit column stride, rows may be padded (X.stride(0) % 4 == 0: the library refuses
    anything else); idx [B] int32 (rows of the batch; None = all rows of X in order).  loss_out: a
    one-element f32 tensor (e.g. losses[i:i+1]) that receives the batch loss.  loss: "mse" (nn.MSELoss) or "huber"
    (nn.HuberLoss(delta=huber_delta)).  No host synchronisation.
    dropout_p > 0: Linear -> ReLU -> Dropout(dropout_p) -> Linear in training mode (vpr_head_train_step_dropout; the mask
    of this step is drawn from (dropout_seed, step, b, j) as include/vpr_amd.h specifies); mask_out: a uint8 [B, hidden]
    tensor that receives the mask (1 = kept)."""
    D, hidden, n_out = _head_train_check(X, Y, W1, b1, W2, b2, m, v)
    p_drop, seed = _dropout_args(dropout_p, dropout_seed)
    if idx is not None:
        _need(idx, torch.int32, "idx", 1)
        B = idx.numel()
    else:
        B = X.shape[0]
    L = _lib.lib()
    if loss_out is not None:
        _need(loss_out, torch.float32, "loss_out")
        if loss_out.numel() != 1:
            raise RuntimeError("head_train_step: loss_out must have one element")
    if mask_out is not None:
        _need(mask_out, torch.uint8, "mask_out", 2)
        if tuple(mask_out.shape) != (B, hidden):
            raise RuntimeError(f"head_train_step: mask_out must be [B, hidden] = [{B}, {hidden}], got {tuple(mask_out.shape)}")
    nbytes = L.vpr_head_train_workspace_bytes(B, D, hidden, n_out)
    if nbytes == 0:
        raise RuntimeError(f"head_train_step: unsupported shape B={B} D={D} hidden={hidden} n_out={n_out} "
                           "(need 1 <= B <= 64, D % 16 == 0, hidden % 32 == 0, n_out <= 8)")
    ws = workspace("head_train", nbytes, X.device)
    args = (_ptr(X), X.stride(0), _ptr(idx), _ptr(Y), Y.stride(0), B, D, hidden, n_out,
            _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(m), _ptr(v), int(step), float(lr),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _loss_kind(loss), float(huber_delta), _ptr(loss_out))
    if p_drop == 0.0 and mask_out is None:
        _call("vpr_head_train_step", *args, _ptr(ws), ws.numel(), _stream())
    else:
        _call("vpr_head_train_step_dropout", *args, p_drop, seed, _ptr(mask_out), _ptr(ws), ws.numel(), _stream())
    for t in (W1, b1, W2, b2, m, v):          # written behind PyTorch's back: version-keyed caches (pose-head weight planes) must see it
        torch.autograd.graph.increment_version(t)


def ln_meanpool_head(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                     Wh: Optional[torch.Tensor] = None, bh: Optional[torch.Tensor] = None,
                     sincos_offset: int = -1, want_pooled: bool = True
                     ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """x [B,T,H] (bf16|f32): pooled = mean_t LayerNorm(x); out = Wh pooled + bh.  -> (pooled, out)."""
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError("ln_meanpool_head: x must be bf16 or f32")
    _need(x, x.dtype, "x", 3)
    _need(gamma, torch.float32, "gamma", 1)
    _need(beta, torch.float32, "beta", 1)
    B, T, H = x.shape
    n_out = 0
    if Wh is not None:
        _need(Wh, torch.float32, "Wh", 2)
        _need(bh, torch.float32, "bh", 1)
        n_out = Wh.shape[0]
        if Wh.shape[1] != H or bh.numel() != n_out:
            raise RuntimeError("ln_meanpool_head: head shapes")
        check_sincos_offset("ln_meanpool_head", int(sincos_offset), n_out)
    pooled = torch.empty((B, H), dtype=torch.float32, device=x.device) if (want_pooled or Wh is None) else None
    out = torch.empty((B, n_out), dtype=torch.float32, device=x.device) if Wh is not None else None
    _call("vpr_ln_meanpool_head", _ptr(x), int(x.dtype == torch.bfloat16), B, T, H, _ptr(gamma), _ptr(beta),
          float(eps), _ptr(pooled), _ptr(Wh), _ptr(bh), n_out, int(sincos_offset), _ptr(out), _stream())
    return pooled, out


def f32_to_bf16(src: torch.Tensor) -> torch.Tensor:
    _need(src, torch.float32, "src")
    dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    _call("vpr_f32_to_bf16", _ptr(src), _ptr(dst), src.numel(), _stream())
    return dst


def _ln_params(what: str, x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pre_bias: Optional[torch.Tensor] = None) -> int:
    """The parameter checks of the three LayerNorm wrappers (gamma / beta bf16 or f32, pre_bias f32, all [C]) -> C."""
    if pre_bias is not None:
        _need(pre_bias, torch.float32, "pre_bias", 1)
    if gamma.dtype not in (torch.bfloat16, torch.float32) or beta.dtype != gamma.dtype:
        raise RuntimeError(f"{what}: gamma/beta must both be bf16 or both f32")
    _need(gamma, gamma.dtype, "gamma", 1)
    _need(beta, beta.dtype, "beta", 1)
    C = x.shape[-1]
    if gamma.numel() != C or beta.numel() != C or (pre_bias is not None and pre_bias.numel() != C):
        raise RuntimeError(f"{what}: parameter size")
    return C


def layernorm_bf16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    """LayerNorm over the last dim of a contiguous bf16 tensor (gamma/beta bf16 or f32) -> bf16."""
    _need(x, torch.bfloat16, "x")
    C = _ln_params("layernorm_bf16", x, gamma, beta)
    y = torch.empty_like(x)
    if x.numel() == 0:                       # no rows: nothing to launch (an empty tensor has no data pointer)
        return y
    _call("vpr_layernorm_bf16", _ptr(x), _ptr(gamma), _ptr(beta), int(gamma.dtype == torch.bfloat16), float(eps),
          _ptr(y), x.numel() // C, C, _stream())
    return y


def patchify_bf16(images: torch.Tensor, patch: int, kpad: int, lead_rows: int = 1) -> torch.Tensor:
    """images [B, Cin, H, W] bf16 -> flattened patches [B * (lead_rows + n), kpad] bf16 in token order
    (lead_rows zero rows per image for the cls slot; K zero-padded to kpad)."""
    _need(images, torch.bfloat16, "images", 4)
    B, Cin, H, W = images.shape
    n = (H // patch) * (W // patch)
    out = torch.empty((B * (lead_rows + n), kpad), dtype=torch.bfloat16, device=images.device)
    if B == 0:                               # no images: nothing to launch (an empty tensor has no data pointer)
        return out
    _call("vpr_patchify_bf16", _ptr(images), B, Cin, H, W, int(patch), int(kpad), int(lead_rows), _ptr(out), _stream())
    return out


def bias_layernorm_bf16(x: torch.Tensor, pre_bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                        eps: float) -> torch.Tensor:
    """LayerNorm(f32(x) + pre_bias) -> bf16; pre_bias [C] f32 is added before the statistics."""
    _need(x, torch.bfloat16, "x")
    C = _ln_params("bias_layernorm_bf16", x, gamma, beta, pre_bias)
    y = torch.empty_like(x)
    if x.numel() == 0:                       # no rows: nothing to launch (an empty tensor has no data pointer)
        return y
    _call("vpr_bias_layernorm_bf16", _ptr(x), _ptr(pre_bias), _ptr(gamma), _ptr(beta),
          int(gamma.dtype == torch.bfloat16), float(eps), _ptr(y), x.numel() // C, C, _stream())
    return y


def add_layernorm_bf16(x: torch.Tensor, res: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                       eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x + res rounded to bf16, LayerNorm of that sum): the residual add fused into the next norm."""
    _need(x, torch.bfloat16, "x")
    _need(res, torch.bfloat16, "res")
    if res.shape != x.shape:
        raise RuntimeError("add_layernorm_bf16: x and res shapes differ")
    C = _ln_params("add_layernorm_bf16", x, gamma, beta)
    s, y = torch.empty_like(x), torch.empty_like(x)
    if x.numel() == 0:
        return s, y
    _call("vpr_add_layernorm_bf16", _ptr(x), _ptr(res), _ptr(s), _ptr(gamma), _ptr(beta),
          int(gamma.dtype == torch.bfloat16), float(eps), _ptr(y), x.numel() // C, C, _stream())
    return s, y


def attention_qkv_bf16(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """qkv [B, T, 3*H*64] bf16 (fused projection output) -> softmax(q k^T / 8) v as [B, T, H*64] bf16."""
    _need(qkv, torch.bfloat16, "qkv", 3)
    B, T, C3 = qkv.shape
    C = C3 // 3
    if C3 != 3 * C or C % heads or C // heads != 64:
        raise RuntimeError("attention_qkv_bf16: needs head_dim 64 and a [B,T,3*H*64] input")
    out = torch.empty((B, T, C), dtype=torch.bfloat16, device=qkv.device)
    _call("vpr_attention_qkv_bf16", _ptr(qkv), _ptr(out), B, T, heads, 64, 0.125, _stream())
    return out


def attention_qkv_split_bf16(qkv: torch.Tensor, B: int, T: int, body_tokens: int, heads: int) -> torch.Tensor:
    """Same attention on the backbone's split row layout: qkv [B*T, 3*H*64] with token t of image b in
    row b*body_tokens + t (t < body_tokens) or B*body_tokens + b*(T-body_tokens) + (t-body_tokens)."""
    _need(qkv, torch.bfloat16, "qkv", 2)
    rows, C3 = qkv.shape
    C = C3 // 3
    if C3 != 3 * C or C % heads or C // heads != 64 or rows != B * T or not (0 <= body_tokens <= T):
        raise RuntimeError("attention_qkv_split_bf16: needs head_dim 64 and a [B*T, 3*H*64] input")
    out = torch.empty((rows, C), dtype=torch.bfloat16, device=qkv.device)
    _call("vpr_attention_qkv_split_bf16", _ptr(qkv), _ptr(out), B, T, int(body_tokens), B * int(body_tokens),
          heads, 64, 0.125, _stream())
    return out


def skinny_linear_bf16(inp: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor,
                       mode: int = 0, stats_bias: Optional[torch.Tensor] = None,
                       row_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Linear layer on a few rows, written into `out` (a row slice of a larger buffer is fine):
    mode 0 out = inp W^T + b; 1 gelu_tanh(inp W^T + b); 2 out += inp W^T; 3 relu; 4 erf-GELU; 5 inp W^T + b into an
    f32 `out`.  With row_stats [N/16, M, 2] f32 (bf16 modes) it also leaves the per-16-column (mean, M2) of
    bf16(out) + stats_bias there (LayerNorm statistics partials)."""
    for t, name in ((inp, "inp"), (weight, "weight"), (out, "out")):
        dtype = torch.float32 if t is out and mode == 5 else torch.bfloat16
        if not t.is_cuda or t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
            raise RuntimeError(f"skinny_linear_bf16: {name} must be a GPU {dtype} matrix with unit column stride")
    M, K = inp.shape
    N = weight.shape[0]
    if weight.shape[1] != K or tuple(out.shape) != (M, N):
        raise RuntimeError("skinny_linear_bf16: shape mismatch")
    if mode != 2:
        if bias is None or not bias.is_cuda or bias.numel() != N or bias.dtype not in (torch.bfloat16, torch.float32) \
                or not bias.is_contiguous():
            raise RuntimeError("skinny_linear_bf16: bias [N] bf16/f32 required")
    if row_stats is not None:
        if mode == 5:
            raise RuntimeError("skinny_linear_bf16: row_stats describe a bf16 output (modes 0-4)")
        _need(row_stats, torch.float32, "row_stats", 3)
        if tuple(row_stats.shape) != (N // 16, M, 2) or N % 16:
            raise RuntimeError("skinny_linear_bf16: row_stats must be [N/16, M, 2] with N % 16 == 0")
        if stats_bias is not None:
            _need(stats_bias, torch.float32, "stats_bias", 1)
        _call("vpr_skinny_linear_stats_bf16", _ptr(inp), inp.stride(0), _ptr(weight), weight.stride(0),
              _ptr(bias) if mode != 2 else None, int(bias is not None and bias.dtype == torch.bfloat16), int(mode),
              _ptr(out), out.stride(0), M, N, K, _ptr(stats_bias), _ptr(row_stats), _stream())
        return out
    _call("vpr_skinny_linear_bf16", _ptr(inp), inp.stride(0), _ptr(weight), weight.stride(0), _ptr(bias) if mode != 2 else None,
          int(bias is not None and bias.dtype == torch.bfloat16), int(mode), _ptr(out), out.stride(0), M, N, K, _stream())
    return out


class ClsLinearConsts(NamedTuple):
    """Static operands of the LayerNorm-fused cls-row linear (see vpr_bias_layernorm_cls_linear_bf16)."""
    w_scaled: torch.Tensor     # [N, C] bf16 = W * gamma
    colsum: torch.Tensor       # [N] f32
    cprime: torch.Tensor       # [N] f32 = W' pre_bias
    bprime: torch.Tensor       # [N] f32 = b + W beta

    @staticmethod
    def build(weight: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
              pre_bias: Optional[torch.Tensor]) -> "ClsLinearConsts":
        w32 = weight.detach().float()
        ws = (w32 * gamma.detach().float()[None, :]).to(torch.bfloat16).contiguous()
        ws32 = ws.float()
        cprime = ws32 @ pre_bias.float() if pre_bias is not None else torch.zeros(weight.shape[0], device=weight.device)
        return ClsLinearConsts(ws, ws32.sum(1).contiguous(), cprime.contiguous(),
                               (bias.detach().float() + w32 @ beta.detach().float()).contiguous())


def bias_layernorm_cls_linear_bf16(x: torch.Tensor, pre_bias: Optional[torch.Tensor], gamma: torch.Tensor,
                                   beta: torch.Tensor, eps: float, cls_row0: int, row_stats: torch.Tensor,
                                   consts: ClsLinearConsts, out: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """y = LayerNorm(x + pre_bias) for every row of x [M, C] (returned), and in the same launch
    out[:] = act(y[cls_row0 : cls_row0 + out.shape[0]] W^T + b) (act = tanh-GELU if gelu), from the raw rows and
    `consts` = ClsLinearConsts.build(W, b, gamma, beta, pre_bias).  row_stats: the statistics partials of those
    rows, left by skinny_linear_bf16(..., row_stats=...) when it wrote them."""
    _need(x, torch.bfloat16, "x", 2)
    for t, name in ((gamma, "gamma"), (beta, "beta")):
        _need(t, torch.bfloat16, name, 1)
    if pre_bias is not None:
        _need(pre_bias, torch.float32, "pre_bias", 1)
    M, C = x.shape
    n_cls, N = out.shape
    _need(consts.w_scaled, torch.bfloat16, "w_scaled", 2)
    for t, name in ((consts.colsum, "colsum"), (consts.cprime, "cprime"), (consts.bprime, "bprime")):
        _need(t, torch.float32, name, 1)
        if t.numel() != N:
            raise RuntimeError("bias_layernorm_cls_linear_bf16: constant vector size")
    if not out.is_cuda or out.dtype != torch.bfloat16 or out.stride(1) != 1:
        raise RuntimeError("bias_layernorm_cls_linear_bf16: out must be a GPU bf16 matrix with unit column stride")
    if consts.w_scaled.shape != (N, C) or gamma.numel() != C or beta.numel() != C:
        raise RuntimeError("bias_layernorm_cls_linear_bf16: shape mismatch")
    _need(row_stats, torch.float32, "row_stats", 3)
    if tuple(row_stats.shape) != (C // 16, n_cls, 2):
        raise RuntimeError("bias_layernorm_cls_linear_bf16: row_stats must be [C/16, n_cls, 2]")
    y = torch.empty_like(x)
    _call("vpr_bias_layernorm_cls_linear_bf16", _ptr(x), _ptr(pre_bias), _ptr(gamma), _ptr(beta), float(eps), _ptr(y),
          M, C, int(cls_row0), n_cls, _ptr(row_stats), _ptr(consts.w_scaled), consts.w_scaled.stride(0), _ptr(consts.colsum),
          _ptr(consts.cprime), _ptr(consts.bprime), int(gelu), _ptr(out), out.stride(0), N, _stream())
    return y
