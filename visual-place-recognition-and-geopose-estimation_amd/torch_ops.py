"""`torch.library` operator layer over the C ABI.

The reference's seam is `nn.Module.forward` (dinov2salad/dinov2salad_validation.py:49-52: `feature_extractor(x)` then
`regressor(features)`; swin_transformer/swin_validation.py:43-46).  The modules of `vpr_amd.modules` call these ops at
that seam, so the HIP hot path is visible to PyTorch's dispatcher like any other operator:

    torch.ops.vpr.salad_aggregate / salad_aggregate_split / salad_aggregate_f32
    torch.ops.vpr.salad_aggregate_train                (training mode: Dropout active in the score / cluster MLPs)
    torch.ops.vpr.salad_aggregate_n / salad_aggregate_f32_n   (any patch-token count 65 .. 576, e.g. 322 px images)
    torch.ops.vpr.salad_aggregate_hires / salad_aggregate_f32_hires   (65 .. 1369 patch tokens: 448 / 518 px images)
    torch.ops.vpr.knn_topk / knn_topk_fp8 / topk_merge
    torch.ops.vpr.retrieval_pose                       (geopose and first-hit ranks from the merged top-k)
    torch.ops.vpr.query_expand / query_expand_finish   (alpha-QE / DBA: weighted mean of a query and its best rows)
    torch.ops.vpr.project_rows                         (PCA / whitening projection of descriptors + L2 re-normalisation)
    torch.ops.vpr.rerank_rows                          (two-tier retrieval: coarse candidates re-ranked on full-precision rows)
    torch.ops.vpr.local_rerank                         (local-feature re-ranking: mutual-nearest-neighbour patch matches)
    torch.ops.vpr.patch_quantize_fp8 / local_rerank_fp8   (the same on e4m3 patch features: half the feature store)
    torch.ops.vpr.local_rerank_hires / local_rerank_fp8_hires   (both for up to 1369 patches per image: 322 to 518 px)
    torch.ops.vpr.spatial_verify / local_rerank_spatial   (matches count only within the dominant shift of the patch grid)
    torch.ops.vpr.similarity_verify / local_rerank_similarity   (... or with one scale, rotation and shift of the patch grid)
    torch.ops.vpr.pose_head / ln_meanpool_head
    torch.ops.vpr.head_train_epoch                     (head-only fine-tuning pass; mutates parameters and AdamW moments)
    torch.ops.vpr.head_train_epoch_dropout             (the same pass with Dropout(p) after the ReLU, training mode)

Each op has
  * a CUDA(HIP) implementation = the ctypes wrapper of `vpr_amd.ops` (same validation, same stream, same workspaces;
    a non-zero C status raises RuntimeError; there is no CPU implementation — a CPU tensor is refused), and
  * a fake (meta) implementation that only computes output shapes / dtypes, so the modules can be traced with
    FakeTensorMode / `torch.export` / `torch.compile(fullgraph=True)` without a GPU (tests/test_torch_ops_cpu.py).
Inference only: no autograd formula is registered (the modules run under torch.no_grad, as the reference's
feature extractor does: dinov2salad_validation.py:50).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops

_W_NAMES = ("w1_sc", "b1_sc", "w2_s", "b2_s", "w2_c", "b2_c", "w1_t", "b1_t", "w2_t", "b2_t")


def _weights(ws: List[Tensor], dustbin: float, f32: bool = False):
    if len(ws) != 10:
        raise RuntimeError("SALAD weights: expected the 10 tensors (w1_sc, b1_sc, w2_s, b2_s, w2_c, b2_c, w1_t, b1_t, w2_t, b2_t)")
    cls = ops.SaladWeightsF32 if f32 else ops.SaladWeights
    return cls(**dict(zip(_W_NAMES, ws)), dustbin=dustbin)


def _desc_width(ws: List[Tensor]) -> int:
    return ws[8].shape[0] + ws[4].shape[0] * ws[2].shape[0]          # t + l * m


def weight_list(w: ops.SaladWeights) -> List[Tensor]:
    return [getattr(w, n) for n in _W_NAMES]


# ------------------------------------------------------------------------------------------------------------ SALAD
@torch.library.custom_op("vpr::salad_aggregate", mutates_args=())
def salad_aggregate(tokens: Tensor, weights: List[Tensor], dustbin: float, sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """tokens [B, 1+n, C] bf16 (cls first) -> (descriptor f32 [B, t+l*m], its bf16 copy).  vpr_salad_aggregate."""
    out, out16 = ops.salad_aggregate(tokens, _weights(weights, dustbin), sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_split", mutates_args=())
def salad_aggregate_split(patch: Tensor, cls: Tensor, weights: List[Tensor], dustbin: float,
                          sinkhorn_iters: int, token_done: bool = False) -> Tuple[Tensor, Tensor]:
    """patch [B, n, C] bf16 + cls [B, C] bf16 (the layout the HIP backbone computes in).  vpr_salad_aggregate_split, or —
    token_done: the token MLP of these cls rows already ran on the backbone's cls-row stream (ops.salad_stage_token) —
    vpr_salad_stage_mlps + vpr_salad_stage_aggregate."""
    out, out16 = ops.salad_aggregate_split(patch, cls, _weights(weights, dustbin), sinkhorn_iters, True, token_done=token_done)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_f32", mutates_args=())
def salad_aggregate_f32(patch: Tensor, cls: Tensor, weights: List[Tensor], dustbin: float,
                        sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """f32 patch [B, n, C] + cls [B, C], f32 weights: the aggregation at the reference's precision.  vpr_salad_aggregate_f32."""
    out, out16 = ops.salad_aggregate_f32((patch, cls), _weights(weights, dustbin, f32=True), sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_train", mutates_args=())
def salad_aggregate_train(tokens: Tensor, cls: Optional[Tensor], weights: List[Tensor], dustbin: float, sinkhorn_iters: int,
                          dropout_p: float, seed: int, pass_index: int, image_base: int) -> Tuple[Tensor, Tensor]:
    """The aggregation in training mode (Dropout(dropout_p) active in the score / cluster MLPs: the hub model under
    dinov2salad_finetuning.py:115's model.train()).  cls None: tokens = [B, 1+n, C] bf16, cls first; else tokens = patch
    [B, n, C] bf16 and cls [B, C] bf16.  The mask is a pure function of (seed, pass_index, image_base + b, token, unit) —
    include/vpr_amd.h; seed is the 64 bits of the mask key (a negative value stands for its two's complement: the schema's
    int is signed).  vpr_salad_aggregate_train."""
    pair = tokens if cls is None else (tokens, cls)
    out, out16 = ops.salad_aggregate_train(pair, _weights(weights, dustbin), dropout_p, seed & 0xFFFFFFFFFFFFFFFF, pass_index,
                                           image_base, sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_n", mutates_args=())
def salad_aggregate_n(patch: Tensor, cls: Optional[Tensor], weights: List[Tensor], dustbin: float,
                      sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """The aggregation for any patch-token count n in 65 .. 576 (include/vpr_amd_salad_anyres.h).  cls None: patch = tokens
    [B, 1+n, C] bf16, cls first; else patch [B, n, C] bf16 and cls [B, C] bf16 — either layout is addressed in place.
    n == 256: the bits of salad_aggregate_split.  vpr_salad_aggregate_n."""
    out, out16 = ops.salad_aggregate_n(patch if cls is None else (patch, cls), _weights(weights, dustbin), sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_f32_n", mutates_args=())
def salad_aggregate_f32_n(patch: Tensor, cls: Optional[Tensor], weights: List[Tensor], dustbin: float,
                          sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """salad_aggregate_n at the reference's precision: f32 tokens (cls None: [B, 1+n, C], cls first; else the pair) and f32
    weights.  n == 256: the bits of salad_aggregate_f32.  vpr_salad_aggregate_f32_n."""
    out, out16 = ops.salad_aggregate_f32_n(patch if cls is None else (patch, cls), _weights(weights, dustbin, f32=True),
                                           sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_hires", mutates_args=())
def salad_aggregate_hires(patch: Tensor, cls: Optional[Tensor], weights: List[Tensor], dustbin: float,
                          sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """The aggregation for any patch-token count n in 65 .. 1369 (include/vpr_amd_salad_hires.h; 448 px = 1024 tokens, 518 px
    = 1369).  The layouts of salad_aggregate_n.  n == 256: the bits of salad_aggregate_split; other n <= 576: those of
    salad_aggregate_n.  vpr_salad_aggregate_hires."""
    out, out16 = ops.salad_aggregate_hires(patch if cls is None else (patch, cls), _weights(weights, dustbin), sinkhorn_iters, True)
    return out, out16


@torch.library.custom_op("vpr::salad_aggregate_f32_hires", mutates_args=())
def salad_aggregate_f32_hires(patch: Tensor, cls: Optional[Tensor], weights: List[Tensor], dustbin: float,
                              sinkhorn_iters: int) -> Tuple[Tensor, Tensor]:
    """salad_aggregate_hires at the reference's precision: f32 tokens (cls None: [B, 1+n, C], cls first; else the pair) and f32
    weights.  vpr_salad_aggregate_f32_hires."""
    out, out16 = ops.salad_aggregate_f32_hires(patch if cls is None else (patch, cls), _weights(weights, dustbin, f32=True),
                                               sinkhorn_iters, True)
    return out, out16


def _salad_fake(tokens, *rest, **_):
    """Descriptor and its bf16 copy, [B, t + l*m]: the first argument carries B and the device, the weight list the width."""
    B, D = tokens.shape[0], _desc_width(next(a for a in rest if isinstance(a, (list, tuple))))
    return tokens.new_empty((B, D), dtype=torch.float32), tokens.new_empty((B, D), dtype=torch.bfloat16)


for _op in (salad_aggregate, salad_aggregate_split, salad_aggregate_f32, salad_aggregate_train, salad_aggregate_n, salad_aggregate_f32_n,
            salad_aggregate_hires, salad_aggregate_f32_hires):
    _op.register_fake(_salad_fake)


# -------------------------------------------------------------------------------------------------------------- kNN
@torch.library.custom_op("vpr::knn_topk", mutates_args=("uncertified",))
def knn_topk(q: Tensor, gallery: Tensor, k: int, index_base: int, norm_bound: float,
             uncertified: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """q [B, D] bf16 x gallery [N, D] bf16 -> (scores f32 [B, k] descending, global indices int32 [B, k], certificate
    status int32 [B]: 0 / 1 = proven exact, 2 = not proven).  `uncertified` (int32 [1], optional) is incremented on the
    device by the number of status-2 queries.  vpr_knn_topk_checked."""
    status = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    v, i = ops.knn_topk(q, gallery, k, index_base, norm_bound=norm_bound, status=status, uncertified=uncertified)
    return v, i, status


@knn_topk.register_fake
def _(q, gallery, k, index_base, norm_bound, uncertified):
    B = q.shape[0]
    return (q.new_empty((B, k), dtype=torch.float32), q.new_empty((B, k), dtype=torch.int32),
            q.new_empty((B,), dtype=torch.int32))


@torch.library.custom_op("vpr::knn_topk_fp8", mutates_args=("uncertified",))
def knn_topk_fp8(q: Tensor, q_scale: Tensor, gallery: Tensor, gallery_scale: Tensor, k: int, index_base: int,
                 norm_bound: float, uncertified: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """e4m3 bytes + per-row f32 scales on both sides (BASELINE config 5).  vpr_knn_topk_fp8_checked."""
    status = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    v, i = ops.knn_topk_fp8(q, q_scale, gallery, gallery_scale, k, index_base, norm_bound=norm_bound, status=status,
                            uncertified=uncertified)
    return v, i, status


@knn_topk_fp8.register_fake
def _(q, q_scale, gallery, gallery_scale, k, index_base, norm_bound, uncertified):
    B = q.shape[0]
    return (q.new_empty((B, k), dtype=torch.float32), q.new_empty((B, k), dtype=torch.int32),
            q.new_empty((B,), dtype=torch.int32))


@torch.library.custom_op("vpr::quantize_fp8_rows", mutates_args=())
def quantize_fp8_rows(x: Tensor) -> Tuple[Tensor, Tensor]:
    """x [rows, D] f32 -> (e4m3 bytes uint8 [rows, D], per-row scale f32 [rows]).  vpr_quantize_fp8_rows."""
    return ops.quantize_fp8_rows(x)


@quantize_fp8_rows.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=torch.uint8), x.new_empty((x.shape[0],), dtype=torch.float32)


@torch.library.custom_op("vpr::topk_merge", mutates_args=())
def topk_merge(vals: Tensor, idxs: Tensor) -> Tuple[Tensor, Tensor]:
    """Per-shard top-k lists [shards, B, k] (global indices) -> merged [B, k], (value desc, index asc).  vpr_topk_merge."""
    return ops.topk_merge(vals, idxs)


@topk_merge.register_fake
def _(vals, idxs):
    _, B, k = vals.shape
    return vals.new_empty((B, k), dtype=torch.float32), vals.new_empty((B, k), dtype=torch.int32)


@torch.library.custom_op("vpr::retrieval_pose", mutates_args=())
def retrieval_pose(vals: Tensor, idx: Tensor, labels_dev: Tensor, mode: str = "top1", temperature: float = 0.01,
                   q_targets: Optional[Tensor] = None, tau: float = 0.0,
                   scaler: Optional[List[float]] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Merged top-k [B, k] + device label table f64 [N, 4] -> (pose f64 [B, 3] = lat, lon, angle_deg; pose f32 [B, 4] in the
    fused head's format; first-hit rank within tau int32 [B]; first same-Region_ID rank int32 [B]).  vpr_retrieval_pose."""
    return ops.retrieval_pose(vals, idx, labels_dev, mode, temperature, q_targets, tau, scaler)


@retrieval_pose.register_fake
def _(vals, idx, labels_dev, mode="top1", temperature=0.01, q_targets=None, tau=0.0, scaler=None):
    B = vals.shape[0]
    return (vals.new_empty((B, 3), dtype=torch.float64), vals.new_empty((B, 4), dtype=torch.float32),
            vals.new_empty((B,), dtype=torch.int32), vals.new_empty((B,), dtype=torch.int32))


@torch.library.custom_op("vpr::query_expand", mutates_args=())
def query_expand(q: Tensor, vals: Tensor, idx: Tensor, rows: Tensor, scales: Optional[Tensor], index_base: int, n_use: int,
                 alpha: float = 3.0, q_weight: float = 1.0, add_query: bool = True) -> Tensor:
    """One shard's partial sum of the expanded queries: q bf16 [B, D], a top-k list [B, k], the shard's rows (bf16, or uint8
    e4m3 bytes + per-row f32 scales) -> f32 [B, D] = add_query * q_weight * q + sum_j vals_j^alpha * row_j over the n_use
    best neighbours this shard owns.  vpr_query_expand."""
    return ops.query_expand(q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, add_query)


@query_expand.register_fake
def _(q, vals, idx, rows, scales, index_base, n_use, alpha=3.0, q_weight=1.0, add_query=True):
    return q.new_empty(q.shape, dtype=torch.float32)


@torch.library.custom_op("vpr::query_expand_finish", mutates_args=())
def query_expand_finish(partials: Tensor, q: Tensor) -> Tuple[Tensor, Tensor]:
    """Shard partials f32 [R, B, D] -> (expanded queries f32 [B, D], unit rows; their bf16 rounding), summed in shard order; a
    query whose sum is zero or not finite stays q.  vpr_query_expand_finish."""
    return ops.query_expand_finish(partials, q)


@query_expand_finish.register_fake
def _(partials, q):
    return q.new_empty(q.shape, dtype=torch.float32), q.new_empty(q.shape, dtype=torch.bfloat16)


@torch.library.custom_op("vpr::project_rows", mutates_args=())
def project_rows(x: Tensor, P: Tensor, c: Tensor, normalize: bool = True) -> Tuple[Tensor, Tensor]:
    """Descriptor projection: x bf16 [rows, D], P bf16 [d, D], c f32 [d] -> (f32 [rows, d], its bf16 rounding) =
    x P^T + c, L2-normalised per row when `normalize` (a row of norm 0 or not finite becomes +0).  vpr_project_rows."""
    return ops.project_rows(x, P, c, normalize, want_f32=True, want_bf16=True)


@project_rows.register_fake
def _(x, P, c, normalize=True):
    shape = (x.shape[0], P.shape[0])
    return x.new_empty(shape, dtype=torch.float32), x.new_empty(shape, dtype=torch.bfloat16)


@torch.library.custom_op("vpr::rerank_rows", mutates_args=())
def rerank_rows(q: Tensor, idx: Tensor, rows: Tensor, index_base: int = 0, k: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Two-tier retrieval: q [B, D] (bf16 | f32), candidates idx int32 [B, kc] (global rows), this shard's fine rows
    [n_local, D] (bf16 | f32) -> (scores f32 [B, k], indices int32 [B, k]): the k best (None: kc) of the candidates the shard
    owns by their f32 dot product with the fine row, (score desc, index asc); the rest is (-inf, -1).  vpr_rerank_rows."""
    return ops.rerank_rows(q, idx, rows, index_base, k)


@rerank_rows.register_fake
def _(q, idx, rows, index_base=0, k=None):
    B, k = idx.shape[0], idx.shape[1] if k is None else k
    return q.new_empty((B, k), dtype=torch.float32), q.new_empty((B, k), dtype=torch.int32)


@torch.library.custom_op("vpr::local_rerank", mutates_args=())
def local_rerank(q_local: Tensor, idx: Tensor, g_local: Tensor, index_base: int = 0, k: Optional[int] = None,
                 min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """Local-feature re-ranking: q_local bf16 [B, n_q, l], candidates idx int32 [B, kc] (global rows), this shard's local
    features bf16 [n_local, n_g, l] -> (scores f32, indices int32, matches int32), each [B, k]: the k best (None: kc) of the
    candidates the shard owns by the summed similarity of their mutual-nearest-neighbour patch pairs (similarity >= min_sim),
    (score desc, index asc); the rest is (-inf, -1, 0).  vpr_local_rerank."""
    return ops.local_rerank(q_local, idx, g_local, index_base, k, min_sim)


@local_rerank.register_fake
def _local_rerank_fake(q_local, idx, g_local, index_base=0, k=None, min_sim=0.0):
    B, k = idx.shape[0], idx.shape[1] if k is None else k
    new = lambda dtype: q_local.new_empty((B, k), dtype=dtype)
    return new(torch.float32), new(torch.int32), new(torch.int32)


@torch.library.custom_op("vpr::patch_quantize_fp8", mutates_args=())
def patch_quantize_fp8(x: Tensor) -> Tensor:
    """Patch features f32 or bf16, any shape -> uint8 of that shape: the e4m3fn byte of x * 2^8, one round-to-nearest-even
    from the f32 value.  vpr_patch_quantize_fp8."""
    return ops.quantize_patch_fp8(x)


@patch_quantize_fp8.register_fake
def _(x):
    return x.new_empty(x.shape, dtype=torch.uint8)


@torch.library.custom_op("vpr::local_rerank_fp8", mutates_args=())
def local_rerank_fp8(q_local: Tensor, idx: Tensor, g_local: Tensor, index_base: int = 0, k: Optional[int] = None,
                     min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """local_rerank on e4m3 patch features: q_local uint8 [B, n_q, l], g_local uint8 [n_local, n_g, l] (patch_quantize_fp8
    bytes, l a multiple of 64); outputs as local_rerank.  vpr_patch_rerank_fp8."""
    return ops.local_rerank_fp8(q_local, idx, g_local, index_base, k, min_sim)


local_rerank_fp8.register_fake(_local_rerank_fake)            # the output shapes of the bf16 form


@torch.library.custom_op("vpr::local_rerank_hires", mutates_args=())
def local_rerank_hires(q_local: Tensor, idx: Tensor, g_local: Tensor, index_base: int = 0, k: Optional[int] = None,
                       min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """local_rerank for 1..1369 patches on either side (322 to 518 px images); outputs as local_rerank, equal to it bit for
    bit at 256 patches and below.  vpr_hires_local_rerank."""
    return ops.local_rerank_hires(q_local, idx, g_local, index_base, k, min_sim)


@torch.library.custom_op("vpr::local_rerank_fp8_hires", mutates_args=())
def local_rerank_fp8_hires(q_local: Tensor, idx: Tensor, g_local: Tensor, index_base: int = 0, k: Optional[int] = None,
                           min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """local_rerank_fp8 for 1..1369 patches on either side; outputs as local_rerank.  vpr_hires_patch_rerank_fp8."""
    return ops.local_rerank_fp8_hires(q_local, idx, g_local, index_base, k, min_sim)


local_rerank_hires.register_fake(_local_rerank_fake)          # the output shapes do not depend on the patch counts
local_rerank_fp8_hires.register_fake(_local_rerank_fake)


@torch.library.custom_op("vpr::spatial_verify", mutates_args=())
def spatial_verify(partner: Tensor, sim: Tensor, n_q: int, gw_q: int, gw_g: int, tol: int = 1) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Spatial verification of a match list: partner int32 [P, n_g] (the query patch of candidate column j; outside 0..n_q-1:
    no match), sim f32 [P, n_g], grids gw_q / gw_g wide -> (score f32 [P], inliers int32 [P], matches int32 [P], shift int32
    [P, 2], inlier_mask uint8 [P, n_g]): the matches within tol bins of the dominant grid shift.  vpr_spatial_verify."""
    return tuple(ops.spatial_verify(partner, sim, n_q, gw_q, gw_g, tol, want_mask=True))


@spatial_verify.register_fake
def _(partner, sim, n_q, gw_q, gw_g, tol=1):
    P, n_g = partner.shape
    ops._spatial_grid_check("spatial_verify", n_q, gw_q, n_g, gw_g, tol)
    new = lambda shape, dtype: partner.new_empty(shape, dtype=dtype)
    return (new((P,), torch.float32), new((P,), torch.int32), new((P,), torch.int32), new((P, 2), torch.int32),
            new((P, n_g), torch.uint8))


@torch.library.custom_op("vpr::local_rerank_spatial", mutates_args=())
def local_rerank_spatial(q_local: Tensor, idx: Tensor, g_local: Tensor, gw_q: int, gw_g: int, tol: int = 1, index_base: int = 0,
                         k: Optional[int] = None, min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """local_rerank_hires (bf16 features) or local_rerank_fp8_hires (uint8 e4m3 bytes) with spatial verification: only the
    matches within tol bins of the pair's dominant shift on the gw_q / gw_g wide patch grids count -> (scores f32, indices
    int32, inliers int32), each [B, k].  vpr_spatial_local_rerank."""
    return ops.local_rerank_spatial(q_local, idx, g_local, gw_q, gw_g, tol, index_base, k, min_sim)


@local_rerank_spatial.register_fake
def _(q_local, idx, g_local, gw_q, gw_g, tol=1, index_base=0, k=None, min_sim=0.0):
    ops._spatial_grid_check("local_rerank_spatial", q_local.shape[1], gw_q, g_local.shape[1], gw_g, tol)
    return _local_rerank_fake(q_local, idx, g_local, index_base, k, min_sim)


@torch.library.custom_op("vpr::similarity_verify", mutates_args=())
def similarity_verify(partner: Tensor, sim: Tensor, n_q: int, gw_q: int, gw_g: int, tol: int = 1) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Verification of a match list under a similarity transform: partner int32 [P, n_g] (the query patch of candidate column
    j; outside 0..n_q-1: no match), sim f32 [P, n_g], grids gw_q / gw_g wide -> (score f32 [P], inliers int32 [P], matches
    int32 [P], model int32 [P, 6], inlier_mask uint8 [P, n_g]): the matches within tol patches of the best two-match
    hypothesis of scale, rotation and shift.  vpr_similarity_verify."""
    return tuple(ops.similarity_verify(partner, sim, n_q, gw_q, gw_g, tol, want_mask=True))


@similarity_verify.register_fake
def _(partner, sim, n_q, gw_q, gw_g, tol=1):
    P, n_g = partner.shape
    ops._similarity_grid_check("similarity_verify", n_q, gw_q, n_g, gw_g, tol)
    new = lambda shape, dtype: partner.new_empty(shape, dtype=dtype)
    return (new((P,), torch.float32), new((P,), torch.int32), new((P,), torch.int32), new((P, 6), torch.int32),
            new((P, n_g), torch.uint8))


@torch.library.custom_op("vpr::local_rerank_similarity", mutates_args=())
def local_rerank_similarity(q_local: Tensor, idx: Tensor, g_local: Tensor, gw_q: int, gw_g: int, tol: int = 1, index_base: int = 0,
                            k: Optional[int] = None, min_sim: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """local_rerank_spatial's arguments, the matches verified under a similarity transform instead of a shift: only those
    within tol patches of the pair's best scale-rotation-shift hypothesis count -> (scores f32, indices int32, inliers
    int32), each [B, k].  vpr_similarity_local_rerank."""
    return ops.local_rerank_similarity(q_local, idx, g_local, gw_q, gw_g, tol, index_base, k, min_sim)


@local_rerank_similarity.register_fake
def _(q_local, idx, g_local, gw_q, gw_g, tol=1, index_base=0, k=None, min_sim=0.0):
    ops._similarity_grid_check("local_rerank_similarity", q_local.shape[1], gw_q, g_local.shape[1], gw_g, tol)
    return _local_rerank_fake(q_local, idx, g_local, index_base, k, min_sim)


# ------------------------------------------------------------------------------------------------------------ heads
@torch.library.custom_op("vpr::pose_head", mutates_args=())
def pose_head(x: Tensor, W1: Optional[Tensor], b1: Optional[Tensor], W2: Tensor, b2: Tensor, sincos_offset: int) -> Tensor:
    """W2 relu(W1 x + b1) + b2 in f32 (W1 None: a single Linear), optional unit-normalised (sin, cos) pair at
    `sincos_offset`.  DINOv2RegressionModel.regressor, dinov2salad_validation.py:43-47,52.  vpr_pose_head[_split]."""
    return ops.pose_head(x, W1, b1, W2, b2, sincos_offset)


@pose_head.register_fake
def _(x, W1, b1, W2, b2, sincos_offset):
    ops.check_sincos_offset("pose_head", sincos_offset, W2.shape[0])
    return x.new_empty((x.shape[0], W2.shape[0]), dtype=torch.float32)


@torch.library.custom_op("vpr::ln_meanpool_head", mutates_args=())
def ln_meanpool_head(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, Wh: Optional[Tensor], bh: Optional[Tensor],
                     sincos_offset: int) -> Tuple[Tensor, Tensor]:
    """x [B, T, H] (bf16 | f32): pooled = mean_t LayerNorm(x) [B, H] f32; out = Wh pooled + bh [B, n_out] f32 ([B, 0]
    without a head).  HF Swin pooler + Linear, swin_validation.py:43-46.  vpr_ln_meanpool_head."""
    pooled, out = ops.ln_meanpool_head(x, gamma, beta, eps, Wh, bh, sincos_offset, want_pooled=True)
    if out is None:
        out = torch.empty((x.shape[0], 0), dtype=torch.float32, device=x.device)
    return pooled, out


@ln_meanpool_head.register_fake
def _(x, gamma, beta, eps, Wh, bh, sincos_offset):
    B, _, H = x.shape
    if Wh is not None:
        ops.check_sincos_offset("ln_meanpool_head", sincos_offset, Wh.shape[0])
    return x.new_empty((B, H), dtype=torch.float32), x.new_empty((B, 0 if Wh is None else Wh.shape[0]), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------- head fine-tuning
@torch.library.custom_op("vpr::head_train_epoch", mutates_args=("W1", "b1", "W2", "b2", "m", "v"))
def head_train_epoch(X: Tensor, Y: Tensor, order: Tensor, batch_size: int, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor,
                     m: Tensor, v: Tensor, first_step: int, lr: float, beta1: float, beta2: float, eps: float,
                     weight_decay: float, loss: str = "mse", huber_delta: float = 1.0) -> Tensor:
    """One pass of head-only fine-tuning over the cached descriptor rows listed in `order` (int32), batches of `batch_size`:
    forward, MSELoss (or HuberLoss), backward and AdamW of Linear(D,hidden)-ReLU-Linear(hidden,n_out) per batch, IN PLACE on the
    parameters and on the moment buffers (ops.head_train_state).  X and Y may have padded rows (unit column stride; X.stride(0) % 4
    == 0).  Returns the batch losses.  dinov2salad_finetuning.py:113-128
    (one epoch of the loop) on descriptors computed once.  vpr_head_train_epoch."""
    return ops.head_train_epoch(X, Y, order, batch_size, W1, b1, W2, b2, m, v, first_step, lr, (beta1, beta2), eps, weight_decay,
                                loss, huber_delta)


@head_train_epoch.register_fake
def _(X, Y, order, batch_size, W1, b1, W2, b2, m, v, first_step, lr, beta1, beta2, eps, weight_decay, loss="mse", huber_delta=1.0):
    return X.new_empty(((order.shape[0] + batch_size - 1) // batch_size,), dtype=torch.float32)


@torch.library.custom_op("vpr::head_train_epoch_dropout", mutates_args=("W1", "b1", "W2", "b2", "m", "v"))
def head_train_epoch_dropout(X: Tensor, Y: Tensor, order: Tensor, batch_size: int, W1: Tensor, b1: Tensor, W2: Tensor, b2: Tensor,
                             m: Tensor, v: Tensor, first_step: int, lr: float, beta1: float, beta2: float, eps: float,
                             weight_decay: float, loss: str, huber_delta: float, dropout_p: float, dropout_seed: int) -> Tensor:
    """head_train_epoch for Linear(D,hidden)-ReLU-Dropout(dropout_p)-Linear(hidden,n_out) in training mode
    (dinov2salad_finetuning_2.py:113-122, swin_attempt_2.py:114-123): the masks are a pure function of (dropout_seed, step,
    position in the batch, hidden unit) — include/vpr_amd.h.  dropout_seed is the 64 bits of the mask key (a negative value
    stands for its two's complement: the schema's int is signed).  vpr_head_train_epoch_dropout."""
    return ops.head_train_epoch(X, Y, order, batch_size, W1, b1, W2, b2, m, v, first_step, lr, (beta1, beta2), eps, weight_decay,
                                loss, huber_delta, dropout_p=dropout_p, dropout_seed=dropout_seed & 0xFFFFFFFFFFFFFFFF)


@head_train_epoch_dropout.register_fake
def _(X, Y, order, batch_size, W1, b1, W2, b2, m, v, first_step, lr, beta1, beta2, eps, weight_decay, loss, huber_delta, dropout_p,
      dropout_seed):
    return X.new_empty(((order.shape[0] + batch_size - 1) // batch_size,), dtype=torch.float32)


OPS = ("head_train_epoch", "head_train_epoch_dropout", "salad_aggregate", "salad_aggregate_split", "salad_aggregate_f32", "salad_aggregate_train", "knn_topk", "knn_topk_fp8", "quantize_fp8_rows",
       "topk_merge", "pose_head", "ln_meanpool_head", "retrieval_pose", "query_expand", "query_expand_finish", "project_rows",
       "rerank_rows", "salad_aggregate_n", "salad_aggregate_f32_n", "salad_aggregate_hires", "salad_aggregate_f32_hires",
       "local_rerank", "patch_quantize_fp8", "local_rerank_fp8", "local_rerank_hires", "local_rerank_fp8_hires",
       "spatial_verify", "local_rerank_spatial", "similarity_verify", "local_rerank_similarity")
