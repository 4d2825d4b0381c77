"""Gallery sharding + distributed top-k (no counterpart in the reference).

Rank r of R owns gallery rows [N*r/R, N*(r+1)/R) and searches them for EVERY query of the
global batch; the only exchange steps are two all-gathers per batch (RCCL over xGMI on GPUs,
gloo in the CPU tests): query descriptors [B_local, D] -> [R*B_local, D], and per-shard top-k
(value f32, global index int32) [B, k] -> [R, B, k], followed by an on-device merge with the same
(value desc, index asc) key, so the answer equals the unsharded search.

The search and merge kernels are injected (`engine`): the product engine is HipEngine (HIP
kernels, no fallback); tests pass an oracle-backed engine to exercise the sharding and the
collectives on CPU.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist

from . import _lib, _streams, ops
from . import torch_ops  # noqa: F401  registers torch.ops.vpr.*


def shard_bounds(N: int, rank: int, world: int) -> Tuple[int, int]:
    return N * rank // world, N * (rank + 1) // world


class HipEngine:
    """Local top-k and merge on the gfx950 kernels."""

    def local_topk(self, q, gallery, k, index_base, scales=None, norm_bound=None, uncertified=None, ws=None,
                   score_events=None, exact_fallback=False):
        """bf16 shard: q bf16.  fp8 shard (uint8 rows + per-row f32 `scales`): the gathered queries are
        quantised per row here (e4m3 + scale, vpr_quantize_fp8_rows) and searched by vpr_knn_topk_fp8.
        `uncertified` (int32 [1] on the device) counts queries whose answer the kernels could not certify as the
        exact top-k (include/vpr_amd.h "Checked forms"); no host sync.  score_events: see ops.knn_topk.
        exact_fallback: read the per-query status back (one sync) and re-run flagged queries exhaustively."""
        plain = ws is None and score_events is None and not exact_fallback      # the dispatcher-visible ops (torch_ops.py)
        if gallery.dtype == torch.uint8:
            if scales is None:
                raise ValueError("fp8 shard needs per-row scales")
            if plain:
                q8, qs = torch.ops.vpr.quantize_fp8_rows(q.float())
                v, i, _ = torch.ops.vpr.knn_topk_fp8(q8, qs, gallery, scales, k, index_base, norm_bound or ops.NORM_BOUND_FP8,
                                                     uncertified)
                return v, i
            q8, qs = ops.quantize_fp8_rows(q.float())
            return ops.knn_topk_fp8(q8, qs, gallery, scales, k, index_base, ws,
                                    norm_bound=norm_bound or ops.NORM_BOUND_FP8, uncertified=uncertified,
                                    score_events=score_events, exact_fallback=exact_fallback)
        if plain:
            v, i, _ = torch.ops.vpr.knn_topk(q, gallery, k, index_base, norm_bound or ops.NORM_BOUND_BF16, uncertified)
            return v, i
        return ops.knn_topk(q, gallery, k, index_base, ws, norm_bound=norm_bound or ops.NORM_BOUND_BF16,
                            uncertified=uncertified, score_events=score_events, exact_fallback=exact_fallback)

    def merge(self, vals, idxs):
        return torch.ops.vpr.topk_merge(vals, idxs)

    def expand_partial(self, q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, add_query):
        """This shard's f32 [B, D] share of the expanded queries (vpr_query_expand)."""
        return torch.ops.vpr.query_expand(q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, add_query)

    def expand_finish(self, partials, q):
        """Shard partials [R, B, D] -> the expanded queries, bf16 [B, D] (vpr_query_expand_finish)."""
        return torch.ops.vpr.query_expand_finish(partials, q)[1]

    def expand_whole(self, q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight):
        """A gallery of one shard: partial and finish in one call; the partial lives in the stream's cached workspace."""
        return ops.query_expand(q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, True, finish=True)[1]

    def rerank(self, q, idx, rows, index_base, k, ws=None):
        """The k best of the candidates idx [B, kc] this shard owns, by fine score (vpr_rerank_rows): (vals, idx) [B, k]."""
        if ws is None:
            return torch.ops.vpr.rerank_rows(q, idx, rows, index_base, k)
        return ops.rerank_rows(q, idx, rows, index_base, k, ws)

    def local_rerank(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        """The k best of the candidates idx [B, kc] this shard owns, by mutual-nearest-neighbour patch matches
        (vpr_local_rerank): (vals, idx, matches) [B, k]."""
        return torch.ops.vpr.local_rerank(q_local_feats, idx, local_feats, index_base, k, min_sim)

    def local_rerank_fp8(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        """local_rerank on e4m3 patch features, both sides uint8 (vpr_patch_rerank_fp8): (vals, idx, matches) [B, k]."""
        return torch.ops.vpr.local_rerank_fp8(q_local_feats, idx, local_feats, index_base, k, min_sim)

    def local_rerank_hires(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        """local_rerank for up to 1369 patches on either side (vpr_hires_local_rerank): (vals, idx, matches) [B, k]."""
        return torch.ops.vpr.local_rerank_hires(q_local_feats, idx, local_feats, index_base, k, min_sim)

    def local_rerank_fp8_hires(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        """local_rerank_fp8 for up to 1369 patches on either side (vpr_hires_patch_rerank_fp8): (vals, idx, matches) [B, k]."""
        return torch.ops.vpr.local_rerank_fp8_hires(q_local_feats, idx, local_feats, index_base, k, min_sim)

    def local_rerank_spatial(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0, gw_q=1, gw_g=1, tol=1):
        """The local re-ranking of either element type with spatial verification, up to 1369 patches on either side
        (vpr_spatial_local_rerank): (vals, idx, inliers) [B, k]."""
        return torch.ops.vpr.local_rerank_spatial(q_local_feats, idx, local_feats, gw_q, gw_g, tol, index_base, k, min_sim)

    def local_rerank_similarity(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0, gw_q=1, gw_g=1, tol=1):
        """local_rerank_spatial with the matches verified under a similarity transform (scale, rotation and shift) instead of a
        shift (vpr_similarity_local_rerank): (vals, idx, inliers) [B, k]."""
        return torch.ops.vpr.local_rerank_similarity(q_local_feats, idx, local_feats, gw_q, gw_g, tol, index_base, k, min_sim)

    def quantize_patch_fp8(self, feats):
        """Local features bf16 or f32 -> their e4m3 store, uint8 of the same shape (vpr_patch_quantize_fp8)."""
        return torch.ops.vpr.patch_quantize_fp8(feats.contiguous())


def pose_labels(labels, device) -> torch.Tensor:
    """The label table for torch.ops.vpr.retrieval_pose: a [N, 4] float64 tensor on `device` (gallery.device_labels /
    GalleryShard.labels_dev) is taken as it is; a host array is copied there once."""
    if not isinstance(labels, torch.Tensor):
        import numpy as np
        labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float64))
    return labels.to(device=device, dtype=torch.float64).contiguous()


def pose_scaler(scaler):
    """None, four numbers (mean_lat, mean_lon, scale_lat, scale_lon), or a postproc.LatLonScaler -> the op's `scaler`."""
    if scaler is None:
        return None
    if hasattr(scaler, "mean_"):
        return [float(scaler.mean_[0]), float(scaler.mean_[1]), float(scaler.scale_[0]), float(scaler.scale_[1])]
    return [float(x) for x in scaler]


def transfer_pose(v, i, labels, mode, temperature, scaler):
    """Merged top-k rows (v, i) -> (pose64 [B, 3] f64: lat, lon, angle_deg; pose4 [B, 4] f32, the fused head's format under
    `scaler`) from the neighbours' labels: torch.ops.vpr.retrieval_pose without truth, so without its recall outputs."""
    pose64, pose4, _, _ = torch.ops.vpr.retrieval_pose(v.contiguous(), i.contiguous(), labels, mode, temperature, None, 0.0, scaler)
    return pose64, pose4


def expansion_params(expand) -> Optional[dict]:
    """None, (n_use, alpha), or a dict with n_use and any of alpha, q_weight, rounds -> the keyword arguments of
    ShardedGallery.search_expanded after `k` (defaults alpha 3, q_weight 1, rounds 1)."""
    if expand is None:
        return None
    if not isinstance(expand, dict):
        n_use, alpha = expand
        expand = {"n_use": n_use, "alpha": alpha}
    unknown = set(expand) - {"n_use", "alpha", "q_weight", "rounds"}
    if unknown or "n_use" not in expand:
        raise ValueError(f"expand: (n_use, alpha) or a dict with n_use and any of alpha, q_weight, rounds; got {expand}")
    out = {"n_use": int(expand["n_use"]), "alpha": float(expand.get("alpha", 3.0)),
           "q_weight": float(expand.get("q_weight", 1.0)), "rounds": int(expand.get("rounds", 1))}
    if out["rounds"] < 1:
        raise ValueError("expand: rounds must be >= 1")
    return out


def all_gather_topk(v: torch.Tensor, i: torch.Tensor, world: int, group=None):
    """Per-shard (vals f32, idx i32) [B,k] -> [world, B, k] on every rank with ONE all-gather: the
    two arrays travel as one int32 buffer [B, 2k] (values bit-cast), since at these sizes
    (5 KB per rank) a collective costs its launch latency, not its bytes."""
    B, k = v.shape
    packed = torch.cat([v.contiguous().view(torch.int32), i.contiguous()], dim=1)          # [B, 2k] int32
    out = torch.empty((world * B, 2 * k), dtype=torch.int32, device=v.device)              # concatenated along dim 0:
    dist.all_gather_into_tensor(out, packed, group=group)                                   # the layout gloo and RCCL share
    out = out.view(world, B, 2 * k)
    return out[:, :, :k].contiguous().view(torch.float32), out[:, :, k:].contiguous()


def _spatial_model(what: str, spatial_model, spatial_tol) -> bool:
    """spatial_model of a search: "shift" (include/vpr_amd_spatial.h) or "similarity" (include/vpr_amd_similarity.h), which needs
    a spatial_tol.  -> whether it is "similarity"."""
    if spatial_model not in ("shift", "similarity"):
        raise ValueError(f'{what}: spatial_model must be "shift" or "similarity", got {spatial_model!r}')
    if spatial_model == "similarity" and spatial_tol is None:
        raise ValueError(f'{what}: spatial_model="similarity" verifies the matches within spatial_tol patches; name spatial_tol')
    return spatial_model == "similarity"


class ShardedGallery:
    def __init__(self, local_rows: torch.Tensor, n_total: int, rank: int = 0, world: int = 1,
                 engine=None, group: Optional[dist.ProcessGroup] = None, scales: Optional[torch.Tensor] = None,
                 norm_bound: Optional[float] = None, force_collectives: bool = False, exact_fallback: bool = False,
                 projection=None, fine_rows: Optional[torch.Tensor] = None, local_feats: Optional[torch.Tensor] = None,
                 local_hires: bool = False, local_grid: Optional[int] = None):
        """local_rows: [n_local, D] bf16, or uint8 e4m3 bytes with per-row f32 `scales` (value = scale * fp8).
        norm_bound: upper bound of the (dequantised) row norms for the exactness certificate; None = L2-normalised
        descriptors (what SALAD emits); `measure_norm_bound()` computes it from the rows.
        force_collectives: run the two all-gathers and the merge even with one rank (exercises the RCCL path on a
        single GPU: bench.py --force-dist).
        exact_fallback: every local search reads its certificate back (one host sync per search) and re-runs the
        queries it could not certify on exact f64 scores — unconditionally exact answers, for offline evaluation; the
        serving path leaves it off and watches `uncertified_queries()` instead (not capturable in a HIP graph).
        projection (projection.DescriptorProjection whose width d is the rows'): the rows are projected descriptors.  search,
        search_expanded and search_local_queries then take queries of the projection's input width and project them first
        (include/vpr_amd_project.h; in search_local_queries before the all-gather, so d-wide rows travel); queries of width d
        are taken as already projected; `expand` works in the projected space.
        fine_rows ([n_local, D_fine] bf16 or f32, this shard's rows of the full-precision descriptors the local rows were made
        from): the second tier of search_reranked (include/vpr_amd_rerank.h); nothing else reads them.
        local_feats ([n_local, n, l] bf16, this shard's images' local features, SaladAggregator.local_features): what
        search_local_reranked matches the queries' patches against (include/vpr_amd_local.h); nothing else reads them.  uint8:
        their e4m3 store (include/vpr_amd_patch_fp8.h; half the bytes), matched by the e4m3 form of the same stage.
        local_hires: search_local_reranked (and what runs it: search_gathered, search_local_queries, GraphedRetrieval) takes up
        to 1369 patches per image on either side instead of 256 (include/vpr_amd_local_hires.h; 322 to 518 px images).
        local_grid: the width gw of the patch grid that local_feats' n patches lie on in raster order (img_size // 14, as
        SaladAggregator.local_features emits them); what search_local_reranked(spatial_tol=) verifies the matches on
        (include/vpr_amd_spatial.h).  None: the gallery has no grid and takes no spatial search."""
        lo, hi = shard_bounds(n_total, rank, world)
        if local_rows.shape[0] != hi - lo:
            raise ValueError(f"rank {rank}: shard has {local_rows.shape[0]} rows, expected {hi - lo}")
        if (local_rows.dtype == torch.uint8) != (scales is not None):
            raise ValueError("fp8 shards (uint8 rows) come with per-row scales, bf16 shards without")
        if scales is not None and scales.numel() != hi - lo:
            raise ValueError("scales: one per local row")
        if projection is not None and projection.d != local_rows.shape[1]:
            raise ValueError(f"projection maps to {projection.d} columns, the rows have {local_rows.shape[1]}")
        if fine_rows is not None:
            if fine_rows.dim() != 2 or fine_rows.shape[0] != hi - lo:
                raise ValueError(f"rank {rank}: fine_rows must be [{hi - lo}, D_fine], one per local row; got {tuple(fine_rows.shape)}")
            if fine_rows.dtype not in (torch.bfloat16, torch.float32):
                raise ValueError(f"fine_rows: bf16 or f32, got {fine_rows.dtype}")
        if local_feats is not None:
            if local_feats.dim() != 3 or local_feats.shape[0] != hi - lo:
                raise ValueError(f"rank {rank}: local_feats must be [{hi - lo}, n, l], one image per local row; "
                                 f"got {tuple(local_feats.shape)}")
            if local_feats.dtype not in (torch.bfloat16, torch.uint8):
                raise ValueError(f"local_feats: bf16 or uint8 (e4m3 bytes), got {local_feats.dtype}")
        if local_grid is not None:
            if local_feats is None:
                raise ValueError("local_grid: the width of the patch grid of local_feats; this gallery has none")
            local_grid = int(local_grid)
            if not 1 <= local_grid <= local_feats.shape[1] or local_feats.shape[1] % local_grid:
                raise ValueError(f"local_grid: {local_grid} does not divide the {local_feats.shape[1]} patches of an image")
        self.local_grid = local_grid
        self.local_feats = local_feats
        self.local_hires = bool(local_hires)
        self.fine_rows = fine_rows
        self.projection = projection
        self.scales = scales
        self.rows, self.n_total, self.rank, self.world = local_rows, n_total, rank, world
        self.index_base = lo
        self.engine = engine if engine is not None else HipEngine()
        self.group = group
        self.norm_bound = norm_bound
        self.exact_fallback = exact_fallback
        self.collective = world > 1 or force_collectives
        # queries whose local answer was not certified exact, summed over every search of this object (device word)
        self.uncertified = torch.zeros(1, dtype=torch.int32, device=local_rows.device) if local_rows.is_cuda else None

    def measure_norm_bound(self, slab: int = 65536) -> float:
        """Largest L2 norm of the (dequantised) local rows, with 0.1 % slack; kept as this shard's norm bound."""
        best = 0.0
        for lo in range(0, self.rows.shape[0], slab):
            r = self.rows[lo:lo + slab]
            x = r.view(torch.float8_e4m3fn).float() * self.scales[lo:lo + slab, None] if self.scales is not None else r.float()
            best = max(best, float(x.norm(dim=1).max()))
        self.norm_bound = best * 1.001
        return self.norm_bound

    @property
    def query_width(self) -> int:
        """Width of the queries a caller hands in: the projection's input width, or the rows' own."""
        return self.rows.shape[1] if self.projection is None else self.projection.d_in

    def project_queries(self, q: torch.Tensor) -> torch.Tensor:
        """Queries as the rows are: [B, D_in] bf16 through the gallery's projection, [B, d] as they are; without a projection
        every query passes unchanged (the search kernels check its width)."""
        if self.projection is None or q.shape[1] == self.rows.shape[1]:
            return q
        if q.shape[1] != self.projection.d_in:
            raise ValueError(f"queries are {q.shape[1]} wide; this gallery takes {self.projection.d_in} (projected here) or "
                             f"{self.rows.shape[1]} (already projected)")
        return self.projection.apply(q)

    def gather_queries(self, q_local: torch.Tensor) -> torch.Tensor:
        if not self.collective:
            return q_local
        if q_local.dim() > 2:           # local features [B_local, n, l]: gathered as rows of n * l
            B = q_local.shape[0]
            return self.gather_queries(q_local.reshape(B, -1)).view(self.world * B, *q_local.shape[1:])
        out = torch.empty((self.world * q_local.shape[0], q_local.shape[1]), dtype=q_local.dtype, device=q_local.device)
        dist.all_gather_into_tensor(out, q_local.contiguous(), group=self.group)
        return out

    def _local(self, q_all: torch.Tensor, k: int, ws=None, score_events=None):
        if isinstance(self.engine, HipEngine):
            return self.engine.local_topk(q_all, self.rows, k, self.index_base, self.scales, self.norm_bound,
                                          self.uncertified, ws, score_events, self.exact_fallback)
        if self.scales is not None:
            return self.engine.local_topk(q_all, self.rows, k, self.index_base, self.scales)
        return self.engine.local_topk(q_all, self.rows, k, self.index_base)

    def _merged(self, v: torch.Tensor, i: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """This shard's (vals, idx) [B, k] -> the gallery's, the same on every rank: one packed all-gather and the merge."""
        if not self.collective:
            return v, i
        vs, is_ = all_gather_topk(v, i, self.world, self.group)
        return self.engine.merge(vs, is_)

    def search(self, q_all: torch.Tensor, k: int, ws=None, score_events=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """q_all [B, D]: the same on every rank.  Returns merged (vals [B,k], idx [B,k]) on every rank.
        score_events (HipEngine only): list collecting (start, end) timing events around the local score stage."""
        return self._merged(*self._local(self.project_queries(q_all), k, ws, score_events))

    def search_reranked(self, q_all: torch.Tensor, k: int, kc: int, q_fine: Optional[torch.Tensor] = None,
                        ws=None, score_events=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Two-tier search (include/vpr_amd_rerank.h): the coarse local search of this shard for kc candidates (k <= kc <= 64,
        through the projection if there is one), those candidates re-ranked to k by their f32 dot product with the shard's
        `fine_rows`, then the packed all-gather and merge of `search` — as many collectives as a plain search.
        q_fine [B, D_fine] bf16 or f32: the queries of the fine tier; None: q_all, which must then be D_fine wide (with a
        projection the caller's D_in-wide queries are the fine queries).  ws, score_events: of the coarse search, as in `search`.
        Sharded meaning: the answer is the k best by fine score among the UNION of the shards' coarse top-kc — each shard
        re-ranks its own kc candidates, so up to world * kc rows are considered, a superset of the global coarse top-kc.  With
        one shard that is the coarse top-kc itself.  Values are fine scores; a candidate whose fine score is NaN comes last
        among the live ones, as -inf."""
        if self.fine_rows is None:
            raise ValueError("search_reranked: this gallery has no fine_rows")
        if not 1 <= kc <= 64:
            raise ValueError(f"search_reranked: one coarse search yields at most 64 candidates; kc = {kc}")
        if not 1 <= k <= kc:
            raise ValueError(f"search_reranked: k must be in 1..kc (k = {k}, kc = {kc})")
        q_fine = q_all if q_fine is None else q_fine
        if q_fine.shape[1] != self.fine_rows.shape[1]:
            raise ValueError(f"search_reranked: the fine queries are {q_fine.shape[1]} wide, the fine rows {self.fine_rows.shape[1]}")
        if q_fine.shape[0] != q_all.shape[0]:
            raise ValueError("search_reranked: q_all and q_fine disagree on B")
        _, i = self._local(self.project_queries(q_all), kc, ws, score_events)
        return self._merged(*self.engine.rerank(q_fine, i.contiguous(), self.fine_rows, self.index_base, k))

    def search_local_reranked(self, q_all: torch.Tensor, k: int, kc: int, q_local_feats: torch.Tensor, min_sim: float = 0.0,
                              ws=None, score_events=None, spatial_tol: Optional[int] = None,
                              q_grid: Optional[int] = None, spatial_model: str = "shift") -> Tuple[torch.Tensor, torch.Tensor]:
        """Local-feature re-ranking (include/vpr_amd_local.h): the coarse local search of this shard for kc candidates
        (k <= kc <= 64, through the projection if there is one), those candidates re-ranked to k by the summed similarity of
        the mutual-nearest-neighbour patch pairs (similarity >= min_sim) between q_local_feats [B, n_q, l] bf16 and the shard's
        `local_feats`, then the packed all-gather and merge of `search` — as many collectives as a plain search.
        ws, score_events: of the coarse search, as in `search`.
        Sharded meaning, as search_reranked: the answer is the k best by local score among the UNION of the shards' coarse
        top-kc — each shard re-ranks its own kc candidates, so up to world * kc images are considered, a superset of the
        global coarse top-kc.  With one shard that is the coarse top-kc itself.  Values are local scores (always finite).
        A gallery of e4m3 local features (uint8 `local_feats`) takes q_local_feats as bf16, quantised here, or as uint8.
        A gallery made with local_hires=True takes up to 1369 patches on either side; when either side exceeds 256 the match
        runs on the engine's local_rerank_hires / local_rerank_fp8_hires, otherwise on the 256-patch entries as always.
        spatial_tol (0..8; None: no verification): only the matches within spatial_tol bins of the pair's dominant shift on the
        patch grids count (include/vpr_amd_spatial.h; the engine's local_rerank_spatial, which routes by the patch counts
        itself).  The gallery's grid is its local_grid; q_grid is the width of the queries' grid, None: the gallery's (the
        queries then hold as many patches as the gallery's images).
        spatial_model (with spatial_tol): "shift", that vote; "similarity": the matches within spatial_tol patches of the pair's
        best hypothesis of one scale, rotation and shift count instead (include/vpr_amd_similarity.h; the engine's
        local_rerank_similarity), which holds under a zoom, where a shift vote smears; every grid side is then at most 37."""
        similarity = _spatial_model("search_local_reranked", spatial_model, spatial_tol)
        if self.local_feats is None:
            raise ValueError("search_local_reranked: this gallery has no local_feats")
        if not 1 <= kc <= 64:
            raise ValueError(f"search_local_reranked: one coarse search yields at most 64 candidates; kc = {kc}")
        if not 1 <= k <= kc:
            raise ValueError(f"search_local_reranked: k must be in 1..kc (k = {k}, kc = {kc})")
        fp8 = self.local_feats.dtype == torch.uint8
        if q_local_feats is None or q_local_feats.dim() != 3 or q_local_feats.dtype not in ((torch.bfloat16, torch.uint8) if fp8
                                                                                          else (torch.bfloat16,)):
            raise ValueError(f"search_local_reranked: q_local_feats must be bf16 {'or uint8 ' if fp8 else ''}[B, n_q, l]")
        if q_local_feats.shape[2] != self.local_feats.shape[2]:
            raise ValueError(f"search_local_reranked: the queries' local features are {q_local_feats.shape[2]} wide, the "
                             f"gallery's {self.local_feats.shape[2]}")
        if q_local_feats.shape[0] != q_all.shape[0]:
            raise ValueError("search_local_reranked: q_all and q_local_feats disagree on B")
        n_max = max(q_local_feats.shape[1], self.local_feats.shape[1])
        if self.local_hires and n_max > _lib.LOCAL_HIRES_MAX_N:
            raise ValueError(f"search_local_reranked: at most {_lib.LOCAL_HIRES_MAX_N} patches per image")
        if not self.local_hires and n_max > 256:
            raise ValueError("search_local_reranked: at most 256 patches per image")
        hires = n_max > _lib.LOCAL_MAX_N
        if spatial_tol is not None:
            if self.local_grid is None:
                raise ValueError("search_local_reranked: spatial_tol needs the gallery's patch grid: ShardedGallery(local_grid=gw)")
            if q_grid is None and q_local_feats.shape[1] != self.local_feats.shape[1]:
                raise ValueError("search_local_reranked: the queries hold another number of patches than the gallery's images; "
                                 "name their grid's width (q_grid)")
            gw_q = self.local_grid if q_grid is None else int(q_grid)
            try:
                grid_check = ops._similarity_grid_check if similarity else ops._spatial_grid_check
                grid_check("search_local_reranked", q_local_feats.shape[1], gw_q, self.local_feats.shape[1], self.local_grid, spatial_tol)
            except RuntimeError as e:
                raise ValueError(str(e)) from None
        elif q_grid is not None:
            raise ValueError("search_local_reranked: q_grid is the queries' grid of a spatial search (spatial_tol)")
        _, i = self._local(self.project_queries(q_all), kc, ws, score_events)
        if similarity:
            v, i, _ = self.engine.local_rerank_similarity(self.local_query_feats(q_local_feats), i.contiguous(), self.local_feats,
                                                          self.index_base, k, min_sim, gw_q, self.local_grid, int(spatial_tol))
        elif spatial_tol is not None:
            v, i, _ = self.engine.local_rerank_spatial(self.local_query_feats(q_local_feats), i.contiguous(), self.local_feats,
                                                       self.index_base, k, min_sim, gw_q, self.local_grid, int(spatial_tol))
        elif fp8:
            entry = self.engine.local_rerank_fp8_hires if hires else self.engine.local_rerank_fp8
            v, i, _ = entry(self.local_query_feats(q_local_feats), i.contiguous(), self.local_feats, self.index_base, k, min_sim)
        else:
            entry = self.engine.local_rerank_hires if hires else self.engine.local_rerank
            v, i, _ = entry(q_local_feats.contiguous(), i.contiguous(), self.local_feats, self.index_base, k, min_sim)
        return self._merged(v, i)

    def local_query_feats(self, q_local_feats: torch.Tensor) -> torch.Tensor:
        """The queries' local features as this gallery's second stage reads them: bf16 ones become their e4m3 store when the
        gallery holds one (one rounding from the value handed in); anything else comes back as it is, contiguous."""
        if self.local_feats is not None and self.local_feats.dtype == torch.uint8 and q_local_feats.dtype != torch.uint8:
            return self.engine.quantize_patch_fp8(q_local_feats)
        return q_local_feats.contiguous()

    def expand(self, q_all: torch.Tensor, vals: torch.Tensor, idx: torch.Tensor, n_use: int, alpha: float = 3.0,
               q_weight: float = 1.0) -> torch.Tensor:
        """Query expansion (alpha-QE, include/vpr_amd_expand.h): q_all [B, D] bf16 and its merged top-k (vals, idx) [B, k], the
        same on every rank -> bf16 [B, D], the same on every rank: normalise(q_weight * q + sum_{j < n_use} vals_j^alpha * row_j).
        Every rank adds up the neighbour rows it owns (rank 0 also the query term); the f32 partials travel in ONE all-gather and
        are added in rank order — an all-reduce would leave the order of the sum to the collective.  A query with nothing to
        add (or a non-finite sum) comes back unchanged."""
        vals, idx = vals.contiguous(), idx.contiguous()
        if not self.collective:
            return self.engine.expand_whole(q_all, vals, idx, self.rows, self.scales, self.index_base, n_use, alpha, q_weight)
        part = self.engine.expand_partial(q_all, vals, idx, self.rows, self.scales, self.index_base, n_use, alpha, q_weight,
                                          self.rank == 0)
        B, D = part.shape
        parts = torch.empty((self.world * B, D), dtype=torch.float32, device=part.device)
        dist.all_gather_into_tensor(parts, part, group=self.group)
        return self.engine.expand_finish(parts.view(self.world, B, D), q_all)

    def search_expanded(self, q_all: torch.Tensor, k: int, n_use: int, alpha: float = 3.0, q_weight: float = 1.0,
                        rounds: int = 1, ws=None, ws2=None, rerank: Optional[int] = None,
                        q_fine: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """search -> expand -> search, `rounds` times: the (vals, idx) of the last search.  The expanded bf16 queries go through
        `search` like any others (an fp8 shard quantises them there).  ws / ws2: kNN workspaces of the first and of the later
        searches (ws2 None: ws again).
        rerank = kc: the LAST search is search_reranked(expanded queries, k, kc); its fine queries are q_fine, or (None) the
        caller's q_all as handed in — the original queries, not the expanded ones."""
        if rerank is not None and q_fine is None:
            q_fine = q_all
        q_all = self.project_queries(q_all)
        v, i = self.search(q_all, k, ws)
        for r in range(rounds):
            q_all = self.expand(q_all, v, i, n_use, alpha, q_weight)
            if rerank is not None and r == rounds - 1:
                return self.search_reranked(q_all, k, rerank, q_fine, ws if ws2 is None else ws2)
            v, i = self.search(q_all, k, ws if ws2 is None else ws2)
        return v, i

    def search_gathered(self, q_all: torch.Tensor, k: int, expand=None, rerank: Optional[int] = None,
                        q_fine: Optional[torch.Tensor] = None, ws=None, ws2=None,
                        score_events=None, local_rerank: Optional[int] = None, q_local_feats: Optional[torch.Tensor] = None,
                        min_sim: float = 0.0, spatial_tol: Optional[int] = None,
                        q_grid: Optional[int] = None, spatial_model: str = "shift") -> Tuple[torch.Tensor, torch.Tensor]:
        """The search that (expand, rerank) name, over queries that are the same on every rank: `search`, `search_reranked`
        (rerank = kc) or `search_expanded` (expand: anything expansion_params takes; with rerank, of its last search).
        q_fine, ws, ws2, score_events: as those take them; an expanded search has no seam for score_events.
        local_rerank = kc: `search_local_reranked` with q_local_feats and min_sim; it is a second stage of its own and combines
        neither with rerank= nor with expand= (ValueError).  spatial_tol, q_grid, spatial_model: of that search; without local_rerank a
        ValueError."""
        expand = expansion_params(expand)
        _spatial_model("search_gathered", spatial_model, spatial_tol)
        if spatial_tol is not None and local_rerank is None:
            raise ValueError("search_gathered: spatial_tol verifies the matches of local_rerank; name its kc")
        if local_rerank is not None:
            if rerank is not None:
                raise ValueError("search_gathered: local_rerank and rerank are two kinds of second stage; name one of them")
            if expand is not None:
                raise ValueError("search_gathered: local_rerank does not combine with expand")
            return self.search_local_reranked(q_all, k, local_rerank, q_local_feats, min_sim, ws, score_events, spatial_tol, q_grid,
                                              spatial_model)
        if expand is not None:
            if score_events is not None:
                raise ValueError("search_gathered: score_events cannot be collected around an expanded search")
            return self.search_expanded(q_all, k, ws=ws, ws2=ws2, rerank=rerank, q_fine=q_fine, **expand)
        if rerank is not None:
            return self.search_reranked(q_all, k, rerank, q_fine, ws, score_events)
        return self.search(q_all, k, ws, score_events)

    def search_local_queries(self, q_local: torch.Tensor, k: int, expand=None, rerank: Optional[int] = None, *,
                             ws=None, ws2=None, score_events=None, local_rerank: Optional[int] = None,
                             q_local_feats: Optional[torch.Tensor] = None, min_sim: float = 0.0,
                             spatial_tol: Optional[int] = None, q_grid: Optional[int] = None,
                             spatial_model: str = "shift") -> Tuple[torch.Tensor, torch.Tensor]:
        """Data-parallel form: each rank contributes B_local queries and gets back its own rows — project, gather, search
        (search_gathered), keep this rank's rows.  The eager callers and GraphedRetrieval all go through here.
        expand: None, or the query expansion to search with (expansion_params).
        rerank = kc: the two-tier form (search_reranked; with `expand`, of its last search).  The fine queries are q_local's
        rows: when a projection made the travelling rows d wide, the D_in-wide ones are gathered as well.
        local_rerank = kc: the local-feature form (search_local_reranked) with this rank's q_local_feats [B_local, n_q, l] bf16,
        gathered across the ranks like the queries when the gallery is collective; not together with rerank= or expand=.
        With e4m3 local features in the gallery, bf16 ones are quantised before that gather (half the bytes travel).
        spatial_tol, q_grid, spatial_model: the spatial verification of that form (search_local_reranked).
        ws, ws2, score_events: handed to search_gathered."""
        _spatial_model("search_local_queries", spatial_model, spatial_tol)
        if local_rerank is not None and rerank is not None:
            raise ValueError("search_local_queries: local_rerank and rerank are two kinds of second stage; name one of them")
        if local_rerank is not None and (q_local_feats is None or q_local_feats.shape[0] != q_local.shape[0]):
            raise ValueError("search_local_queries: local_rerank needs q_local_feats, one image per query")
        q_proj = self.project_queries(q_local)
        q_all = self.gather_queries(q_proj)
        q_fine = None
        if rerank is not None:
            q_fine = q_all if q_proj is q_local else self.gather_queries(q_local)
        feats_all = None
        if local_rerank is not None:
            bf16 = isinstance(q_local_feats, torch.Tensor) and q_local_feats.dtype == torch.bfloat16 and q_local_feats.dim() == 3
            feats_all = self.gather_queries(self.local_query_feats(q_local_feats) if bf16 else q_local_feats.contiguous())
        v, i = self.search_gathered(q_all, k, expand, rerank, q_fine, ws, ws2, score_events, local_rerank, feats_all, min_sim,
                                    spatial_tol, q_grid, spatial_model)
        b = q_local.shape[0]
        return v[self.rank * b:(self.rank + 1) * b], i[self.rank * b:(self.rank + 1) * b]

    def uncertified_queries(self, reduce: bool = True) -> int:
        """Host read (one sync) of the counter: 0 means every answer so far was certified exact on the device.
        The device word counts THIS rank's shard searches only; a query flagged on another rank's shard makes the merged
        top-k just as unproven, so with a sharded gallery the count is summed over the group (reduce=True: a collective —
        every rank must call it; reduce=False returns the per-shard count)."""
        if self.uncertified is None:
            return 0
        if reduce and self.collective:
            total = self.uncertified.clone()
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
            return int(total)
        return int(self.uncertified)


class GraphedRetrieval:
    """One batch of retrieval — {query all-gather, local shard search, packed top-k all-gather, merge} — captured once
    into a HIP graph and replayed per batch (SURVEY §7 step 5 / BASELINE config 5: "hipGraph-captured per-batch
    retrieval").  Static shapes: B_local queries per rank, k, this shard.  The kernels take stream-ordered arguments
    and pre-allocated workspaces; RCCL's collectives are captured like any other stream work (every rank must
    capture and replay in lockstep).  With one rank and no forced collectives the graph holds the local search only.
    Replay: copy the queries into `self.q`, `replay()`, read `self.vals` / `self.idx` (this rank's B_local rows).
    labels (the full [N, 4] label table, gallery.device_labels): the graph also runs torch.ops.vpr.retrieval_pose on this
    rank's merged rows; `self.pose64` ([B_local, 3] f64: lat, lon, angle_deg) and `self.pose4` ([B_local, 4] f32, the fused
    head's format under `scaler`) are rewritten by every replay like vals / idx.  Without labels both stay None.
    expand ((n_use, alpha) or a dict, expansion_params): the graph holds the two-pass form, ShardedGallery.search_expanded —
    vals / idx and the poses are those of the last search, which runs in a kNN workspace of its own.
    A gallery with a projection: `self.q` has the projection's input width and the projection is captured inside the graph,
    ahead of the gather.
    rerank (kc): the graph holds the two-tier form, ShardedGallery.search_reranked (with `expand`, of its last search): the fine
    queries are `self.q`, vals are fine scores, and the poses come from the re-ranked rows.
    local_rerank (kc): the graph holds the local-feature form, ShardedGallery.search_local_reranked (not with `rerank` or
    `expand`): `self.q_feats` [B_local, n, l] bf16 (n, l: the gallery's) is a second static input,
    filled by __call__(q_local, q_local_feats); vals are local scores.  A gallery of e4m3 local features makes it uint8:
    __call__ takes bf16 features, quantised into it before the replay, or uint8 ones.
    spatial_tol (with local_rerank): the graph holds the spatially verified form (search_local_reranked(spatial_tol=)) on a
    gallery made with local_grid; the queries lie on the gallery's grid.  spatial_model: "shift" or "similarity", as
    search_local_reranked takes it."""

    def __init__(self, gallery: ShardedGallery, batch_local: int, k: int, labels=None, mode: str = "top1",
                 temperature: float = 0.01, scaler=None, expand=None, rerank: Optional[int] = None,
                 local_rerank: Optional[int] = None, min_sim: float = 0.0, spatial_tol: Optional[int] = None,
                 spatial_model: str = "shift"):
        self.g, self.k = gallery, k
        _spatial_model("GraphedRetrieval", spatial_model, spatial_tol)
        self.spatial_model = spatial_model
        self.spatial_tol = None if spatial_tol is None else int(spatial_tol)
        if self.spatial_tol is not None:
            if local_rerank is None:
                raise ValueError("GraphedRetrieval: spatial_tol verifies the matches of local_rerank; name its kc")
            if gallery.local_grid is None:
                raise ValueError("GraphedRetrieval: spatial_tol needs the gallery's patch grid: ShardedGallery(local_grid=gw)")
        self.rerank = None if rerank is None else int(rerank)
        self.local_rerank = None if local_rerank is None else int(local_rerank)
        self.min_sim, self.q_feats = float(min_sim), None
        if self.local_rerank is not None:
            if rerank is not None or expand is not None:
                raise ValueError("GraphedRetrieval: local_rerank combines neither with rerank nor with expand")
            if gallery.local_feats is None:
                raise ValueError("GraphedRetrieval: local_rerank needs a gallery with local_feats")
            self.q_feats = torch.zeros((batch_local, *gallery.local_feats.shape[1:]), dtype=gallery.local_feats.dtype,
                                       device=gallery.rows.device)
        self.expand = expansion_params(expand)
        self.labels = None if labels is None else pose_labels(labels, gallery.rows.device)
        self.mode, self.temperature, self.scaler = mode, temperature, pose_scaler(scaler)
        self.pose64 = self.pose4 = None
        if gallery.exact_fallback:
            raise RuntimeError("GraphedRetrieval: exact_fallback reads the certificate back on the host — not capturable")
        if gallery.collective and dist.get_backend(gallery.group) != "nccl":
            raise RuntimeError("GraphedRetrieval: collectives can only be captured on the RCCL ('nccl') backend; "
                               f"this process group is '{dist.get_backend(gallery.group)}' — use the eager search")
        rows = gallery.rows
        dev, D = rows.device, rows.shape[1]
        self.q = torch.zeros((batch_local, gallery.query_width), dtype=torch.bfloat16, device=dev)
        B = batch_local * (gallery.world if gallery.collective else 1)
        self.ws = ops.knn_workspace(B, rows.shape[0], D, max(k, self.rerank or 0, self.local_rerank or 0), dev)
        self.ws2 = None if self.expand is None else ops.workspace("knn_expanded", self.ws.numel(), dev)
        counted = gallery.uncertified.clone() if gallery.uncertified is not None else None
        self._captured = _streams.Captured(self._run, dev)      # the warm-up also sets the communicator up
        if counted is not None:                  # the warm-up's all-zero queries (every score ties) are not searches; the
            gallery.uncertified.copy_(counted)   # device is idle since the warm-up and the capture ran nothing
        self.vals, self.idx = self._captured.out

    def close(self) -> None:
        """Destroy the graph and forget what the package keyed by its private stream (_streams.Captured.close)."""
        self._captured.close()

    def _run(self):
        v, i = self.g.search_local_queries(self.q, self.k, self.expand, self.rerank, ws=self.ws, ws2=self.ws2,
                                           local_rerank=self.local_rerank, q_local_feats=self.q_feats, min_sim=self.min_sim,
                                           spatial_tol=self.spatial_tol, spatial_model=self.spatial_model)
        if self.labels is not None:
            self.pose64, self.pose4 = transfer_pose(v, i, self.labels, self.mode, self.temperature, self.scaler)
        return v, i

    def __call__(self, q_local: torch.Tensor, q_local_feats: Optional[torch.Tensor] = None):
        self.q.copy_(q_local)
        if self.q_feats is not None:
            self.q_feats.copy_(self.g.local_query_feats(q_local_feats))
        self._captured.graph.replay()
        return self.vals, self.idx
