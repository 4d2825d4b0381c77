"""Gallery builder, on-disk format and retrieval-based geopose (the reference has
no retrieval code — its label files `cleaned_dataset_files/labels_{train,val}.csv`
(`filename,timestamp,latitude,longitude,angle,Region_ID`) are the side table this uses).

On-disk format (a directory; every array is a plain .npy so shards can be memory-mapped):
  meta.json            {"version":1, "n":N, "d":8448, "dtype":"bf16"|"fp8_e4m3", "label_columns":[...]}
  descriptors.npy      [N, D] uint16 (bf16 bit patterns) or uint8 (e4m3 bytes)
  scales.npy           [N] float32            (fp8 only: value = scale * fp8)
  labels.npy           [N, 4] float64         latitude, longitude, angle (deg), Region_ID
  filenames.txt        one per row (optional)
  projection.npz       (optional) the projection.DescriptorProjection the rows went through; "d" is then the stored,
                       projected width.  A directory without it loads as ever.
  fine_descriptors.npy (optional) [N, D_fine] uint16 (bf16 bit patterns): the full-precision descriptors the rows were made
                       from, the second tier of ShardedGallery.search_reranked.  A directory without it loads as ever.
  local_features.npy   (optional) [N, n, l] uint16 (bf16 bit patterns): every image's n L2-normalised patch descriptors of
                       width l (SaladAggregator.local_features), what ShardedGallery.search_local_reranked matches the
                       queries' patches against.  A directory without it loads as ever.
  local_features_fp8.npy (optional, instead of local_features.npy: a directory never holds both) [N, n, l] uint8: the same
                       features as OCP e4m3 bytes of x * 2^8 (ops.quantize_patch_fp8, include/vpr_amd_patch_fp8.h), half the
                       bytes; the search then matches on them (ops.local_rerank_fp8).
Rank r of R loads rows [N*r/R, N*(r+1)/R) only.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _streams, ops
from .projection import DescriptorProjection
from .retrieval import ShardedGallery, shard_bounds

LABEL_COLUMNS = ("latitude", "longitude", "angle", "Region_ID")
PROJECTION_FILE = "projection.npz"
FINE_FILE = "fine_descriptors.npy"
LOCAL_FILE = "local_features.npy"
LOCAL_FP8_FILE = "local_features_fp8.npy"


@dataclass
class GalleryShard:
    rows: torch.Tensor                    # [n_local, D] bf16 or uint8 on the GPU
    scales: Optional[torch.Tensor]        # [n_local] f32 (fp8) or None
    labels: np.ndarray                    # [N, 4] float64 — the FULL side table (small), host
    n_total: int
    index_base: int
    dtype: str
    labels_dev: Optional[torch.Tensor] = None   # [N, 4] float64 on the GPU: the same table for ops.retrieval_pose (device_labels)
    projection: Optional["DescriptorProjection"] = None   # what the rows went through (projection.npz), or None
    local: Optional[torch.Tensor] = None  # [n_local, n, l] bf16 (local_features.npy) or uint8 (local_features_fp8.npy) on the GPU (load_local), or None
    fine: Optional[torch.Tensor] = None   # [n_local, D_fine] bf16 on the GPU (fine_descriptors.npy; load_fine), or None


def save_gallery(path: str, descriptors: torch.Tensor, labels: np.ndarray, scales: Optional[torch.Tensor] = None,
                 filenames: Optional[Sequence[str]] = None, projection: Optional[DescriptorProjection] = None,
                 fine: Optional[torch.Tensor] = None, local: Optional[torch.Tensor] = None) -> None:
    """descriptors: [N,D] torch.bfloat16 (bf16 gallery) or torch.uint8 (+ scales: fp8 gallery).
    projection: the DescriptorProjection the rows went through (project_gallery); written as projection.npz.
    fine: [N, D_fine] torch.bfloat16, the full-precision descriptors of the same rows; written as fine_descriptors.npy.
    local: [N, n, l] torch.bfloat16, the local features of the same rows, written as local_features.npy; or torch.uint8, their
    e4m3 store, written as local_features_fp8.npy.  The file that is not written is removed."""
    os.makedirs(path, exist_ok=True)
    if local is not None and (local.dim() != 3 or local.dtype not in (torch.bfloat16, torch.uint8)
                              or local.shape[0] != descriptors.shape[0]):
        raise ValueError(f"local must be bfloat16 or uint8 (e4m3 bytes) [N, n, l] with one image per descriptor ({descriptors.shape[0]})")
    if fine is not None and (fine.dim() != 2 or fine.dtype != torch.bfloat16 or fine.shape[0] != descriptors.shape[0]):
        raise ValueError(f"fine must be bfloat16 [N, D_fine] with one row per descriptor ({descriptors.shape[0]})")
    if projection is not None and projection.d != descriptors.shape[1]:
        raise ValueError(f"projection maps to {projection.d} columns, the rows have {descriptors.shape[1]}")
    d = descriptors.detach().cpu().contiguous()
    if d.dtype == torch.bfloat16:
        arr, dtype = d.view(torch.uint16).numpy(), "bf16"
    elif d.dtype == torch.uint8:
        if scales is None:
            raise ValueError("fp8 gallery needs per-row scales")
        arr, dtype = d.numpy(), "fp8_e4m3"
        np.save(os.path.join(path, "scales.npy"), scales.detach().cpu().to(torch.float32).numpy())
    else:
        raise ValueError("descriptors must be bfloat16 or uint8 (e4m3 bytes)")
    labels = np.asarray(labels, dtype=np.float64)
    if labels.shape != (arr.shape[0], len(LABEL_COLUMNS)):
        raise ValueError(f"labels must be [N,{len(LABEL_COLUMNS)}] = {LABEL_COLUMNS}")
    np.save(os.path.join(path, "descriptors.npy"), arr)
    np.save(os.path.join(path, "labels.npy"), labels)
    if filenames is not None:
        with open(os.path.join(path, "filenames.txt"), "w") as f:
            f.write("\n".join(filenames))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"version": 1, "n": int(arr.shape[0]), "d": int(arr.shape[1]), "dtype": dtype,
                   "label_columns": list(LABEL_COLUMNS)}, f)
    proj_path = os.path.join(path, PROJECTION_FILE)
    if projection is not None:
        projection.save(proj_path)
    elif os.path.exists(proj_path):            # a directory written over: the old rows' projection does not describe the new ones
        os.remove(proj_path)
    fine_path = os.path.join(path, FINE_FILE)
    if fine is not None:
        np.save(fine_path, fine.detach().cpu().contiguous().view(torch.uint16).numpy())
    elif os.path.exists(fine_path):            # nor do the old fine rows
        os.remove(fine_path)
    for name, dtype, view in ((LOCAL_FILE, torch.bfloat16, torch.uint16), (LOCAL_FP8_FILE, torch.uint8, torch.uint8)):
        local_path = os.path.join(path, name)
        if local is not None and local.dtype == dtype:
            np.save(local_path, local.detach().cpu().contiguous().view(view).numpy())
        elif os.path.exists(local_path):       # nor the old local features, of either kind
            os.remove(local_path)


def device_labels(labels: np.ndarray, device: torch.device) -> torch.Tensor:
    """The label side table as ops.retrieval_pose reads it: [N, 4] float64 (latitude, longitude, angle, Region_ID) on
    `device`.  It is the FULL table, replicated on every rank (the merged top-k holds global rows): 32 MB at 1M rows."""
    labels = np.ascontiguousarray(labels, dtype=np.float64)
    if labels.ndim != 2 or labels.shape[1] != len(LABEL_COLUMNS):
        raise ValueError(f"labels must be [N,{len(LABEL_COLUMNS)}] = {LABEL_COLUMNS}")
    return torch.from_numpy(labels).to(device)


_device_labels = device_labels       # load_gallery_shard's flag of the same name shadows the function inside it


def load_gallery_shard(path: str, device: torch.device, rank: int = 0, world: int = 1,
                       device_labels: bool = False, load_fine: bool = False, load_local: bool = False) -> GalleryShard:
    """device_labels: also place the label table on `device` (GalleryShard.labels_dev), for the on-device retrieval pose.
    load_fine: also read this rank's slice of fine_descriptors.npy (GalleryShard.fine); the file must then exist.
    load_local: also read this rank's slice of local_features.npy (GalleryShard.local, bf16) or, where the directory holds
    that one, of local_features_fp8.npy (uint8); one of them must then exist."""
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    if meta.get("version") != 1:
        raise ValueError("unknown gallery format version")
    lo, hi = shard_bounds(meta["n"], rank, world)
    desc = np.load(os.path.join(path, "descriptors.npy"), mmap_mode="r")
    rows = torch.from_numpy(np.array(desc[lo:hi])).to(device)          # copy of this rank's rows only
    scales = None
    if meta["dtype"] == "bf16":
        rows = rows.view(torch.bfloat16)
    else:
        sc = np.load(os.path.join(path, "scales.npy"), mmap_mode="r")
        scales = torch.from_numpy(np.array(sc[lo:hi])).to(device)
    labels = np.load(os.path.join(path, "labels.npy"))
    labels_dev = _device_labels(labels, device) if device_labels else None
    proj_path = os.path.join(path, PROJECTION_FILE)
    projection = DescriptorProjection.load(proj_path) if os.path.exists(proj_path) else None
    fine = None
    if load_fine:
        fine_path = os.path.join(path, FINE_FILE)
        if not os.path.exists(fine_path):
            raise ValueError(f"load_fine: {path} has no {FINE_FILE}")
        arr = np.load(fine_path, mmap_mode="r")
        if arr.shape[0] != meta["n"]:
            raise ValueError(f"{FINE_FILE} has {arr.shape[0]} rows, the gallery {meta['n']}")
        fine = torch.from_numpy(np.array(arr[lo:hi])).to(device).view(torch.bfloat16)
    local = None
    if load_local:
        name = LOCAL_FILE if os.path.exists(os.path.join(path, LOCAL_FILE)) else LOCAL_FP8_FILE
        if not os.path.exists(os.path.join(path, name)):
            raise ValueError(f"load_local: {path} has no {LOCAL_FILE} and no {LOCAL_FP8_FILE}")
        arr = np.load(os.path.join(path, name), mmap_mode="r")
        if arr.ndim != 3 or arr.shape[0] != meta["n"] or arr.dtype != (np.uint16 if name == LOCAL_FILE else np.uint8):
            raise ValueError(f"{name} is {arr.dtype} {arr.shape}, the gallery has {meta['n']} rows")
        local = torch.from_numpy(np.array(arr[lo:hi])).to(device)
        local = local.view(torch.bfloat16) if name == LOCAL_FILE else local
    return GalleryShard(rows, scales, labels, meta["n"], lo, meta["dtype"], labels_dev, projection, local=local, fine=fine)


def labels_from_csv(csv_path: str) -> Tuple[np.ndarray, List[str]]:
    """Reads the reference's label CSV layout -> ([N,4] float64, filenames)."""
    import pandas as pd
    df = pd.read_csv(csv_path)
    return df[list(LABEL_COLUMNS)].to_numpy(dtype=np.float64), df["filename"].tolist()


@torch.no_grad()
def build_descriptors(extractor, image_batches: Iterable[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Runs DinoV2Salad over batches of preprocessed images -> (f32 [N,8448], bf16 [N,8448]) on the GPU."""
    f32, b16 = [], []
    for images in image_batches:
        d, d16 = extractor.features(images, want_bf16=True)
        f32.append(d), b16.append(d16)
    return torch.cat(f32), torch.cat(b16)


# ---------------------------------------------------------------------------- retrieval -> pose
def label_transfer(topk_scores: torch.Tensor, topk_idx: torch.Tensor, labels: np.ndarray, mode: str = "top1",
                   temperature: float = 0.01) -> np.ndarray:
    """Geopose from retrieval: returns [B,3] = (lat, lon, angle_deg).
    mode "top1": the best match's labels.  mode "weighted": softmax(score / temperature) over the
    k matches — weighted mean for lat/lon, weighted circular mean for the angle."""
    idx = topk_idx.detach().cpu().numpy().astype(np.int64)
    sc = topk_scores.detach().cpu().numpy().astype(np.float64)
    valid = idx >= 0
    safe = np.where(valid, idx, 0)
    lat, lon, ang = labels[safe, 0], labels[safe, 1], np.deg2rad(labels[safe, 2])
    if mode == "top1":
        return np.stack([lat[:, 0], lon[:, 0], np.rad2deg(ang[:, 0]) % 360.0], 1)
    if mode != "weighted":
        raise ValueError("mode must be 'top1' or 'weighted'")
    w = np.where(valid, np.exp((sc - sc[:, :1]) / temperature), 0.0)
    w = w / w.sum(1, keepdims=True)
    a = np.rad2deg(np.arctan2((w * np.sin(ang)).sum(1), (w * np.cos(ang)).sum(1))) % 360.0
    return np.stack([(w * lat).sum(1), (w * lon).sum(1), a], 1)


def positives_by_distance(query_latlon: np.ndarray, gallery_latlon: np.ndarray, tau: float) -> List[np.ndarray]:
    """Gallery rows within Euclidean distance tau (label units) of each query."""
    q, g = np.asarray(query_latlon, dtype=np.float64), np.asarray(gallery_latlon, dtype=np.float64)
    d2 = ((q[:, None, :] - g[None, :, :]) ** 2).sum(-1)
    return [np.nonzero(row <= tau * tau)[0] for row in d2]


def positives_by_region(query_region: np.ndarray, gallery_region: np.ndarray) -> List[np.ndarray]:
    g = np.asarray(gallery_region)
    return [np.nonzero(g == r)[0] for r in np.asarray(query_region)]


# --------------------------------------------------------------------------- gallery projection
@torch.no_grad()
def project_gallery(rows_bf16: torch.Tensor, projection: DescriptorProjection, fp8: bool = False):
    """Gallery rows bf16 [N, D] on the GPU through `projection` (include/vpr_amd_project.h) -> (rows, scales): unit rows
    bf16 [N, d] and None, or with fp8 the e4m3 bytes and per-row scales that ops.quantize_fp8_rows makes of the f32 output
    (d % 128 == 0: the e4m3 search's K-step)."""
    if fp8 and projection.d % 128 != 0:
        raise ValueError(f"project_gallery: an e4m3 gallery needs d % 128 == 0, got d = {projection.d}")
    if not fp8:
        return projection.apply(rows_bf16), None
    P, c = projection.operands(rows_bf16.device)
    N = rows_bf16.shape[0]
    q = torch.empty((N, projection.d), dtype=torch.uint8, device=rows_bf16.device)
    sc = torch.empty((N,), dtype=torch.float32, device=rows_bf16.device)
    for lo in range(0, N, ops.PROJECT_CHUNK_ROWS):                 # the f32 rows exist one chunk at a time
        f32, _ = ops.project_rows(rows_bf16[lo:lo + ops.PROJECT_CHUNK_ROWS], P, c, True, want_f32=True, want_bf16=False)
        q[lo:lo + ops.PROJECT_CHUNK_ROWS], sc[lo:lo + ops.PROJECT_CHUNK_ROWS] = ops.quantize_fp8_rows(f32)
    return q, sc


# ------------------------------------------------------------------------- gallery augmentation
@torch.no_grad()
def augment_gallery(sharded: ShardedGallery, n_use: int, alpha: float = 3.0, batch: int = 512):
    """Database-side augmentation (DBA): every gallery row becomes the L2-normalised sum of score^alpha * row over its n_use
    best matches in the WHOLE gallery — the row itself is the first of them (it finds itself at rank 0), so the query term
    is off (q_weight = 0) and n_use counts the row.  Returns this rank's new rows in the shard's own format: bf16
    [n_local, D], or (e4m3 bytes [n_local, D], scales [n_local]) through quantize_fp8_rows.  Run once, offline; search the
    result like any gallery.
    Every rank runs ceil(ceil(N / world) / batch) iterations of {gather, search, expand}, so a sharded gallery stays in
    lockstep; a short (or empty) last batch is padded with copies of the rank's row 0, whose results are dropped — not with
    zero rows, whose all-tied scores would count as uncertified searches."""
    rows, scales = sharded.rows, sharded.scales
    n_local, D = rows.shape
    if n_local < 1:
        raise ValueError("augment_gallery: this rank's shard is empty")
    world = sharded.world if sharded.collective else 1
    per_rank = -(-sharded.n_total // max(sharded.world, 1))
    out = torch.empty((n_local, D), dtype=torch.bfloat16, device=rows.device)
    for it in range(-(-per_rank // batch)):
        lo, hi = min(it * batch, n_local), min((it + 1) * batch, n_local)
        sel = torch.zeros(batch, dtype=torch.long, device=rows.device)
        sel[:hi - lo] = torch.arange(lo, hi, device=rows.device)
        q = rows[sel]
        if scales is not None:
            q = (q.view(torch.float8_e4m3fn).float() * scales[sel, None]).to(torch.bfloat16)
        q_all = sharded.gather_queries(q.contiguous())
        v, i = sharded.search(q_all, n_use)
        e = sharded.expand(q_all, v, i, n_use, alpha, 0.0)
        first = sharded.rank * batch if world > 1 else 0
        out[lo:hi] = e[first:first + hi - lo]
    if scales is None:
        return out
    return ops.quantize_fp8_rows(out.float())


# ------------------------------------------------------------------- hipGraph-captured retrieval
class GraphedLocalTopK:
    """Local shard search captured once into a HIP graph and replayed per batch (BASELINE config 5:
    'hipGraph-captured per-batch retrieval').  Static shapes: B queries, k, this shard.  The
    kernels take only stream-ordered arguments and a pre-allocated workspace, so the capture holds
    5 kernel nodes (scores, select x2, rescore, order) and replay costs one launch."""

    def __init__(self, shard: GalleryShard, batch: int, k: int):
        self.shard, self.k = shard, k
        dev = shard.rows.device
        D = shard.rows.shape[1]
        self.fp8 = shard.dtype != "bf16"
        self.q = torch.zeros((batch, D), dtype=shard.rows.dtype, device=dev)
        self.q_scale = torch.ones((batch,), dtype=torch.float32, device=dev) if self.fp8 else None
        self.ws = ops.knn_workspace(batch, shard.rows.shape[0], D, k, dev)
        self._captured = _streams.Captured(self._run, dev, 1)
        self.vals, self.idx = self._captured.out

    def close(self) -> None:
        """Destroy the graph and forget what the package keyed by its private stream (also runs when it is collected)."""
        self._captured.close()

    def _run(self):
        s = self.shard
        if self.fp8:
            return ops.knn_topk_fp8(self.q, self.q_scale, s.rows, s.scales, self.k, s.index_base, self.ws)
        return ops.knn_topk(self.q, s.rows, self.k, s.index_base, self.ws)

    def __call__(self, q: torch.Tensor, q_scale: Optional[torch.Tensor] = None):
        self.q.copy_(q)
        if self.fp8:
            self.q_scale.copy_(q_scale)
        self._captured.graph.replay()
        return self.vals, self.idx


def sharded_gallery_from(shard: GalleryShard, rank: int = 0, world: int = 1, group=None) -> ShardedGallery:
    """A loaded shard (bf16 rows, or e4m3 bytes + per-row scales) as the distributed search object."""
    return ShardedGallery(shard.rows, shard.n_total, rank, world, group=group, scales=shard.scales,
                          projection=shard.projection, fine_rows=shard.fine, local_feats=shard.local)
