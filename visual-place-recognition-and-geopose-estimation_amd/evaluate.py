"""Drop-in evaluation entry points: same function name, arguments and printed/returned quantities as
the reference's validation scripts, running on the MI355X path.

  calculate_validation_scores(checkpoint_path, val_csv_path, image_dir)
      dinov2salad/dinov2salad_validation.py:55-116   (DINOv2+SALAD descriptor -> MLP head -> lat/lon)
  calculate_swin_validation_scores(checkpoint_path, val_csv_path, image_dir, preds_csv)
      swin_transformer/swin_validation.py:48-134     (Swin pooler + Linear head, ID-sorted preds.csv)

What differs from the reference loop: images are decoded on the host (PIL, by a thread
pool running a few batches ahead into pinned buffers: vpr_amd.loader) but resized / normalised on the
GPU (vpr_amd.preprocess, PIL-exact), batches stay on the device until
the end (one D2H copy instead of one per batch), the model objects are passed in or built from a
state dict instead of being fetched by name (torch.hub / from_pretrained need the network), and
the scaler is a LatLonScaler (JSON or the campus constants) instead of a joblib pickle.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import pandas as pd
import torch
from PIL import Image

from . import postproc, reports
from .graphed import GraphedForward
from .loader import ImageBatchLoader
from .modules import DINOv2RegressionModel, DinoV2Salad, load_reference_checkpoint
from .preprocess import HALF_MEAN, HALF_STD, IMAGENET_MEAN, IMAGENET_STD, ResizeNormalize


def _existing_rows(val_csv_path: str, image_dir: str) -> pd.DataFrame:
    val_df = pd.read_csv(val_csv_path)
    filtered = val_df[val_df["filename"].apply(lambda x: os.path.exists(os.path.join(image_dir, x)))]
    if len(val_df) != len(filtered):
        print(f"Warning: {len(val_df) - len(filtered)} images listed in the validation CSV were not found in the image directory.")
    return filtered.reset_index(drop=True)


def _graphed(model, dev: torch.device):
    """The model forward as one HIP-graph replay per batch (graphed.GraphedForward; a forward that cannot be captured
    falls back to the eager call by itself); the model itself on a CPU device."""
    return GraphedForward(model) if dev.type == "cuda" else model


def _batches(image_dir: str, filenames, batch_size: int, device):
    """(row indices, uint8 [B,H,W,3] device tensor) per batch, decode and host-to-device copy running ahead of the
    consumer (loader.ImageBatchLoader: same bytes, batches and order as the serial PIL loop it replaces)."""
    for idxs, _, u8 in ImageBatchLoader(image_dir, filenames, batch_size, device):
        yield idxs, u8


@torch.no_grad()
def calculate_validation_scores(checkpoint_path: str, val_csv_path: str, image_dir: str, *,
                                base_model: Optional[DinoV2Salad] = None, arch: str = "vit_base",
                                scaler: Optional[postproc.LatLonScaler] = None, batch_size: int = 16,
                                device: str = "cuda", verbose: bool = True, graph: bool = True,
                                dtype: torch.dtype = torch.bfloat16) -> dict:
    """dtype: torch.bfloat16 (default: the MI355X path — HIP backbone kernels, bf16-operand SALAD) or torch.float32 =
    the reference's own precision (dinov2salad_validation.py:65-66,80-81: `.cuda()`, no cast): f32 weights, the f32
    PyTorch block loop (erf GELU, f32 LayerNorm / attention), the f32-accurate SALAD aggregation
    (vpr_salad_aggregate_f32) and the f32 head — the yardstick the bf16 path is held to (tests/test_precision_gpu.py)."""
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("dtype must be torch.bfloat16 or torch.float32")
    df = _existing_rows(val_csv_path, image_dir)
    dev = torch.device(device)
    if base_model is None:
        base_model = DinoV2Salad(arch)
    base_model = base_model.to(dev).to(dtype).eval()
    model = DINOv2RegressionModel(base_model).to(dev)
    load_reference_checkpoint(model, checkpoint_path)            # checkpoint['model_state_dict'] or a bare state dict
    model.eval()
    if hasattr(getattr(base_model, "backbone", None), "fold_layerscale") and dtype == torch.bfloat16:
        base_model.backbone.gelu = "erf"                         # the checkpoint was trained behind nn.GELU(): exact form, not the GEMM epilogue's tanh
        base_model.backbone.fold_layerscale()                    # AFTER the load (a load un-folds): LayerScale into proj / fc2, enables the HIP backbone path
    if dtype == torch.bfloat16:
        base_model.aggregator.pack()
    else:
        base_model.aggregator.pack_f32()
    scaler = scaler or postproc.LatLonScaler.campus()
    prep = ResizeNormalize(224, "bilinear", HALF_MEAN, HALF_STD, dtype)            # validation.py:18-22

    filenames = df["filename"].tolist()
    preds_std = torch.empty((len(filenames), 2), dtype=torch.float32, device=dev)
    # one HIP-graph launch per batch instead of ~300 kernel launches: the host (and its GIL) belongs to the decode threads
    fwd = GraphedForward(model) if graph and dev.type == "cuda" else model
    for idxs, u8 in _batches(image_dir, filenames, batch_size, dev):
        x = prep(u8)
        preds_std[torch.tensor(idxs, device=dev)] = fwd(x)
    all_preds = scaler.inverse_transform(preds_std.cpu().numpy())                  # fp32 in -> fp32 out (:84)
    all_targets = df[["latitude", "longitude"]].to_numpy(dtype=np.float32)
    final_loss = postproc.final_loss(all_preds, all_targets)                        # :101
    if verbose:
        print(all_preds.shape, all_targets.shape)
        print(f"final_loss: {final_loss}")
        print("\nSample Predictions (Original Scale):")
        for i in range(min(5, len(all_preds))):
            (pl, po), (tl, to) = all_preds[i], all_targets[i]
            print(f"Prediction: (Lat: {pl:.6f}, Lon: {po:.6f}), True: (Lat: {tl:.6f}, Lon: {to:.6f}), "
                  f"Error: (Lat: {abs(pl - tl):.6f}, Lon: {abs(po - to):.6f})")
    return {"final_loss": final_loss, "preds": all_preds, "targets": all_targets, "preds_standardised": preds_std.cpu().numpy(),
            "filenames": filenames}


@torch.no_grad()
def calculate_swin_validation_scores(model, val_csv_path: str, image_dir: str, preds_csv: Optional[str] = None, *,
                                     checkpoint_path: Optional[str] = None, scaler: Optional[postproc.LatLonScaler] = None,
                                     batch_size: int = 16, device: str = "cuda", verbose: bool = True, graph: bool = True) -> dict:
    """`model`: a vpr_amd.modules.SwinRegressionModel (backbone object inside).  Preprocessing follows the
    HF Swin image processor: bicubic resize to 224, /255, ImageNet mean/std."""
    df = _existing_rows(val_csv_path, image_dir)
    dev = torch.device(device)
    model = model.to(dev).eval()
    if checkpoint_path:
        load_reference_checkpoint(model, checkpoint_path)
    scaler = scaler or postproc.LatLonScaler.campus()
    prep = ResizeNormalize(224, "bicubic", IMAGENET_MEAN, IMAGENET_STD, torch.float32)
    filenames = df["filename"].tolist()
    preds_std = torch.empty((len(filenames), 2), dtype=torch.float32, device=dev)
    fwd = _graphed(model, dev)             # Swin-T at batch 16 is launch-bound: the graph replay is 2x the eager forward
    for idxs, u8 in _batches(image_dir, filenames, batch_size, dev):
        preds_std[torch.tensor(idxs, device=dev)] = fwd(prep(u8))
    all_preds = scaler.inverse_transform(preds_std.cpu().numpy())
    all_targets = df[["latitude", "longitude"]].to_numpy(dtype=np.float32)
    final_loss = postproc.final_loss(all_preds, all_targets)                        # swin_validation.py:100
    if verbose:
        print(all_preds.shape)
        print(all_targets.shape)
        print(f"final_loss: {final_loss}")
    if preds_csv:
        reports.write_id_sorted_preds(preds_csv, filenames, all_preds)              # :121-134
        if verbose:
            print("Saved predictions to preds.csv")
    return {"final_loss": final_loss, "preds": all_preds, "targets": all_targets, "filenames": filenames}


# ---------------------------------------------------------------------------------------------------------------
# Swin-Base validation + test-set entry point: swin_transformer/val_and_test_swin_2.py
IMAGE_EXTENSIONS = ["*.jpg", "*.jpeg", "*.png", "*.bmp", "*.gif", "*.JPEG"]        # :44


def _loadable(path: str, decode: bool = False) -> bool:
    """The reference's per-file check (CampusDataset :73-90 `img.verify()`, TestImageDataset :150-155 returning None
    for the collate functions :179-195 to drop): a file that PIL cannot open is skipped with a message, not fatal.
    decode=True (test split): the full decode is attempted as well — the reference's TestImageDataset.__getitem__
    catches DECODE errors too (a truncated JPEG passes verify() and fails in convert('RGB')) and drops the item,
    where a verify()-only filter would let the file through and abort the run inside the batch loader."""
    try:
        with Image.open(path) as im:
            im.verify()
        if decode:
            with Image.open(path) as im:                     # verify() leaves the object unusable: reopen
                im.convert("RGB")
        return True
    except Exception as e:                                   # FileNotFoundError, UnidentifiedImageError, OSError, ...
        print(f"Warning: Skipping invalid/corrupt image file: {path} ({e})")
        return False


@torch.no_grad()
def _predict_files(model, image_dir: str, filenames, prep, scaler, batch_size: int, dev) -> np.ndarray:
    preds_std = torch.empty((len(filenames), 2), dtype=torch.float32, device=dev)
    fwd = _graphed(model, dev)
    for idxs, u8 in _batches(image_dir, filenames, batch_size, dev):
        preds_std[torch.tensor(idxs, device=dev)] = fwd(prep(u8))
    return scaler.inverse_transform(preds_std.cpu().numpy())


@torch.no_grad()
def validate_and_test_swin(model, val_csv_path: str, val_image_dir: str, test_image_dir: Optional[str] = None,
                           save_dir: Optional[str] = None, *, checkpoint_path: Optional[str] = None,
                           scaler: Optional[postproc.LatLonScaler] = None, image_size: int = 384, batch_size: int = 32,
                           device: str = "cuda", verbose: bool = True) -> dict:
    """`model`: a vpr_amd.modules.SwinMLPRegressionModel (reference class `SwinRegressionModel`, :164-177).
    Validation split (:247-293): rows whose image is missing or unreadable are skipped with a warning, predictions are
    de-normalised, MSE / RMSE / MAE / MAE-lat / MAE-lon are printed in the reference's format and
    `validation_predictions.csv` is written ('%.6f').  Test split (:296-342, when `test_image_dir` exists): every image
    file of IMAGE_EXTENSIONS in basename order, unreadable ones dropped, `test_predictions_sorted.csv` sorted by
    filename.  Preprocessing = the HF Swin image processor the script builds (:199): bicubic resize to `image_size`
    (384 for swin-base-patch4-window12-384, :39-40), /255, ImageNet mean/std — on the GPU, PIL-exact."""
    import glob
    dev = torch.device(device)
    model = model.to(dev).eval()
    if checkpoint_path:
        load_reference_checkpoint(model, checkpoint_path)                         # bare state dict, :231
    scaler = scaler or postproc.LatLonScaler.campus()
    prep = ResizeNormalize(image_size, "bicubic", IMAGENET_MEAN, IMAGENET_STD, torch.float32)
    out = {}

    val_df = pd.read_csv(val_csv_path)
    keep = []
    for i, f in enumerate(val_df["filename"]):
        p = os.path.join(val_image_dir, f)
        if not os.path.isfile(p):
            print(f"Warning: Image file not found and skipped: {p}")              # :92
        elif _loadable(p):
            keep.append(i)
    if not keep:
        raise ValueError("No valid image files found for the provided validation dataframe and image directory.")   # :95
    vdf = val_df.iloc[keep].reset_index(drop=True)
    names = vdf["filename"].tolist()
    preds = _predict_files(model, val_image_dir, names, prep, scaler, batch_size, dev)
    targets = vdf[["latitude", "longitude"]].to_numpy(dtype=np.float32)           # the script's float32 target tensors (:120)
    out.update(val_filenames=names, val_preds=preds, val_targets=targets, metrics=postproc.regression_metrics(preds, targets))
    if verbose:
        print("\n" + reports.format_metrics(preds, targets))
        print("-" * 30)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
        path = os.path.join(save_dir, "validation_predictions.csv")              # :35
        reports.write_validation_csv(path, names, targets, preds)
        if verbose:
            print(f"Successfully saved validation prediction results to: {path}")

    if test_image_dir is None or not os.path.isdir(test_image_dir):
        if verbose:
            print(f"Warning: Test image directory not found: {test_image_dir}. Skipping test set prediction.")   # :23
        return out
    paths = []
    for ext in IMAGE_EXTENSIONS:
        paths.extend(glob.glob(os.path.join(test_image_dir, ext)))
    paths.sort(key=lambda p: os.path.basename(p))                                 # :133
    if not paths:
        print(f"No image files ({', '.join(IMAGE_EXTENSIONS)}) found in {test_image_dir}")                       # :136
        return out
    tnames = [os.path.basename(p) for p in paths if _loadable(p, decode=True)]    # None items dropped by the collate (:189-191)
    if not tnames:
        print("No test predictions were made. Check test data directory and image files.")                       # :321
        return out
    tpreds = _predict_files(model, test_image_dir, tnames, prep, scaler, batch_size, dev)
    out.update(test_filenames=tnames, test_preds=tpreds)
    if save_dir:
        path = os.path.join(save_dir, "test_predictions_sorted.csv")              # :36
        reports.write_test_csv(path, tnames, tpreds)
        if verbose:
            print(f"Successfully saved sorted test prediction results to: {path}")
    return out


# ---------------------------------------------------------------------------------------------------------------
# Angle (sin/cos head) validation: loop, metric, prints and CSV layout of angle_prediction/efficient_net/
# validation_script.py:162-221 / test_script.py:255-276 — the reference's only angle-validation callers.  Their
# backbone (EfficientNet-B0) is out of scope; the loop is backbone-agnostic and here serves the Swin / DINOv2 sin/cos
# models of vpr_amd.modules (output order [sin, cos]; order="cossin" decodes the EfficientNet convention).
@torch.no_grad()
def calculate_angle_validation_scores(model, val_csv_path: str, image_dir: str, results_csv: Optional[str] = None, *,
                                      test_image_dir: Optional[str] = None, test_csv: Optional[str] = None,
                                      checkpoint_path: Optional[str] = None, order: str = "sincos", image_size: int = 224,
                                      batch_size: int = 32, device: str = "cuda", verbose: bool = True, prep=None) -> dict:
    """`model`: pixel_values -> [B, 2] (SwinSinCosRegressionModel, SwinAngleRegressorSinCos, DinoV2AngleRegressorSinCos).
    Decoding as validation_script.py:179-182: atan2 -> degrees -> (+360) % 360; error min(d, 360 - d) (:188-189); MAAE =
    mean over the processed samples (:200-206).  Preprocessing default = the HF Swin processor (bicubic resize to
    `image_size`, /255, ImageNet statistics) on the GPU; pass `prep` for another one (dtype must suit the model)."""
    import glob
    if order not in ("sincos", "cossin"):
        raise ValueError("order must be 'sincos' or 'cossin'")
    dev = torch.device(device)
    model = model.to(dev).eval()
    if checkpoint_path:
        load_reference_checkpoint(model, checkpoint_path)
    prep = prep or ResizeNormalize(image_size, "bicubic", IMAGENET_MEAN, IMAGENET_STD, torch.float32)

    def predict_deg(directory, names):
        out = torch.empty((len(names), 2), dtype=torch.float32, device=dev)
        fwd = _graphed(model, dev)
        for idxs, u8 in _batches(directory, names, batch_size, dev):
            out[torch.tensor(idxs, device=dev)] = fwd(prep(u8)).float()
        s, c = (out[:, 0], out[:, 1]) if order == "sincos" else (out[:, 1], out[:, 0])
        return ((torch.rad2deg(torch.atan2(s, c)) + 360.0) % 360.0).cpu().numpy()            # f32, as the script's tensors

    df = _existing_rows(val_csv_path, image_dir)
    names = df["filename"].tolist()
    pred = predict_deg(image_dir, names)
    true = df["angle"].to_numpy()
    diff = np.abs(pred - true.astype(np.float32))
    err = np.minimum(diff, np.float32(360.0) - diff)
    maae = float(err.astype(np.float64).sum() / max(len(names), 1))
    if verbose:
        print("\n===================================")
        print("Prediction complete.")
        print(f"Total validation samples processed: {len(names)}")
        print(f"Mean Absolute Angular Error (MAAE): {maae:.4f} degrees")
        print("===================================")
    res = {"filenames": names, "pred_deg": pred, "true_deg": true, "angular_error": err, "maae": maae}
    if results_csv:
        reports.write_angle_validation_csv(results_csv, names, true, pred)
        if verbose:
            print(f"Prediction results saved to: {results_csv}")
    if test_image_dir and os.path.isdir(test_image_dir):
        paths = []
        for ext in IMAGE_EXTENSIONS:
            paths.extend(glob.glob(os.path.join(test_image_dir, ext)))
        tnames = sorted(os.path.basename(p) for p in paths if _loadable(p, decode=True))
        if tnames:
            tpred = predict_deg(test_image_dir, tnames)
            res.update(test_filenames=tnames, test_pred_deg=tpred)
            if test_csv:
                reports.write_angle_test_csv(test_csv, tnames, tpred)
    return res


# ---------------------------------------------------------------------------------------------------------------
# Retrieval-based geopose (north-star stage; the reference has no retrieval — SURVEY fact 3, §8f-2): the same CSV + image
# directory conventions as the validation scripts, with the gallery built from the training split.
def _check_grid(extractor, image_size: int) -> None:
    """The extractor's position grid is built for one image size (DinoV2Salad(arch, img_size)): refuse another one here, by
    name, before any device work — not as a shape error inside the position-embedding add."""
    bb = extractor.backbone
    got = (int(image_size) // bb.patch) ** 2
    if got != bb.num_patches:
        raise ValueError(f"image_size={image_size} gives {got} patch tokens per image (patch {bb.patch}), but the extractor was built "
                         f"for {bb.num_patches}: construct it with DinoV2Salad(arch, img_size={image_size})")


@torch.no_grad()
def build_gallery_from_images(extractor: DinoV2Salad, csv_path: str, image_dir: str, out_dir: str, *, fp8: bool = False,
                              batch_size: int = 64, device: str = "cuda", image_size: int = 224, graph: bool = True,
                              projection=None, whiten: bool = True, keep_fine: bool = False, keep_local=False,
                              local_hires: bool = False) -> int:
    """labels CSV (`filename,timestamp,latitude,longitude,angle,Region_ID`, cleaned_dataset_files/labels_train.csv:1) +
    images -> on-disk gallery (gallery.save_gallery: bf16 rows, or e4m3 rows + per-row scales with fp8=True).
    Preprocessing = the DINOv2+SALAD validation transform (dinov2salad_validation.py:18-22).  Returns the row count.
    image_size: the size the extractor was built for (DinoV2Salad(arch, img_size=322) with image_size=322); ValueError otherwise.
    projection: None, a projection.DescriptorProjection, or an int d = fit PCA (whiten: with whitening) on this gallery's own
    descriptors (projection.fit_projection) — the rows are projected to d columns on the device (gallery.project_gallery)
    and the projection is saved with the gallery, where calculate_retrieval_scores finds it.
    keep_fine: an e4m3 or projected gallery also keeps the bf16 full descriptors (fine_descriptors.npy), the second tier of
    calculate_retrieval_scores(rerank=); a plain bf16 gallery's rows are those descriptors already, and nothing is added.
    keep_local: the gallery also keeps every image's local features (local_features.npy: [N, n, 128] bf16 from the same
    backbone pass, DinoV2Salad.features(want_local=True); at most 256 patch tokens), what
    calculate_retrieval_scores(local_rerank=) matches against.  keep_local="fp8": their e4m3 store instead
    (local_features_fp8.npy: [N, n, 128] uint8, features(want_local="fp8"); half the bytes — 32 KB per image at n = 256).
    local_hires (with keep_local): an extractor of 257 to 1369 patch tokens is accepted (features(hires=True); img_size 322 to
    518).  The files keep their format, only n differs: 135 KB bf16 or 68 KB e4m3 per image at 322 px (n = 529), 350 KB or
    175 KB at 518 px (n = 1369)."""
    from . import gallery as G, ops
    if keep_local not in (False, True, "fp8"):
        raise ValueError(f"build_gallery_from_images: keep_local must be False, True or 'fp8', got {keep_local!r}")
    _check_grid(extractor, image_size)
    dev = torch.device(device)
    extractor = extractor.to(dev).to(torch.bfloat16).eval()
    df = _existing_rows(csv_path, image_dir)
    names = df["filename"].tolist()
    prep = ResizeNormalize(image_size, "bilinear", HALF_MEAN, HALF_STD, torch.bfloat16)
    desc = torch.empty((len(names), 8448), dtype=torch.float32, device=dev)
    local = None
    if keep_local:
        features = lambda x: extractor.features(x, want_local=keep_local, hires=local_hires)
        local = torch.empty((len(names), extractor.backbone.num_patches, extractor.aggregator.cluster_dim),
                            dtype=torch.uint8 if keep_local == "fp8" else torch.bfloat16, device=dev)
        fwd = GraphedForward(features, module=extractor) if graph and dev.type == "cuda" else features
    else:
        fwd = GraphedForward(extractor) if graph and dev.type == "cuda" else extractor
    for idxs, u8 in _batches(image_dir, names, batch_size, dev):
        sel = torch.tensor(idxs, device=dev)
        if keep_local:
            desc[sel], local[sel] = fwd(prep(u8))
        else:
            desc[sel] = fwd(prep(u8))
    labels = df[list(G.LABEL_COLUMNS)].to_numpy(dtype=np.float64)
    fine = desc.to(torch.bfloat16) if keep_fine and (fp8 or projection is not None) else None
    if projection is not None:
        from .projection import fit_projection
        d16 = desc.to(torch.bfloat16)
        if isinstance(projection, int):
            projection = fit_projection(d16, projection, whiten=whiten)
        rows, scales = G.project_gallery(d16, projection, fp8=fp8)
        G.save_gallery(out_dir, rows, labels, scales=scales, filenames=names, projection=projection, fine=fine, local=local)
    elif fp8:
        rows, scales = ops.quantize_fp8_rows(desc)
        G.save_gallery(out_dir, rows, labels, scales=scales, filenames=names, fine=fine, local=local)
    else:
        G.save_gallery(out_dir, desc.to(torch.bfloat16), labels, filenames=names, local=local)
    return len(names)


def retrieval_metrics(vals: torch.Tensor, idx: torch.Tensor, labels: np.ndarray, targets: np.ndarray, regions: np.ndarray,
                      angles: np.ndarray, tau: float, mode: str, on_device: bool = False, temperature: float = 0.01) -> dict:
    """The metric block of calculate_retrieval_scores from the top-k lists vals / idx [Q, k] (device), the gallery's label
    table [N, 4] and the queries' targets [Q, 2] (lat, lon), Region_IDs [Q] and angles [Q] (degrees).
    on_device=False: gallery.label_transfer and recall_at_k over positives_by_distance / positives_by_region on the host
    ([Q, N] intermediates).  on_device=True: pose and both first-hit ranks from ONE torch.ops.vpr.retrieval_pose call over
    all Q rows; nothing of size [Q, N] is built, and the recalls are recall_from_first_hit of those ranks (the same
    numbers).  The label table and the queries' (lat, lon, Region_ID) are copied to the device for the call."""
    from . import gallery as G
    kk = idx.shape[1]
    targets = np.asarray(targets, dtype=np.float64)
    if on_device:
        from . import torch_ops  # noqa: F401  registers torch.ops.vpr.*
        q = np.concatenate([targets, np.asarray(regions, dtype=np.float64)[:, None]], axis=1)
        pose_d, _, hit_tau, hit_region = torch.ops.vpr.retrieval_pose(
            vals.contiguous(), idx.contiguous(), G.device_labels(labels, vals.device), mode, temperature,
            torch.from_numpy(q).to(vals.device), float(tau), None)
        pose, ht, hr = pose_d.cpu().numpy(), hit_tau.cpu().numpy(), hit_region.cpu().numpy()
        r1_tau, rk_tau = postproc.recall_from_first_hit(ht, 1), postproc.recall_from_first_hit(ht, kk)
        r1_region = postproc.recall_from_first_hit(hr, 1)
        top = idx.cpu().numpy()
    else:
        pose = G.label_transfer(vals, idx, labels, mode=mode, temperature=temperature)
        top = idx.cpu().numpy()
        pos_d = G.positives_by_distance(targets, labels[:, :2], tau)
        pos_r = G.positives_by_region(regions, labels[:, 3])
        r1_tau, rk_tau = postproc.recall_at_k(top[:, :1], pos_d), postproc.recall_at_k(top, pos_d)
        r1_region = postproc.recall_at_k(top[:, :1], pos_r)
    return {"topk_scores": vals.cpu().numpy(), "topk_indices": top, "pose": pose,
            "final_loss": postproc.final_loss(pose[:, :2], targets),
            "maae": postproc.mean_absolute_angular_error(pose[:, 2], np.asarray(angles, dtype=np.float64)),
            "recall_at_1_tau": r1_tau, f"recall_at_{kk}_tau": rk_tau, "recall_at_1_region": r1_region}


@torch.no_grad()
def calculate_retrieval_scores(extractor: DinoV2Salad, gallery_dir: str, val_csv_path: str, image_dir: str, *, k: int = 10,
                               tau: float = 25.0, mode: str = "top1", batch_size: int = 64, device: str = "cuda", graph: bool = True,
                               image_size: int = 224, rank: int = 0, world: int = 1, group=None, verbose: bool = True,
                               on_device: bool = False, query_expansion=None, rerank: Optional[int] = None,
                               local_rerank: Optional[int] = None, min_sim: float = 0.0, local_hires: bool = False,
                               spatial_tol: Optional[int] = None, spatial_model: str = "shift") -> dict:
    """Validation split through descriptor -> sharded cosine top-k -> label transfer:
      pose      (lat, lon, angle) of the best match, or the softmax-weighted mean of the k matches (gallery.label_transfer);
      final_loss on lat/lon with the validation scripts' formula (dinov2salad_validation.py:101), MAAE on the angle
                (swin_angle_finetuning_gemini.py:131-146);
      Recall@1 / Recall@k with positives = gallery rows within `tau` label units of the query (Euclidean on the projected
                lat/lon) and, separately, rows of the same Region_ID.
    With world > 1 every rank runs this with its shard (load_gallery_shard) and its share of the queries is gathered by
    ShardedGallery.search_local_queries; the metrics are then those of this rank's queries.
    on_device: the metrics come from the k neighbours alone, on the GPU (retrieval_metrics) — for galleries where the host
    path's [Q, N] arrays do not fit.
    query_expansion: None, or (n_use, alpha) / a dict with n_use and any of alpha, q_weight, rounds: every batch is searched,
    expanded on the device (ShardedGallery.search_expanded) and searched again; the metrics are those of the last search.
    A gallery saved with a projection (projection.npz) has every query batch projected on the device before its search.
    rerank (kc): two-tier retrieval — every (last) search yields kc coarse candidates, re-ranked to k on the gallery's fine
    descriptors (fine_descriptors.npy, build_gallery_from_images(keep_fine=True); a plain bf16 gallery is its own fine tier)
    with the batch's bf16 descriptors as fine queries (ShardedGallery.search_reranked); topk_scores are then fine scores.
    local_rerank (kc): local-feature re-ranking — every search yields kc coarse candidates, re-ranked to k by the mutual-
    nearest-neighbour matches (similarity >= min_sim) between the query's and the candidates' patch features
    (local_features.npy, build_gallery_from_images(keep_local=True); ShardedGallery.search_local_reranked); topk_scores are
    then local scores.  Not together with rerank or query_expansion.  A gallery that keeps the e4m3 store instead
    (local_features_fp8.npy, keep_local="fp8") is matched in that form: the queries' features are features(want_local="fp8").
    local_hires (with local_rerank): the gallery's and the queries' images hold up to 1369 patch tokens (a gallery built with
    build_gallery_from_images(local_hires=True); features(hires=True) and ShardedGallery(local_hires=True)); per image the
    gallery then keeps 135 KB bf16 or 68 KB e4m3 at 322 px, 350 KB or 175 KB at 518 px.
    spatial_tol (with local_rerank; 0..8): the matches are verified spatially (include/vpr_amd_spatial.h;
    ShardedGallery.search_local_reranked(spatial_tol=)) on the patch grid of `image_size`, image_size // 14 wide on both sides;
    topk_scores are then the verified scores.  spatial_model (with spatial_tol): "shift", or "similarity" for the verification
    under one scale, rotation and shift (include/vpr_amd_similarity.h), as search_local_reranked takes it."""
    from . import gallery as G
    from .retrieval import ShardedGallery, _spatial_model
    _spatial_model("calculate_retrieval_scores", spatial_model, spatial_tol)
    _check_grid(extractor, image_size)
    if spatial_tol is not None and local_rerank is None:
        raise ValueError("calculate_retrieval_scores: spatial_tol verifies the matches of local_rerank; name its kc")
    dev = torch.device(device)
    extractor = extractor.to(dev).to(torch.bfloat16).eval()
    if local_rerank is not None and (rerank is not None or query_expansion is not None):
        raise ValueError("calculate_retrieval_scores: local_rerank combines neither with rerank nor with query_expansion")
    if local_rerank is not None and not any(os.path.exists(os.path.join(gallery_dir, f)) for f in (G.LOCAL_FILE, G.LOCAL_FP8_FILE)):
        raise ValueError(f"local_rerank: {gallery_dir} has no {G.LOCAL_FILE} (build_gallery_from_images(keep_local=True)) "
                         f"and no {G.LOCAL_FP8_FILE} (keep_local='fp8')")
    has_fine = os.path.exists(os.path.join(gallery_dir, G.FINE_FILE))
    shard = G.load_gallery_shard(gallery_dir, dev, rank, world, load_fine=rerank is not None and has_fine,
                                 load_local=local_rerank is not None)
    fine = shard.fine
    if rerank is not None and fine is None:
        if shard.dtype != "bf16" or shard.projection is not None:
            raise ValueError(f"rerank: {gallery_dir} has no {G.FINE_FILE} (build_gallery_from_images(keep_fine=True))")
        fine = shard.rows
    # offline evaluation: unconditionally exact neighbours (queries the device certificate flags are re-run on f64 scores)
    sg = ShardedGallery(shard.rows, shard.n_total, rank, world, group=group, scales=shard.scales, exact_fallback=True,
                        projection=shard.projection, fine_rows=fine, local_feats=shard.local,
                        local_hires=local_hires, local_grid=None if spatial_tol is None else image_size // 14)
    df = _existing_rows(val_csv_path, image_dir)
    names = df["filename"].tolist()
    prep = ResizeNormalize(image_size, "bilinear", HALF_MEAN, HALF_STD, torch.bfloat16)
    kk = min(k, shard.n_total)
    vals = torch.empty((len(names), kk), dtype=torch.float32, device=dev)
    idx = torch.empty((len(names), kk), dtype=torch.int32, device=dev)
    want_local = local_rerank is not None and ("fp8" if shard.local.dtype == torch.uint8 else True)
    features = lambda x: extractor.features(x, want_bf16=True, want_local=want_local, hires=local_hires)
    fwd = GraphedForward(features, module=extractor) if graph and dev.type == "cuda" else features
    two_tier = {} if rerank is None else {"rerank": int(rerank)}     # named only when asked for
    for idxs, u8 in _batches(image_dir, names, batch_size, dev):
        _, d16, *feats = fwd(prep(u8))
        if local_rerank is not None:
            two_tier = {"local_rerank": int(local_rerank), "q_local_feats": feats[0], "min_sim": float(min_sim)}
            if spatial_tol is not None:
                two_tier["spatial_tol"] = int(spatial_tol)
                if spatial_model != "shift":                 # the default names nothing: the call is the one it always was
                    two_tier["spatial_model"] = spatial_model
        v, i = sg.search_local_queries(d16, kk, query_expansion, **two_tier)
        sel = torch.tensor(idxs, device=dev)
        vals[sel], idx[sel] = v, i
    res = {"filenames": names}
    res.update(retrieval_metrics(vals, idx, shard.labels, df[["latitude", "longitude"]].to_numpy(dtype=np.float64),
                                 df["Region_ID"].to_numpy(), df["angle"].to_numpy(dtype=np.float64), tau, mode,
                                 on_device=on_device))
    res["uncertified_queries"] = sg.uncertified_queries()        # flagged on the device (and re-run exactly), for the record
    if verbose:
        print(f"final_loss: {res['final_loss']}")
        print(f"Mean Absolute Angular Error (MAAE): {res['maae']:.4f} degrees")
        print(f"Recall@1 (tau={tau}): {res['recall_at_1_tau']:.4f}  Recall@{kk}: {res[f'recall_at_{kk}_tau']:.4f}  "
              f"Recall@1 (Region_ID): {res['recall_at_1_region']:.4f}")
    return res
