"""Host-side mirror of the reference's model interface, with the hot ops running as HIP kernels.

Same class names, constructor arguments, sub-module names and state-dict keys as the reference,
so its checkpoints load and its evaluation loops run unchanged:

  DINOv2RegressionModel(base_model)     dinov2salad/dinov2salad_validation.py:36-52
        .feature_extractor (frozen)  -> [B, 8448]; .regressor = Linear(8448,512)-ReLU-Linear(512,2)
        keys regressor.0.weight/bias, regressor.2.weight/bias
  SwinRegressionModel(backbone)         swin_transformer/swin_validation.py:37-46
        .backbone, .regressor = Linear(hidden, 2); key regressor.weight/bias
  SwinMLPRegressionModel(backbone)      swin_transformer/val_and_test_swin_2.py:164-177
        .regressor = Linear(hidden,512)-ReLU-Dropout-Linear(512,2); keys regressor.0.*, regressor.3.*
  SwinSinCosRegressionModel(backbone)   angle_prediction/swin/swin_angle_finetuning_sin_cos.py:52-62
        Linear(hidden,2) + F.normalize(eps=1e-6) -> unit [sin, cos]
  SwinAngleRegressorSinCos(backbone)    angle_prediction/swin/swin_angle_finetuning_gemini.py:92-128
        Linear(H,H/2)-ReLU-Dropout-Linear(H/2,2) -> raw [sin, cos]; keys regressor.0.*, regressor.3.*
  DinoV2AngleRegressorSinCos(backbone)  angle_prediction/dinov2salad/dino_v2_gemini.py:99-114
        DINOv2 CLS -> Dropout -> head = Linear(hidden,2) -> raw [sin, cos]; keys backbone.* (HF layout accepted), head.*
The reference builds its backbones with from_pretrained(NAME) inside __init__ (a network fetch);
here the backbone object is passed in.  `DinoV2Salad` is the `feature_extractor`:
DINOv2 (PyTorch) + SaladAggregator (HIP), keys `aggregator.*` as in serizba/salad.
All forwards are inference-only (torch.no_grad) and require GPU tensors.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops
from . import torch_ops  # noqa: F401  registers torch.ops.vpr.* (torch.library custom ops over the C ABI)
from .backbone import DinoV2, SplitTokens

_vpr = torch.ops.vpr      # the forwards below call the dispatcher-visible ops (CUDA impl = ctypes -> C ABI; fake impl for tracing)


class SaladAggregator(nn.Module):
    """Parameters laid out like serizba/salad's SALAD module (1x1 convs for score / cluster
    features, Linears for the token features, scalar dust_bin); forward = vpr_salad_aggregate."""

    def __init__(self, num_channels: int = 1024, num_clusters: int = 64, cluster_dim: int = 128,
                 token_dim: int = 256, hidden: int = 512):
        super().__init__()
        self.num_channels, self.num_clusters = num_channels, num_clusters
        self.cluster_dim, self.token_dim, self.hidden = cluster_dim, token_dim, hidden
        self.token_features = nn.Sequential(nn.Linear(num_channels, hidden), nn.ReLU(), nn.Linear(hidden, token_dim))
        self.cluster_features = nn.Sequential(nn.Conv2d(num_channels, hidden, 1), nn.Dropout(0.3), nn.ReLU(),
                                              nn.Conv2d(hidden, cluster_dim, 1))
        self.score = nn.Sequential(nn.Conv2d(num_channels, hidden, 1), nn.Dropout(0.3), nn.ReLU(),
                                   nn.Conv2d(hidden, num_clusters, 1))
        self.dust_bin = nn.Parameter(torch.tensor(1.0))
        self._packed: Optional[ops.SaladWeights] = None
        self._packed_f32: Optional[ops.SaladWeightsF32] = None

    def pack(self) -> ops.SaladWeights:
        """Kernel-format weights (bf16 matrices, f32 biases); call again after loading a state dict."""
        m2 = lambda w: w.detach().reshape(w.shape[0], -1)
        bf = lambda w: w.to(torch.bfloat16).contiguous()
        f32 = lambda b: b.detach().to(torch.float32).contiguous()
        s, c, t = self.score, self.cluster_features, self.token_features
        self._packed = ops.SaladWeights(
            w1_sc=bf(torch.cat([m2(s[0].weight), m2(c[0].weight)], 0)), b1_sc=f32(torch.cat([s[0].bias, c[0].bias], 0)),
            w2_s=bf(m2(s[3].weight)), b2_s=f32(s[3].bias), w2_c=bf(m2(c[3].weight)), b2_c=f32(c[3].bias),
            w1_t=bf(m2(t[0].weight)), b1_t=f32(t[0].bias), w2_t=bf(m2(t[2].weight)), b2_t=f32(t[2].bias),
            dustbin=self._dustbin_after_pack())
        return self._packed

    def _dustbin_after_pack(self) -> float:
        """dust_bin as a host number, read LAST in pack() / pack_f32(): the device-to-host copy blocks the host until the
        current stream has run everything queued before it, the casts and concatenations of the pack among them.  That is
        the hand-over of the packed tensors to every stream: when pack() returns they are complete, so a caller on any
        stream may use them (tests/test_stream_handover_gpu.py holds this).  Not for use under graph capture."""
        return float(self.dust_bin.detach().cpu())

    def pack_f32(self) -> ops.SaladWeightsF32:
        """f32 kernel-format weights for the f32-accurate aggregation (vpr_salad_aggregate_f32): the parameters as they
        are, no bf16 rounding (the reference keeps the aggregator in fp32: dinov2salad_validation.py:65-66)."""
        m2 = lambda w: w.detach().reshape(w.shape[0], -1).to(torch.float32).contiguous()
        f32 = lambda b: b.detach().to(torch.float32).contiguous()
        s, c, t = self.score, self.cluster_features, self.token_features
        self._packed_f32 = ops.SaladWeightsF32(
            w1_sc=torch.cat([m2(s[0].weight), m2(c[0].weight)], 0).contiguous(), b1_sc=f32(torch.cat([s[0].bias, c[0].bias], 0)),
            w2_s=m2(s[3].weight), b2_s=f32(s[3].bias), w2_c=m2(c[3].weight), b2_c=f32(c[3].bias),
            w1_t=m2(t[0].weight), b1_t=f32(t[0].bias), w2_t=m2(t[2].weight), b2_t=f32(t[2].bias),
            dustbin=self._dustbin_after_pack())
        return self._packed_f32

    def token_stage(self, cls_rows: torch.Tensor, owner_raw_stream: int, n: int) -> None:
        """The token MLP of these cls rows (images of n patch tokens) on the current stream, into the workspace of
        `owner_raw_stream` (backbone.DinoV2.cls_tail_hook: the backbone's cls-row stream has the cls tokens ~0.3 ms before
        the main stream has the patch tokens, so the stage costs the step nothing).  n == 256 only (vpr_salad_stage_token)."""
        w = self._packed or self.pack()
        ops.salad_stage_token(cls_rows, w, n, owner_raw_stream)

    @torch.no_grad()
    def forward(self, tokens, want_bf16: bool = False):
        """tokens [B, 1+n, C] (cls first) or a backbone.SplitTokens pair -> descriptor [B, 8448] f32 (and a bf16 copy).
        bf16 tokens: the bf16-operand kernels (benchmark path); f32 tokens: the f32-accurate aggregation with f32
        weights — the reference's precision (its extractor runs in fp32).
        Always eval arithmetic, whatever `.training` says: the two Dropout(0.3) layers of score / cluster_features are
        never applied here.  The training-mode descriptor (those Dropouts active, as under the fine-tuning script's
        model.train()) is forward_train."""
        split = isinstance(tokens, SplitTokens)
        first = tokens.patch if split else tokens
        f32, n = first.dtype == torch.float32, first.shape[1] - (0 if split else 1)
        if n > _lib.SALAD_HIRES_MAX_N:  # before any launch: the backbone may have run, the aggregation has no kernel for this grid
            side = math.isqrt(_lib.SALAD_HIRES_MAX_N)
            raise ValueError(f"SaladAggregator: {n} patch tokens per image, but the aggregation takes at most {_lib.SALAD_HIRES_MAX_N} "
                             f"({side} x {side}: {side * 14} px images at patch 14, DINOv2's own position grid)")
        w = (self._packed_f32 or self.pack_f32()) if f32 else (self._packed or self.pack())
        weights = torch_ops.weight_list(w)
        if n == 256 and not f32:        # the n = 256 bf16 ops take their layout as it comes; only they have a token_ready form
            if split:
                desc, desc16 = _vpr.salad_aggregate_split(tokens.patch, tokens.cls, weights, w.dustbin, 3, bool(tokens.token_ready))
            else:
                desc, desc16 = _vpr.salad_aggregate(tokens, weights, w.dustbin, 3)
            return (desc, desc16) if want_bf16 else desc
        if split:
            patch, cls = tokens.patch.contiguous(), tokens.cls.contiguous()
        elif n == 256:                  # salad_aggregate_f32 takes the pair only
            patch, cls = tokens[:, 1:].contiguous(), tokens[:, 0].contiguous()
        else:                           # any other grid (include/vpr_amd_salad_anyres.h, _hires.h): the hub layout addressed in place
            patch, cls = tokens.contiguous(), None
        if n == 256:
            op = _vpr.salad_aggregate_f32
        elif n <= _lib.SALAD_MAX_N:
            op = _vpr.salad_aggregate_f32_n if f32 else _vpr.salad_aggregate_n
        else:                           # 577 .. 1369 tokens (448 / 518 px): the stage A that keeps no score matrix in LDS
            op = _vpr.salad_aggregate_f32_hires if f32 else _vpr.salad_aggregate_hires
        desc, desc16 = op(patch, cls, weights, w.dustbin, 3)
        return (desc, desc16) if want_bf16 else desc

    @torch.no_grad()
    def local_features(self, tokens: torch.Tensor, fp8: bool = False, hires: bool = False) -> torch.Tensor:
        """Per-patch local descriptors for local-feature re-ranking (include/vpr_amd_local.h): patch tokens [B, n, C] (no cls
        row; bf16 or f32) -> [B, n, cluster_dim] bf16, the cluster_features MLP of every patch in eval arithmetic (its Dropout
        is never applied), L2-normalised per patch in f32; an all-zero output row stays zero.  bf16 tokens on the GPU run the
        two layers on the MFMA GEMM (bf16 operands and hidden layer, f32 accumulation); anything else runs them in f32 torch
        with the f32 weights.  n > 256 (322 px and up) raises before any launch: the matching kernel holds one image's
        patches in a single tile set.
        fp8=True: [B, n, cluster_dim] uint8 instead, the e4m3 store of include/vpr_amd_patch_fp8.h (ops.quantize_patch_fp8),
        quantised from the f32 normalised value in one rounding, not through bf16; on the GPU only.
        hires=True: the limit is 1369 patches (518 px), the range of include/vpr_amd_local_hires.h; the features are the same
        code per patch, so at n <= 256 the result is the default call's bit for bit."""
        if tokens.dim() != 3 or tokens.shape[2] != self.num_channels:
            raise ValueError(f"SaladAggregator.local_features: tokens must be [B, n, {self.num_channels}] patch tokens, "
                             f"got {tuple(tokens.shape)}")
        B, n, C = tokens.shape
        if hires and n > _lib.LOCAL_HIRES_MAX_N:
            raise ValueError(f"SaladAggregator.local_features(hires=True): {n} patch tokens per image, but local-feature "
                             f"re-ranking takes at most {_lib.LOCAL_HIRES_MAX_N} (518 px images at patch 14)")
        if not hires and n > _lib.LOCAL_MAX_N:
            raise ValueError(f"SaladAggregator.local_features: {n} patch tokens per image, but local-feature re-ranking takes at "
                             f"most {_lib.LOCAL_MAX_N} (224 px images at patch 14)")
        x = tokens.reshape(B * n, C)
        if x.is_cuda and x.dtype == torch.bfloat16:
            w = self._packed or self.pack()
            h = ops.gemm_nt_bf16(x.contiguous(), w.w1_sc[self.hidden:], w.b1_sc[self.hidden:], relu=True, out_dtype=torch.bfloat16)
            f = ops.gemm_nt_bf16(h, w.w2_c, w.b2_c)
        else:
            w = self._packed_f32 or self.pack_f32()
            h = torch.relu(x.float() @ w.w1_sc[self.hidden:].T + w.b1_sc[self.hidden:])
            f = h @ w.w2_c.T + w.b2_c
        norm = f.norm(dim=1, keepdim=True)
        f = torch.where(norm > 0, f / norm, torch.zeros_like(f))
        if fp8:
            return ops.quantize_patch_fp8(f.contiguous()).view(B, n, self.cluster_dim)
        return f.to(torch.bfloat16).view(B, n, self.cluster_dim)

    def dropout_p(self) -> float:
        """p of the two Dropout layers (score[1], cluster_features[1]); the fused kernel draws one mask rate for both."""
        ps, pc = float(self.score[1].p), float(self.cluster_features[1].p)
        if ps != pc:
            raise ValueError(f"SaladAggregator: score[1].p = {ps} and cluster_features[1].p = {pc} differ; the training-mode "
                             "aggregation applies one dropout rate to both MLPs")
        return ps

    @torch.no_grad()
    def forward_train(self, tokens, seed: int, pass_index: int, image_base: int = 0, want_bf16: bool = False):
        """The descriptor in training mode: Dropout(p) of score[1] / cluster_features[1] active (the hub model while
        dinov2salad_finetuning.py:115 has it in train(); the token MLP has no dropout).  tokens = [B, 1+n, C] bf16 (cls
        first) or a backbone.SplitTokens pair of bf16 tensors.  The mask is a pure function of (seed, pass_index,
        image_base + b, token, unit) — include/vpr_amd.h, vpr_salad_aggregate_train — so the same image gets the same mask
        in any batching: pass the image's global index through image_base.  Reads p from the modules at every call (equal
        p required: ValueError otherwise).  Independent of `.training`."""
        p = self.dropout_p()
        w = self._packed or self.pack()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        seed = seed - (1 << 64) if seed >= 1 << 63 else seed          # the op's int is signed
        if isinstance(tokens, SplitTokens):
            desc, desc16 = _vpr.salad_aggregate_train(tokens.patch, tokens.cls, torch_ops.weight_list(w), w.dustbin, 3, p, seed,
                                                      int(pass_index), int(image_base))
        else:
            desc, desc16 = _vpr.salad_aggregate_train(tokens, None, torch_ops.weight_list(w), w.dustbin, 3, p, seed,
                                                      int(pass_index), int(image_base))
        return (desc, desc16) if want_bf16 else desc


class DinoV2Salad(nn.Module):
    """`feature_extractor`: images [B,3,img_size,img_size] -> L2-normalised descriptor [B, 8448].  img_size: any multiple of
    the patch size whose grid has 65 .. 1369 tokens (322 -> 23 x 23 = 529, the resolution DINOv2-SALAD is published at; 448 ->
    1024; 518 -> 37 x 37 = 1369, DINOv2's own position grid and the largest the aggregation takes)."""

    def __init__(self, arch: str = "vit_large", img_size: int = 224):
        super().__init__()
        self.backbone = DinoV2(arch, img_size)
        self.aggregator = SaladAggregator(self.backbone.embed_dim)

    token_on_cls_stream = True      # SALAD's token MLP rides on the backbone's cls-row stream (bit-identical; A/B switch)

    @torch.no_grad()
    def tokens(self, x: torch.Tensor) -> torch.Tensor:
        """Final-norm tokens [B, 1+n, C] bf16, cls first (the hub model's layout)."""
        t = self.backbone(x)
        return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)

    @torch.no_grad()
    def features(self, x: torch.Tensor, want_bf16: bool = False, events: Optional[list] = None, want_local=False,
                 hires: bool = False):
        """images -> descriptor (and its bf16 copy): backbone tokens stay in the layout the backbone
        computed them in (SplitTokens on the HIP path), no re-layout copy before SALAD.
        events: a list -> a (start, end) pair of timing events around the aggregation on the current stream is appended
        (bench.py: the SALAD stage as the step runs it, token MLP on the backbone's cls-row stream).
        want_local: the result gains a last element, the local features [B, n, 128] bf16 of the same backbone pass
        (SaladAggregator.local_features; at most 256 patch tokens, ValueError before the backbone runs otherwise).  The
        descriptor is the default call's, bit for bit.  want_local="fp8": that element is their e4m3 store instead, uint8
        [B, n, 128] (local_features(fp8=True)); True keeps the bf16 result bit for bit.
        hires=True (with want_local): up to 1369 patch tokens (img_size 322, 448, 518), the features that
        ops.local_rerank_hires / local_rerank_fp8_hires and ShardedGallery(local_hires=True) take."""
        if want_local not in (False, True, "fp8"):
            raise ValueError(f"DinoV2Salad.features: want_local must be False, True or 'fp8', got {want_local!r}")
        if want_local:
            if hires and self.backbone.num_patches > _lib.LOCAL_HIRES_MAX_N:
                raise ValueError(f"DinoV2Salad.features(want_local=True, hires=True): {self.backbone.num_patches} patch tokens per "
                                 f"image, but local-feature re-ranking takes at most {_lib.LOCAL_HIRES_MAX_N} (518 px images at patch 14)")
            if not hires and self.backbone.num_patches > _lib.LOCAL_MAX_N:
                raise ValueError(f"DinoV2Salad.features(want_local=True): {self.backbone.num_patches} patch tokens per image, but "
                                 f"local-feature re-ranking takes at most {_lib.LOCAL_MAX_N} (224 px images at patch 14)")
            keep: list = []
            out = self._features(x, want_bf16, events, keep)
            local = self.aggregator.local_features(keep[0], fp8=want_local == "fp8", hires=hires)
            return (*out, local) if want_bf16 else (out, local)
        return self._features(x, want_bf16, events)

    def _features(self, x: torch.Tensor, want_bf16: bool, events: Optional[list], keep_patch: Optional[list] = None):
        # the token stage on the cls-row stream exists for 256 tokens only; any other grid runs the token MLP in the aggregation
        hook = self.token_on_cls_stream and self.backbone.num_patches == 256
        self.backbone.cls_tail_hook = self.aggregator.token_stage if hook else None
        try:
            t = self.backbone(x, split=True)
        finally:
            self.backbone.cls_tail_hook = None
        if t.patch.dtype not in (torch.bfloat16, torch.float32):
            t = SplitTokens(t.patch.to(torch.bfloat16), t.cls.to(torch.bfloat16))
        if keep_patch is not None:
            keep_patch.append(t.patch)
        if events is None:
            return self.aggregator(t, want_bf16=want_bf16)      # f32 tokens (an f32 model) take the f32-accurate aggregation
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.aggregator(t, want_bf16=want_bf16)
        e1.record()
        events.append((e0, e1))
        return out

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.features(x)


def _mlp_head_args(seq: nn.Sequential):
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    if len(lin) != 2:
        raise RuntimeError("expected Linear -> ReLU -> [Dropout] -> Linear")
    f = lambda p: p.detach().to(torch.float32).contiguous()
    return f(lin[0].weight), f(lin[0].bias), f(lin[1].weight), f(lin[1].bias)


class DINOv2RegressionModel(nn.Module):
    def __init__(self, base_model: nn.Module):
        super().__init__()
        self.feature_extractor = base_model
        for p in self.feature_extractor.parameters():
            p.requires_grad = False
        self.regressor = nn.Sequential(nn.Linear(8448, 512), nn.ReLU(), nn.Linear(512, 2))

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        features = self.feature_extractor(x)
        return _vpr.pose_head(features.float().contiguous(), *_mlp_head_args(self.regressor), -1)


def _swin_hidden(backbone: nn.Module, pixel_values: torch.Tensor):
    """Pre-LayerNorm last hidden state [B,T,H] of an HF SwinModel, plus its final LayerNorm."""
    emb, dims = backbone.embeddings(pixel_values)
    enc = backbone.encoder(emb, dims)
    return enc[0].contiguous(), backbone.layernorm


class SwinRegressionModel(nn.Module):
    """backbone: an HF `SwinModel` (or anything with .embeddings/.encoder/.layernorm/.config)."""

    def __init__(self, backbone: nn.Module):
        super().__init__()
        self.backbone = backbone
        self.regressor = nn.Linear(self.backbone.config.hidden_size, 2)
        self.normalize_output = False

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        h, ln = _swin_hidden(self.backbone, pixel_values)
        _, out = _vpr.ln_meanpool_head(h, ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(), ln.eps,
                                       self.regressor.weight.detach().float().contiguous(),
                                       self.regressor.bias.detach().float().contiguous(),
                                       0 if self.normalize_output else -1)
        return out


class SwinSinCosRegressionModel(SwinRegressionModel):
    """Unit-normalised [sin, cos] output (F.normalize(out, dim=1, p=2, eps=1e-6))."""

    def __init__(self, backbone: nn.Module):
        super().__init__(backbone)
        self.normalize_output = True


class SwinMLPRegressionModel(nn.Module):
    def __init__(self, backbone: nn.Module, dropout_prob: float = 0.3, hidden: int = 512):
        super().__init__()
        self.backbone = backbone
        self.regressor = nn.Sequential(nn.Linear(self.backbone.config.hidden_size, hidden), nn.ReLU(),
                                       nn.Dropout(dropout_prob), nn.Linear(hidden, 2))

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        h, ln = _swin_hidden(self.backbone, pixel_values)
        pooled, _ = _vpr.ln_meanpool_head(h, ln.weight.detach().float().contiguous(), ln.bias.detach().float().contiguous(), ln.eps,
                                          None, None, -1)
        return _vpr.pose_head(pooled, *_mlp_head_args(self.regressor), -1)


class SwinAngleRegressorSinCos(SwinMLPRegressionModel):
    """angle_prediction/swin/swin_angle_finetuning_gemini.py:92-128 (there also called `SwinRegressionModel`; renamed
    because swin_validation.py's class owns that name here): Swin pooler -> Linear(H, H/2) -> ReLU -> Dropout ->
    Linear(H/2, 2) = raw (sin, cos), NOT unit-normalised (its loss is an MSE on the pair); decoded with
    postproc.sincos_to_degrees (:131-136).  Keys regressor.0.*, regressor.3.*."""

    def __init__(self, backbone: nn.Module, dropout_rate: float = 0.0):
        super().__init__(backbone, dropout_rate, hidden=backbone.config.hidden_size // 2)


class DinoV2AngleRegressorSinCos(nn.Module):
    """angle_prediction/dinov2salad/dino_v2_gemini.py:99-114: DINOv2 CLS token -> Dropout -> `head` = Linear(hidden, 2) =
    raw (sin, cos); decoded by prediction_to_angle_deg (:135-141) = postproc.sincos_to_degrees.  The reference builds
    the backbone with AutoModel.from_pretrained("facebook/dinov2-base") (a fetch); here a vpr_amd.backbone.DinoV2 is
    passed in, and its load hook takes the Hugging Face key layout the reference's checkpoints carry
    (`backbone.embeddings.*`, `backbone.encoder.layer.N.*`), so `load_state_dict(torch.load(best_model.pth))` works
    unchanged.  Keys: backbone.*, head.weight [2, hidden], head.bias [2]."""

    def __init__(self, backbone: DinoV2, dropout_rate: float = 0.1):
        super().__init__()
        self.backbone = backbone
        self.dropout = nn.Dropout(dropout_rate)                # eval: identity
        self.head = nn.Linear(backbone.embed_dim, 2)

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor) -> torch.Tensor:
        t = self.backbone(pixel_values, split=True)            # final-norm tokens; the cls rows are a contiguous [B, C]
        pooled = t.cls.float().contiguous()
        return _vpr.pose_head(pooled, None, None, self.head.weight.detach().float().contiguous(),
                              self.head.bias.detach().float().contiguous(), -1)


class FusedGeoPoseHead(nn.Module):
    """(lat, lon, sin, cos) in ONE kernel call from two independent MLP heads on the same features:
    hidden layers are row-concatenated and the output layer is block-diagonal, so each half is its
    own head (the zero blocks add exact zeros; only the f32 summation order of the split-K
    partition can differ from a separate call, ~1e-7).  pos: DINOv2RegressionModel
    .regressor; ang: Linear-ReLU-Linear(…,2) giving [sin, cos], unit-normalised if `normalize`."""

    def __init__(self, pos: nn.Sequential, ang: nn.Sequential, normalize: bool = True):
        super().__init__()
        self.pos, self.ang, self.normalize = pos, ang, normalize
        self._packed = None

    def pack(self):
        W1p, b1p, W2p, b2p = _mlp_head_args(self.pos)
        W1a, b1a, W2a, b2a = _mlp_head_args(self.ang)
        hp, ha = W1p.shape[0], W1a.shape[0]
        W1 = torch.cat([W1p, W1a], 0).contiguous()
        b1 = torch.cat([b1p, b1a], 0).contiguous()
        W2 = torch.zeros(4, hp + ha, dtype=torch.float32, device=W1.device)
        W2[:2, :hp] = W2p
        W2[2:, hp:] = W2a
        self._packed = (W1, b1, W2, torch.cat([b2p, b2a], 0).contiguous())
        self._packed_order = (self._packed, ops.handover())     # built by queued work of the current stream: lent in forward
        return self._packed

    @torch.no_grad()
    def forward(self, features: torch.Tensor) -> torch.Tensor:
        packed = self._packed or self.pack()
        of, order = getattr(self, "_packed_order", None) or (None, None)
        if of is packed:                # (a caller may also set _packed itself: such matrices are ordered by whoever made them)
            order.lend(packed)          # a stream other than the packing one waits for the pack, once
        W1, b1, W2, b2 = packed
        return _vpr.pose_head(features, W1, b1, W2, b2, 2 if self.normalize else -1)


def load_reference_checkpoint(model: nn.Module, path: str) -> nn.Module:
    """Accepts both checkpoint forms the reference writes: {'model_state_dict': ...}
    (dinov2salad_finetuning.py:130-135, loaded at dinov2salad_validation.py:68-69) and bare
    state dicts (swin_attempt_2.py:255, loaded at val_and_test_swin_2.py:231).  The load is strict,
    as the reference's: the `feature_extractor.*` keys of the hub model (`backbone.model.blocks.N.attn.qkv`,
    `ls1.gamma`, `patch_embed.proj`, `mask_token`, 37x37 `pos_embed`) are mapped onto DinoV2's by its
    load hook (backbone.DinoV2._adopt_foreign_keys / checkpoint.py).  A load un-folds LayerScale: call
    `backbone.fold_layerscale()` and `aggregator.pack()` afterwards (evaluate.py does)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    state = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    model.load_state_dict(state)
    for m in model.modules():
        if hasattr(m, "_packed"):
            m._packed = None
        if hasattr(m, "_packed_f32"):
            m._packed_f32 = None
    return model
