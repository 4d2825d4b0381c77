"""DINOv2 ViT backbone in plain PyTorch-ROCm (plumbing: the hand-written HIP path starts at the
token tensor it returns).

Stands in for the backbone half of `torch.hub.load("serizba/salad", "dinov2_salad")`
(dinov2salad/dinov2salad_validation.py:65), which wraps facebookresearch/dinov2 ViT-B/14 and
hands SALAD the final-norm patch tokens + cls token.  Architecture only (random init; no weights
exist offline): patch-14 conv embed, cls token, learned position embedding, pre-norm blocks with
LayerScale, final LayerNorm.  Returns tokens [B, 1+n, C] with the cls token in row 0 — the
layout vpr_salad_aggregate consumes directly (no permute to [B,C,16,16]).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _streams, ops
from ._cache import tensor_key

def gemm_autotune(enable: bool = True, tuning: bool = True, max_ms_per_gemm: int = 30) -> None:
    """PyTorch TunableOp for the backbone's four hipBLASLt GEMM shapes: during the (untimed) warm-up
    steps each new shape is timed against the library's candidate kernels and the fastest is kept
    in memory (PyTorch also dumps them to a scratch file in the temp dir at exit); call
    gemm_autotune(True, tuning=False) afterwards so the timed region only replays the choices.
    Plumbing around the library GEMMs, not a kernel."""
    import tempfile
    import torch.cuda.tunable as tun
    tun.enable(enable)
    tun.tuning_enable(enable and tuning)
    if enable and tuning:
        tun.set_max_tuning_duration(max_ms_per_gemm)
        tun.set_filename(os.path.join(tempfile.gettempdir(), f"vpr_tunableop_{os.getpid()}.csv"))


CONFIGS = {
    # name: (embed_dim, depth, heads)
    "vit_small": (384, 12, 6),
    "vit_base": (768, 12, 12),       # what the reference's hub entry uses (C = 768)
    "vit_large": (1024, 24, 16),     # BASELINE.json north star (C = 1024)
}


def _ln_width_ok(C: int) -> bool:
    """The row widths the HIP LayerNorm kernels take."""
    return C % 8 == 0 and C <= 2048


def _hip_attention_ok(head_dim: int, T: int) -> bool:
    """The domain of the short-sequence HIP attention kernel (K, V of one (image, head) resident in LDS)."""
    return head_dim == 64 and T <= 288


def _ln(norm: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    """LayerNorm: the hand-written HIP kernel for GPU bf16 activations, PyTorch's otherwise (CPU)."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and _ln_width_ok(x.shape[-1]):
        return ops.layernorm_bf16(x, norm.weight, norm.bias, norm.eps)
    return norm(x)


class SplitTokens(NamedTuple):
    """Final-norm tokens as the HIP backbone path holds them: patch [B, n, C] and cls [B, C], both
    contiguous (vpr_salad_aggregate_split consumes the pair without a copy).  token_ready: the backbone's cls-row
    stream already ran `cls_tail_hook` on these cls rows (the SALAD token MLP), ordered before the current stream."""
    patch: torch.Tensor
    cls: torch.Tensor
    token_ready: bool = False

    def joined(self) -> torch.Tensor:
        """[B, 1+n, C], cls first (the reference / torch.hub layout)."""
        return torch.cat([self.cls.unsqueeze(1), self.patch], dim=1)


class Block(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, init_values: float = 1e-5):
        super().__init__()
        self.heads = heads
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.ls1 = nn.Parameter(init_values * torch.ones(dim))
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.fc1 = nn.Linear(dim, int(dim * mlp_ratio))
        self.fc2 = nn.Linear(int(dim * mlp_ratio), dim)
        self.ls2 = nn.Parameter(init_values * torch.ones(dim))

    folded = False      # inference-only: LayerScale folded into proj / fc2 (saves two passes per block)

    @torch.no_grad()
    def fold_layerscale(self) -> None:
        """ls * (W a + b) == (diag(ls) W) a + ls * b: rewrite proj / fc2 once, then skip the two
        elementwise multiplies in forward.  Changes rounding only (bf16 weights are re-rounded).
        ls1 / ls2 become ones, so the parameters always describe the same function whichever way they
        are read: a state dict saved from a folded model loads into a fresh one correctly (ls = 1 there),
        and `folded` is only the licence to skip a multiply by one."""
        if self.folded:
            return
        for lin, ls in ((self.proj, self.ls1), (self.fc2, self.ls2)):
            w = (ls.float()[:, None] * lin.weight.float()).to(lin.weight.dtype)
            b = (ls.float() * lin.bias.float()).to(lin.bias.dtype)
            lin.weight.copy_(w)
            lin.bias.copy_(b)
            ls.fill_(1.0)
        self.folded = True

    def _load_from_state_dict(self, *args, **kwargs):
        # Any load may bring unfolded weights and real LayerScale values back: the fold licence ends
        # here (the loaded ls1 / ls2 are applied again until fold_layerscale() is called anew).
        super()._load_from_state_dict(*args, **kwargs)
        self.folded = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, T, C = x.shape
        qkv = self.qkv(_ln(self.norm1, x)).view(B, T, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])
        y = self.proj(a.transpose(1, 2).reshape(B, T, C))
        x = x + (y if self.folded else self.ls1 * y)
        y = self.fc2(F.gelu(self.fc1(_ln(self.norm2, x))))
        x = x + (y if self.folded else self.ls2 * y)
        return x


PATCH, CLS = 0, 1       # the two row ranges of the split row layout [B*n patch rows | B cls rows]
ATT, MLP = 0, 1         # the two halves of a block: proj -> LayerNorm 2, and fc2 -> the LayerNorm before the next qkv


class _BlockStages:
    """One block of the HIP path as its launches: qkv, [attention,] x += att Wproj^T, LayerNorm 2, fc1 + GELU, x += hh Wfc2^T,
    and the LayerNorm before the next qkv (the next block's norm1, or the final norm).  Each GEMM stage has a PATCH form (a
    library GEMM) and a CLS form (vpr_skinny_linear_bf16: a library GEMM spends 9-14 us on 64 rows); a LayerNorm is the
    same launch on any rows.  A method takes the row views it reads and writes and issues one launch on the current
    stream: the drivers (DinoV2._blocks_side_chain, _blocks_in_stream, _forward_hip) decide only order, stream and buffers.
    The residual add lives in the proj / fc2 GEMM (beta = 1, in place: the f32 accumulator is added to the stream before
    the single bf16 rounding) and their biases never enter the bf16 stream: the running sum of the biases is a static [C]
    f32 vector per LayerNorm (DinoV2._cumulative_bias), added inside the kernel (vpr_bias_layernorm_bf16)."""
    def __init__(self, m: "DinoV2", blk: Block, nxt: nn.LayerNorm, bias_att: torch.Tensor, bias_mlp: torch.Tensor):
        self.m, self.blk = m, blk
        self.lin, self.norm, self.bias = (blk.proj, blk.fc2), (blk.norm2, nxt), (bias_att, bias_mlp)     # by half

    def qkv(self, part: int, h: torch.Tensor, out: torch.Tensor) -> None:
        lin = self.blk.qkv
        if part == CLS:
            ops.skinny_linear_bf16(h, lin.weight, lin.bias, out, 0)
        else:
            torch.addmm(lin.bias, h, lin.weight.t(), out=out)

    def add(self, half: int, part: int, a: torch.Tensor, x: torch.Tensor, row_stats: Optional[torch.Tensor] = None) -> None:
        """x += a W^T (proj / fc2).  row_stats (CLS): the launch also leaves these rows' statistics partials for ln(half)."""
        w = self.lin[half].weight
        if part == CLS:
            ops.skinny_linear_bf16(a, w, None, x, 2, None if row_stats is None else self.bias[half], row_stats)
        else:
            x.addmm_(a, w.t())

    def ln(self, half: int, x: torch.Tensor, cls_linear: Optional[tuple] = None) -> torch.Tensor:
        """The LayerNorm that ends a half, on rows x.  cls_linear = (first cls row, row_stats, ClsLinearConsts, out): the CLS
        form of the stage that follows (fc1 + GELU / the next qkv) rides in the launch (vpr_bias_layernorm_cls_linear_bf16)."""
        n = self.norm[half]
        if cls_linear is None:
            return ops.bias_layernorm_bf16(x, self.bias[half], n.weight, n.bias, n.eps)
        return ops.bias_layernorm_cls_linear_bf16(x, self.bias[half], n.weight, n.bias, n.eps, *cls_linear, gelu=half == ATT)

    def fc1(self, part: int, h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """GELU(h Wfc1^T + b) in the form DinoV2.gelu names, into `out` or a new tensor of the current stream's allocator pool."""
        lin, gelu = self.blk.fc1, self.m.gelu
        if gelu not in ("tanh", "erf"):
            raise ValueError("DinoV2.gelu must be 'tanh' or 'erf'")
        if part == CLS:
            out = h.new_empty((h.shape[0], lin.weight.shape[0])) if out is None else out
            return ops.skinny_linear_bf16(h, lin.weight, lin.bias, out, 1 if gelu == "tanh" else 4)
        if gelu == "tanh":
            return torch._addmm_activation(lin.bias, h, lin.weight.t(), use_gelu=True, out=out)
        return torch._C._nn.gelu_(torch.addmm(lin.bias, h, lin.weight.t(), out=out))

    def rows(self, part: int, att: torch.Tensor, x: torch.Tensor, nst: Optional["_BlockStages"] = None, qkv_next=None) -> torch.Tensor:
        """Everything between this block's attention and the next one on ONE row range (att, x, qkv_next: its rows), in
        order; nst: the next block's stages, None after the last block.  -> the normalised rows."""
        self.add(ATT, part, att, x)
        hh = self.fc1(part, self.ln(ATT, x))
        self.add(MLP, part, hh, x)
        h = self.ln(MLP, x)
        if nst is not None:
            nst.qkv(part, h, qkv_next)
        return h


class DinoV2(nn.Module):
    def __init__(self, arch: str = "vit_large", img_size: int = 224, patch: int = 14):
        super().__init__()
        dim, depth, heads = CONFIGS[arch]
        self.embed_dim = dim
        self.patch = patch
        self.num_patches = (img_size // patch) ** 2
        self.patch_embed = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + self.num_patches, dim))
        self.blocks = nn.ModuleList(Block(dim, heads) for _ in range(depth))
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        self._register_load_state_dict_pre_hook(self._adopt_foreign_keys)

    # None: 0.1 for facebookresearch/dinov2 (hub) key layouts, 0 for Hugging Face ones (checkpoint.py)
    pos_embed_interpolate_offset: Optional[float] = None

    def _adopt_foreign_keys(self, state_dict, prefix, *unused) -> None:
        """load_state_dict pre-hook (runs for a load through ANY ancestor, e.g. the strict load of
        dinov2salad_validation.py:69 on DINOv2RegressionModel): rewrites, in place, the keys under this
        module's prefix from the hub / serizba-salad (`model.` level, attn.qkv, ls1.gamma, patch_embed.proj,
        mask_token, 37x37 pos_embed) or Hugging Face layout into this class's names — checkpoint.py."""
        from .checkpoint import convert_state_dict
        mine = [k for k in state_dict if k.startswith(prefix)]
        if not mine:
            return
        sub = {}
        for k in mine:
            rest = k[len(prefix):]
            sub[rest[6:] if rest.startswith("model.") else rest] = state_dict.pop(k)
        for k, v in convert_state_dict(sub, self.num_patches, self.pos_embed_interpolate_offset).items():
            state_dict[prefix + k] = v

    @torch.no_grad()
    def forward(self, x: torch.Tensor, split: bool = False):
        """x [B,3,H,W] -> final-norm tokens [B, 1+n, C] (cls first), contiguous; with split=True a
        SplitTokens(patch [B,n,C], cls [B,C]) pair (what the HIP path computes in; no copy)."""
        if self.auto_fold and x.is_cuda and x.dtype == torch.bfloat16 and not all(b.folded for b in self.blocks):
            self.fold_layerscale()      # inference-only module: a load un-folds (Block._load_from_state_dict), the next GPU forward re-folds
        order = self.__dict__.get("_fold_order")
        if order is not None and x.is_cuda:
            order.lend(())              # a stream other than the folding one waits for the fold, once (the weights are never freed)
        if self._hip_split_ok(x):
            st = self._forward_hip_split(x)
            return st if split else st.joined()
        x = self.patch_embed(x).flatten(2).transpose(1, 2)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self.pos_embed
        if self._hip_ok(x):
            x = self._forward_hip(x)
        else:
            for blk in self.blocks:
                x = blk(x)
            x = _ln(self.norm, x).contiguous()
        return SplitTokens(x[:, 1:].contiguous(), x[:, 0].contiguous()) if split else x

    # GELU of the HIP path's fc1: "tanh" = inside the library GEMM's epilogue (hipBLASLt offers only the tanh
    # form; |gelu_tanh - gelu_erf| <= 4.7e-4, below the bf16 spacing of every output above 0.12) or "erf" = the
    # exact nn.GELU() DINOv2 uses, as a separate in-place pass (+45 us per block at B = 64).  The f32 / CPU block
    # loop is always erf.  evaluate.py (reference checkpoints) selects "erf"; bench.py keeps the default.
    gelu = "tanh"

    auto_fold = True        # fold LayerScale at the first bf16 GPU forward after a load, so a freshly loaded checkpoint never
                            # lands on the slow PyTorch block loop by accident (bench.py --no-fold turns it off for the A/B)
    hip_split = True
    # Two switches of the in-stream schedule (cls_side_chain = False).  cls_after_gemm: each cls-row launch comes right AFTER
    # the library GEMM that used the same weight matrix (the 2-8 MB it streams could then be cache-resident); measured equal
    # to "before": 11.20 / 11.16 vs 11.12 / 11.17 ms per step — the launches are latency-, not bandwidth-bound.  fuse_ln_cls:
    # the two cls-row linears that directly follow a LayerNorm (qkv, fc1) ride in its launch (vpr_bias_layernorm_cls_linear_bf16):
    # 0.03-0.05 ms per step, 11.17/11.23 vs 11.22/11.26 — within noise, so the simpler path is the default
    cls_after_gemm = True
    fuse_ln_cls = False

    def _hip_split_ok(self, img: torch.Tensor) -> bool:
        P, C = self.patch, self.embed_dim
        return (self.hip_split and img.is_cuda and img.dtype == torch.bfloat16 and img.dim() == 4
                and img.shape[2] % P == 0 and img.shape[3] % P == 0 and img.shape[3] % 8 == 0
                and (img.shape[2] // P) * (img.shape[3] // P) == self.num_patches
                and img.shape[1] * P * img.shape[3] * 2 <= 48 * 1024
                and _ln_width_ok(C) and _hip_attention_ok(C // self.blocks[0].heads, 1 + self.num_patches)
                and all(b.folded for b in self.blocks))

    def _embed_consts(self, img: torch.Tensor):
        """(patch-embedding weight [C, kpad] bf16, additive token offsets [B*n + B, C] bf16 in the
        split row layout: pos[1+p] + conv bias for the patch rows, cls + pos[0] for the cls rows)."""
        B, K = img.shape[0], img.shape[1] * self.patch * self.patch
        kpad = (K + 63) // 64 * 64
        # one entry per batch size (an evaluation loop alternates between its full and its last, ragged batch)
        ps = (self.patch_embed.weight, self.patch_embed.bias, self.pos_embed, self.cls_token)
        return self._cache("_embed_cache", 3).get((img.device, B, kpad, tensor_key(*ps)), self._build_embed_consts,
                                                  (img.device, B, K, kpad), ps)

    def _build_embed_consts(self, dev: torch.device, B: int, K: int, kpad: int):
        pe, C, n = self.patch_embed, self.embed_dim, self.num_patches
        w = torch.zeros((C, kpad), dtype=torch.bfloat16, device=dev)
        w[:, :K] = pe.weight.detach().reshape(C, K).to(dev, torch.bfloat16)
        pos = self.pos_embed.detach().float().to(dev)[0]                             # [1+n, C]
        body = (pos[1:] + pe.bias.detach().float().to(dev)).to(torch.bfloat16)       # [n, C]
        tail = (pos[0] + self.cls_token.detach().float().to(dev).view(C)).to(torch.bfloat16)
        off = torch.cat([body.unsqueeze(0).expand(B, -1, -1).reshape(B * n, C),
                         tail.unsqueeze(0).expand(B, -1)], dim=0).contiguous()
        return w, off

    def _cache(self, name: str, capacity: int):
        """This module's graph-safe cache `name` (_cache.Cache), made on first use; kept out of the module's attributes proper."""
        c = self.__dict__.get(name)
        if c is None:
            c = self.__dict__[name] = ops.cache(capacity)
        return c

    cls_side_chain = True
    side_sync = "events"        # fork / join of the cls side chain (_streams): "events" (torch.cuda.Event), "light" (HIP events without the
                                # system-scope fence), "signals" (stream memory operations: measured SLOWER in the step).  bench.py --side-sync

    def _stages(self, device: torch.device, deferred_biases: bool = True) -> list:
        """The blocks as _BlockStages, each with the LayerNorm that follows it and its two cumulative-bias rows."""
        cum = self._cumulative_bias(device).unbind(0) if deferred_biases else [None] * (2 * len(self.blocks))
        norms = [b.norm1 for b in self.blocks][1:] + [self.norm]
        return [_BlockStages(self, blk, nxt, cum[2 * i], cum[2 * i + 1]) for i, (blk, nxt) in enumerate(zip(self.blocks, norms))]

    def _blocks_side_chain(self, stages: list, x: torch.Tensor, h: torch.Tensor, B: int, n: int) -> "SplitTokens":
        """The blocks with the cls rows on their own stream.  Between two attentions the B cls rows need six small kernels
        (_BlockStages.rows: 28 us of kernel time alone) that depend on nothing but the cls rows of the attention output;
        in-stream they cost the step ~0.1 ms more (11.17 vs 11.08 ms), launch gaps mostly.  Here the side stream is forked right
        after each attention and joined right before the next one, ~400 us of patch-row GEMMs later (an earlier attempt forked
        and joined around every single cls-row launch and lost 0.6 ms to cross-queue waits: 12.8 vs 12.2 ms per step).
        The chain does NOT run under the GEMMs (profiles/cls_chain_bench.txt): a library GEMM workgroup takes all 512 registers
        per lane of every SIMD of its CU and one workgroup sits on each CU, so a cls-row kernel is dispatched while the GEMM
        runs, stays open until the GEMM's workgroups retire (8-10x its own time) and then runs at the head of the next
        main-stream kernel, which it delays by about its own duration.  What the chain costs the step is therefore the cls
        kernels' own time, and the join still never waits: the chain ends ~80 us before the block's last GEMM does.
        The main stream touches only patch rows, the side stream only cls rows: no shared writes.  Lifetimes: what the main
        stream allocated and the side stream reads (`att`) or writes (`qkv_next`) stays referenced until after the join; the
        side stream's temporaries (rows(CLS), inside the stream context) come from that stream's allocator pool, the patch
        rows' (rows(PATCH), outside it, `hh` among them) from the main stream's.  Under graph capture fork / join are "events"."""
        Mp, C, dev = B * n, self.embed_dim, x.device
        main = torch.cuda.current_stream(dev)
        # high priority: the cls-row workgroups take the first CU slots a retiring GEMM workgroup frees (the library
        # GEMMs fill every CU's register file: nothing starts beside them, whatever its size)
        side = _streams.side_stream(dev, main.cuda_stream, "cls", int(os.environ.get("VPR_SIDE_PRIORITY", "-1")))
        mode = self.side_sync if not torch.cuda.is_current_stream_capturing() else "events"     # capture: plain event nodes
        if mode not in ("events", "light", "signals"):
            raise RuntimeError(f"DinoV2.side_sync: unknown mode {mode!r}")
        sync = _streams.fork_join(dev, main.cuda_stream, mode)      # "events": a fresh object; else kept per main stream
        xp, xc = x[:Mp], x[Mp:]
        qkv = torch.empty((Mp + B, 3 * C), dtype=torch.bfloat16, device=dev)
        stages[0].qkv(PATCH, h[:Mp], qkv[:Mp])
        stages[0].qkv(CLS, h[Mp:], qkv[Mp:])
        for st, nst in zip(stages, stages[1:] + [None]):
            att = ops.attention_qkv_split_bf16(qkv, B, 1 + n, n, st.blk.heads)
            qkv_next = torch.empty_like(qkv) if nst is not None else None
            sync.fork(main, side)
            with torch.cuda.stream(side):
                hc = st.rows(CLS, att[Mp:], xc, nst, qkv_next[Mp:] if nst is not None else None)
                hooked = nst is None and self.cls_tail_hook is not None
                if hooked:                  # e.g. SALAD's token MLP: needs the final cls rows only, rides on this stream
                    self.cls_tail_hook(hc, main.cuda_stream, n)
                joined = sync.mark(side)
            hp = st.rows(PATCH, att[:Mp], xp, nst, qkv_next[:Mp] if nst is not None else None)
            sync.join(main, joined)        # the side chain ended during the block's last GEMM (~80 us ago): satisfied on arrival
            qkv = qkv_next                 # (att stayed referenced up to here)
        return SplitTokens(hp.view(B, n, C), hc, hooked)

    # optional callable(cls_rows [B, C] bf16, raw handle of the main stream, patch tokens per image n): run on the cls-row side
    # stream right after the final LayerNorm of the cls rows, before that stream is joined (modules.DinoV2Salad installs SALAD's token MLP here)
    cls_tail_hook = None

    def _forward_hip_split(self, img: torch.Tensor) -> "SplitTokens":
        """The whole backbone on the GPU in the split row layout [B*n patch rows | B cls rows]:
        every linear layer runs as one library GEMM over the B*n patch rows — at n = 256 an exact
        number of 256-row tiles (64 tile rows at B = 64; the cls-first [B, 257, C] layout gives 64.25,
        i.e. a fourth, almost empty wave of tiles: hipBLASLt measures 88/117/96 us instead of
        105/133/148 us for qkv/fc1/fc2) — plus a 64-row GEMM over the cls rows.
        * patch embedding = HIP patchify + one GEMM (instead of MIOpen's implicit-GEMM conv +
          transposes + cat + add); cls / position / conv-bias terms are a static additive matrix
          consumed by the first LayerNorm kernel, which writes the residual stream anyway;
        * the blocks: _BlockStages, driven by _blocks_side_chain (default) or _blocks_in_stream; bias + GELU in the fc1 GEMM
          epilogue (hipBLASLt's tanh form; vs an f32 reference the max error equals erf-GELU's 0.016: bf16 rounding dominates);
        * attention: vpr_attention_qkv_split_bf16 (token -> row mapping inside the kernel)."""
        B, n, C, P = img.shape[0], self.num_patches, self.embed_dim, self.patch
        Mp, M, dev = B * n, B * n + B, img.device
        w, off = self._embed_consts(img)
        a = ops.patchify_bf16(img.contiguous(), P, w.shape[1], 0)               # [Mp, kpad]
        raw = ops.zero_rows_bf16(M, C, dev)         # persistent per (device, stream, shape): its cls rows are zero and nothing ever writes them
        torch.mm(a, w.t(), out=raw[:Mp])
        n0 = self.blocks[0].norm1
        x, h = ops.add_layernorm_bf16(raw, off, n0.weight, n0.bias, n0.eps)
        run = self._blocks_side_chain if self.cls_side_chain else self._blocks_in_stream
        return run(self._stages(dev), x, h, B, n)

    def _blocks_in_stream(self, stages: list, x: torch.Tensor, h: torch.Tensor, B: int, n: int) -> "SplitTokens":
        """The blocks on one stream: every LayerNorm is one launch over all rows, every GEMM stage its PATCH and its CLS
        launch in the order `cls_after_gemm` says.  With `fuse_ln_cls` the CLS launches of fc1 and qkv ride in the
        LayerNorm before them, and the CLS launches of proj and fc2 leave that LayerNorm's statistics partials in `rs`.
        Tried and dropped: proj over all B*n + B rows in one GEMM (50 us vs 38 + 8)."""
        Mp, M, C = B * n, B * n + B, self.embed_dim
        fuse = self.fuse_ln_cls and C % 32 == 0 and self.gelu == "tanh"     # the fused launch has the tanh form only
        order = (PATCH, CLS) if self.cls_after_gemm else (CLS, PATCH)
        rs = torch.empty((C // 16, B, 2), dtype=torch.float32, device=x.device) if fuse else None   # stream-ordered reuse
        fc = self._cls_fused_consts(x.device) if fuse else None
        parts = lambda t: (t[:Mp], t[Mp:])       # a tensor's (PATCH rows, CLS rows)
        xs = parts(x)
        qkv = x.new_empty((M, 3 * C))
        cls_qkv_done = False                     # True once a fused LayerNorm launch has produced qkv[Mp:]
        for i, (st, nst) in enumerate(zip(stages, stages[1:] + [None])):
            hs, qs = parts(h), parts(qkv)
            for part in order if not cls_qkv_done else (PATCH,):
                st.qkv(part, hs[part], qs[part])
            atts = parts(ops.attention_qkv_split_bf16(qkv, B, 1 + n, n, st.blk.heads))
            for part in order:
                st.add(ATT, part, atts[part], xs[part], rs)
            hhs = parts(x.new_empty((M, st.blk.fc1.weight.shape[0])))
            hs = parts(st.ln(ATT, x, (Mp, rs, fc[2 * i + 1], hhs[CLS]) if fuse else None))
            for part in order if not fuse else (PATCH,):
                st.fc1(part, hs[part], hhs[part])
            for part in order:
                st.add(MLP, part, hhs[part], xs[part], rs if nst is not None else None)
            if nst is not None:
                qkv = x.new_empty((M, 3 * C))
            cls_qkv_done = fuse and nst is not None
            h = st.ln(MLP, x, (Mp, rs, fc[2 * i + 2], qkv[Mp:]) if cls_qkv_done else None)
        return SplitTokens(h[:Mp].view(B, n, C), h[Mp:])

    def _hip_ok(self, x: torch.Tensor) -> bool:
        return x.is_cuda and x.dtype == torch.bfloat16 and _ln_width_ok(x.shape[-1]) and all(b.folded for b in self.blocks)

    residual_in_gemm = True

    def _forward_hip(self, x: torch.Tensor) -> torch.Tensor:
        """The cls-first layout [B, T, C]: same math as the block loop, with x carrying the residual stream and h the normalised
        copy.  residual_in_gemm: _BlockStages.rows on one row range, all B*T rows in their PATCH forms: per block LN r1 w1 twice
        (67 MB each) instead of add+LN r2 w2 (135 MB each), for ~8 us of extra C reads in the two GEMMs.  Otherwise: biased proj /
        fc2, every residual add fused into the LayerNorm that follows it (vpr_add_layernorm_bf16).  qkv stays blk.qkv(h) either way."""
        B, T, C = x.shape
        x = x.contiguous()
        n0 = self.blocks[0].norm1
        h = ops.layernorm_bf16(x, n0.weight, n0.bias, n0.eps)

        def attention(blk, h):
            if _hip_attention_ok(C // blk.heads, T):
                return ops.attention_qkv_bf16(blk.qkv(h), blk.heads)
            qkv = blk.qkv(h).view(B, T, 3, blk.heads, C // blk.heads).permute(2, 0, 3, 1, 4)
            return F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2]).transpose(1, 2).reshape(B, T, C)

        stages = self._stages(x.device, self.residual_in_gemm)
        if self.residual_in_gemm:
            x2 = x.view(B * T, C)          # fresh tensor from forward(): safe to update in place
            for st in stages:
                h = st.rows(PATCH, attention(st.blk, h).view(B * T, C), x2).view(B, T, C)
            return h
        for st in stages:
            blk, (n2, nxt) = st.blk, st.norm
            x, h = ops.add_layernorm_bf16(x, blk.proj(attention(blk, h)), n2.weight, n2.bias, n2.eps)
            y = blk.fc2(st.fc1(PATCH, h.view(B * T, C))).view(B, T, C)
            x, h = ops.add_layernorm_bf16(x, y, nxt.weight, nxt.bias, nxt.eps)
        return h.view(B, T, C)

    def _cls_fused_consts(self, device: torch.device):
        """ClsLinearConsts of the LayerNorm-fused cls-row linears: entry 2i = block i's (norm1, qkv) with the
        cumulative bias before it (entry 0 unused: block 0's first LayerNorm is the embedding add+LN), entry
        2i+1 = block i's (norm2, fc1).  Static, rebuilt when the parameters change identity / version."""
        ps = [p for b in self.blocks for p in (b.qkv.weight, b.qkv.bias, b.fc1.weight, b.fc1.bias, b.proj.bias, b.fc2.bias,
                                               b.norm1.weight, b.norm1.bias, b.norm2.weight, b.norm2.bias)]
        return self._cache("_clsf", 2).get((device, tensor_key(*ps)), self._build_cls_fused_consts, (device,), ps)

    def _build_cls_fused_consts(self, device: torch.device) -> list:
        cum = self._cumulative_bias(device)
        out = []
        for i, b in enumerate(self.blocks):
            out.append(None if i == 0 else
                       ops.ClsLinearConsts.build(b.qkv.weight, b.qkv.bias, b.norm1.weight, b.norm1.bias, cum[2 * i - 1]))
            out.append(ops.ClsLinearConsts.build(b.fc1.weight, b.fc1.bias, b.norm2.weight, b.norm2.bias, cum[2 * i]))
        return out

    def _cumulative_bias(self, device: torch.device):
        """cum[2i] = sum of proj/fc2 biases up to and including block i's proj; cum[2i+1] adds its fc2
        (f32, one [2L, C] tensor; rebuilt when a bias changes identity or version, e.g. after a state-dict load)."""
        ps = [p for b in self.blocks for p in (b.proj.bias, b.fc2.bias)]
        return self._cache("_cum_bias", 2).get((device, tensor_key(*ps)), self._build_cumulative_bias, (device,), ps)

    def _build_cumulative_bias(self, device: torch.device) -> torch.Tensor:
        rows, acc = [], torch.zeros(self.embed_dim, dtype=torch.float32, device=device)
        for blk in self.blocks:
            acc = acc + blk.proj.bias.detach().float().to(device)
            rows.append(acc)
            acc = acc + blk.fc2.bias.detach().float().to(device)
            rows.append(acc)
        return torch.stack(rows).contiguous()

    def fold_layerscale(self) -> "DinoV2":
        """Fold every block.  The fold rewrites proj / fc2 in place on the current stream while `folded` flips on the host at
        once: the hand-over to any other stream that runs a forward next is `_fold_order` (ops.handover, lent in forward)."""
        rewrote = not all(b.folded for b in self.blocks)
        for blk in self.blocks:
            blk.fold_layerscale()
        if rewrote and self.pos_embed.is_cuda:
            self.__dict__["_fold_order"] = ops.handover()
        return self

    def flops_per_image(self) -> float:
        T, C, L = 1 + self.num_patches, self.embed_dim, len(self.blocks)
        per_block = 2 * T * C * 3 * C + 2 * T * C * C + 4 * T * T * C + 2 * 2 * T * C * 4 * C
        return L * per_block + 2 * self.num_patches * C * 3 * self.patch * self.patch
