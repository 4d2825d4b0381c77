"""f64 stage references, per-element bounds and wiring checks for ONE forward of the backbone's HIP paths, launch by launch
— TEST ORACLE of vpr_amd.backbone (_BlockStages and its three drivers), plus a plain-torch restatement of the launch chain
that runs without a device (so that the checker itself can be shown to fail).

A forward is a `Trace`: its stage records (`Stage`: block, stage, part, the operands captured BEFORE the launch and the
results captured AFTER it), the three cached constant sets the forward used, what it returned and what the cls tail hook
received.  tests/backbone_trace.py records one on the GPU; `restate()` below makes one on the CPU.

Everything is judged against `Params`: the module's own parameters after fold_layerscale(), bf16 values as f64 — never
a cached constant and never the weight tensor a launch happened to receive.  Every reference is ANCHORED on the captured
input of its stage, so errors do not compound and each bound is the bound of one launch; in exchange `check_trace` also
asserts the WIRING bit for bit (each stage's input is the captured output of the stage that must feed it; a launch on
one row range leaves the other rows of its buffer alone; the returned tokens are the last LayerNorm's output), without
which an anchored reference would pass a stage that read a stale buffer.

Bounds (u = 2^-24, hu = half the bf16 spacing, S = |A||W|^T, K the reduction length):
  library / skinny GEMM, bf16 out      oracle.gemm.gemm_bound: hu(y) + K u S + 2u(|s| + 2|b|)
  residual GEMM  x += a W^T            the same with x in the bias slot: ONE rounding of x + a W^T
  LayerNorm                            oracle.layernorm.ref_and_bound on v = x + c (c the f64 deferred bias), plus
                                       2 |γ_j| e_c / σ_i for the f32 running sum of the biases, e_c = 2L u Σ|biases|
  fc1 + GELU                           hu(f) + 1.13 (K u S + 8u(|s| + |b|)) (1 + 2^-8) + 16u(|z| + 1) (f32 activation)
  attention                            oracle.attention.bound
  embedding sum                        hu(raw) + hu(off) + hu(sum) + K u S: GEMM output and offsets each rounded once
  fused cls-row linear                 see _fused_linear_ref_bound
  row statistics of skinny mode 2      the (mean, M2) bounds of tests/test_skinny_edges_gpu.py on bf16(out) + c
The erf form on the patch rows is two launches (biased GEMM to bf16, then an in-place erf-GELU on those bf16 values):
each is judged on its own captured input.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import attention as oattn
from . import gemm as ogemm
from . import layernorm as oln

U = 2.0 ** -24
hu = ogemm.half_ulp_bf16
BF16 = torch.bfloat16

SPLIT_MODES = ("split_side", "split_after", "split_before", "fused")
CLS_FIRST_MODES = ("cf_resid", "cf_add")
MODES = SPLIT_MODES + CLS_FIRST_MODES
PATCH, CLS, ALL = "patch", "cls", "all"

MUTATIONS = ("c_att_for_c_mlp", "c_mlp_for_c_att", "cls_proj_bias_missing", "swap_norms", "fc1_wrong_block", "cum_bf16",
             "two_roundings", "gelu_form", "cls_pos_on_patch0", "ln_before_add", "patch_writes_cls", "consts_wrong_bias")


class StageFailure(AssertionError):
    def __init__(self, stage: str, block: int, what: str):
        super().__init__(f"block {block} stage {stage}: {what}")
        self.stage, self.block = stage, block


class Stage:
    """One launch.  inp / out: name -> tensor (CPU) before / after the launch; ref: operands kept by reference (weights,
    parameters, constant sets); whole: (buffer before, buffer after, first row) of the buffer an in-place launch wrote
    a row range of, where that could be captured (not next to a concurrent stream)."""
    def __init__(self, block, stage, part, label, inp, out, scalars=None, ref=None, whole=None, stream="main"):
        self.block, self.stage, self.part, self.label = block, stage, part, label
        self.inp, self.out, self.scalars, self.ref, self.whole, self.stream = inp, out, scalars or {}, ref or {}, whole, stream

    def key(self):
        return (self.block, self.stage, self.part, self.label)


class Trace:
    def __init__(self, stages, B, n, cum=None, embed=None, fused=None, result=None, hook=None):
        self.stages, self.B, self.n = stages, B, n
        self.cum, self.embed, self.fused, self.result, self.hook = cum, embed, fused, result, hook


class Params:
    """The DinoV2 module's parameters after fold_layerscale(): bf16 values as f64, and the deferred biases in f64."""
    def __init__(self, m):
        assert all(b.folded for b in m.blocks), "fold_layerscale() first"
        d = lambda t: t.detach().double().cpu()
        C = self.C = m.embed_dim
        self.patch, self.n = m.patch, m.num_patches
        self.pe_w, self.pe_b = d(m.patch_embed.weight).reshape(C, -1), d(m.patch_embed.bias)
        self.pos, self.cls = d(m.pos_embed)[0], d(m.cls_token).view(C)
        self.blocks = []
        for b in m.blocks:
            self.blocks.append({k: (d(getattr(b, k).weight), d(getattr(b, k).bias)) for k in ("norm1", "qkv", "proj", "norm2", "fc1", "fc2")})
            assert float(b.ls1.detach().min()) == float(b.ls1.detach().max()) == 1.0
        self.heads = m.blocks[0].heads
        self.norm, self.eps = (d(m.norm.weight), d(m.norm.bias)), m.norm.eps
        L = self.L = len(self.blocks)
        self.norm_after = [self.blocks[i + 1]["norm1"] for i in range(L - 1)] + [self.norm]
        self.c_att, self.c_mlp, acc = [], [], torch.zeros(C, dtype=torch.float64)
        for b in self.blocks:
            acc = acc + b["proj"][1]
            self.c_att.append(acc)
            acc = acc + b["fc2"][1]
            self.c_mlp.append(acc)
        # the f32 running sum of _build_cumulative_bias against the f64 one: 2L additions, each within u of the partial sum
        self.e_c = 2 * L * U * sum(b["proj"][1].abs() + b["fc2"][1].abs() for b in self.blocks)


def gelu_f64(z: torch.Tensor, form: str) -> torch.Tensor:
    if form == "tanh":
        return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    if form == "erf":
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))
    raise ValueError(form)


def im2col(img: torch.Tensor, P: int, kpad: int) -> torch.Tensor:
    """[B, Cin, H, W] -> [B*n, kpad] in the image's dtype: patch p of image b, its (c, y, x) pixels, zero-padded."""
    B, Cin, H, W = img.shape
    a = img.reshape(B, Cin, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), Cin * P * P)
    out = torch.zeros((a.shape[0], kpad), dtype=img.dtype)
    out[:, :a.shape[1]] = a
    return out


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def gemm_stage(a, w, b=None, x=None, K=None):
    """(y, bound, s, S) of bf16(a W^T [+ b | + x]): b [N] a bias, x [M, N] the residual stream the GEMM accumulates into."""
    a, w = a.double(), w.double()
    K = a.shape[1] if K is None else K
    s, S = a @ w.T, a.abs() @ w.abs().T
    add = b.double()[None, :] if b is not None else (x.double() if x is not None else torch.zeros(()))
    y = s + add
    pre = K * U * S + 2 * U * (s.abs() + 2 * add.abs())
    return y, hu(y.abs() + pre) + pre, s, S


def two_rounding_bound(y, s, S, K):
    """x += bf16(a W^T): the product rounded before the add."""
    pre = K * U * S + 2 * U * s.abs()
    pre = pre + hu(s.abs() + pre)
    return hu(y.abs() + pre) + pre


def fc1_ref_bound(h, w, b, form, allow_u=16.0):
    """GELU_form(h W^T + b) and the bf16-mode bound of the skinny edge tests (1.13-Lipschitz activation) plus
    allow_u · u (|z| + 1) for the f32 evaluation of the activation."""
    h, w, b = h.double(), w.double(), b.double()
    s, S = h @ w.T, h.abs() @ w.abs().T
    z = s + b[None, :]
    ref = gelu_f64(z, form)
    pre = 1.13 * (h.shape[1] * U * S + 8 * U * (s.abs() + b.abs()[None, :]))
    return ref, hu(ref.abs() + pre) + pre * (1 + 2.0 ** -8) + allow_u * U * (z.abs() + 1), z


def ln_stage(x, c, norm, eps, e_c=None):
    """LayerNorm(x + c; norm) in f64 and its bound; e_c: the per-column error of the f32 deferred bias."""
    v = x.double() + (c if c is not None else 0.0)
    ref, bound = oln.ref_and_bound(v, norm[0], norm[1], eps)
    if e_c is not None:
        sigma = ((v - v.mean(1, keepdim=True)).pow(2).mean(1, keepdim=True) + eps).sqrt()
        bound = bound + 2 * norm[0].abs()[None, :] * e_c[None, :] / sigma
    return ref, bound


def _fused_linear_ref_bound(x, c, e_c, norm, eps, w_scaled, w, b, gelu):
    """The cls-row linear of the fused launch, act(LN(x + c) W^T + b), restated as the kernel computes it with the GIVEN
    W' = w_scaled:  pre = rstd (x W'^T + c' - mean colsum) + b',  colsum = Σ W', c' = W' c, b' = b + W β (f64 here).
    Error of the kernel's f32 evaluation with its f32 constants (C = K):
      the K-loop K u S'; the products and sums 4u (|z| + |c'| + |mean colsum|); the constants as built in f32:
      e_c' = K u |W'||c| + |W'| e_c, e_colsum = K u Σ|W'|, e_b' = K u (|b| + |W||β|); the merged statistics 40 u max|v|
      on the mean and 2 · 40 u relative on rstd; u |pre| for the fma; through the activation (1.13 / 1) and one rounding."""
    x, Wp, W, b = x.double(), w_scaled.double(), w.double(), b.double()
    gamma, beta = norm
    K = x.shape[1]
    v = x + c
    mean = v.mean(1, keepdim=True)
    sigma = ((v - mean).pow(2).mean(1, keepdim=True) + eps).sqrt()
    rstd = 1.0 / sigma
    z, Sp = x @ Wp.T, x.abs() @ Wp.abs().T
    colsum, A = Wp.sum(1)[None, :], Wp.abs().sum(1)[None, :]
    cp = (Wp @ c)[None, :]
    bp = (b + W @ beta)[None, :]
    core = z + cp - mean * colsum
    pre = rstd * core + bp
    e_cp = K * U * (Wp.abs() @ c.abs())[None, :] + (Wp.abs() @ e_c)[None, :]
    e_bp = K * U * (b.abs() + W.abs() @ beta.abs())[None, :]
    e_mean = 40 * U * v.abs().amax(1, keepdim=True)
    e_pre = (rstd * (K * U * (Sp + mean.abs() * colsum.abs()) + 4 * U * (z.abs() + cp.abs() + (mean * colsum).abs())
                     + e_cp + mean.abs() * K * U * A + e_mean * colsum.abs())
             + 2 * 40 * U * (rstd * core).abs() + e_bp + U * (bp.abs() + pre.abs()))
    lip = 1.13 if gelu else 1.0
    ref = gelu_f64(pre, "tanh") if gelu else pre
    bound = hu(ref.abs() + lip * e_pre) + lip * e_pre * (1 + 2.0 ** -8) + (16 * U * (pre.abs() + 1) if gelu else 0.0)
    return ref, bound


# ------------------------------------------------------------------------------------------------ the constant builders
def check_consts(tr: Trace, p: Params, fail) -> None:
    C, L = p.C, p.L
    if tr.cum is not None:
        cum = tr.cum.double().cpu()
        if tuple(cum.shape) != (2 * L, C):
            fail("cumulative bias shape")
        for i in range(L):
            for row, ref, name in ((2 * i, p.c_att[i], "c_att"), (2 * i + 1, p.c_mlp[i], "c_mlp")):
                if not bool(((cum[row] - ref).abs() <= p.e_c + 1e-300).all()):
                    fail(f"cumulative bias row {row} is not {name}[{i}] within e_c")
    if tr.embed is not None:
        w, off = (t.cpu() for t in tr.embed)
        K = p.pe_w.shape[1]
        if not (torch.equal(w[:, :K].double(), p.pe_w) and bool((w[:, K:] == 0).all())):
            fail("patch-embedding weight is not the zero-padded conv weight")
        B, n = tr.B, tr.n
        ref = torch.cat([(p.pos[1:] + p.pe_b).repeat(B, 1), (p.cls + p.pos[0]).expand(B, C)])
        if tuple(off.shape) != tuple(ref.shape) or not bool(((off.double() - ref).abs() <= hu(ref)).all()):
            fail("token offsets are not pos[1+p] + bias | cls + pos[0] within half a bf16 spacing")
    if tr.fused is not None:
        if len(tr.fused) != 2 * L or tr.fused[0] is not None:
            fail("fused constant list")
        for j in range(1, 2 * L):
            i, blk = j // 2, p.blocks[j // 2]
            norm, lin, c = (blk["norm2"], blk["fc1"], p.c_att[i]) if j % 2 else (blk["norm1"], blk["qkv"], p.c_mlp[i - 1])
            ws, colsum, cprime, bprime = (t.double().cpu() for t in tr.fused[j])
            W, b = lin
            wg = W * norm[0][None, :]
            if not bool(((ws - wg).abs() <= hu(wg)).all()):
                fail(f"fused entry {j}: w_scaled is not W γ of its documented pair")
            A = ws.abs()
            if not bool(((colsum - ws.sum(1)).abs() <= C * U * A.sum(1)).all()):
                fail(f"fused entry {j}: colsum")
            if not bool(((cprime - ws @ c).abs() <= C * U * (A @ c.abs()) + A @ p.e_c).all()):
                fail(f"fused entry {j}: cprime is not W' c of its documented bias row")
            if not bool(((bprime - (b + W @ norm[1])).abs() <= C * U * (b.abs() + W.abs() @ norm[1].abs())).all()):
                fail(f"fused entry {j}: bprime")


# ------------------------------------------------------------------------------------------------------------- the checker
def check_trace(tr: Trace, p: Params, mode: str, gelu: str = "tanh", lib_two_roundings: bool = False,
                lib_gelu_allow_u: float = 16.0, sdpa_gate_only: bool = False) -> dict:
    """Judges every stage of `tr` (module docstring) and asserts the wiring; -> worst err/bound per stage kind.  Raises
    StageFailure naming the first stage that fails.  The three keyword switches are the measured allowances for what the
    LIBRARY computes on the patch rows (they never apply to the project's own kernels)."""
    assert mode in MODES and gelu in ("tanh", "erf")
    split, fused = mode in SPLIT_MODES, mode == "fused" and gelu == "tanh" and p.C % 32 == 0
    B, n, C, L = tr.B, tr.n, p.C, p.L
    T, Mp = 1 + n, B * n
    M = B * T
    worst = {}
    by = {}
    for s in tr.stages:
        if s.key() in by:
            raise StageFailure(s.stage, s.block, "recorded twice")
        by[s.key()] = s

    def get(i, stage, part, label=None, need=True):
        hits = [s for k, s in by.items() if k[:3] == (i, stage, part) and (label is None or k[3] == label)]
        if len(hits) != 1:
            if need or hits:
                raise StageFailure(stage, i, f"{len(hits)} records of part {part}")
            return None
        return hits[0]

    def judge(s, kind, got, ref, bound, what=""):
        got = got.double().reshape(ref.shape)
        if not bool(torch.isfinite(got).all()):
            raise StageFailure(s.stage, s.block, f"{what} non-finite output")
        err = (got - ref).abs()
        ratio = float((err / bound).max()) if err.numel() else 0.0
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        if ratio > 1.0:
            at = int((err / bound).argmax())
            raise StageFailure(s.stage, s.block, f"{what} part {s.part}: worst err/bound {ratio:.3f} (err {float(err.reshape(-1)[at]):.3e}) "
                                                 f"at row {at // ref.shape[-1]} column {at % ref.shape[-1]}")

    def wired(s, got, want, what):
        if not _same(got, want):
            raise StageFailure(s.stage, s.block, f"wiring: {what}")

    def scalars(s, **want):
        for name, value in want.items():
            if name in s.scalars and s.scalars[name] != value:
                raise StageFailure(s.stage, s.block, f"scalar argument {name} = {s.scalars[name]!r}, expected {value!r}")

    def untouched(s):
        if s.whole is None:
            return
        before, after, row0 = s.whole
        rows = next(iter(s.out.values())).shape[0] if s.stage != "attention" else 0
        keep = torch.ones(before.shape[0], dtype=torch.bool)
        keep[row0:row0 + rows] = False
        if not _same(before[keep], after[keep]):
            raise StageFailure(s.stage, s.block, f"part {s.part}: the launch changed rows outside [{row0}, {row0 + rows})")

    parts = (PATCH, CLS) if split else (ALL,)
    span = {PATCH: slice(0, Mp), CLS: slice(Mp, M), ALL: slice(0, M)}

    def fail_consts(what):
        raise StageFailure("consts", -1, what)
    check_consts(tr, p, fail_consts)

    # ---- what precedes the blocks
    if split:
        P = p.patch
        s = get(-1, "embed_patchify", ALL)
        a = s.out["a"]
        img = s.inp["img"]
        if not _same(a, im2col(img, P, a.shape[1])):
            raise StageFailure(s.stage, -1, "not the zero-padded im2col of the image")
        worst["embed_patchify"] = 0.0
        g = get(-1, "embed_gemm", PATCH)
        wired(g, g.inp["a"], a, "the GEMM does not read the patchify output")
        K = p.pe_w.shape[1]
        y, bound, sg, Sg = gemm_stage(a[:, :K], p.pe_w)
        judge(g, "embed_gemm", g.out["y"], y, bound)
        untouched(g)
        scalars(s, patch=P, kpad=(p.pe_w.shape[1] + 63) // 64 * 64, lead_rows=0)
        e = get(-1, "embed_add_ln", ALL)
        scalars(e, eps=p.eps)
        wired(e, e.inp["raw"][:Mp], g.out["y"], "add+LN does not read the GEMM output")
        if bool((e.inp["raw"][Mp:] != 0).any()):
            raise StageFailure(e.stage, -1, "the cls rows of the raw-token buffer are not zero")
        off_ref = torch.cat([(p.pos[1:] + p.pe_b).repeat(B, 1), (p.cls + p.pos[0]).expand(B, C)])
        ref = torch.cat([y, torch.zeros(B, C, dtype=torch.float64)]) + off_ref
        S_all = torch.cat([Sg, torch.zeros(B, C, dtype=torch.float64)])
        raw_abs = torch.cat([y.abs(), torch.zeros(B, C, dtype=torch.float64)]) + K * U * S_all
        b_sum = hu(raw_abs) + hu(off_ref) + K * U * S_all
        judge(e, "embed_add_ln.sum", e.out["x"], ref, b_sum + hu(ref.abs() + b_sum), "sum")
        n0 = p.blocks[0]["norm1"]
        judge(e, "embed_add_ln.ln", e.out["h"], *ln_stage(e.out["x"], None, n0, p.eps), "LayerNorm")
        x_now, h_now = e.out["x"], e.out["h"]
    else:
        s = get(-1, "ln_first", ALL)
        scalars(s, eps=p.eps)
        judge(s, "ln_first", s.out["h"], *ln_stage(s.inp["x"].reshape(M, C), None, p.blocks[0]["norm1"], p.eps))
        x_now, h_now = s.inp["x"].reshape(M, C), s.out["h"].reshape(M, C)

    lin_pending = None          # the cls rows a fused LayerNorm launch produced for the next linear stage
    for i, blk in enumerate(p.blocks):
        # ---- qkv
        outs = []
        for part in parts:
            s = get(i, "qkv", part, need=not (fused and part == CLS and i > 0))
            if s is None:
                outs.append(lin_pending)
                continue
            wired(s, s.inp["h"], h_now[span[part]], "qkv does not read the LayerNorm output before it")
            y, bound, _, _ = gemm_stage(s.inp["h"].reshape(-1, C), *blk["qkv"])
            judge(s, "qkv", s.out["y"], y, bound)
            untouched(s)
            outs.append(s.out["y"].reshape(-1, 3 * C))
        qkv = torch.cat(outs)
        # ---- attention
        s = get(i, "attention", ALL)
        scalars(s, heads=p.heads, B=B, T=T, body_tokens=n)
        if s.label == "sdpa":
            q5 = qkv.view(B, T, 3, p.heads, 64).permute(2, 0, 3, 1, 4)
            for j, name in enumerate("qkv"):
                wired(s, s.inp[name], q5[j], f"SDPA's {name} is not the projection just written")
            att = s.out["att"].transpose(1, 2).reshape(M, C)
            tok = qkv.view(B, T, 3 * C)
            bound, ref = oattn.bound(tok, p.heads, terms=T, gate=None)
            err = (att.double().view(B, T, C) - ref).abs()
            worst["attention.sdpa_vs_derived"] = float((err / bound).max())
            gate = torch.full_like(bound, oattn.GATE)
            judge(s, "attention.sdpa", att, ref.reshape(M, C), (gate if sdpa_gate_only else torch.minimum(bound, gate)).reshape(M, C))
        else:
            wired(s, s.inp["qkv"], qkv, "attention does not read the qkv rows just written")
            att = s.out["att"].reshape(M, C)
            tok = oattn.from_split_rows(qkv, B, T, n) if split else qkv.view(B, T, 3 * C)
            bound, ref = oattn.bound(tok, p.heads)
            if split:
                bound, ref = oattn.to_split_rows(bound, n), oattn.to_split_rows(ref, n)
            judge(s, "attention", att, ref.reshape(M, C), bound.reshape(M, C))
        # ---- the two halves
        a_now = att
        for half, (add_name, ln_name, lin_name, c_ref, norm) in enumerate((("proj_add", "ln2", "proj", p.c_att[i], blk["norm2"]),
                                                                           ("fc2_add", "ln_next", "fc2", p.c_mlp[i], p.norm_after[i]))):
            W, bias = blk[lin_name]
            x_after, stats = [], None
            for part in parts:
                s = get(i, add_name, part)
                untouched(s)
                wired(s, s.inp["a"], a_now[span[part]], f"{add_name} does not read the rows of the stage before it")
                if mode == "cf_add":
                    y, bound, _, _ = gemm_stage(s.inp["a"], W, bias)
                    judge(s, add_name, s.out["y"], y, bound)
                    x_after.append(s.out["y"])
                    continue
                wired(s, s.inp["x"], x_now[span[part]], "the residual stream before this half is not the one after the previous half")
                y, bound, sv, Sv = gemm_stage(s.inp["a"], W, x=s.inp["x"])
                if lib_two_roundings and s.label == "addmm_":
                    bound = two_rounding_bound(y, sv, Sv, s.inp["a"].shape[1])
                judge(s, add_name + ("" if part == ALL else "." + part), s.out["x"], y, bound)
                x_after.append(s.out["x"])
                if "row_stats" in s.out:            # per 16 columns the (mean, centred sum of squares) of bf16(out) + c, f32 sums of 16
                    stats = s
                    t = s.out["x"].double() + c_ref
                    blocks = t.view(t.shape[0], -1, 16)
                    mean = blocks.mean(-1)
                    dev = blocks - mean[..., None]
                    mag = blocks.abs().amax(-1) + p.e_c.view(-1, 16).amax(-1) / U / 8     # 8 u mag then holds e_c: the kernel adds the f32 c
                    e_d = (10 * U * mag)[..., None]
                    rs = s.out["row_stats"].double().permute(1, 0, 2)
                    judge(s, add_name + ".stats", rs[..., 0], mean, 8 * U * mag + 1e-300, "row_stats mean")
                    judge(s, add_name + ".stats", rs[..., 1], (dev ** 2).sum(-1),
                          (2 * dev.abs() * e_d + e_d ** 2).sum(-1) + 40 * U * (dev ** 2).sum(-1) + 1e-300, "row_stats M2")
            x_after = torch.cat(x_after)
            # ---- the LayerNorm that ends the half
            lin_pending = None
            h_parts = []
            for s in [q for q in (get(i, ln_name, part, need=False) for part in (ALL, PATCH, CLS)) if q is not None]:
                sl = span[s.part]
                scalars(s, eps=p.eps)
                if mode == "cf_add":
                    wired(s, s.inp["x"].reshape(M, C), x_now, "add+LN does not read the residual stream")
                    wired(s, s.inp["res"].reshape(M, C), x_after, "add+LN does not read the linear output before it")
                    want = (s.inp["x"].float() + s.inp["res"].float()).to(BF16)
                    wired(s, s.out["x"], want, "the sum is not x + res rounded once")
                    judge(s, ln_name, s.out["h"], *ln_stage(s.out["x"].reshape(M, C), None, norm, p.eps))
                    x_after = s.out["x"].reshape(M, C)
                else:
                    wired(s, s.inp["x"], x_after[sl], "LayerNorm does not read the stream after the residual GEMM before it")
                    judge(s, ln_name, s.out["h"], *ln_stage(s.inp["x"], c_ref, norm, p.eps, p.e_c))
                if "lin" in s.out:
                    if stats is None or not _same(s.inp["row_stats"], stats.out["row_stats"]):
                        raise StageFailure(s.stage, i, "wiring: row_stats are not those the skinny launch before it wrote")
                    row0 = s.scalars["cls_row0"]
                    if row0 != Mp or bool(s.scalars["gelu"]) != (half == 0):
                        raise StageFailure(s.stage, i, f"fused launch: cls_row0 {row0}, gelu {s.scalars['gelu']}")
                    nb = blk["fc1"] if half == 0 else p.blocks[i + 1]["qkv"]
                    ref, bound = _fused_linear_ref_bound(s.inp["x"][Mp:], c_ref, p.e_c, norm, p.eps, s.ref["consts"][0].cpu(),
                                                         nb[0], nb[1], half == 0)
                    judge(s, ln_name + ".lin", s.out["lin"], ref, bound, "cls-row linear")
                    lin_pending = s.out["lin"]
                h_parts.append((sl.start, s.out["h"].reshape(-1, C)))
            h_now = torch.cat([t for _, t in sorted(h_parts, key=lambda q: q[0])])
            if h_now.shape[0] != M:
                raise StageFailure(ln_name, i, f"LayerNorm launches cover {h_now.shape[0]} of {M} rows")
            x_now = x_after
            if half == 1:
                break
            # ---- fc1 + GELU
            outs = []
            for part in parts:
                lib_erf = gelu == "erf" and part != CLS
                s = get(i, "fc1", part, label="addmm" if lib_erf else None, need=not (fused and part == CLS))
                if s is None:
                    outs.append(lin_pending)
                    continue
                wired(s, s.inp["h"], h_now[span[part]], "fc1 does not read the LayerNorm output before it")
                untouched(s)
                if lib_erf:
                    y, bound, _, _ = gemm_stage(s.inp["h"], *blk["fc1"])
                    judge(s, "fc1.pre", s.out["y"], y, bound)
                    g2 = get(i, "fc1", part, label="gelu_")
                    wired(g2, g2.inp["y"], s.out["y"], "gelu_ does not read the biased GEMM's output")
                    z = g2.inp["y"].double()
                    ref = gelu_f64(z, "erf")
                    judge(g2, "fc1.gelu_", g2.out["y"], ref, hu(ref) + lib_gelu_allow_u * U * (z.abs() + 1))
                    outs.append(g2.out["y"])
                    continue
                library = s.label == "_addmm_activation"
                ref, bound, _ = fc1_ref_bound(s.inp["h"], *blk["fc1"], gelu, lib_gelu_allow_u if library else 16.0)
                judge(s, "fc1" + ("" if part == ALL else "." + part), s.out["y"], ref, bound)
                outs.append(s.out["y"])
            a_now = torch.cat(outs)

    # ---- what the forward returned, and what the hook saw
    last = h_now
    if split:
        patch, cls = tr.result
        if not (_same(patch, last[:Mp]) and _same(cls, last[Mp:])):
            raise StageFailure("result", L - 1, "SplitTokens is not the last LayerNorm's output")
    elif not _same(tr.result, last):
        raise StageFailure("result", L - 1, "the returned tokens are not the last LayerNorm's output")
    if mode == "split_side":
        if tr.hook is None or not _same(tr.hook, last[Mp:]):
            raise StageFailure("result", L - 1, "cls_tail_hook did not receive the final cls rows")
    return worst


# -------------------------------------------------------------------------------------- the restatement (CPU, plain torch)
def _lin32(a, w, b=None):
    y = a.float() @ w.float().T
    return y if b is None else y + b.float()[None, :]


def _gelu32(z, form):
    return F.gelu(z, approximate="tanh" if form == "tanh" else "none")


def _ln32(v32, norm, eps):
    return F.layer_norm(v32, (v32.shape[-1],), norm[0].float(), norm[1].float(), eps).to(BF16)


def _row_stats32(t32):
    """[N/16, M, 2] f32: per 16-column block the (mean, centred sum of squares) of t32 [M, N]."""
    blocks = t32.view(t32.shape[0], -1, 16)
    mean = blocks.mean(-1)
    return torch.stack([mean, ((blocks - mean[..., None]) ** 2).sum(-1)], -1).permute(1, 0, 2).contiguous()


class ClsConsts(NamedTuple):
    w_scaled: torch.Tensor
    colsum: torch.Tensor
    cprime: torch.Tensor
    bprime: torch.Tensor


def _cls_consts32(lin, norm, c32):
    w32 = lin[0].float()
    ws = (w32 * norm[0].float()[None, :]).to(BF16)
    return ClsConsts(ws, ws.float().sum(1), ws.float() @ c32, lin[1].float() + w32 @ norm[1].float())


def restate(p: Params, img: torch.Tensor, mode: str, gelu: str = "tanh", mutate: Optional[str] = None) -> Trace:
    """The launch chain of one forward in plain torch on the CPU: f32 accumulation, one bf16 rounding where the kernels
    round, the deferred biases as an f32 running sum.  Emits the stage records the recorder makes of the real forward.
    mutate: one of MUTATIONS — the same chain with that one fault (tests/test_backbone_stages_cpu.py)."""
    assert mode in MODES and (mutate is None or mutate in MUTATIONS)
    split, fused = mode in SPLIT_MODES, mode == "fused" and gelu == "tanh"
    side = mode == "split_side"
    B, C, L, P, n = img.shape[0], p.C, p.L, p.patch, p.n
    T, Mp = 1 + n, B * n
    M = B * T
    st = []
    parts = (PATCH, CLS) if split else (ALL,)
    span = {PATCH: slice(0, Mp), CLS: slice(Mp, M), ALL: slice(0, M)}
    label = {"gemm_b": {PATCH: "addmm", CLS: "skinny:0", ALL: "linear"}, "add": {PATCH: "addmm_", CLS: "skinny:2", ALL: "addmm_"}}

    cum, acc = [], torch.zeros(C)
    for b in p.blocks:
        acc = acc + b["proj"][1].float()
        cum.append(acc)
        acc = acc + b["fc2"][1].float()
        cum.append(acc)
    cum = torch.stack(cum)
    if mutate == "cum_bf16":
        cum = cum.to(BF16).float()
    tr = Trace(st, B, n, cum=None if mode == "cf_add" else cum)

    K = p.pe_w.shape[1]
    if split:
        kpad = (K + 63) // 64 * 64
        a = im2col(img.to(BF16), P, kpad)
        w = torch.zeros((C, kpad), dtype=BF16)
        w[:, :K] = p.pe_w.to(BF16)
        pos = p.pos.float()
        body = (pos[1:] + p.pe_b.float()).to(BF16)
        if mutate == "cls_pos_on_patch0":
            body[0] = (pos[0] + pos[1] + p.pe_b.float()).to(BF16)
        off = torch.cat([body.repeat(B, 1), (pos[0] + p.cls.float()).to(BF16).expand(B, C)]).contiguous()
        tr.embed = (w, off)
        if mutate == "cls_pos_on_patch0":       # the builder is right, the launch adds a wrong row: keep the constants clean
            tr.embed = (w, torch.cat([(pos[1:] + p.pe_b.float()).to(BF16).repeat(B, 1), off[Mp:]]))
        st.append(Stage(-1, "embed_patchify", ALL, "patchify_bf16", {"img": img.to(BF16)}, {"a": a}))
        raw = torch.zeros((M, C), dtype=BF16)
        before = raw.clone()
        raw[:Mp] = _lin32(a, w).to(BF16)
        st.append(Stage(-1, "embed_gemm", PATCH, "mm", {"a": a}, {"y": raw[:Mp].clone()}, whole=(before, raw.clone(), 0)))
        x = (raw.float() + off.float()).to(BF16)
        h = _ln32(x.float(), p.blocks[0]["norm1"], p.eps)
        st.append(Stage(-1, "embed_add_ln", ALL, "add_layernorm_bf16", {"raw": raw.clone(), "off": off}, {"x": x.clone(), "h": h}))
    else:
        tok = _lin32(im2col(img.to(BF16), P, K), p.pe_w.to(BF16), p.pe_b).view(B, n, C)
        x = (torch.cat([p.cls.float().expand(B, 1, C), tok], 1) + p.pos.float()).to(BF16).reshape(M, C)
        h = _ln32(x.float(), p.blocks[0]["norm1"], p.eps)
        st.append(Stage(-1, "ln_first", ALL, "layernorm_bf16", {"x": x.clone()}, {"h": h}))

    norms2 = [b["norm2"] for b in p.blocks]
    norms_after = list(p.norm_after)
    if mutate == "swap_norms":
        norms2[1], norms_after[1] = norms_after[1], norms2[1]
    if fused:
        consts = [None]
        for i, b in enumerate(p.blocks):
            if i:
                consts.append(_cls_consts32(b["qkv"], b["norm1"], cum[2 * i] if mutate == "consts_wrong_bias" else cum[2 * i - 1]))
            consts.append(_cls_consts32(b["fc1"], b["norm2"], cum[2 * i]))
        tr.fused = consts

    pending = None
    for i, blk in enumerate(p.blocks):
        last = i == L - 1
        qkv = torch.empty((M, 3 * C), dtype=BF16)
        for part in parts:
            if fused and part == CLS and i > 0:
                qkv[span[part]] = pending
                continue
            hh = h[span[part]]
            before = qkv.clone()
            qkv[span[part]] = _lin32(hh, *blk["qkv"]).to(BF16)
            st.append(Stage(i, "qkv", part, label["gemm_b"][part], {"h": hh.clone()}, {"y": qkv[span[part]].clone()},
                            whole=None if side else (before, qkv.clone(), span[part].start)))
        tok = oattn.from_split_rows(qkv, B, T, n) if split else qkv.view(B, T, 3 * C)
        att = oattn.attention_f64(tok, p.heads).to(BF16)
        att = oattn.to_split_rows(att, n) if split else att.reshape(M, C)
        st.append(Stage(i, "attention", ALL, "attention", {"qkv": qkv.clone()}, {"att": att}, {"heads": p.heads}))
        a_now = att
        for half in (0, 1):
            add_name, ln_name, lin_name = (("proj_add", "ln2", "proj"), ("fc2_add", "ln_next", "fc2"))[half]
            W, bias = blk[lin_name]
            norm = (norms2, norms_after)[half][i]
            c = cum[2 * i + half]
            if (mutate == "c_att_for_c_mlp" and half == 1 and i == 1) or (mutate == "c_mlp_for_c_att" and half == 0 and i == 1):
                c = cum[2 * i + 1 - half]
            x_prev = x.clone()
            want_stats = fused and not (half == 1 and last)
            rs = None
            if mode == "cf_add":
                y = _lin32(a_now, W, bias).to(BF16)
                st.append(Stage(i, add_name, ALL, "linear", {"a": a_now.clone()}, {"y": y}))
                s = (x.float() + y.float()).to(BF16)
                h = _ln32(s.float(), norm, p.eps)
                st.append(Stage(i, ln_name, ALL, "add_layernorm_bf16", {"x": x.clone(), "res": y}, {"x": s.clone(), "h": h}))
                x = s
            else:
                for part in parts:
                    sl = span[part]
                    xb, prod = x[sl].clone(), _lin32(a_now[sl], W)
                    if mutate == "two_roundings" and part != CLS and i == 1:
                        prod = prod.to(BF16).float()
                    before = x.clone()
                    x[sl] = (xb.float() + prod).to(BF16)
                    if mutate == "patch_writes_cls" and part == PATCH and i == 1 and half == 0:
                        x[Mp:] = (x[Mp:].float() * (1 + 2.0 ** -6)).to(BF16)
                    out = {"x": x[sl].clone()}
                    lab = label["add"][part]
                    if want_stats and part == CLS:
                        rs = _row_stats32(x[sl].float() + c[None, :])
                        out["row_stats"], lab = rs, lab + "+stats"
                    st.append(Stage(i, add_name, part, lab, {"x": xb, "a": a_now[sl].clone()}, out,
                                    whole=None if side else (before, x.clone(), sl.start)))
                src = x_prev if (mutate == "ln_before_add" and i == 1 and half == 0) else x
                v = src.float() + c[None, :]
                if mutate == "cls_proj_bias_missing" and split and i >= 1:
                    v[Mp:] = v[Mp:] - p.blocks[1]["proj"][1].float()[None, :]
                h = _ln32(v, norm, p.eps)
                for part in (PATCH, CLS) if side else (ALL,):
                    sl = span[part]
                    s = Stage(i, ln_name, part, "bias_layernorm_bf16", {"x": src[sl].clone(), "c": c.clone()}, {"h": h[sl].clone()})
                    if want_stats:
                        k = consts[2 * i + 1 + half]
                        vc = v[Mp:]
                        mean = vc.mean(1, keepdim=True)
                        rstd = 1.0 / ((vc - mean).pow(2).mean(1, keepdim=True) + p.eps).sqrt()
                        lin = rstd * (_lin32(src[Mp:], k.w_scaled) + k.cprime[None, :] - mean * k.colsum[None, :]) + k.bprime[None, :]
                        pending = (_gelu32(lin, "tanh") if half == 0 else lin).to(BF16)
                        s.label = "bias_layernorm_cls_linear_bf16"
                        s.inp["row_stats"], s.out["lin"] = rs, pending
                        s.scalars, s.ref = {"cls_row0": Mp, "gelu": half == 0, "eps": p.eps}, {"consts": k}
                    st.append(s)
            if half == 1:
                break
            w1, b1 = p.blocks[1]["fc1"] if (mutate == "fc1_wrong_block" and i == 2) else blk["fc1"]
            form = gelu if mutate != "gelu_form" else ("erf" if gelu == "tanh" else "tanh")
            hid = torch.empty((M, w1.shape[0]), dtype=BF16)
            for part in parts:
                sl = span[part]
                if fused and part == CLS:
                    hid[sl] = pending
                    continue
                before = hid.clone()
                whole = lambda: None if side else (before, hid.clone(), sl.start)
                if gelu == "erf" and part != CLS:
                    z = _lin32(h[sl], w1, b1).to(BF16)
                    hid[sl] = z
                    st.append(Stage(i, "fc1", part, "addmm", {"h": h[sl].clone()}, {"y": z}, whole=whole()))
                    hid[sl] = _gelu32(z.float(), form).to(BF16)
                    st.append(Stage(i, "fc1", part, "gelu_", {"y": z}, {"y": hid[sl].clone()}))
                    continue
                hid[sl] = _gelu32(_lin32(h[sl], w1, b1), form).to(BF16)
                lab = {PATCH: "_addmm_activation", ALL: "_addmm_activation", CLS: "skinny:1" if gelu == "tanh" else "skinny:4"}[part]
                st.append(Stage(i, "fc1", part, lab, {"h": h[sl].clone()}, {"y": hid[sl].clone()}, whole=whole()))
            a_now = hid
    tr.result = (h[:Mp].clone(), h[Mp:].clone()) if split else h.clone()
    tr.hook = h[Mp:].clone() if side else None
    return tr
