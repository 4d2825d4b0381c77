"""CPU restatement of the regression / angle heads — TEST ORACLE.

  mlp_head            DINOv2RegressionModel.regressor  dinov2salad/dinov2salad_validation.py:43-47,52
                      Swin-Base MLP head (Dropout = identity in eval)
                                                       swin_transformer/val_and_test_swin_2.py:168-177
                      sin/cos MLP head   angle_prediction/swin/swin_angle_finetuning_gemini.py:101-106
  linear head         swin_transformer/swin_validation.py:41,46
  unit-normalised [sin, cos]  F.normalize(out, dim=1, p=2, eps=1e-6)
                      angle_prediction/swin/swin_angle_finetuning_sin_cos.py:56-62
  swin_pooler         HF SwinModel: LayerNorm(last hidden) -> mean over tokens
                      (call site swin_transformer/swin_validation.py:43-45)
Pinned by tests/golden/head_dinov2salad.json (reference class imported) and swin_pool_head.npz.

Error bounds of the HIP kernels against these f64 restatements (u = 2^-24, the unit roundoff of f32; the style of
oracle/gemm.py): mlp_head_bound, ln_meanpool_bound; exact_head_operands gives operands on which every kernel form
must return the f64 result bit for bit; mlp_head_emulated restates the kernels' arithmetic on the CPU (f32, K-steps of
32, split-K slices, bf16 (hi, lo) planes), with switches for the mistakes the bounds must reject
(tests/test_oracle_selfchecks.py).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MAX_SLICES = 64          # no form of the first layer splits K into more slices (pose_f32_plan, pose_split_plan / VPR_POSE_KS <= 64)


def _normalize_pair(out: torch.Tensor, off: int) -> torch.Tensor:
    """F.normalize(p=2, eps=1e-6) of the columns [off, off + 1].  off < 0 (or None): no normalise.  A non-negative off needs
    off + 2 <= n_out, the rule of include/vpr_amd.h: anything else raises, as every entry point of the library refuses it."""
    if off is None or off < 0:
        return out
    if off + 2 > out.shape[1]:
        raise RuntimeError(f"sincos_offset {off} needs sincos_offset + 2 <= n_out = {out.shape[1]}")
    out = out.clone()
    out[:, off:off + 2] = F.normalize(out[:, off:off + 2], dim=1, p=2, eps=1e-6)
    return out


def mlp_head(x, W1, b1, W2, b2, sincos_offset: int = -1, dtype=torch.float64):
    x, W2, b2 = x.to(dtype), W2.to(dtype), b2.to(dtype)
    if W1 is not None:
        x = torch.relu(x @ W1.to(dtype).T + b1.to(dtype))
    return _normalize_pair(x @ W2.T + b2, sincos_offset)


def swin_pooler(last_hidden, gamma, beta, eps: float, dtype=torch.float64):
    """[B,T,H] -> [B,H]: LayerNorm over H then mean over T."""
    h = last_hidden.to(dtype)
    y = F.layer_norm(h, (h.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)
    return y.mean(dim=1)


def ln_meanpool_head(last_hidden, gamma, beta, eps, Wh=None, bh=None, sincos_offset: int = -1,
                     dtype=torch.float64):
    pooled = swin_pooler(last_hidden, gamma, beta, eps, dtype)
    if Wh is None:
        return pooled, None
    return pooled, _normalize_pair(pooled @ Wh.to(dtype).T + bh.to(dtype), sincos_offset)


# ---------------------------------------------------------------------------------------------- error bounds
def normalized_pair_bound(raw: torch.Tensor, bound: torch.Tensor, off: int) -> torch.Tensor:
    """Bound after the pair normalise.  raw [B, n_out] f64 un-normalised reference, bound its per-element bound.
    With v the exact pair, v' = v + δ the computed one and r = |v| >= 1e-6 (so the eps clamp is idle):
        |v/|v| - v'/|v'|| <= |v - v'|/|v| + ||v'| - |v||/|v| <= 2 |δ| / r,
    plus the kernel's own a*a + b*b, sqrt and divide: a few roundings of values of magnitude <= 1 (4 u).
    Columns outside the pair keep their bound.  The bound is useless (inf) for r -> 0: test inputs keep r away from 0."""
    if off is None or off < 0:
        return bound
    out = bound.clone()
    r = raw[:, off:off + 2].norm(dim=1)
    d = bound[:, off:off + 2].norm(dim=1)
    pair = torch.where(r >= 1e-6, 2 * d / r, torch.full_like(r, float("inf"))) + 4 * U
    out[:, off] = pair
    out[:, off + 1] = pair
    return out


def mlp_head_bound(x, W1, b1, W2, b2, split: bool, sincos_offset: int = -1, slices: int = MAX_SLICES):
    """Per-element bound [B, n_out] (f64) of |kernel - mlp_head(f64)| for vpr_pose_head (split=False), vpr_pose_head_split /
    vpr_pose_head_fused (split=True) and the linear head (W1 None), before the pair normalise unless sincos_offset >= 0.

    First layer, unit j of row b: z_j = Σ_d x_d W1_jd + b1_j, S_j = Σ_d |x_d| |W1_jd| + |b1_j|.
      * f32 accumulation: D products are added one after the other in some order (MFMA steps, waves, LDS), then `slices`
        slabs and the bias.  Every addition rounds a partial sum of magnitude <= S_j, so
            |fl(z_j) - z_j| <= (D + slices) u S_j.
        (The products are exact in the exact-f32 form's fmaf chain; the bf16 x bf16 products of the split forms are exact
        in f32.)
      * split forms: v = hi + lo + e with hi = bf16(v), lo = bf16(v - hi); four products replace x_d W1_jd.  The budget
        csrc/pose_head.hip documents is 2^-16 |x_d W1_jd| per product, hence + 2^-16 Σ_d |x_d| |W1_jd|.
    ReLU is 1-Lipschitz: the hidden unit h_j = relu(z_j) inherits the bound e_j — and where z_j < -e_j the computed
    pre-activation is negative too, both sides give exactly 0 and the unit carries no error at all (e_j = 0).
    Second layer, output o: the error of h reaches it through Σ_j |W2_oj| e_j; its own sum is hidden fused multiply-adds,
    6 + 2 cross-lane / cross-wave additions and the bias (hidden + 8 roundings of partial sums <= Σ_j |W2_oj| h_j + |b2_o|):
        |out_o - ref_o| <= Σ_j |W2_oj| e_j + (hidden + 8) u (Σ_j |W2_oj| h_j + |b2_o|).
    Linear head (W1 None): D fmaf steps over 256 threads, a block sum and the bias: (D + 8) u (Σ_d |x_d| |W2_od| + |b2_o|).
    Normalised pair: normalized_pair_bound."""
    x, W2, b2 = x.double(), W2.double(), b2.double()
    if W1 is None:
        D = x.shape[1]
        raw = x @ W2.T + b2
        bound = (D + 8) * U * (x.abs() @ W2.abs().T + b2.abs())
        return normalized_pair_bound(raw, bound, sincos_offset)
    W1, b1 = W1.double(), b1.double()
    hidden, D = W1.shape
    P = x.abs() @ W1.abs().T                          # Σ_d |x_d| |W1_jd|
    e = (D + slices) * U * (P + b1.abs())
    if split:
        e = e + 2.0 ** -16 * P
    z = x @ W1.T + b1
    e = torch.where(z < -e, torch.zeros_like(e), e)
    h = torch.relu(z)
    raw = h @ W2.T + b2
    bound = e @ W2.abs().T + (hidden + 8) * U * (h @ W2.abs().T + b2.abs())
    return normalized_pair_bound(raw, bound, sincos_offset)


def ln_meanpool_bound(last_hidden, gamma, beta, eps, Wh=None, bh=None, sincos_offset: int = -1):
    """(pooled_bound [B, H], out_bound [B, n_out] or None), f64: per-element bounds of |vpr_ln_meanpool_head - f64|,
    derived from the depth of the kernel's sums (an element of a sum that passes through d additions contributes at most
    d u times its magnitude).  A lane holds H / 64 elements of a row, added one after the other, then 6 cross-lane
    additions: d = H / 64 + 5 <= 29 for each of the two sums of a token.
      mean      δm_t = (d + 1) u mean_i |x_ti|                      (the sum, one division)
      variance  the kernel centres on its own mean m̂: mean_i (x - m̂)^2 = var + (m - m̂)^2 exactly, each term is rounded
                twice (the difference, the fma) and the sum has depth d:  relative error (d + 3) u + δm_t^2 / σ_t^2
      rstd      half of that, + 3 u (the eps addition, sqrt, divide);  σ_t = sqrt(var_t + eps), ẑ = (x - mean) / σ
      y         (x - m̂) rstd γ + β: the mean's error enters as δm_t |γ_j| / σ_t, the difference, two products and the
                addition are one rounding each:
        δ_tj = |γ_j| δm_t / σ_t + |γ_j ẑ_tj| (((d + 3) u + δm_t^2 / σ_t^2) / 2 + 6 u) + u |y_tj|,   y = ẑ γ + β,
    i.e. relative to |x - mean| rstd |γ| + |β|, plus the mean's own error carried by rstd |γ|.
    Pooling: a wave adds its ceil(T / 16) tokens one after the other, the 16 wave sums meet in a tree of depth 6, one
    division:   pooled_bound_j = mean_t δ_tj + (ceil(T / 16) + 7) u · mean_t |y_tj|.
    Head: Σ_j |Wh_oj| pooled_bound_j + 32 u (Σ_j |Wh_oj| |pooled_j| + |bh_o|)  (H / 64 <= 24 fmaf per lane, 6 cross-lane
    additions, the bias), then normalized_pair_bound.  (That sum carries the pooled bound through H terms of one sign: the
    GPU tests also check the head stage by itself on the pooled vector the kernel returned.)"""
    v, gm, bt = last_hidden.double(), gamma.double(), beta.double()
    T, H = v.shape[1], v.shape[2]
    d = H // 64 + 5
    mean = v.mean(-1, keepdim=True)
    sigma = ((v - mean).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    z = (v - mean) / sigma
    y = z * gm + bt
    dm = (d + 1) * U * v.abs().mean(-1, keepdim=True)
    rel = ((d + 3) * U + (dm / sigma) ** 2) / 2 + 6 * U
    delta = gm.abs() * dm / sigma + (gm * z).abs() * rel + U * y.abs()
    pooled_bound = delta.mean(1) + (-(-T // 16) + 7) * U * y.abs().mean(1)
    if Wh is None:
        return pooled_bound, None
    Wh, bh = Wh.double(), bh.double()
    pooled = y.mean(1)
    raw = pooled @ Wh.T + bh
    bound = pooled_bound @ Wh.abs().T + 32 * U * (pooled.abs() @ Wh.abs().T + bh.abs())
    return pooled_bound, normalized_pair_bound(raw, bound, sincos_offset)


# ---------------------------------------------------------------------------------------------- test operands
def head_case_inputs(B, D, hidden, n_out, seed, sincos_offset: int = -1):
    """Random f32 operands of one head case, shared by the GPU edge tests and the CPU self-checks: unit-variance x, weights
    and biases at nn.Linear's initial scale, one hidden unit and one output with weights 2^-10 smaller (an error confined to
    small-magnitude elements still shows against the per-element bound), and — when a pair is normalised — that pair's
    biases moved to (1.5, -2): its norm stays far from 0, where the bound of the normalise is infinite.
    hidden == 0: the linear head, W1 = b1 = None and W2 [n_out, D]."""
    g = torch.Generator().manual_seed(seed)
    lin = lambda o, i: ((torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5, (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5)
    x = torch.randn(B, D, generator=g)
    W1 = b1 = None
    if hidden:
        W1, b1 = lin(hidden, D)
        W1[hidden // 2] *= 2.0 ** -10
        b1[hidden // 2] *= 2.0 ** -10
    W2, b2 = lin(n_out, hidden if hidden else D)
    if n_out > 2:
        W2[n_out - 1] *= 2.0 ** -10
        b2[n_out - 1] *= 2.0 ** -10
    if sincos_offset is not None and sincos_offset >= 0:
        b2[sincos_offset] = 1.5
        b2[sincos_offset + 1] = -2.0
    return x, W1, b1, W2, b2


# (B, D, hidden, n_out, sincos_offset, VPR_POSE_KS or None) of the split-form K edges: hidden = 16 and D / 32 = 1 (three of
# the four waves idle), 3, 7 (odd: the single-step tail loop), 17 (two uneven slices), and 4 steps forced into 3 slices of
# 2 (the third is empty).  Shared by tests/test_heads_edges_gpu.py and the CPU self-checks.
SPLIT_K_EDGE_CASES = ((5, 32, 16, 4, 2, None), (3, 96, 16, 2, 0, None), (65, 224, 16, 4, 2, None), (7, 544, 16, 3, -1, None),
                      (4, 128, 16, 2, -1, 3))


def split_case_slices(D: int, ks) -> int:
    """Slab count of the split forms at hidden = 16, B <= 130 (pose_split_plan: at least 8 K-steps per slice)."""
    return ks if ks else max(1, min(32, (D // 32) // 8))


def ln_case_rows(kind: str, B: int, T: int, H: int, g) -> torch.Tensor:
    """[B, T, H] f32 token rows for the vpr_ln_meanpool_head edge tests.
      unit        1.5 N(0, 1) + 0.3;
      offset1000  1000 + N(0, 1): |mean| / σ = 1000, where E[x^2] - mean^2 in f32 is noise (the kernel is two-pass);
      constant    one bf16-representable value per row: H of them add exactly, var = 0 and the output is β;
      alternating image 0's tokens are one pattern at two alternating scales, +1 and -64, plus unit noise: LayerNorm maps them to
                  ±(the normalised pattern), which cancel in the mean up to 1 / T — a mean over the wrong token count, or a
                  token counted twice, moves every pooled element by about 1 / T; image 1 as "unit"."""
    if kind == "unit":
        return torch.randn(B, T, H, generator=g) * 1.5 + 0.3
    if kind == "offset1000":
        return 1000 + torch.randn(B, T, H, generator=g)
    if kind == "constant":
        return (torch.randint(-64, 65, (B, T, 1), generator=g).float() / 4).expand(B, T, H).clone()
    if kind == "alternating":
        x = torch.randn(B, T, H, generator=g) * 1.5 + 0.3
        pattern = 8 * torch.randn(H, generator=g)
        scale = torch.where(torch.arange(T) % 2 == 0, 1.0, -64.0)
        x[0] = scale[:, None] * pattern[None, :] + torch.randn(T, H, generator=g)
        return x
    raise ValueError(kind)


def exact_head_operands(B, D, hidden, n_out, seed):
    """(x, W1, b1, W2, b2) f32 on which every form of the head must equal the f64 result bit for bit (before the normalise).
    x = i / 8 (|i| <= 8), W1 = j / 4 (|j| <= 4): bf16-representable, so every `lo` plane is zero and every product is a
    multiple of 2^-5.  b1 on the same grid.  W2 = k / 2 (|k| <= 2), b2 on a grid of 2^-6.  Every partial sum of the first
    layer, in any order, is a multiple of 2^-5 bounded by A_j = max_b Σ_d |x_bd| |W1_jd| + |b1_j|, and of the second layer a
    multiple of 2^-6 bounded by Σ_j |W2_oj| A_j + |b2_o|: the generator asserts both stay below 2^24 units, so f32 adds
    exactly in any order.  Hidden units come in three kinds, j mod 4:
      0  positive in every row (b1_j = +(Σ|x||W1| + 1));     1  negative in every row (b1_j = -(that)): dead;
      2  exactly 0 in row 0 (b1_j = -x_0 · W1_j), either sign elsewhere;     3  W1_j = 0, b1_j = 0: exactly 0 in every row.
    hidden == 0: the linear head on the same grids (W1 = b1 = None, W2 [n_out, D])."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    x = ri(-8, 8, B, D) / 8
    if hidden == 0:
        W2, b2 = ri(-2, 2, n_out, D) / 2, ri(-256, 256, n_out) / 64
        assert float((x.abs() @ W2.abs().T + b2.abs()).max()) * 64 < 2 ** 24
        return x.float(), None, None, W2.float(), b2.float()
    W1 = ri(-4, 4, hidden, D) / 4
    P = (x.abs() @ W1.abs().T).amax(0)                # max over rows of Σ_d |x_d| |W1_jd|
    kind = torch.arange(hidden) % 4
    b1 = torch.zeros(hidden, dtype=torch.float64)
    b1[kind == 0] = (P + 1)[kind == 0]
    b1[kind == 1] = -(P + 1)[kind == 1]
    b1[kind == 2] = -(x[0] @ W1.T)[kind == 2]
    W1[kind == 3] = 0
    W2, b2 = ri(-2, 2, n_out, hidden) / 2, ri(-256, 256, n_out) / 64
    A = (x.abs() @ W1.abs().T).amax(0) + b1.abs()
    assert float(A.max()) * 32 < 2 ** 24 and float((W2.abs() @ A + b2.abs()).max()) * 64 < 2 ** 24
    out = tuple(t.float() for t in (x, W1, b1, W2, b2))
    assert all(torch.equal(t, t.to(torch.bfloat16).float()) for t in out[:2])
    return out


# ---------------------------------------------------------------------------------------------- CPU emulation
def _split_planes(v: torch.Tensor):
    hi = v.to(torch.bfloat16).float()
    return hi, (v - hi).to(torch.bfloat16).float()


def mlp_head_emulated(x, W1, b1, W2, b2, split: bool, slices: int = 2, mutate: str = None, perm=None):
    """f32 restatement of the kernels' arithmetic (un-normalised outputs): K-steps of 32 columns, `slices` split-K slabs
    added in slice order, bias, ReLU, second layer in f32.  split: bf16 (hi, lo) planes of x and W1 and four products per
    step (lo·lo, lo·hi, hi·lo, hi·hi: smallest first), accumulated in f32 as the MFMAs do.  perm: a permutation of the
    K-steps (summation order).  mutate names one mistake the bounds must reject:
      "lo_zero"  W1's lo plane dropped;   "x_lo_zero"  x's lo plane dropped (split8 with lo = 0);   "drop_step"  one 32-wide K-step skipped;
      "bias_after_relu"  relu(z) + b1;    "slice_twice"  slab 0 added twice."""
    x, W1, b1, W2, b2 = (t.float() for t in (x, W1, b1, W2, b2))
    B, D = x.shape
    hidden = W1.shape[0]
    steps = [(s, min(s + 32, D)) for s in range(0, D, 32)]
    if perm is not None:
        steps = [steps[i] for i in perm]
    if mutate == "drop_step":
        del steps[len(steps) // 2]
    if split:
        xh, xl = _split_planes(x)
        wh, wl = _split_planes(W1)
        if mutate == "lo_zero":
            wl = torch.zeros_like(wl)
        if mutate == "x_lo_zero":
            xl = torch.zeros_like(xl)
    per = -(-len(steps) // slices)
    slabs = []
    for k in range(slices):
        acc = torch.zeros(B, hidden)
        for a, b in steps[k * per:(k + 1) * per]:
            if split:
                for p, q in ((xl, wl), (xh, wl), (xl, wh), (xh, wh)):
                    acc = acc + p[:, a:b] @ q[:, a:b].T
            else:
                acc = acc + x[:, a:b] @ W1[:, a:b].T
        slabs.append(acc)
    if mutate == "slice_twice":
        slabs.insert(1, slabs[0])
    z = torch.zeros(B, hidden)
    for slab in slabs:
        z = z + slab
    h = torch.relu(z) + b1 if mutate == "bias_after_relu" else torch.relu(z + b1)
    return h @ W2.T + b2
