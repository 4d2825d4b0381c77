"""f64 reference and per-element error bound of the MFMA GEMMs (vpr_gemm_nt_bf16, vpr_gemm256_nt_bf16,
vpr_gemm_nt_group_bf16):  y = act(A W^T + b)  on bf16 operands, f32 accumulation, f32 or bf16 output.

Bound, with s = Σ_k a_k w_k exact (f64) and S = Σ_k |a_k w_k|: the products of two bf16 values are exact in f32, so
the f32 accumulation of K of them in any order is off by at most K u S (u = 2^-24), and the bias add by u |s + b|;
ReLU is 1-Lipschitz.  Hence
    f32 out:   |y - f(s + b)| <= K u S + 2 u (|s| + 2 |b|)
    bf16 out:  the same term, plus half the bf16 spacing at |f(s + b)| (+ that term: the rounding may cross a binade).
The same model as the skinny-linear edge tests (tests/test_skinny_edges_gpu.py).

Exact operands: small integers times powers of two such that every partial sum of every order is an integer
multiple of the scale below 2^24 of it — f32 then sums exactly, the result does not depend on the summation order,
and every kernel, tile form, K split and K walk must return f(s + b) rounded once: the f32 value itself, or its
round-to-nearest-even bf16 (ties included: the integer sums above 256 land on bf16 ties often).
exact_e4m3_operands is the same idea for the e4m3 score kernels (integer elements, power-of-two row scales).
"""
import torch

U = 2.0 ** -24


def rows_of(a_store: torch.Tensor, M: int, K: int, lda: int, a_group_rows: int = 0, a_group_stride: int = 0):
    """The [M, K] matrix the kernels read from the flat storage `a_store` (elements): row r at
    (r // a_group_rows) * a_group_stride + (r % a_group_rows) * lda, or r * lda without row groups."""
    flat = a_store.reshape(-1)
    r = torch.arange(M, dtype=torch.int64)
    base = (r // a_group_rows) * a_group_stride + (r % a_group_rows) * lda if a_group_rows > 0 else r * lda
    return flat[base[:, None] + torch.arange(K, dtype=torch.int64)[None, :]]


def gemm_ref(a, w, bias=None, relu=False, a_group_rows=0, a_group_stride=0, lda=None, M=None):
    """(y, s, S) in f64: y = act(A W^T + b), s = A W^T, S = |A| |W|^T.  `a` is either the [M, K] operand or, with lda
    given, the flat storage the kernels address (row groups resolved as they do).  w [N, K] (padding columns of a
    wider storage already sliced off); bias [N] or None."""
    K = w.shape[1]
    if lda is not None:
        A = rows_of(a, M, K, lda, a_group_rows, a_group_stride)
    else:
        A = a[:, :K]
    A, W = A.double(), w.double()
    s = A @ W.T
    S = A.abs() @ W.abs().T
    y = s + (bias.double()[None, :] if bias is not None else 0.0)
    if relu:
        y = y.clamp_min(0)
    return y, s, S


def half_ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """Half the spacing of bf16 numbers at |x| (normal range; the spacing of the smallest normal below it)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -126)).exponent - 9)


def gemm_bound(y, s, S, K, bias=None, out_bf16=False):
    """Per-element bound of |kernel - y| (see the module docstring)."""
    b = bias.double().abs()[None, :] if bias is not None else 0.0
    pre = K * U * S + 2 * U * (s.abs() + 2 * b)
    if not out_bf16:
        return pre
    return half_ulp_bf16(y.abs() + pre) + pre


def exact_value(y: torch.Tensor, out_bf16: bool) -> torch.Tensor:
    """What a kernel must return for exact operands: f(s + b) as f32 (exact), or its RNE bf16 (torch rounds to
    nearest even), as f64."""
    y32 = y.float()
    assert torch.equal(y32.double(), y), "operands are not exact: the f64 result is not an f32 value"
    return (y32.to(torch.bfloat16) if out_bf16 else y32).double()


def exact_operands(M, N, K, seed, with_bias=True):
    """bf16 A [M, K], W [N, K] and f32 bias [N] on which f32 accumulation is exact in any order.
    a = i / 8 with |i| <= 8, w = j / 4 with |j| <= 8 (so |a w| <= 2 on a grid of 1/32), bias on the same 1/32 grid with
    |bias| <= 64: every partial sum is a multiple of 2^-5 of magnitude <= 2K + 64 < 2^13 + 64, i.e. fits in 19 bits
    for K <= 4096."""
    assert K <= 4096
    g = torch.Generator().manual_seed(seed)
    a = (torch.randint(-8, 9, (M, K), generator=g).double() / 8).to(torch.bfloat16)
    w = (torch.randint(-8, 9, (N, K), generator=g).double() / 4).to(torch.bfloat16)
    b = (torch.randint(-2048, 2049, (N,), generator=g).double() / 32).float() if with_bias else None
    return a, w, b


def exact_e4m3_operands(B, N, D, seed):
    """(q, q_scale, g, g_scale, want): e4m3 rows q [B, D], g [N, D] as uint8 with per-row f32 scales, and the f64 score
    matrix want[b, n] = q_scale[b] g_scale[n] Σ_d q[b, d] g[n, d] that every e4m3 score kernel must return bit for bit.
    Elements are integers in [-8, 8] (3 mantissa bits hold them all), so a product is an integer of magnitude <= 64 and
    every partial sum of every order an integer below 64 D <= 2^15 for D <= 512: f32 accumulates exactly.  The scales are
    powers of two that vary per row (2^-3 .. 2^-9 and 2^-2 .. 2^-6): acc * q_scale * g_scale only moves the exponent."""
    assert D <= 512
    gen = torch.Generator().manual_seed(seed)
    qv = torch.randint(-8, 9, (B, D), generator=gen).float()
    gv = torch.randint(-8, 9, (N, D), generator=gen).float()
    q, g = qv.to(torch.float8_e4m3fn).view(torch.uint8), gv.to(torch.float8_e4m3fn).view(torch.uint8)
    q_scale = torch.ldexp(torch.ones(B), -3 - torch.arange(B) % 7).float()
    g_scale = torch.ldexp(torch.ones(N), -2 - torch.arange(N) % 5).float()
    want = (qv.double() @ gv.double().T) * q_scale.double()[:, None] * g_scale.double()[None, :]
    return q, q_scale, g, g_scale, want


def random_operands(M, N, K, seed, with_bias=True):
    """Random bf16 operands at the scales of a trained layer (unit-variance activations, 1/sqrt(K) weights) and an f32
    bias of a few units, with one column of tiny biases and small weights: an error confined to small-magnitude columns
    still shows against the per-element bound."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    w[N // 2] *= 2.0 ** -10
    w = w.to(torch.bfloat16)
    b = None
    if with_bias:
        b = torch.randn(N, generator=g)
        b[N // 2] *= 2.0 ** -10
    return a, w, b
