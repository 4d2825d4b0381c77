"""Skinny linear kernel (vpr_skinny_linear_bf16 / _stats_bf16) against f64 in the modes the backbone and SALAD use
but no other test calls directly: 3 (ReLU, SALAD token MLP), 4 (exact erf-GELU, DinoV2(gelu="erf")) and 5 (f32
output, SALAD token features), at K / N / M that run both the unrolled and the remainder K loop for every wave
count, ragged column blocks and row groups, into column slices of a wider buffer.

Bounds, with s = Σ_k a_k w_k exact (f64) and S = Σ_k |a_k w_k|: the f32 accumulation of K products (in MFMA
k-steps, wave partials merged in a fixed order) is off by at most K u S (u = 2^-24), the bias add and the
epilogue by a few u of |s + b|, and the activations are 1.13-Lipschitz (erf-GELU; ReLU 1), so
    bf16 modes: |y - f(s + b)| <= half the bf16 spacing at |f(s + b)| + 1.13 (K u S + 8 u (|s| + |b|)) · (1 + 2^-8)
    mode 5:     |y - (s + b)|   <= K u S + 2 u (|s| + 2 |b|)
(the f32 output is bounded by the f32 accumulation model, not by a bf16 ulp).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_SWEEP = (32, 96, 1056, 4096)
N_SWEEP = (1, 3, 17, 2049)
M_SWEEP = (1, 16, 17, 65)
SENTINEL = -777.0


def _half_ulp_bf16(x):
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -126)).exponent - 9)


def _act(mode, x):
    if mode == 3:
        return x.clamp_min(0)
    if mode == 4:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    return x


def _operands(M, N, K, bias_dtype, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g).to(bias_dtype)
    return a, w, b


def _ref_bound(a, w, b, mode):
    K = a.shape[1]
    s = a.double() @ w.double().T
    S = a.double().abs() @ w.double().abs().T
    bb = b.double()[None, :]
    ref = _act(mode, s + bb)
    if mode == 5:
        return ref, K * U * S + 2 * U * (s.abs() + 2 * bb.abs())
    pre = 1.13 * (K * U * S + 8 * U * (s.abs() + bb.abs()))
    return ref, _half_ulp_bf16(ref.abs() + pre) + pre * (1 + 2.0 ** -8)


def _run(dev, a, w, b, mode):
    """Into the column slice [1 : M+1, 2 : 2+N] of a sentinel-filled buffer whose row stride is 2 mod 4 (the scalar
    store path of the bf16 modes); returns (slice, whole buffer)."""
    from vpr_amd import ops
    M, N = a.shape[0], w.shape[0]
    width = N + 4 + (2 - (N + 4)) % 4                       # >= N + 2, == 2 (mod 4): the slice starts 8-byte aligned
    dtype = torch.float32 if mode == 5 else torch.bfloat16
    buf = torch.full((M + 2, width), SENTINEL, dtype=dtype, device=dev)
    out = buf[1:M + 1, 2:2 + N]
    assert out.stride(0) % 4 == 2 and out.data_ptr() % 8 == 0
    ops.skinny_linear_bf16(a.to(dev), w.to(dev), b.to(dev), out, mode)
    return out, buf


def _check(out, buf, ref, bound, what):
    M, N = ref.shape
    err = (out.cpu().double() - ref).abs()
    assert torch.isfinite(out).all(), what
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}"
    outside = buf.clone()
    outside[1:M + 1, 2:2 + N] = SENTINEL
    assert bool((outside == SENTINEL).all()), f"{what}: wrote outside its slice"


@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("mode", [3, 4, 5])
def test_skinny_modes_against_f64(dev, mode, K):
    for N in N_SWEEP:
        for M in M_SWEEP:
            for bias_dtype in (torch.bfloat16, torch.float32):
                a, w, b = _operands(M, N, K, bias_dtype, seed=K * 7 + N * 3 + M)
                out, buf = _run(dev, a, w, b, mode)
                ref, bound = _ref_bound(a, w, b, mode)
                _check(out, buf, ref, bound, f"mode {mode} M={M} N={N} K={K} bias {bias_dtype}")


@pytest.mark.parametrize("nw", [None, 4, 8, 16])
@pytest.mark.parametrize("mbw", [None, 1, 4])
def test_skinny_switches_within_bound_and_deterministic(dev, tune, nw, mbw):
    """Every VPR_SKINNY_NW x VPR_SKINNY_MBW: a different K partition / row grouping, so not bit-identical to the
    default, but within the f64 bound and the same bits run to run."""
    tune("VPR_SKINNY_NW", nw)
    tune("VPR_SKINNY_MBW", mbw)
    for K in K_SWEEP:
        for (M, N) in ((17, 2049), (65, 17), (1, 3)):
            for mode in (3, 4, 5):
                a, w, b = _operands(M, N, K, torch.float32, seed=K + N + M + mode)
                out, buf = _run(dev, a, w, b, mode)
                ref, bound = _ref_bound(a, w, b, mode)
                what = f"NW={nw} MBW={mbw} mode {mode} M={M} N={N} K={K}"
                _check(out, buf, ref, bound, what)
                again, _ = _run(dev, a, w, b, mode)
                assert torch.equal(out, again), what


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K,mode", [(1, 16, 32, 0), (17, 48, 1056, 0), (65, 2048, 96, 2), (16, 1024, 4096, 2)])
def test_skinny_row_stats(dev, M, N, K, mode, with_bias):
    """row_stats [N/16, M, 2] = (mean, centred sum of squares) of bf16(out) + stats_bias per 16-column block, of the
    values the kernel wrote (f32 sums of 16 terms: 8 u of the block's magnitude)."""
    from vpr_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
    b = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if mode != 2 else None
    out = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)            # mode 2 accumulates into it
    sb = (torch.randn(N, generator=g) * 50).to(dev) if with_bias else None     # a large offset per column
    rs = torch.full((N // 16, M, 2), SENTINEL, dtype=torch.float32, device=dev)
    before = out.clone()
    ops.skinny_linear_bf16(a, w, b, out, mode, sb, rs)
    s = a.double() @ w.double().T
    ref_out = (before.double() + s) if mode == 2 else (s + b.double())
    bound_out = _half_ulp_bf16(ref_out.abs()) * 1.01 + 64 * K * U * (a.double().abs() @ w.double().abs().T) + 1e-30
    assert bool(((out.double() - ref_out).abs() <= bound_out).all())
    t = out.double() + (sb.double() if with_bias else 0.0)                     # what the next LayerNorm reads
    blocks = t.view(M, N // 16, 16)
    mean = blocks.mean(-1)
    m2 = ((blocks - mean[..., None]) ** 2).sum(-1)
    mag = blocks.abs().amax(-1)
    e_mean = 8 * U * mag
    e_d = (10 * U * mag)[..., None]                                              # t rounded to f32, minus the mean
    e_m2 = (2 * (blocks - mean[..., None]).abs() * e_d + e_d ** 2).sum(-1) + 40 * U * m2
    assert bool(((rs[:, :, 0].T.double() - mean).abs() <= e_mean).all())
    assert bool(((rs[:, :, 1].T.double() - m2).abs() <= e_m2).all())


def test_skinny_refusals(dev):
    from vpr_amd import ops
    a = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(16, 64, dtype=torch.bfloat16, device=dev)
    b = torch.zeros(16, device=dev)
    with pytest.raises(RuntimeError):                                            # mode 5 writes f32
        ops.skinny_linear_bf16(a, w, b, torch.zeros(4, 16, dtype=torch.bfloat16, device=dev), 5)
    with pytest.raises(RuntimeError):                                            # K % 32
        ops.skinny_linear_bf16(a[:, :40], w[:, :40], b, torch.zeros(4, 16, device=dev), 5)
    with pytest.raises(RuntimeError):                                            # no statistics of an f32 output
        ops.skinny_linear_bf16(a, w, b, torch.zeros(4, 16, device=dev), 5, None,
                               torch.zeros(1, 4, 2, device=dev))
