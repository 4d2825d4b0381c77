"""The skinny linear kernel's fetch forms (VPR_SKINNY_FETCH: 1 / unset = four neighbouring lanes fetch 64 contiguous bytes of a
row and the fragment crosses to its MFMA lane; 0 = a lane fetches the fragment it feeds) against f64, in all six modes and with
both bias types, at the bounds of tests/test_skinny_edges_gpu.py:

    bf16 modes: |y - f(s + b)| <= half the bf16 spacing at |f(s + b)| + 1.13 (K u S + 8 u (|s| + |b|)) (1 + 2^-8)
    mode 5:     |y - (s + b)|   <= K u S + 2 u (|s| + 2 |b|)

with s the exact product, S = sum |a_k w_k|, u = 2^-24, f the mode's activation (tanh-GELU, like erf-GELU, is 1.13-Lipschitz)
and, in mode 2, b = the value already in `out`.  Shapes: one K-step with idle waves; ragged rows with K no multiple of a wave's
slice; a ragged last column block; fc2's K depth with several load batches per wave and a partly filled second row block.
The forms differ only in which lane requests a fragment: the K partition, the order of the sums and the epilogue are one, so both
give the bits of the library before the quad fetch (tests/golden/skinny_parent_bits.npz: two seeded cases, inputs and that
library's outputs).  Which form ran therefore shows in a kernel trace only (skinny_linear_kernel<..., true / false>)."""
import math
import os

import numpy as np
import pytest
import torch

from test_skinny_edges_gpu import U, _half_ulp_bf16

pytestmark = pytest.mark.gpu

SHAPES = ((1, 16, 32), (5, 48, 96), (64, 40, 1024), (17, 1024, 4096))
SENTINEL = -777.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinny_parent_bits.npz")


def _act(mode, x):
    if mode == 1:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    if mode == 3:
        return x.clamp_min(0)
    if mode == 4:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    return x


_CASES = {}


def _case(M, N, K, mode, bias_dtype):
    """Operands, the f64 reference and its bound: computed once per case, shared by the fetch forms, never written."""
    key = (M, N, K, mode, bias_dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(M * 131 + N * 7 + K + mode)
        a = torch.randn(M, K, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16)
        b = None if mode == 2 else torch.randn(N, generator=g).to(bias_dtype)
        out0 = torch.randn(M, N, generator=g).to(torch.float32 if mode == 5 else torch.bfloat16)      # mode 2 adds onto it
        sb = torch.randn(N, generator=g) * 50                                                          # a large offset per column
        s = a.double() @ w.double().T
        S = a.double().abs() @ w.double().abs().T
        bb = out0.double() if mode == 2 else b.double()[None, :]
        ref = _act(mode, s + bb)
        if mode == 5:
            bound = K * U * S + 2 * U * (s.abs() + 2 * bb.abs())
        else:
            pre = 1.13 * (K * U * S + 8 * U * (s.abs() + bb.abs()))
            bound = _half_ulp_bf16(ref.abs() + pre) + pre * (1 + 2.0 ** -8)
        _CASES[key] = (a, w, b, out0, sb, ref, bound)
    return _CASES[key]


def _run(dev, a, w, b, out0, mode, sb=None):
    """Into the slice [1 : M + 1, 4 : 4 + N] of a sentinel-filled buffer (row stride N + 8: the 8-byte store path; the scalar
    one is test_skinny_edges_gpu's) -> (slice, buffer, row_stats or None)."""
    from vpr_amd import ops
    M, N = out0.shape
    buf = torch.full((M + 2, N + 8), SENTINEL, dtype=out0.dtype, device=dev)
    out = buf[1:M + 1, 4:4 + N]
    out.copy_(out0)
    rs = None if sb is None else torch.full((N // 16, M, 2), SENTINEL, dtype=torch.float32, device=dev)
    ops.skinny_linear_bf16(a.to(dev), w.to(dev), None if b is None else b.to(dev), out, mode, None if sb is None else sb.to(dev), rs)
    return out, buf, rs


def _check(out, buf, ref, bound, what):
    M, N = ref.shape
    assert torch.isfinite(out).all(), what
    err = (out.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}"
    outside = buf.clone()
    outside[1:M + 1, 4:4 + N] = SENTINEL
    assert bool((outside == SENTINEL).all()), f"{what}: wrote outside its slice"


@pytest.mark.parametrize("fetch", [None, 0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fetch_forms_against_f64(dev, tune, fetch, M, N, K):
    tune("VPR_SKINNY_FETCH", fetch)
    for mode in range(6):
        for bias_dtype in (torch.bfloat16, torch.float32):
            a, w, b, out0, _, ref, bound = _case(M, N, K, mode, bias_dtype)
            what = f"fetch {fetch} mode {mode} M={M} N={N} K={K} bias {bias_dtype}"
            out, buf, _ = _run(dev, a, w, b, out0, mode)
            _check(out, buf, ref, bound, what)
            again, _, _ = _run(dev, a, w, b, out0, mode)
            assert torch.equal(out, again), f"{what}: two calls, different bits"


@pytest.mark.parametrize("fetch", [None, 0])
@pytest.mark.parametrize("M,N,K", [s for s in SHAPES if s[1] % 16 == 0])
def test_row_stats_merge_to_the_rows_mean_and_variance(dev, tune, fetch, M, N, K):
    """row_stats [N / 16, M, 2] = (mean, centred sum of squares) per 16-column block of t = bf16(out) + stats_bias, merged here
    in f64 by row_stats_merge's formula (mean = avg mean_p, M2 = sum M2_p + 16 sum (mean_p - mean)^2).  Per block the f32 sums
    of 16 terms are off by e_mean = 8 u mag and e_m2 = sum(2 |d| e_d + e_d^2) + 40 u M2_p with e_d = 10 u mag (the bounds of
    test_skinny_row_stats); through the merge that is E_mean = avg e_mean for the mean and, for M2,
    sum e_m2 + 16 sum (2 |mean_p - mean| (e_mean_p + E_mean) + (e_mean_p + E_mean)^2)."""
    tune("VPR_SKINNY_FETCH", fetch)
    for mode in (0, 2):
        a, w, b, out0, sb, ref, bound = _case(M, N, K, mode, torch.bfloat16)
        out, buf, rs = _run(dev, a, w, b, out0, mode, sb)
        _check(out, buf, ref, bound, f"stats fetch {fetch} mode {mode} M={M} N={N} K={K}")
        t = out.cpu().double() + sb.double()
        blocks = t.view(M, N // 16, 16)
        mean_p, mag = blocks.mean(-1), blocks.abs().amax(-1)
        d = blocks - mean_p[..., None]
        e_mean_p, e_d = 8 * U * mag, (10 * U * mag)[..., None]
        e_m2_p = (2 * d.abs() * e_d + e_d ** 2).sum(-1) + 40 * U * (d ** 2).sum(-1)
        E_mean = e_mean_p.mean(-1)
        mean64 = t.mean(-1)
        m2_64 = ((t - mean64[:, None]) ** 2).sum(-1)
        dm = (mean_p - mean64[:, None]).abs()
        em = e_mean_p + E_mean[:, None]
        E_m2 = e_m2_p.sum(-1) + 16 * (2 * dm * em + em ** 2).sum(-1)
        got_mean_p, got_m2_p = rs[:, :, 0].T.cpu().double(), rs[:, :, 1].T.cpu().double()
        got_mean = got_mean_p.mean(-1)
        got_m2 = got_m2_p.sum(-1) + 16 * ((got_mean_p - got_mean[:, None]) ** 2).sum(-1)
        assert bool(((got_mean - mean64).abs() <= E_mean).all())
        assert bool(((got_m2 - m2_64).abs() <= E_m2).all())
        assert bool(((got_m2 / N - m2_64 / N).abs() <= E_m2 / N).all())      # the variance the LayerNorm divides by


@pytest.mark.parametrize("fetch", [None, 0, 1])
def test_both_forms_give_the_bits_of_the_library_before_the_quad_fetch(dev, tune, fetch):
    from vpr_amd import _lib, ops
    tune("VPR_SKINNY_FETCH", fetch)
    assert _lib.tuning_get("VPR_SKINNY_FETCH") == fetch
    z = np.load(GOLDEN)
    bf = lambda name: torch.from_numpy(z[name].view(np.int16)).view(torch.bfloat16).to(dev)
    for tag in ("gelu", "acc"):
        mode = int(z[tag + "_mode"])
        bias = bf(tag + "_bias") if tag + "_bias" in z else None
        out = bf(tag + "_out0").clone()
        sb = torch.from_numpy(z[tag + "_stats_bias"]).to(dev) if tag + "_stats_bias" in z else None
        rs = None if sb is None else torch.empty(tuple(z[tag + "_row_stats"].shape), dtype=torch.float32, device=dev)
        ops.skinny_linear_bf16(bf(tag + "_in"), bf(tag + "_w"), bias, out, mode, sb, rs)
        assert torch.equal(out, bf(tag + "_out")), f"{tag}: fetch {fetch} changed the output's bits"
        if rs is not None:
            assert torch.equal(rs.cpu(), torch.from_numpy(z[tag + "_row_stats"])), f"{tag}: fetch {fetch} changed the statistics' bits"
