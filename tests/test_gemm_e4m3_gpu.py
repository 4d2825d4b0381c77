"""The e4m3 score kernels bit for bit.  The bf16 GEMMs are pinned on exact small-integer operands in
tests/test_gemm_edges_gpu.py; the e4m3 forms — the 128-row tile (gemm_nt_fp8_kernel), the 256 x 256 tile
(gemm256_kernel<true>) and the fp8 branch of the streaming kernel, which share one block-scaled MFMA step — are otherwise
compared only with each other, under a tolerance for summation order.  Here the operands are exact
(oracle/gemm.py::exact_e4m3_operands: integer elements, power-of-two row scales, D <= 512), so acc * q_scale * g_scale is
one f32 value in any summation order and every valid column of every row of the score matrix must equal the f64 value.
The score stage runs through ops.knn_topk_fp8 (k = 1; the top-k output is not the subject) and is read back with
ops.knn_scores_view; the padding columns up to ldS are not part of the contract."""
import functools

import pytest
import torch

from oracle import gemm as og

pytestmark = pytest.mark.gpu

GEMM128, GEMM256 = "vpr::gemm_nt_fp8_kernel", "vpr::gemm256_kernel<true, 10>"


@functools.lru_cache(maxsize=None)
def _case(B, N, D):
    return og.exact_e4m3_operands(B, N, D, seed=B + N + D)


def _scores(dev, B, N, D):
    from vpr_amd import ops
    q, qs, g, gs, want = _case(B, N, D)
    ws = ops.knn_workspace(B, N, D, 1, dev)
    ws.zero_()
    ops.knn_topk_fp8(q.to(dev), qs.to(dev), g.to(dev), gs.to(dev), 1, 0, ws)
    return ops.knn_scores_view(ws, B, N, D, 1).cpu().double(), want


def _assert_equal(got, want, what):
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} scores differ from the exact value, first at "
                           f"{tuple(bad.nonzero()[0].tolist())}: got {got[bad][0].item()!r}, want {want[bad][0].item()!r}")


# 128-row tile: one K-step, 2 x 2 ragged tiles / three K-steps, 2 m-tiles x 3 n-tiles (tile_m-fastest raster with a
# remainder) / the smallest B on the GEMM route, one ragged column tile.  256 x 256 tile: its minimum of two K-tiles, and four.
@pytest.mark.parametrize("B,N,D,kernel", [(150, 130, 128, GEMM128), (150, 257, 384, GEMM128), (65, 3, 256, GEMM128),
                                          (256, 300, 256, GEMM256), (512, 257, 512, GEMM256)])
def test_e4m3_gemm_scores_are_exact(dev, tune, B, N, D, kernel):
    from vpr_amd import _lib
    tune("VPR_KNN_GEMM_KSPLIT", 0)           # one slab: the view shows the whole sum
    # the name is resolved at D = 8448: B = 65 / 150 take the 128-row tile at any D, B = 256 / 512 the 256-row tile for D >= 256
    assert _lib.lib().vpr_knn_scores_kernel_name(1, B, N).decode() == kernel
    got, want = _scores(dev, B, N, D)
    _assert_equal(got, want, f"e4m3 GEMM route B={B} N={N} D={D}")


@pytest.mark.parametrize("B,N,D", [(64, 130, 128), (150, 130, 128), (150, 257, 384)])
def test_e4m3_stream_scores_are_exact(dev, tune, B, N, D):
    """The streaming kernel's fp8 branch (the same MFMA step): B = 64 takes it by default, the others with the GEMM
    routes switched off."""
    from vpr_amd import _lib
    tune("VPR_KNN_GEMM_MIN_B", 100000)
    assert _lib.lib().vpr_knn_scores_kernel_name(1, B, N).decode().startswith("vpr::knn_scores_kernel<true, ")
    got, want = _scores(dev, B, N, D)
    _assert_equal(got, want, f"e4m3 stream route B={B} N={N} D={D}")
