"""What include/vpr_amd_local_hires.h adds to the contract of include/vpr_amd_local.h, restated in numpy: the fixed order of the
score's f32 sum over blocks of 256 columns, and the input that tells this order from a plain ascending sum.  Everything else of
the contract is tests/local_match_ref.py and tests/local_match_fp8_ref.py, which have no patch limit.  Shared by
tests/test_local_match_hires_cpu.py and tests/test_local_match_hires_gpu.py; it imports nothing of the package."""
import numpy as np
import torch

import local_match_ref as ref

MAX_N = 1369            # VPR_LOCAL_HIRES_MAX_N
BLOCK = 256             # columns of a block of the sum
FLT_MAX = np.float32(np.finfo(np.float32).max)


def sum_roundings(n_g):
    """VPR_LOCAL_HIRES_SUM_ROUNDINGS(n_g)"""
    return ref.SUM_ROUNDINGS + (n_g + BLOCK - 1) // BLOCK


def clamp(x):
    return np.float32(min(max(x, -FLT_MAX), FLT_MAX))


def block_sum(v):
    """256 f32 values -> the block's sum in the order of vpr_amd_local.h: thread t holds v[t]; per wave of 64 the butterfly
    v += v[lane xor 32, 16, 8, 4, 2, 1]; the four wave sums added to +0 in ascending wave order.  Every operation in f32."""
    w = np.asarray(v, dtype=np.float32).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, lane ^ o]).astype(np.float32)
    s = np.float32(0.0)
    for k in range(4):
        s = np.float32(s + w[k, 0])
    return s


def score_in_stated_order(contrib):
    """contrib f32 [n_g] (S[c(j)][j] of a matched column, +0 of an unmatched one) -> the score as the header states it: block
    sums added in ascending block order to a running f32 that starts at +0, each block sum and the running sum clamped."""
    contrib = np.asarray(contrib, dtype=np.float32)
    n_g = contrib.shape[0]
    padded = np.zeros((n_g + BLOCK - 1) // BLOCK * BLOCK, dtype=np.float32)
    padded[:n_g] = contrib
    run = np.float32(0.0)
    with np.errstate(over="ignore"):
        for t in range(padded.shape[0] // BLOCK):
            run = clamp(np.float32(run + clamp(block_sum(padded[t * BLOCK:(t + 1) * BLOCK]))))
    return run


def ascending_sum(contrib):
    """The plain f32 sum in ascending column order: what the stated order is told from."""
    s = np.float32(0.0)
    for x in np.asarray(contrib, dtype=np.float32):
        s = np.float32(s + x)
    return s


ORDER_PIN_SEED, ORDER_PIN_N, ORDER_PIN_L = 5, MAX_N, 256


def order_pin_input(seed=ORDER_PIN_SEED, n=ORDER_PIN_N, l=ORDER_PIN_L):
    """Integer features in -16 .. 16 (exact in bf16; every S an integer below 2^17, exact in f32): a query and one image that
    holds the query's patches permuted, so that every column is matched at S = |q_i|^2 ~ 23000 and the matched sum passes 2^24,
    where f32 additions round and their order shows.  Returns (q bf16 [1, n, l], g bf16 [1, n, l])."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-16, 17, (n, l)).astype(np.float32)
    g = q[rng.permutation(n)]
    return torch.from_numpy(q[None]).to(torch.bfloat16), torch.from_numpy(g[None].copy()).to(torch.bfloat16)


def matched_contrib(q, g, min_sim=0.0):
    """One pair (torch [n_q, l], [n_g, l], exact in f64) -> (f32 [n_g]: the matched similarities by column, +0 elsewhere; the
    restatement's dict of that pair)."""
    p = ref.pair(ref.f64(q), ref.f64(g), min_sim)
    j = np.arange(p["S"].shape[1])
    c = np.maximum(p["col_nn"], 0)
    contrib = np.where(p["matched"], p["S"][c, j], 0.0)
    assert np.array_equal(contrib.astype(np.float32).astype(np.float64), contrib)        # every similarity exact in f32
    return contrib.astype(np.float32), p
