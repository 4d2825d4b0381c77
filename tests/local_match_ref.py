"""The contract of include/vpr_amd_local.h restated in float64 (numpy): the similarity matrix, the argmax and tie rules, the match
set, the score and the order.  Shared by tests/test_local_match_cpu.py and tests/test_local_match_gpu.py; it imports nothing of
the package."""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of f32
SUM_ROUNDINGS = 10      # VPR_LOCAL_SUM_ROUNDINGS


def gamma(L):
    return L * U / (1 - L * U)


def f64(t):
    """torch (bf16 / f32) or numpy -> float64 numpy, exactly."""
    return t.double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def similarity(q, g):
    """S[i][j] = sum_d q[i][d] g[j][d] in f64 from [n_q, l] and [n_g, l]; `finite` is False where an f32 S would not be a number
    (a NaN or Inf operand, or a magnitude beyond f32)."""
    with np.errstate(all="ignore"):
        S = f64(q) @ f64(g).T
        finite = np.isfinite(S.astype(np.float32))
    return S, finite


def nearest(S, finite):
    """r(i) over columns and c(j) over rows: the argmax of the finite entries, ties to the lowest index, -1 without one."""
    masked = np.where(finite, S, -np.inf)
    row_nn = np.where(finite.any(1), masked.argmax(1), -1).astype(np.int32)      # argmax returns the first maximum
    col_nn = np.where(finite.any(0), masked.argmax(0), -1).astype(np.int32)
    return row_nn, col_nn


def matched_columns(S, row_nn, col_nn, min_sim):
    """Boolean [n_g]: c(j) >= 0, r(c(j)) == j and S[c(j)][j] >= min_sim (min_sim as the f32 the device compares with)."""
    j = np.arange(S.shape[1])
    c = np.maximum(col_nn, 0)
    return (col_nn >= 0) & (row_nn[c] == j) & (S[c, j] >= float(np.float32(min_sim)))


def pair(q, g, min_sim):
    """One (query, candidate) pair -> dict(S, finite, row_nn, col_nn, matched, matches, score (f64))."""
    S, finite = similarity(q, g)
    row_nn, col_nn = nearest(S, finite)
    m = matched_columns(S, row_nn, col_nn, min_sim)
    j = np.nonzero(m)[0]
    return dict(S=S, finite=finite, row_nn=row_nn, col_nn=col_nn, matched=m, matches=int(m.sum()),
                score=float(S[col_nn[j], j].sum()))


def f32_key(v):
    """The total order of f32 bit patterns (+0 above -0) as an integer."""
    bits = int(np.float32(v).view(np.int32))
    return bits if bits >= 0 else -(bits & 0x7fffffff) - 1


def order(scores, matches, cand, live, k):
    """One query: live candidates by (f32 score desc, index asc, position asc), the first k; the tail is (-inf, -1, 0)."""
    vals, out, mt = np.full(k, -np.inf, dtype=np.float32), np.full(k, -1, dtype=np.int32), np.zeros(k, dtype=np.int32)
    pos = sorted(np.nonzero(live)[0], key=lambda t: (-f32_key(scores[t]), int(cand[t]), int(t)))[:k]
    for p, t in enumerate(pos):
        vals[p], out[p], mt[p] = scores[t], cand[t], matches[t]
    return vals, out, mt


def local_rerank(q_local, idx, g_local, index_base=0, k=None, min_sim=0.0):
    """vpr_local_rerank with f64 sums.  q_local [B, n_q, l], idx int32 [B, kc], g_local [n_local, n_g, l] (torch) ->
    dict of numpy arrays: vals f32 / idx / matches [B, k] and the optional outputs pair_score f32 / pair_matches [B, kc],
    row_nn [B, kc, n_q], col_nn [B, kc, n_g] ((-inf, 0, -1, -1) for a candidate the shard does not own), and pair_score64."""
    cand = idx.numpy().astype(np.int64)
    B, kc = cand.shape
    k = kc if k is None else k
    n_q, n_g, n_local = q_local.shape[1], g_local.shape[1], g_local.shape[0]
    q64, g64 = f64(q_local), f64(g_local)
    out = dict(vals=np.empty((B, k), np.float32), idx=np.empty((B, k), np.int32), matches=np.empty((B, k), np.int32),
               pair_score=np.full((B, kc), -np.inf, np.float32), pair_score64=np.full((B, kc), -np.inf), pair_matches=np.zeros((B, kc), np.int32),
               row_nn=np.full((B, kc, n_q), -1, np.int32), col_nn=np.full((B, kc, n_g), -1, np.int32))
    for b in range(B):
        rel = cand[b] - index_base
        live = (rel >= 0) & (rel < n_local)
        for t in np.nonzero(live)[0]:
            p = pair(q64[b], g64[rel[t]], min_sim)
            out["pair_score64"][b, t] = p["score"]
            out["pair_score"][b, t] = np.float32(p["score"])
            out["pair_matches"][b, t] = p["matches"]
            out["row_nn"][b, t], out["col_nn"][b, t] = p["row_nn"], p["col_nn"]
        out["vals"][b], out["idx"][b], out["matches"][b] = order(out["pair_score"][b], out["pair_matches"][b], cand[b], live, k)
    return out


# ------------------------------------------------------------------------------------------------ the recipe
def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def recipe(seed, n, l, n_distract=20, noise=0.02):
    """A query of n unit features; the true image = the same features permuted plus noise of norm `noise`; `n_distract` images of
    random unit features; everything rounded to bf16.  Returns (q bf16 [1, n, l], gallery bf16 [n_distract + 1, n, l]) with the
    true image LAST."""
    rng = np.random.default_rng(seed)
    q = unit(rng.standard_normal((n, l)))
    true = unit(q[rng.permutation(n)] + noise * unit(rng.standard_normal((n, l))))
    gal = np.concatenate([unit(rng.standard_normal((n_distract, n, l))), true[None]])
    return torch.from_numpy(q[None]).to(torch.bfloat16), torch.from_numpy(gal).to(torch.bfloat16)


def places(seed, N, D, B, n, l, views=4):
    """B places seen `views` times each: the views share a global descriptor up to small noise (the global search cannot tell
    them apart) but only ONE of them holds the query's patches (permuted, with noise); the rest of the gallery is random.
    Returns (global rows bf16 [N, D], local features bf16 [N, n, l], queries bf16 [B, D], their local features [B, n, l],
    the row of each query's true view)."""
    rng = np.random.default_rng(seed)
    q, ql = unit(rng.standard_normal((B, D))), unit(rng.standard_normal((B, n, l)))
    rows, local = unit(rng.standard_normal((N, D))), unit(rng.standard_normal((N, n, l)))
    perm = rng.permutation(N)
    true = np.empty(B, dtype=np.int64)
    for b in range(B):
        mine = perm[b * views:(b + 1) * views]
        rows[mine] = unit(q[b] + 0.05 * unit(rng.standard_normal((views, D))))
        true[b] = mine[rng.integers(views)]
        local[true[b]] = unit(ql[b][rng.permutation(n)] + 0.02 * unit(rng.standard_normal((n, l))))
    bf = lambda x: torch.from_numpy(x).to(torch.bfloat16)
    return bf(rows), bf(local), bf(q), bf(ql), true
