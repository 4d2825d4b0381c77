"""The contract of include/vpr_amd_spatial.h restated in numpy: the shift bins, the votes, the window sum, the three-part key of
the dominant shift, the inliers — integer logic, exactly — and the score as the f32 sum in the order that
tests/local_match_hires_ref.py states (imported: the order is stated once).  The match list of the composed call comes from the
f64 restatements of the matching (tests/local_match_ref.py, tests/local_match_fp8_ref.py).  Also the inputs of the tests: lists
with a planted shift, two-hot integer features whose similarities are exact in bf16 and in e4m3, and the recipe (a shifted true
image against a scrambled distractor).  Shared by tests/test_spatial_cpu.py and tests/test_spatial_gpu.py; it imports nothing of
the package."""
import numpy as np
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref

MAX_N, MAX_BINS, MAX_TOL = 1369, 5329, 8          # VPR_SPATIAL_MAX_N, VPR_SPATIAL_MAX_BINS, VPR_SPATIAL_MAX_TOL
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def dims(n_q, gw_q, n_g, gw_g):
    """(gh_q, gh_g, W, H) of the two grids; the rules of the header are asserted."""
    assert 1 <= gw_q <= n_q and n_q % gw_q == 0 and 1 <= gw_g <= n_g and n_g % gw_g == 0
    gh_q, gh_g = n_q // gw_q, n_g // gw_g
    return gh_q, gh_g, gw_q + gw_g - 1, gh_q + gh_g - 1


def bins_of(partner, sim, n_q, gw_q, gw_g):
    """One pair: partner int [n_g], sim f32 [n_g] -> (is_match bool [n_g], bin int64 [n_g], -1 where the column holds no match).
    A partner outside 0 .. n_q - 1 is no match whatever its value; so is a non-finite sim."""
    partner = np.asarray(partner, dtype=np.int64)
    sim = np.asarray(sim, dtype=np.float32)
    n_g = partner.shape[0]
    _, gh_g, W, _ = dims(n_q, gw_q, n_g, gw_g)
    ok = (partner >= 0) & (partner < n_q) & np.isfinite(sim)
    i = np.where(ok, partner, 0)
    j = np.arange(n_g)
    dx, dy = i % gw_q - j % gw_g, i // gw_q - j // gw_g
    return ok, np.where(ok, (dy + gh_g - 1) * W + (dx + gw_g - 1), -1)


def verify(partner, sim, n_q, gw_q, gw_g, tol):
    """vpr_spatial_verify for one pair -> dict(score f32, inliers, matches, shift (dx, dy), mask uint8 [n_g], votes, support)."""
    assert 0 <= tol <= MAX_TOL
    sim = np.asarray(sim, dtype=np.float32)
    n_g = sim.shape[0]
    _, gh_g, W, H = dims(n_q, gw_q, n_g, gw_g)
    assert W * H <= MAX_BINS
    ok, b = bins_of(partner, sim, n_q, gw_q, gw_g)
    votes = np.bincount(b[ok], minlength=W * H).reshape(H, W).astype(np.int64)
    padded = np.zeros((H + 2 * tol, W + 2 * tol), dtype=np.int64)
    padded[tol:tol + H, tol:tol + W] = votes
    support = np.zeros((H, W), dtype=np.int64)
    for oy in range(2 * tol + 1):
        for ox in range(2 * tol + 1):
            support += padded[oy:oy + H, ox:ox + W]
    if not ok.any():
        return dict(score=np.float32(0.0), inliers=0, matches=0, shift=(I32_MIN, I32_MIN), mask=np.zeros(n_g, np.uint8),
                    votes=votes, support=support)
    # the key: support descending, the bin's own votes descending, the bin index ascending
    dom = min(range(W * H), key=lambda t: (-int(support.flat[t]), -int(votes.flat[t]), t))
    by, bx = divmod(dom, W)
    inl = ok & (np.abs(b % W - bx) <= tol) & (np.abs(b // W - by) <= tol)
    assert int(inl.sum()) == int(support[by, bx])
    score = refh.score_in_stated_order(np.where(inl, sim, np.float32(0.0)).astype(np.float32))
    return dict(score=score, inliers=int(inl.sum()), matches=int(ok.sum()), shift=(bx - (gw_g - 1), by - (gh_g - 1)),
                mask=inl.astype(np.uint8), votes=votes, support=support)


def verify_batch(partner, sim, n_q, gw_q, gw_g, tol):
    """partner [P, n_g], sim [P, n_g] (numpy or torch) -> dict of arrays as the device call returns them."""
    partner = partner.numpy() if isinstance(partner, torch.Tensor) else np.asarray(partner)
    sim = sim.numpy() if isinstance(sim, torch.Tensor) else np.asarray(sim)
    P, n_g = partner.shape
    out = dict(score=np.zeros(P, np.float32), inliers=np.zeros(P, np.int32), matches=np.zeros(P, np.int32),
               shift=np.zeros((P, 2), np.int32), inlier_mask=np.zeros((P, n_g), np.uint8))
    for p in range(P):
        r = verify(partner[p], sim[p], n_q, gw_q, gw_g, tol)
        out["score"][p], out["inliers"][p], out["matches"][p], out["shift"][p], out["inlier_mask"][p] = \
            r["score"], r["inliers"], r["matches"], r["shift"], r["mask"]
    return out


def match_list(p):
    """The dict of local_match_ref.pair -> (partner int32 [n_g]: c(j) of a matched column, else -1; sim f32 [n_g]: S[c(j)][j]
    of a matched column, else +0).  Every matched similarity must be exact in f32."""
    j = np.arange(p["S"].shape[1])
    c = np.maximum(p["col_nn"], 0)
    s = np.where(p["matched"], p["S"][c, j], 0.0)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return np.where(p["matched"], p["col_nn"], -1).astype(np.int32), s.astype(np.float32)


def local_rerank_spatial(q_local, idx, g_local, gw_q, gw_g, tol, index_base=0, k=None, min_sim=0.0):
    """vpr_spatial_local_rerank on features whose similarities are exact in f32.  q_local [B, n_q, l], g_local [n_local, n_g, l]:
    bf16 features or uint8 e4m3 bytes (torch); idx int32 [B, kc].  -> dict of numpy arrays: vals f32 / idx / inliers [B, k] and
    pair_score f32 / pair_inliers / pair_matches [B, kc], pair_shift [B, kc, 2], row_nn [B, kc, n_q], col_nn [B, kc, n_g]."""
    if q_local.dtype == torch.uint8:
        q64, g64 = ref8.decode(q_local), ref8.decode(g_local)
    else:
        q64, g64 = ref.f64(q_local), ref.f64(g_local)
    cand = idx.numpy().astype(np.int64)
    B, kc = cand.shape
    k = kc if k is None else k
    n_q, n_g, n_local = q64.shape[1], g64.shape[1], g64.shape[0]
    out = dict(vals=np.empty((B, k), np.float32), idx=np.empty((B, k), np.int32), inliers=np.empty((B, k), np.int32),
               pair_score=np.full((B, kc), -np.inf, np.float32), pair_inliers=np.zeros((B, kc), np.int32),
               pair_matches=np.zeros((B, kc), np.int32), pair_shift=np.full((B, kc, 2), I32_MIN, np.int32),
               row_nn=np.full((B, kc, n_q), -1, np.int32), col_nn=np.full((B, kc, n_g), -1, np.int32))
    memo = {}
    for b in range(B):
        rel = cand[b] - index_base
        live = (rel >= 0) & (rel < n_local)
        for t in np.nonzero(live)[0]:
            if (b, rel[t]) not in memo:
                p = ref.pair(q64[b], g64[rel[t]], min_sim)
                memo[b, rel[t]] = (p, verify(*match_list(p), n_q, gw_q, gw_g, tol))
            p, v = memo[b, rel[t]]
            out["pair_score"][b, t], out["pair_inliers"][b, t], out["pair_matches"][b, t] = v["score"], v["inliers"], v["matches"]
            out["pair_shift"][b, t] = v["shift"]
            out["row_nn"][b, t], out["col_nn"][b, t] = p["row_nn"], p["col_nn"]
            assert v["matches"] == p["matches"]
        out["vals"][b], out["idx"][b], out["inliers"][b] = ref.order(out["pair_score"][b], out["pair_inliers"][b], cand[b], live, k)
    return out


# ------------------------------------------------------------------------------------------------ hand-made lists
def planted_list(rng, n_q, gw_q, n_g, gw_g, shift, noise=0):
    """A list in which every candidate patch whose shifted position lies on the query grid is matched to it (shift = (dx, dy)),
    and `noise` further columns to random query patches.  Similarities are small integers / 4: every sum is exact."""
    gh_q = n_q // gw_q
    j = np.arange(n_g)
    x, y = j % gw_g + shift[0], j // gw_g + shift[1]
    ok = (x >= 0) & (x < gw_q) & (y >= 0) & (y < gh_q)
    partner = np.where(ok, y * gw_q + x, -1).astype(np.int32)
    free = np.nonzero(~ok)[0]
    if noise and free.size:
        pick = rng.choice(free, min(noise, free.size), replace=False)
        partner[pick] = rng.integers(0, n_q, pick.size)
    sim = (rng.integers(1, 9, n_g) / 4.0).astype(np.float32)
    return partner, sim


# ---------------------------------------------------------------------------- integer features with exact similarities
L = 128                 # two halves of 64


def two_hot(codes, kind="bf16", l=L):
    """codes int [..] in 0 .. (l/2)^2 - 1 -> features [.., l] with a 1 at code % (l/2) in the first half and at l/2 + code //
    (l/2) in the second: a patch's similarity with itself is 2, with any other code at most 1.  kind "bf16": bf16 tensors;
    "e4m3": the uint8 store whose byte values are these integers (the features v * 2^-8: the similarities are 2^-16 times
    the integers)."""
    codes = np.asarray(codes)
    h = l // 2
    assert codes.min() >= 0 and codes.max() < h * h
    v = np.zeros(codes.shape + (l,), dtype=np.float32)
    np.put_along_axis(v, (codes % h)[..., None], 1.0, -1)
    np.put_along_axis(v, (h + codes // h)[..., None], 1.0, -1)
    return torch.from_numpy(v).to(torch.bfloat16) if kind == "bf16" else torch.from_numpy(ref8.encode_ints(v))


def unit_sim(kind):
    """The similarity of two features that share one hot position."""
    return 1.0 if kind == "bf16" else 2.0 ** -16


def shifted_codes(q_codes, gw, shift, fresh):
    """The image whose patch at (x, y) is the query's patch at (x + dx, y + dy) — a match then has the shift (dx, dy) — and
    a code of `fresh` (none of them the query's) where that falls off the grid."""
    n = q_codes.shape[0]
    gh = n // gw
    j = np.arange(n)
    x, y = j % gw + shift[0], j // gw + shift[1]
    ok = (x >= 0) & (x < gw) & (y >= 0) & (y < gh)
    out = np.where(ok, q_codes[np.where(ok, y * gw + x, 0)], 0)
    out[~ok] = fresh[:int((~ok).sum())]
    return out


def recipe_codes(seed, gw, shift=(2, 1)):
    """The recipe on a gw x gw grid: (query codes [n], gallery codes [2, n]): image 0 is the distractor, every query patch at a
    scrambled position; image 1 is the true place, the query shifted by `shift`."""
    rng = np.random.default_rng(seed)
    n = gw * gw
    codes = rng.permutation((L // 2) ** 2)
    q = codes[:n]
    return q, np.stack([q[rng.permutation(n)], shifted_codes(q, gw, shift, codes[n:])])


def spatial_places(seed, N, D, B, gw, kind="bf16"):
    """B places seen four times each with near-equal global descriptors: one view is the query's grid shifted by (2, 1), another
    holds every query patch at a scrambled position, the rest of the gallery is unrelated.  Two-hot features (two_hot).
    Returns (rows bf16 [N, D], local [N, n, l], queries bf16 [B, D], their local features, the rows of the shifted views and of
    the scrambled ones)."""
    rng = np.random.default_rng(seed)
    n = gw * gw
    q, rows = ref.unit(rng.standard_normal((B, D))), ref.unit(rng.standard_normal((N, D)))
    codes = rng.integers(0, (L // 2) ** 2, (N, n))
    qc = np.stack([rng.permutation((L // 2) ** 2) for _ in range(B)])
    perm = rng.permutation(N)
    true, scrambled = np.empty(B, np.int64), np.empty(B, np.int64)
    for b in range(B):
        mine = perm[4 * b:4 * b + 4]
        rows[mine] = ref.unit(q[b] + 0.05 * ref.unit(rng.standard_normal((4, D))))
        true[b], scrambled[b] = mine[0], mine[1]
        codes[true[b]] = shifted_codes(qc[b, :n], gw, (2, 1), qc[b, n:])
        codes[scrambled[b]] = qc[b, :n][rng.permutation(n)]
    bf = lambda x: torch.from_numpy(x).to(torch.bfloat16)
    return bf(rows), two_hot(codes, kind), bf(q), two_hot(qc[:, :n], kind), true, scrambled
