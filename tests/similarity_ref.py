"""The contract of include/vpr_amd_similarity.h restated in numpy: the match list in column order, the 256 two-match hypotheses
and their admissibility, the inlier test, the winner — integer logic, exactly, with every intermediate asserted to fit an int32
— and the score as the f32 sum in the order that tests/local_match_hires_ref.py states (imported: the order is stated once).
The match list of the composed call comes from tests/spatial_ref.py (match_list) and the f64 restatements of the matching.  Also
the inputs of the tests: lists planted under a similarity transform, and the recipe (a view zoomed by 3/2 against a distractor
that holds a coherent block of the query).  Shared by tests/test_similarity_cpu.py and tests/test_similarity_gpu.py; it imports
nothing of the package."""
import numpy as np
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref
import spatial_ref as sref

MAX_N, MAX_SIDE, HYPOTHESES, MAX_SCALE, MAX_TOL = 1369, 37, 256, 2, 8     # the VPR_SIM_* macros
I32_MIN, I32_MAX = sref.I32_MIN, sref.I32_MAX
NO_MODEL = (I32_MIN,) * 6
L = sref.L


def check_grid(n_q, gw_q, n_g, gw_g):
    assert 1 <= gw_q <= n_q <= MAX_N and n_q % gw_q == 0 and 1 <= gw_g <= n_g <= MAX_N and n_g % gw_g == 0
    assert max(gw_q, n_q // gw_q, gw_g, n_g // gw_g) <= MAX_SIDE


def pair_indices(M):
    """(s, t) int64 [256] of the hypotheses of M >= 2 matches."""
    h = np.arange(HYPOTHESES, dtype=np.int64)
    s = h * M // HYPOTHESES
    return s, (s + 1 + (97 * h) % (M - 1)) % M


def hypotheses(g, q):
    """g, q int64 [M, 2] (M >= 2): the positions of the matches in column order -> dict of [256] arrays: s, t, dg [256, 2],
    dq [256, 2], re, im, n2g, n2q, admissible."""
    s, t = pair_indices(g.shape[0])
    dg, dq = g[t] - g[s], q[t] - q[s]
    re = dq[:, 0] * dg[:, 0] + dq[:, 1] * dg[:, 1]
    im = dq[:, 1] * dg[:, 0] - dq[:, 0] * dg[:, 1]
    n2g, n2q = (dg ** 2).sum(1), (dq ** 2).sum(1)
    ok = (n2g > 0) & (n2q > 0) & (n2g <= MAX_SCALE ** 2 * n2q) & (n2q <= MAX_SCALE ** 2 * n2g) & (re > 0) & (np.abs(im) <= re)
    return dict(s=s, t=t, dg=dg, dq=dq, re=re, im=im, n2g=n2g, n2q=n2q, admissible=ok)


def residuals(g, q, hyp):
    """|(q - q_s) dg - dq (g - g_s)|^2 int64 [256, M] in complex integer arithmetic; every value must fit an int32."""
    a = q[None, :, :] - q[hyp["s"]][:, None, :]                                 # [256, M, 2]
    b = g[None, :, :] - g[hyp["s"]][:, None, :]
    dg, dq = hyp["dg"][:, None, :], hyp["dq"][:, None, :]
    lre = (a[..., 0] * dg[..., 0] - a[..., 1] * dg[..., 1]) - (dq[..., 0] * b[..., 0] - dq[..., 1] * b[..., 1])
    lim = (a[..., 0] * dg[..., 1] + a[..., 1] * dg[..., 0]) - (dq[..., 0] * b[..., 1] + dq[..., 1] * b[..., 0])
    assert np.abs(lre).max() <= 4 * 36 * 36 and np.abs(lim).max() <= 4 * 36 * 36
    r = lre ** 2 + lim ** 2
    assert r.max() <= 2 * 5184 ** 2 <= I32_MAX
    return r


def verify(partner, sim, n_q, gw_q, gw_g, tol):
    """vpr_similarity_verify for one pair -> dict(score f32, inliers, matches, model (6 ints), mask uint8 [n_g], counts int64
    [256] (0 where not admissible), admissible bool [256])."""
    assert 0 <= tol <= MAX_TOL
    partner = np.asarray(partner, dtype=np.int64)
    sim = np.asarray(sim, dtype=np.float32)
    n_g = sim.shape[0]
    check_grid(n_q, gw_q, n_g, gw_g)
    ok = (partner >= 0) & (partner < n_q) & np.isfinite(sim)                    # the match rule of the spatial header
    cols = np.nonzero(ok)[0]
    M = int(cols.size)
    none = dict(score=np.float32(0.0), inliers=0, matches=M, model=NO_MODEL, mask=np.zeros(n_g, np.uint8),
                counts=np.zeros(HYPOTHESES, np.int64), admissible=np.zeros(HYPOTHESES, bool))
    if M < 2:
        return none
    g = np.stack([cols % gw_g, cols // gw_g], 1)
    q = np.stack([partner[cols] % gw_q, partner[cols] // gw_q], 1)
    hyp = hypotheses(g, q)
    assert (hyp["s"] != hyp["t"]).all()
    bound = tol * tol * hyp["n2g"]
    assert bound.max() <= I32_MAX
    inl = residuals(g, q, hyp) <= bound[:, None]
    counts = np.where(hyp["admissible"], inl.sum(1), 0)
    if not hyp["admissible"].any():
        return none
    h = min(np.nonzero(hyp["admissible"])[0], key=lambda t: (-int(counts[t]), int(t)))
    assert inl[h, hyp["s"][h]] and inl[h, hyp["t"][h]] and counts[h] >= 2       # the two defining matches are inliers
    mask = np.zeros(n_g, bool)
    mask[cols[inl[h]]] = True
    score = refh.score_in_stated_order(np.where(mask, sim, np.float32(0.0)).astype(np.float32))
    model = (int(h), int(cols[hyp["s"][h]]), int(cols[hyp["t"][h]]), int(hyp["re"][h]), int(hyp["im"][h]), int(hyp["n2g"][h]))
    return dict(score=score, inliers=int(counts[h]), matches=M, model=model, mask=mask.astype(np.uint8), counts=counts,
                admissible=hyp["admissible"])


def scale_rotation(model):
    """(scale, rotation in degrees) of a model row, None for NO_MODEL."""
    _, _, _, re, im, n2g = (int(v) for v in model)
    if n2g <= 0:
        return None
    return float(np.hypot(re, im) / n2g), float(np.degrees(np.arctan2(im, re)))


def verify_batch(partner, sim, n_q, gw_q, gw_g, tol):
    """partner [P, n_g], sim [P, n_g] (numpy or torch) -> dict of arrays as the device call returns them."""
    partner = partner.numpy() if isinstance(partner, torch.Tensor) else np.asarray(partner)
    sim = sim.numpy() if isinstance(sim, torch.Tensor) else np.asarray(sim)
    P, n_g = partner.shape
    out = dict(score=np.zeros(P, np.float32), inliers=np.zeros(P, np.int32), matches=np.zeros(P, np.int32),
               model=np.zeros((P, 6), np.int32), inlier_mask=np.zeros((P, n_g), np.uint8))
    for p in range(P):
        r = verify(partner[p], sim[p], n_q, gw_q, gw_g, tol)
        out["score"][p], out["inliers"][p], out["matches"][p], out["model"][p], out["inlier_mask"][p] = \
            r["score"], r["inliers"], r["matches"], r["model"], r["mask"]
    return out


def local_rerank_similarity(q_local, idx, g_local, gw_q, gw_g, tol, index_base=0, k=None, min_sim=0.0):
    """vpr_similarity_local_rerank on features whose similarities are exact in f32: the arguments and the result of
    spatial_ref.local_rerank_spatial, with pair_model [B, kc, 6] in the place of pair_shift."""
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
               pair_matches=np.zeros((B, kc), np.int32), pair_model=np.full((B, kc, 6), I32_MIN, np.int32),
               row_nn=np.full((B, kc, n_q), -1, np.int32), col_nn=np.full((B, kc, n_g), -1, np.int32))
    memo = {}
    for b in range(B):
        rel = cand[b] - index_base
        live = (rel >= 0) & (rel < n_local)
        for t in np.nonzero(live)[0]:
            if (b, rel[t]) not in memo:
                p = ref.pair(q64[b], g64[rel[t]], min_sim)
                memo[b, rel[t]] = (p, verify(*sref.match_list(p), n_q, gw_q, gw_g, tol))
            p, v = memo[b, rel[t]]
            out["pair_score"][b, t], out["pair_inliers"][b, t], out["pair_matches"][b, t] = v["score"], v["inliers"], v["matches"]
            out["pair_model"][b, t] = v["model"]
            out["row_nn"][b, t], out["col_nn"][b, t] = p["row_nn"], p["col_nn"]
            assert v["matches"] == p["matches"]
        out["vals"][b], out["idx"][b], out["inliers"][b] = ref.order(out["pair_score"][b], out["pair_inliers"][b], cand[b], live, k)
    return out


# ------------------------------------------------------------------------------------------------ hand-made lists
def planted_similarity_list(rng, n_q, gw_q, n_g, gw_g, num, den, centre=None, rot90=False, noise=0):
    """A list in which candidate patch (x, y) is matched to the query patch at round-half-up((num / den) ((x, y) - c)) + c' — c
    the centre of the candidate grid (or `centre`), c' that of the query grid — wherever that lies on the query grid; rot90:
    the offset is turned by 90 degrees first (no admissible model).  Several columns may name one query patch (scale < 1), as a
    list handed to the verification alone may.  `noise` further columns go to random query patches.  Similarities are small
    integers / 4: every sum is exact."""
    gh_q, gh_g = n_q // gw_q, n_g // gw_g
    j = np.arange(n_g)
    cx, cy = centre if centre is not None else ((gw_g - 1) / 2, (gh_g - 1) / 2)
    ox, oy = j % gw_g - cx, j // gw_g - cy
    if rot90:
        ox, oy = -oy, ox
    x = np.floor(ox * num / den + (gw_q - 1) / 2 + 0.5).astype(np.int64)
    y = np.floor(oy * num / den + (gh_q - 1) / 2 + 0.5).astype(np.int64)
    ok = (x >= 0) & (x < gw_q) & (y >= 0) & (y < gh_q)
    partner = np.where(ok, y * gw_q + x, -1).astype(np.int32)
    free = np.nonzero(~ok)[0]
    if noise and free.size:
        pick = rng.choice(free, min(noise, free.size), replace=False)
        partner[pick] = rng.integers(0, n_q, pick.size)
    sim = (rng.integers(1, 9, n_g) / 4.0).astype(np.float32)
    return partner, sim


# ------------------------------------------------------------------------------------------------------ the recipe
two_hot, unit_sim, shifted_codes = sref.two_hot, sref.unit_sim, sref.shifted_codes


def zoomed_codes(q_codes, gw, fresh, num=3, den=2):
    """The zoomed view: the candidate patch at (x, y) shows the query patch at floor(1.5 (x - c) + c + 0.5) per axis,
    c = (gw - 1) / 2, and a code of `fresh` (none of them the query's) where that falls off the grid.  In doubled integers:
    floor((num (2 x - (gw - 1)) + den (gw - 1) + den) / (2 den))."""
    n = q_codes.shape[0]
    assert n == gw * gw
    j = np.arange(n)
    src = lambda v: (num * (2 * v - (gw - 1)) + den * (gw - 1) + den) // (2 * den)
    x, y = src(j % gw), src(j // gw)
    ok = (x >= 0) & (x < gw) & (y >= 0) & (y < gw)
    out = np.where(ok, q_codes[np.where(ok, y * gw + x, 0)], 0)
    out[~ok] = fresh[:int((~ok).sum())]
    return out


def block_distractor_codes(rng, q_codes, gw, shift=(2, 1), lo=1, hi=9):
    """The block distractor: a permutation of the query's codes in which the patches at lo <= x, y < hi show the query patch at
    (x + dx, y + dy) — an 8 x 8 block at one coherent shift — made by swapping codes; the rest stays scrambled."""
    n = q_codes.shape[0]
    out = q_codes[rng.permutation(n)].copy()
    where = {int(c): i for i, c in enumerate(out)}
    for y in range(lo, hi):
        for x in range(lo, hi):
            j, want = y * gw + x, int(q_codes[(y + shift[1]) * gw + x + shift[0]])
            i, have = where[want], int(out[j])
            out[j], out[i] = want, have
            where[want], where[have] = j, i
    for y in range(lo, hi):
        for x in range(lo, hi):
            assert out[y * gw + x] == q_codes[(y + shift[1]) * gw + x + shift[0]]
    assert np.array_equal(np.sort(out), np.sort(q_codes))
    return out


def recipe_codes(seed, gw):
    """The recipe on a gw x gw grid: (query codes [n], gallery codes [2, n]): image 0 is the block distractor, image 1 the true
    place, the query zoomed by 3/2."""
    rng = np.random.default_rng(seed)
    n = gw * gw
    codes = rng.permutation((L // 2) ** 2)
    q = codes[:n]
    return q, np.stack([block_distractor_codes(rng, q, gw), zoomed_codes(q, gw, codes[n:])])


def code_match_list(q_codes, g_codes, sim=1.0):
    """The match list of two images of unique codes: matching is code equality."""
    where = {int(c): i for i, c in enumerate(q_codes)}
    partner = np.array([where.get(int(c), -1) for c in g_codes], np.int32)
    return partner, np.where(partner >= 0, np.float32(sim), np.float32(0.0)).astype(np.float32)


def similarity_places(seed, N, D, B, gw, kind="bf16"):
    """B places seen four times each with near-equal global descriptors: one view is the query zoomed by 3/2, another the block
    distractor, the rest of the gallery is unrelated.  Two-hot features.  Returns (rows bf16 [N, D], local [N, n, l], queries
    bf16 [B, D], their local features, the rows of the zoomed views and of the distractors)."""
    rng = np.random.default_rng(seed)
    n = gw * gw
    q, rows = ref.unit(rng.standard_normal((B, D))), ref.unit(rng.standard_normal((N, D)))
    codes = rng.integers(0, (L // 2) ** 2, (N, n))
    qc = np.stack([rng.permutation((L // 2) ** 2) for _ in range(B)])
    perm = rng.permutation(N)
    true, distractor = np.empty(B, np.int64), np.empty(B, np.int64)
    for b in range(B):
        mine = perm[4 * b:4 * b + 4]
        rows[mine] = ref.unit(q[b] + 0.05 * ref.unit(rng.standard_normal((4, D))))
        true[b], distractor[b] = mine[0], mine[1]
        codes[true[b]] = zoomed_codes(qc[b, :n], gw, qc[b, n:])
        codes[distractor[b]] = block_distractor_codes(rng, qc[b, :n], gw)
    bf = lambda x: torch.from_numpy(x).to(torch.bfloat16)
    return bf(rows), two_hot(codes, kind), bf(q), two_hot(qc[:, :n], kind), true, distractor
