"""The matrix of match-kernel instantiations (csrc/local_match.hip::local_match_dispatch) and the inputs that run each of them:
(route, element, width) over the four routes that reach the two match kernels, with and without the match list, 12 widths each
= 48 cells, every cell its own compiled kernel.  Per cell the smallest shapes that cross every seam of its kernel, and per shape
inputs whose similarities are exact in f32, so that every comparison with the f64 restatements (tests/local_match_ref.py,
tests/local_match_fp8_ref.py, tests/spatial_ref.py) is bit for bit: (a) random integers with one matched pair planted exactly at
the threshold, (b) all-negative similarities, (c) non-finite patches on both sides of every seam, (d) on the spatial routes a
gallery of shifted, locally scrambled and unrelated images, (e) a one-hot diagonal.  Pure numpy / torch, no device; shared by
tests/test_local_match_matrix_cpu.py (premises of the inputs, and that they tell a wrong kernel from a right one) and
tests/test_local_match_matrix_gpu.py.  It imports nothing of the package."""
import functools
from collections import namedtuple

import numpy as np
import torch

import local_match_fp8_ref as ref8
import local_match_ref as ref
import spatial_ref as sref

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# ---------------------------------------------------------------------------------------------------------- the matrix
KINDS = ("bf16", "e4m3")
WIDTHS = {"bf16": (32, 64, 96, 128, 160, 192, 224, 256), "e4m3": (64, 128, 192, 256)}      # the LM_CASE lists of the dispatch
MAX_N_256 = 256                 # LM_MAX_N: above it on either side the call with the match list runs the hires kernel
GROUP = 4                       # LM_GROUP: candidates per workgroup of the 256-patch kernel
ROW_BLOCK = 256                 # LH_BLOCK: rows of a row block of the hires kernel, columns of a block of the score's sum
# route -> (the kernel, with the match list, the public entry per element)
ROUTES = {"rerank": ("256", False, {"bf16": "local_rerank", "e4m3": "local_rerank_fp8"}),
          "hires": ("hires", False, {"bf16": "local_rerank_hires", "e4m3": "local_rerank_fp8_hires"}),
          "spatial": ("256", True, {"bf16": "local_rerank_spatial", "e4m3": "local_rerank_spatial"}),
          "spatial_hires": ("hires", True, {"bf16": "local_rerank_spatial", "e4m3": "local_rerank_spatial"})}
CELLS = [(route, kind, l) for route in ROUTES for kind in KINDS for l in WIDTHS[kind]]

PLAIN_FIELDS = ("vals", "idx", "matches", "pair_score", "pair_matches", "row_nn", "col_nn")
SPATIAL_FIELDS = ("vals", "idx", "inliers", "pair_score", "pair_inliers", "pair_matches", "pair_shift", "row_nn", "col_nn")


def kernel_of(route):
    return ROUTES[route][0]


def has_list(route):
    return ROUTES[route][1]


def fields_of(route):
    return SPATIAL_FIELDS if has_list(route) else PLAIN_FIELDS


def kernel_for_counts(n_q, n_g):
    """The kernel launch_local_match_list chooses."""
    return "hires" if n_q > MAX_N_256 or n_g > MAX_N_256 else "256"


def elem_bytes(kind):
    return 2 if kind == "bf16" else 1


def chunks_per_row(kind, l):
    """CPR: 16-byte chunks of a feature row."""
    return l * elem_bytes(kind) // 16


def elems_per_chunk(kind):
    return 16 // elem_bytes(kind)


def swizzle_class(kind, l):
    """(SH, MASK) of lm_off for the cell's CPR."""
    cpr = chunks_per_row(kind, l)
    return (0, 15) if cpr % 16 == 0 else (1, 7) if cpr % 8 == 0 else (2, 3)


def chunk_cols(kind, l):
    """CW of the hires kernel: lh_chunk_cols."""
    return 256 if l * elem_bytes(kind) <= 256 else 128


def staging_trips(kind, l):
    """NST of the hires kernel."""
    return chunk_cols(kind, l) * chunks_per_row(kind, l) // 512


def k_step(kind):
    """Feature positions of one MFMA step."""
    return 16 if kind == "bf16" else 64


def unit_sim(kind):
    """The similarity of two features of integer value 1 at one position."""
    return 1.0 if kind == "bf16" else 2.0 ** -16


# ---------------------------------------------------------------------------------------------------------- the shapes
# (n_q, gw_q, n_g, gw_g); the grid widths matter on the spatial routes only (there every count factors into its grid and the
# pair passes sv_check_grid).
#   256-patch kernel: a partial 32-tile on both sides; the limit beside one short of it; n_g small with all eight waves busy;
#     and the mirror of that.
#   hires kernel: n_g just over one and just over two chunks of the cell's own CW (129 and 257 at CW = 128, 257 at CW = 256;
#     385 is a fourth chunk of 128 and a second of 256), n_q just over one row block, n_g over one block of the score's sum,
#     and one shape below 256 on both sides, which these entries run on the hires kernel too.
#   with the list the hires kernel runs only above 256 on either side: 132 = 12 x 11 and 272 = 16 x 17 stand for 129 and 257,
#     391 = 17 x 23 for 385.
SHAPES = {"rerank": ((33, 33, 65, 65), (256, 16, 255, 17), (256, 16, 33, 33), (65, 65, 256, 16)),
          "hires": ((257, 257, 129, 129), (129, 129, 257, 257), (31, 31, 385, 35), (33, 33, 65, 65)),
          "spatial": ((36, 6, 66, 11), (256, 16, 255, 17), (256, 16, 36, 6), (66, 11, 256, 16)),
          "spatial_hires": ((272, 16, 132, 12), (132, 12, 272, 16), (36, 6, 391, 17))}
B, KC, N_LOCAL, BASE = 2, 6, 3, 5          # KC is no multiple of GROUP: the second group of a query holds two candidates


def seams(n, cw):
    """Patch indices on both sides of every seam below n: the 32-tile, the chunk of cw columns, the block of 256, the end; and
    two away from any seam, so that the smallest image holds four."""
    return sorted({p for p in (1, n // 2, 31, 32, cw - 1, cw, ROW_BLOCK - 1, ROW_BLOCK, n - 2, n - 1) if 0 <= p < n})


# ---------------------------------------------------------------------------------------------------------- the inputs
Case = namedtuple("Case", "name q idx g base k min_sim gw_q gw_g tol meta")


def to_kind(kind, v):
    """Integer-valued (or e4m3-exact) f32 numpy -> bf16 features, or the e4m3 store whose byte values they are."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return torch.from_numpy(v).to(torch.bfloat16) if kind == "bf16" else torch.from_numpy(ref8.encode_ints(v))


def values(t):
    """Features as stored -> f64 numpy of what they stand for."""
    return ref8.decode(t) if t.dtype == torch.uint8 else ref.f64(t)


def cell_seed(route, kind, l, salt=0):
    return [list(ROUTES).index(route), KINDS.index(kind), l, salt]


def candidate_lists(rng, first=(0, 0)):
    """The mix of the existing suites (mostly rows of the shard, duplicates included, some padding and foreign rows), with
    fixed entries on top: query b's list opens with image first[b]; the second group of query 0 (positions 4, 5) opens with a
    dead candidate and ends with a live one."""
    idx = rng.integers(BASE, BASE + N_LOCAL, (B, KC))
    other = rng.choice(np.array([-1, BASE - 1, BASE + N_LOCAL, I32_MIN, I32_MAX, -7]), (B, KC))
    idx = np.where(rng.random((B, KC)) < 0.2, other, idx)
    for b, r in enumerate(first):
        idx[b, 0] = BASE + r
    idx[0, 4], idx[0, 5] = -1, BASE + 1
    return torch.from_numpy(idx.astype(np.int32))


def plant_threshold_pair(q, g, i0, j0, a=3, b=20):
    """q [n_q, l], g [n_g, l] integer values, in place: query patch i0 = e_a + e_b, candidate patch j0 = 2 e_a + e_b, so that
    S[i0][j0] = 3; every other candidate patch has g[a] + g[b] <= 2 and every other query patch 2 q[a] + q[b] <= 2 (one sign is
    turned where it was not so): the pair is each other's only best, a mutual match sitting exactly at 3 units."""
    flip = g[:, a] + g[:, b] >= 3
    g[flip, b] *= -1
    flip = 2 * q[:, a] + q[:, b] >= 3
    q[flip, a] *= -1
    q[i0], g[j0] = 0, 0
    q[i0, a], q[i0, b], g[j0, a], g[j0, b] = 1, 1, 2, 1


def integer_values(route, kind, l, n_q, n_g, salt):
    """Input (a) as values: entries -2 .. 2, the threshold pair planted in (query 0, image 0) at the last patch of either
    side."""
    rng = np.random.default_rng(cell_seed(route, kind, l, salt) + [n_q, n_g])
    q = rng.integers(-2, 3, (B, n_q, l)).astype(np.float32)
    g = rng.integers(-2, 3, (N_LOCAL, n_g, l)).astype(np.float32)
    plant_threshold_pair(q[0], g[0], n_q - 1, n_g - 1)
    return rng, q, g


def plant_non_finite(kind, t, rows, l):
    """t [n, l] as stored, in place: in turn a whole NaN patch, a single NaN element, +Inf and -Inf elements (bf16), or a
    whole 0x7F patch, a single 0xFF, a single 0x7F and a whole 0xFF patch (e4m3: the NaN bytes of either sign)."""
    nan, inf = float("nan"), float("inf")
    for n, r in enumerate(rows):
        d = (7 * n + 5) % l
        if kind == "bf16":
            if n % 4 == 0:
                t[r] = nan
            else:
                t[r, d] = (nan, inf, -inf)[n % 4 - 1]
        elif n % 4 in (0, 3):
            t[r] = 0x7F if n % 4 == 0 else 0xFF
        else:
            t[r, d] = 0xFF if n % 4 == 1 else 0x7F


def shifted_rows(q, gw_q, n_g, gw_g, shift, fresh):
    """sref.shifted_codes on feature rows, for two grids: the image whose patch at (x, y) of its grid is the query's patch at
    (x + dx, y + dy) where that lies on the query's grid (a match then has the shift (dx, dy)), and a row of `fresh` elsewhere."""
    gh_q = q.shape[0] // gw_q
    j = np.arange(n_g)
    x, y = j % gw_g + shift[0], j // gw_g + shift[1]
    ok = (x >= 0) & (x < gw_q) & (y >= 0) & (y < gh_q)
    out = fresh[:n_g].copy()
    out[ok] = q[(y * gw_q + x)[ok]]
    return out


SCRAMBLE_TILE = 5       # displacements of the scrambled image stay within +-4 bins: inside any window of the largest tolerance


def scrambled_rows(rng, q, gw_q, n_g, gw_g, fresh):
    """The image that holds the query's patches permuted inside tiles of 5 x 5 grid positions: as many matches as patches both
    grids share, their shifts spread over up to 81 bins, all within VPR_SPATIAL_MAX_TOL of each other."""
    gh_q, gh_g = q.shape[0] // gw_q, n_g // gw_g
    src = np.arange(n_g)
    for y0 in range(0, gh_g, SCRAMBLE_TILE):
        for x0 in range(0, gw_g, SCRAMBLE_TILE):
            tile = np.array([y * gw_g + x for y in range(y0, min(y0 + SCRAMBLE_TILE, gh_g)) for x in range(x0, min(x0 + SCRAMBLE_TILE, gw_g))])
            src[tile] = tile[rng.permutation(tile.size)]
    x, y = src % gw_g, src // gw_g
    ok = (x < gw_q) & (y < gh_q)
    out = fresh[:n_g].copy()
    out[ok] = q[(y * gw_q + x)[ok]]
    return out


def planted_shift(gw_q, gw_g):
    """The shift of the shifted image: (2, 1), or further to the right where the candidate's grid is the narrower one, so that
    the shift always pushes some of its columns off the query's grid (the scrambled image then holds more matches)."""
    return (max(2, gw_q - gw_g + 2), 1)


def spatial_gallery(route, kind, l, n_q, gw_q, n_g, gw_g):
    """Input (d): two queries of random integer patches (entries -2 .. 2: a patch's similarity with itself is about 2 l, with
    another about 2 sqrt(l) in size); image 0 = query 0 shifted by planted_shift, image 1 = query 0 scrambled, image 2
    unrelated, image 3 = query 1 shifted by (-2, -1).  Everything that is no copy is fresh random."""
    rng = np.random.default_rng(cell_seed(route, kind, l, 4) + [n_q, n_g])
    q = rng.integers(-2, 3, (B, n_q, l)).astype(np.float32)
    fresh = lambda: rng.integers(-2, 3, (n_g, l)).astype(np.float32)
    g = np.stack([shifted_rows(q[0], gw_q, n_g, gw_g, planted_shift(gw_q, gw_g), fresh()), scrambled_rows(rng, q[0], gw_q, n_g, gw_g, fresh()), fresh(),
                  shifted_rows(q[1], gw_q, n_g, gw_g, (-2, -1), fresh())])
    o = BASE                                                               # image r is row o + r of the gallery
    idx = torch.tensor([[o, o + 1, o + 2, o + 3, -1, o + 1], [o + 3, o + 2, I32_MAX, o, o + 1, o + 3]], dtype=torch.int32)
    return q, idx, g


ONE_HOT_VALUES = np.array([1, 2, -1.5, 0.5], dtype=np.float32)       # the candidate's value at d' (asymmetric)
ONE_HOT_GRID = 8                                                     # every width is a multiple of 8: l = 8 x (l / 8)
ONE_HOT_TALL = 264                                                   # = 8 x 33: over 256, so that the list takes the hires kernel


def one_hot_pair(route, kind, l):
    """Input (e) as values: (ones [n, l], valued [n', l]): row d of `ones` holds a single 1 at d, row d' of `valued` the
    asymmetric value at d'; n = n' = l, plus one all-zero patch on both sides at l = 256 on the hires entry (the chunk seam at
    256 then lies inside the image) and all-zero patches up to 264 on the valued side with the list on the hires kernel."""
    ones = np.zeros((l, l), dtype=np.float32)
    valued = np.zeros((l, l), dtype=np.float32)
    ones[np.arange(l), np.arange(l)] = 1
    valued[np.arange(l), np.arange(l)] = ONE_HOT_VALUES[np.arange(l) % 4]
    pad = lambda v, n: np.concatenate([v, np.zeros((n - v.shape[0], l), dtype=np.float32)])
    if route == "hires" and l == 256:
        ones, valued = pad(ones, 257), pad(valued, 257)
    if route == "spatial_hires":
        valued = pad(valued, ONE_HOT_TALL)
    return ones, valued


@functools.lru_cache(maxsize=None)
def cases(route, kind, l):
    """Every input of one cell, in the order the GPU test runs them."""
    u = unit_sim(kind)
    spatial = has_list(route)
    cw = chunk_cols(kind, l) if kernel_of(route) == "hires" else MAX_N_256
    out = []
    for n_q, gw_q, n_g, gw_g in SHAPES[route]:
        if spatial:
            assert kernel_for_counts(n_q, n_g) == kernel_of(route)
        grid = dict(gw_q=gw_q if spatial else None, gw_g=gw_g if spatial else None)
        tag = f"{n_q}x{n_g}"
        # (a) random integers, at both thresholds
        rng, qv, gv = integer_values(route, kind, l, n_q, n_g, 0)
        idx = candidate_lists(rng)
        q, g = to_kind(kind, qv), to_kind(kind, gv)
        for units, k in ((0, None), (3, 1)):
            out.append(Case(f"a/{tag}/min_sim={units}", q, idx, g, BASE, k, units * u, tol=1 if spatial else None,
                            meta=dict(input="a", units=units, planted=(n_q - 1, n_g - 1)), **grid))
        # (b) every similarity negative
        rng = np.random.default_rng(cell_seed(route, kind, l, 1) + [n_q, n_g])
        qb, gb = rng.integers(1, 3, (B, n_q, l)).astype(np.float32), -rng.integers(1, 3, (N_LOCAL, n_g, l)).astype(np.float32)
        out.append(Case(f"b/{tag}", to_kind(kind, qb), candidate_lists(rng), to_kind(kind, gb), BASE, None, -(4 * l + 1) * u,
                        tol=0 if spatial else None, meta=dict(input="b"), **grid))
        # (c) input (a) with non-finite patches on both sides of every seam, in query 0 and image 0
        rng, qv, gv = integer_values(route, kind, l, n_q, n_g, 2)
        q, g = to_kind(kind, qv), to_kind(kind, gv)
        rows, cols = seams(n_q, ROW_BLOCK), seams(n_g, cw)
        plant_non_finite(kind, q[0], rows, l)
        plant_non_finite(kind, g[0], cols, l)
        out.append(Case(f"c/{tag}", q, candidate_lists(rng), g, BASE, None, 0.0, tol=sref.MAX_TOL if spatial else None,
                        meta=dict(input="c", rows=rows, cols=cols), **grid))
        # (d) the shifted-integer gallery
        if spatial:
            qv, idx, gv = spatial_gallery(route, kind, l, n_q, gw_q, n_g, gw_g)
            q, g = to_kind(kind, qv), to_kind(kind, gv)
            for tol in (0, 1, sref.MAX_TOL):
                out.append(Case(f"d/{tag}/tol={tol}", q, idx, g, BASE, None, 1.5 * l * u, tol=tol,
                                meta=dict(input="d", shifts=(planted_shift(gw_q, gw_g), (-2, -1))), **grid))
    # (e) the one-hot diagonal, in both roles
    ones, valued = one_hot_pair(route, kind, l)
    for role, (qv, gv) in (("ones-valued", (ones, valued)), ("valued-ones", (valued, ones))):
        grid = dict(gw_q=ONE_HOT_GRID if spatial else None, gw_g=ONE_HOT_GRID if spatial else None)
        if spatial:
            assert kernel_for_counts(qv.shape[0], gv.shape[0]) == kernel_of(route)
        out.append(Case(f"e/{role}", to_kind(kind, qv[None]), torch.tensor([[1]], dtype=torch.int32),
                        to_kind(kind, np.stack([np.zeros_like(gv), gv])), 0, None, -1.0, tol=1 if spatial else None,
                        meta=dict(input="e"), **grid))
    return tuple(out)


def expected(case):
    """The restatement's outputs of one case (dict of numpy arrays)."""
    if case.tol is not None:
        return sref.local_rerank_spatial(case.q, case.idx, case.g, case.gw_q, case.gw_g, case.tol, case.base, case.k, case.min_sim)
    fn = ref8.local_rerank_fp8 if case.q.dtype == torch.uint8 else ref.local_rerank
    return fn(case.q, case.idx, case.g, case.base, case.k, case.min_sim)


def live_pairs(case):
    """The distinct (query, image) pairs the case's lists name: [(b, image row in g)]."""
    cand = case.idx.numpy().astype(np.int64) - case.base
    return sorted({(b, int(r)) for b in range(cand.shape[0]) for r in cand[b] if 0 <= r < case.g.shape[0]})


# ------------------------------------------------------------------------------------- the cheaper second set of inputs
def agreement_inputs(kind, l):
    """Input (a) at 256 patches and below for the test that sets the routes against each other: (n_q, gw_q, n_g, gw_g, q, idx, g,
    all_inliers).  all_inliers: the bin plane is at most 9 x 9, so that at VPR_SPATIAL_MAX_TOL every match is an inlier and the
    call with the list must give the plain calls' scores."""
    out = []
    for n_q, gw_q, n_g, gw_g, every in ((36, 6, 66, 11, False), (256, 16, 255, 17, False), (36, 6, 9, 3, True), (25, 5, 25, 5, True)):
        rng, qv, gv = integer_values("rerank", kind, l, n_q, n_g, 7)
        if every:
            assert max(gw_q + gw_g, n_q // gw_q + n_g // gw_g) - 2 <= sref.MAX_TOL
        out.append((n_q, gw_q, n_g, gw_g, to_kind(kind, qv), candidate_lists(rng), to_kind(kind, gv), every))
    return out
