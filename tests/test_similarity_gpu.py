"""GPU: verification of patch matches under a similarity transform (include/vpr_amd_similarity.h) against its numpy restatement
(tests/similarity_ref.py).  vpr_similarity_verify on hand-made lists, every output bit for bit: every list length around the
block and wave seams, every grid shape, tol, planted scales and a rotated list, duplicates, junk partners, non-finite
similarities, ties, a list whose only admissible hypothesis is the last one, the order of the score's sum.
vpr_similarity_local_rerank, both element types and both match kernels, on two-hot integer features whose similarities are
exact: every output bit for bit; equality with the plain calls when all matches share one shift; equal bits from the two match
kernels; the edges of the contract; bit-identity across batch, position, padding, optional outputs, runs and graph replay;
Gaussian unit features through the restatement's integer stage; the recipe (a view zoomed by 3/2 against a distractor that
holds a coherent block); and the wiring through the sharded and graphed searches and the evaluation."""
import ctypes

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref
import similarity_ref as mref
import spatial_ref as sref
from test_spatial_gpu import assert_equal_bits, bits, candidates, rccl_one_rank, run_plain, spatial_gallery  # noqa: F401

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = mref.I32_MIN, mref.I32_MAX
KINDS = ("bf16", "e4m3")
VERIFY = ("score", "inliers", "matches", "model", "inlier_mask")
MAIN = ("vals", "idx", "inliers")
PAIR = ("pair_score", "pair_inliers", "pair_matches", "pair_model", "row_nn", "col_nn")
ALL = MAIN + PAIR


def run_verify(dev, partner, sim, n_q, gw_q, gw_g, tol, want_mask=True):
    from vpr_amd import ops
    out = ops.similarity_verify(torch.as_tensor(partner).to(dev), torch.as_tensor(sim).to(dev), n_q, gw_q, gw_g, tol, want_mask=want_mask)
    torch.cuda.synchronize()
    return {f: (None if t is None else t.cpu().numpy()) for f, t in zip(out._fields, out)}


def run(dev, q, idx, g, gw_q, gw_g, tol, base=0, k=None, min_sim=0.0, debug=True):
    from vpr_amd import ops
    out = ops.local_rerank_similarity(q.to(dev), idx.to(dev), g.to(dev), gw_q, gw_g, tol, base, k, min_sim, debug=debug)
    torch.cuda.synchronize()
    res = dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), inliers=out[2].cpu().numpy())
    if debug:
        res.update({f: getattr(out[3], f).cpu().numpy() for f in out[3]._fields})
    return res


def run_spatial(dev, q, idx, g, gw, tol, ms):
    from vpr_amd import ops
    out = ops.local_rerank_spatial(q.to(dev), idx.to(dev), g.to(dev), gw, gw, tol, 0, None, ms)
    torch.cuda.synchronize()
    return dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), inliers=out[2].cpu().numpy())


def check_verify(dev, partner, sim, n_q, gw_q, gw_g, tols):
    """Every output and the mask against the restatement; asking for the mask changes nothing else."""
    for tol in tols:
        got = run_verify(dev, partner, sim, n_q, gw_q, gw_g, tol)
        want = mref.verify_batch(partner, sim, n_q, gw_q, gw_g, tol)
        assert_equal_bits(got, want, VERIFY)
        bare = run_verify(dev, partner, sim, n_q, gw_q, gw_g, tol, want_mask=False)
        assert bare["inlier_mask"] is None
        assert_equal_bits(bare, want, VERIFY[:-1])
    return want


# ---------------------------------------------------------------------------------- vpr_similarity_verify, hand-made lists
def keep_first(partner, M):
    """The list with only its first M matches (in column order) kept."""
    out = np.full_like(partner, -1)
    cols = np.nonzero(partner >= 0)[0][:M]
    out[cols] = partner[cols]
    return out


def mixed_lists(rng, n_q, gw_q, n_g, gw_g):
    """Lists of every kind on one pair of grids: planted shifts and scales with noise, junk and non-finite similarities, a
    rotated list, random partners, duplicates, one match, none."""
    gh_q, gh_g = n_q // gw_q, n_g // gw_g
    lists = []
    for _ in range(3):
        shift = (int(rng.integers(-(gw_g - 1) // 2, gw_q // 2 + 1)), int(rng.integers(-(gh_g - 1) // 2, gh_q // 2 + 1)))
        lists.append(sref.planted_list(rng, n_q, gw_q, n_g, gw_g, shift, noise=n_g // 4))
    for num, den in ((3, 2), (2, 3), (1, 1), (2, 1), (1, 2), (5, 4)):
        lists.append(mref.planted_similarity_list(rng, n_q, gw_q, n_g, gw_g, num, den, noise=n_g // 8))
    lists.append(mref.planted_similarity_list(rng, n_q, gw_q, n_g, gw_g, 1, 1, rot90=True))
    partner = np.stack([p for p, _ in lists] + [rng.integers(0, n_q, n_g).astype(np.int32), np.full(n_g, min(3, n_q - 1), np.int32),
                                                np.full(n_g, -1, np.int32), np.full(n_g, -1, np.int32)])
    sim = np.stack([s for _, s in lists] + [(rng.integers(-8, 9, n_g) / 4.0).astype(np.float32)] * 4)
    partner[-2, n_g // 2] = n_q - 1                                               # exactly one match
    for p in range(1, 6):
        junk = rng.random(n_g) < 0.1
        partner[p][junk] = rng.choice(np.array([-1, I32_MIN, I32_MAX, n_q, n_q + 1, -7, 1 << 20]), int(junk.sum()))
        bad = rng.random(n_g) < 0.05
        sim[p][bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    return partner, sim


GRIDS = [(1, 1, 1, 1), (2, 1, 2, 1), (2, 2, 2, 1), (74, 2, 74, 37), (256, 16, 256, 16), (529, 23, 529, 23), (1369, 37, 1369, 37),
         (256, 16, 529, 23), (529, 23, 256, 16), (60, 4, 35, 7), (37, 1, 37, 37), (1369, 37, 289, 17)]


@pytest.mark.parametrize("n_q,gw_q,n_g,gw_g", GRIDS)
def test_verify_hand_made_lists_bit_for_bit(dev, n_q, gw_q, n_g, gw_g):
    rng = np.random.default_rng(n_q * 7 + gw_q + n_g * 3 + gw_g)
    partner, sim = mixed_lists(rng, n_q, gw_q, n_g, gw_g)
    want = check_verify(dev, partner, sim, n_q, gw_q, gw_g, (0, 1, 2, 8))
    assert want["matches"][-1] == 0 and want["matches"][-2] == 1 and (want["model"][-2:] == I32_MIN).all() and (want["inliers"][-2:] == 0).all()
    if n_g >= 35 and min(gw_q, n_q // gw_q, gw_g, n_g // gw_g) >= 2:
        assert want["inliers"].max() >= 8 and (want["model"][want["inliers"] > 0, 0] >= 0).all()
        assert want["matches"][-4] == n_g and want["matches"][-3] == n_g and want["inliers"][-3] == 0        # duplicates: dq = 0


@pytest.mark.parametrize("M", [0, 1, 2, 3, 16, 17, 255, 256, 257, 1369])
def test_verify_every_list_length(dev, M):
    """M matches on 37 x 37 grids: the first M columns of a pure shift, of a 3/2 zoom and of a scramble, and M matches spread
    over all six blocks of columns; M = 255, 256, 257 put one, none and two hypotheses on some match as s."""
    rng = np.random.default_rng(M)
    n, gw = 1369, 37
    base = [sref.planted_list(rng, n, gw, n, gw, (0, 0))[0], np.arange(n, dtype=np.int32)[rng.permutation(n)],
            mref.planted_similarity_list(rng, n, gw, n, gw, 3, 2, noise=n)[0]]
    spread = np.full(n, -1, np.int32)
    cols = np.sort(rng.permutation(n)[:M])
    spread[cols] = np.clip(cols + 38, 0, n - 1)                                   # the shift (1, 1), clipped at the end
    partner = np.stack([keep_first(p, M) for p in base] + [spread])
    sim = (rng.integers(1, 9, partner.shape) / 4.0).astype(np.float32)
    want = check_verify(dev, partner, sim, n, gw, gw, (0, 1, 8))
    assert (want["matches"] == M).all()
    if M >= 2:
        assert want["inliers"][0] == M and want["model"][0, 3:].tolist() == [want["model"][0, 5], 0, want["model"][0, 5]]
    else:
        assert (want["inliers"] == 0).all() and (want["model"] == I32_MIN).all() and (want["score"].view(np.int32) == 0).all()


def test_verify_ties_duplicates_and_the_last_hypothesis(dev):
    n, gw = 256, 16
    j = np.arange(n)
    lists = []
    partner = np.full(n, -1, np.int32)
    partner[:10] = j[:10]
    partner[16:26] = j[16:26] + 1 + 3 * gw
    lists.append(partner.copy())                                               # 10 : 10, equal counts: the lowest h
    partner[26] = j[26] + 1 + 3 * gw
    lists.append(partner.copy())                                               # 10 : 11: the count decides before h
    dup = np.full(n, -1, np.int32)
    dup[[3, 200]] = 17
    lists.append(dup)                                                          # two columns, one partner: dq = 0
    lists.append(np.where(j % 2 == 0, 0, n - 1).astype(np.int32))              # every column to one of two patches
    # a list whose only admissible hypothesis is h = 255: a list turned by 90 degrees has none; the two matches of h = 255 are
    # put at their own positions (partner = column), which makes that pair the shift (0, 0); the restatement confirms that no
    # pair of one of them with a turned match became admissible
    rot, _ = mref.planted_similarity_list(np.random.default_rng(0), n, gw, n, gw, 1, 1, rot90=True)
    assert (rot >= 0).all()
    s, t = (int(v[255]) for v in mref.pair_indices(n))
    rot[s], rot[t] = s, t
    v = mref.verify(rot, np.ones(n, np.float32), n, gw, gw, 1)
    assert v["admissible"].sum() == 1 and v["admissible"][255]
    lists.append(rot)
    partner = np.stack(lists)
    sim = np.ones(partner.shape, np.float32)
    want = check_verify(dev, partner, sim, n, gw, gw, (0, 1, 2, 8))
    got = run_verify(dev, partner, sim, n, gw, gw, 0)
    assert got["inliers"][:2].tolist() == [10, 11] and got["model"][0, 0] == 0 and got["inlier_mask"][0, :10].all() and got["inlier_mask"][1, 16:27].all()
    assert got["matches"][2:4].tolist() == [2, n] and got["inliers"][2] == 0 and (got["model"][2] == I32_MIN).all()
    assert got["model"][4, 0] == 255 and got["inliers"][4] >= 2 and want["model"][4, 0] == 255


def test_verify_score_is_summed_in_the_stated_order(dev):
    """Every column matched with one shift, similarities ~ 23000 (integers, exact): the sum passes 2^24 and rounds, so the order
    shows: the device's bits are those of the stated order and not those of a plain ascending sum."""
    q, g = refh.order_pin_input()
    contrib, _ = refh.matched_contrib(q[0], g[0])
    n = contrib.shape[0]
    partner = np.arange(n, dtype=np.int32)[None]
    got = run_verify(dev, partner, contrib[None], n, 37, 37, 0)
    want, plain = refh.score_in_stated_order(contrib), refh.ascending_sum(contrib)
    assert float(want) > 2.0 ** 24 and want.view(np.int32) != plain.view(np.int32)
    assert got["score"].view(np.int32)[0] == want.view(np.int32) and got["inliers"][0] == got["matches"][0] == n
    assert got["model"][0].tolist() == [0, 0, 1, 1, 0, 1] and got["inlier_mask"].all()
    # an overflowing sum is clamped block by block: no Inf, no Inf - Inf
    huge = np.full((2, 300), np.finfo(np.float32).max, np.float32)
    huge[1, 256:] *= -1
    got = run_verify(dev, np.arange(300, dtype=np.int32)[None].repeat(2, 0), huge, 300, 20, 20, 0)
    assert got["score"][0] == np.finfo(np.float32).max and got["score"][1] == 0.0 and got["inliers"].tolist() == [300, 300]


# --------------------------------------------------------------------------- vpr_similarity_local_rerank, exact features
def similarity_gallery(rng, kind, B, n_q, gw_q, n_g, gw_g, n_local):
    """spatial_gallery (shifted, scrambled and random images), with every fourth image on equal square grids replaced by the
    query zoomed by 3/2 and every fifth by the block distractor (grids of 11 and more)."""
    C = (mref.L // 2) ** 2
    qc = np.stack([rng.permutation(C) for _ in range(B)])
    q, g = spatial_gallery(np.random.default_rng(int(rng.integers(1 << 30))), kind, B, n_q, gw_q, n_g, gw_g, n_local)
    if n_q == n_g and gw_q == gw_g and gw_q * gw_q == n_q and gw_q >= 3:
        q = mref.two_hot(qc[:, :n_q], kind)
        for r in range(n_local):
            if r % 4 == 0:
                g[r] = mref.two_hot(mref.zoomed_codes(qc[r % B, :n_q], gw_q, qc[r % B, n_q:]), kind)
            elif r % 5 == 1 and gw_q >= 11:
                g[r] = mref.two_hot(mref.block_distractor_codes(rng, qc[r % B, :n_q], gw_q), kind)
            elif r % 3 == 2:
                g[r] = mref.two_hot(mref.shifted_codes(qc[r % B, :n_q], gw_q, (1, -2), qc[r % B, n_q:]), kind)
    return q, g


# (B, kc, k_out, n_q, gw_q, n_g, gw_g): both match kernels (both sides <= 256: the 256-patch one), the block seam at 289,
# unequal grids on either side, the longest candidate list
SHAPES = [(1, 1, 1, 1, 1, 1, 1), (3, 4, 4, 2, 2, 2, 1), (3, 4, 1, 9, 3, 9, 3), (1, 128, 128, 9, 3, 9, 3), (1, 4, 1, 256, 16, 256, 16),
          (3, 4, 4, 256, 16, 256, 16), (1, 128, 1, 256, 16, 256, 16), (3, 1, 1, 289, 17, 289, 17), (1, 4, 4, 289, 17, 289, 17),
          (1, 4, 1, 529, 23, 529, 23), (3, 4, 4, 256, 16, 529, 23), (1, 4, 4, 529, 23, 256, 16), (3, 4, 1, 96, 12, 60, 4)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,kc,k,n_q,gw_q,n_g,gw_g", SHAPES)
def test_exact_features_bit_for_bit(dev, kind, B, kc, k, n_q, gw_q, n_g, gw_g):
    rng = np.random.default_rng(B * 1000 + kc * 7 + n_q + 3 * n_g)
    n_local, base = 6, 5
    q, g = similarity_gallery(rng, kind, B, n_q, gw_q, n_g, gw_g, n_local)
    idx = candidates(rng, B, kc, n_local, base)
    idx[0, 0] = base                                                           # at least one live pair
    ms = 1.5 * mref.unit_sim(kind)
    for tol in (0, 1, 8) if kc < 128 else (1,):
        got = run(dev, q, idx, g, gw_q, gw_g, tol, base, k, ms)
        want = mref.local_rerank_similarity(q, idx, g, gw_q, gw_g, tol, base, k, ms)
        assert_equal_bits(got, want, ALL)
    assert (want["pair_matches"] > 0).any()
    if n_q >= 256 and n_q == n_g:
        assert want["pair_inliers"].max() >= 100


@pytest.mark.parametrize("kind", KINDS)
def test_exact_features_at_1369_patches(dev, kind):
    rng = np.random.default_rng(1369)
    q, g = similarity_gallery(rng, kind, 1, 1369, 37, 1369, 37, 3)            # the zoomed view, the block distractor, a shift
    idx = torch.tensor([[1, 0, -1, 2]], dtype=torch.int32)
    ms = 1.5 * mref.unit_sim(kind)
    got = run(dev, q, idx, g, 37, 37, 1, 0, None, ms)
    want = mref.local_rerank_similarity(q, idx, g, 37, 37, 1, 0, None, ms)
    assert_equal_bits(got, want, ALL)
    assert got["pair_matches"][0].tolist() == [1369, 625, 0, 36 * 35] and got["pair_inliers"][0, [1, 3]].tolist() == [625, 36 * 35]
    assert got["pair_inliers"][0, 0] < 100 and got["idx"][0].tolist() == [2, 0, 1, -1]


@pytest.mark.parametrize("kind", KINDS)
def test_when_all_matches_share_one_shift_the_plain_calls_come_back(dev, kind):
    """Pure translations (all matches share one shift, M >= 2) at every tol: the pair's score and count and the order are those of
    local_rerank_hires — and of local_rerank at 256 patches and below — bit for bit."""
    rng = np.random.default_rng(5)
    ms = 1.5 * mref.unit_sim(kind)
    C = (mref.L // 2) ** 2
    for n, gw, tol in ((9, 3, 0), (256, 16, 0), (289, 17, 1), (529, 23, 8)):
        B, kc, n_local = 2, 6, 5
        codes = rng.permutation(C)
        qc = codes[:B * n].reshape(B, n)
        fresh = codes[B * n:]
        lim = min(3, gw - 2)                                                   # at least two matches stay on the grid
        gc = np.stack([mref.shifted_codes(qc[r % B], gw, (int(rng.integers(-lim, lim + 1)), int(rng.integers(-lim, lim + 1))),
                                          rng.permutation(fresh)) for r in range(n_local)])
        q, g = mref.two_hot(qc, kind), mref.two_hot(gc, kind)
        idx = candidates(rng, B, kc, n_local, 0)
        idx[:, 0] = torch.arange(B)
        got = run(dev, q, idx, g, gw, gw, tol, 0, None, ms)
        live = (idx.numpy() >= 0) & (idx.numpy() < n_local)
        own = live & (idx.numpy() % B == np.arange(B)[:, None])                # the query's own shifted views
        assert (got["pair_matches"][own] >= 2).all() and (got["pair_matches"][live & ~own] == 0).all()
        assert np.array_equal(got["pair_inliers"], got["pair_matches"])
        for hires in (True, False) if n <= 256 else (True,):
            plain = run_plain(dev, kind, q, idx, g, 0, None, ms, hires)
            assert_equal_bits(got, plain, ("vals", "idx", "pair_score", "pair_matches", "row_nn", "col_nn"))
            assert_equal_bits(dict(inliers=got["inliers"], pair_inliers=got["pair_inliers"]),
                              dict(inliers=plain["matches"], pair_inliers=plain["pair_matches"]), ("inliers", "pair_inliers"))
        assert got["pair_matches"].max() > (n * 5) // 10 or n <= 9


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_match_kernels_give_the_same_bits(dev, kind):
    """Both sides at 256 patches run the 256-patch match kernel.  The same gallery with one more grid row of NaN features (272
    patches, no similarity with anything) runs the hires kernel on the same similarities: every output is the same, bit for
    bit — the positions of the first 256 columns do not move."""
    rng = np.random.default_rng(11)
    B, kc, n, gw, n_local = 3, 7, 256, 16, 6
    q, g = similarity_gallery(rng, kind, B, n, gw, n, gw, n_local)
    pad = torch.full((n_local, gw, mref.L), float("nan"), dtype=torch.bfloat16) if kind == "bf16" else torch.full((n_local, gw, mref.L), 0x7F, dtype=torch.uint8)
    g_tall = torch.cat([g, pad], 1).contiguous()
    idx = candidates(rng, B, kc, n_local, 0)
    idx[0, 0] = 0                                                              # the first query's own zoomed view
    ms = 1.5 * mref.unit_sim(kind)
    for tol in (0, 2):
        small = run(dev, q, idx, g, gw, gw, tol, 0, 4, ms)
        tall = run(dev, q, idx, g_tall, gw, gw, tol, 0, 4, ms)
        assert_equal_bits(tall, small, MAIN + PAIR[:5])
        assert np.array_equal(tall["col_nn"][:, :, :n], small["col_nn"]) and (tall["col_nn"][:, :, n:] == -1).all()
        assert_equal_bits(small, mref.local_rerank_similarity(q, idx, g, gw, gw, tol, 0, 4, ms), ALL)
    assert small["pair_inliers"].max() >= 100


# -------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("kind", KINDS)
def test_edges(dev, kind):
    rng = np.random.default_rng(17)
    n, gw, base, n_local = 289, 17, 100, 6
    q, g = similarity_gallery(rng, kind, 4, n, gw, n, gw, n_local)
    nan = float("nan") if kind == "bf16" else 0x7F
    g[1] = nan                                                                 # never named by a live index: never read
    g[2, 3], g[2, 255, 0], g[2, 256, 1], g[2, 288, 127] = nan, nan, nan, nan   # NaN patches beside live ones, at the block seam
    q[1, 5], q[1, 255, 7], q[1, 256] = nan, nan, nan
    g[4, 200:] = 0                                                             # zero feature rows
    q[3] = 0                                                                   # an all-zero query: every S is 0
    idx = torch.tensor([[102, -1, I32_MIN, I32_MAX, 99, 106, 102, 100, 104, 1, 2],
                        [105, 102, 102, 104, -1, -1, 103, 100, 106, 99, 0],
                        [-1, I32_MIN, I32_MAX, 99, 106, 1, 2, 3, 4, 5, -7],         # an all-padding query
                        [104, 100, 103, 105, 102, 104, -1, -1, -1, -1, -1]], dtype=torch.int32)
    assert not (idx == 101).any()
    for ms in (1.5 * mref.unit_sim(kind), 0.0):
        for k in (1, 11):
            got = run(dev, q, idx, g, gw, gw, 1, base, k, ms)
            want = mref.local_rerank_similarity(q, idx, g, gw, gw, 1, base, k, ms)
            assert_equal_bits(got, want, ALL)
    assert np.isfinite(got["pair_score"][idx.numpy() == 102]).all()
    assert (got["vals"][2] == -np.inf).all() and (got["idx"][2] == -1).all() and (got["inliers"][2] == 0).all()
    assert (got["pair_model"][2] == I32_MIN).all() and (got["pair_matches"][2] == 0).all() and (got["pair_inliers"][2] == 0).all()
    assert got["idx"][0].tolist().count(102) == 2                              # duplicates: scored as often as they occur
    none = run(dev, q, idx, g, gw, gw, 1, 1000, 3, 0.0)                        # a shard that owns nothing of the list
    assert (none["idx"] == -1).all() and (none["vals"] == -np.inf).all() and (none["pair_score"] == -np.inf).all()
    assert (none["row_nn"] == -1).all() and (none["col_nn"] == -1).all() and (none["pair_model"] == I32_MIN).all()
    high = run(dev, q, idx, g, gw, gw, 1, base, 11, 1e6)                       # min_sim above every similarity: no match anywhere
    live = (idx.numpy() >= base) & (idx.numpy() < base + n_local)
    assert (high["pair_matches"] == 0).all() and (high["pair_score"][live] == 0).all() and (high["pair_model"] == I32_MIN).all()
    assert_equal_bits(high, mref.local_rerank_similarity(q, idx, g, gw, gw, 1, base, 11, 1e6), ALL)


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_call_leaves_its_outputs_untouched(dev, kind):
    from vpr_amd import _lib, ops
    lib = _lib.lib()
    B, kc, n, l = 2, 3, 1370, 64
    es = 2 if kind == "bf16" else 1
    feats = torch.zeros(B * n * l * es, dtype=torch.uint8, device=dev)
    idx = torch.zeros((B, kc), dtype=torch.int32, device=dev)
    outs = [torch.full((B * kc * n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(9)]
    need = lib.vpr_similarity_workspace_bytes(B, kc, 289)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_q=289, gw_q=17, n_g=289, gw_g=17, tol=1, l=l, min_sim=0.0, fp8=int(kind == "e4m3"), ws_bytes=need):
        return lib.vpr_similarity_local_rerank(p(feats), n_q, p(idx), B, kc, p(feats), n_g, l, B, 0, min_sim, kc, *[p(o) for o in outs],
                                               fp8, gw_q, gw_g, tol, p(ws), ws_bytes, ops._stream())

    unsupported, invalid = -2, -1
    for kw, status in ((dict(n_q=1370, gw_q=10), unsupported), (dict(n_g=1370, gw_g=10), unsupported), (dict(gw_q=0), unsupported),
                       (dict(gw_g=16), unsupported), (dict(tol=9), unsupported), (dict(tol=-1), invalid), (dict(fp8=2), invalid),
                       (dict(n_q=1368, gw_q=38), unsupported), (dict(n_g=1369, gw_g=1), unsupported), (dict(min_sim=float("nan"), tol=9), invalid),
                       (dict(l=48), unsupported), (dict(l=32 if kind == "e4m3" else 16), unsupported), (dict(ws_bytes=need - 1), unsupported)):
        assert call(**kw) == status, kw
    vout = [torch.full((B * n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(5)]
    verify = lambda **kw: lib.vpr_similarity_verify(p(outs[0]), p(outs[1]), B, kw.get("n_q", 289), kw.get("gw_q", 17), kw.get("n_g", 289),
                                                    kw.get("gw_g", 17), kw.get("tol", 1), *[p(o) for o in vout], ops._stream())
    for kw, status in ((dict(gw_q=0), unsupported), (dict(tol=9), unsupported), (dict(n_g=1370, gw_g=10), unsupported), (dict(tol=-1), invalid),
                       (dict(n_q=1368, gw_q=36), unsupported), (dict(n_g=1369, gw_g=1369), unsupported)):
        assert verify(**kw) == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A5A5A5A).all()) for o in outs + vout) and bool((ws == 0xA5).all())
    assert call() == 0 and verify() == 0                                       # and the same pointers with a supported shape run
    torch.cuda.synchronize()
    assert not bool((outs[0] == 0x5A5A5A5A).all()) and not bool((vout[0] == 0x5A5A5A5A).all())


# -------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("kind", KINDS)
def test_bit_identical_across_batch_position_padding_runs_outputs_and_graph_replay(dev, kind):
    from vpr_amd import ops
    rng = np.random.default_rng(23)
    B, kc, n, gw, n_local, base, tol = 5, 6, 529, 23, 7, 40, 1
    q, g = similarity_gallery(rng, kind, B, n, gw, n, gw, n_local)
    idx = candidates(rng, B, kc, n_local, base)
    ms = 1.5 * mref.unit_sim(kind)
    go = lambda q_, idx_, debug=True: run(dev, q_, idx_, g, gw, gw, tol, base, 4, ms, debug)
    full = go(q, idx)
    assert full["pair_inliers"].max() >= 225
    assert_equal_bits(go(q, idx), full, ALL)                                   # across runs
    assert_equal_bits(go(q, idx, False), full, MAIN)                           # without the optional outputs
    perm = torch.from_numpy(rng.permutation(B))
    moved = go(q[perm], idx[perm])                                             # across position in the batch
    assert_equal_bits({f: moved[f][np.argsort(perm.numpy())] for f in ALL}, full, ALL)
    for b in (0, 2, 4):                                                        # across B
        assert_equal_bits(go(q[b:b + 1], idx[b:b + 1]), {f: full[f][b:b + 1] for f in ALL}, ALL)
    pad = torch.cat([idx, torch.full((B, 7), -1, dtype=torch.int32)], 1)       # across trailing padding (another grid, too)
    padded = go(q, pad)
    assert_equal_bits(padded, full, MAIN)
    assert_equal_bits({f: padded[f][:, :kc] for f in PAIR}, full, PAIR)
    # under graph replay, with new inputs copied into the captured tensors
    qd, id_, gd = q.to(dev), idx.to(dev), g.to(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.local_rerank_similarity(qd, id_, gd, gw, gw, tol, base, 4, ms)     # warm-up: workspace, LDS opt-in
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.local_rerank_similarity(qd, id_, gd, gw, gw, tol, base, 4, ms)
    for order in (perm, torch.arange(B)):
        qd.copy_(q[order])
        id_.copy_(idx[order])
        graph.replay()
        torch.cuda.synchronize()
        assert_equal_bits(dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), inliers=out[2].cpu().numpy()),
                          go(q[order], idx[order], False), MAIN)


# ---------------------------------------------------------------------------------------------- Gaussian unit features
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,gw", [(256, 16), (529, 23)])
def test_gaussian_unit_features_through_the_integer_stage(dev, kind, n, gw):
    """On unit Gaussian features the device's neighbours may differ from the f64 ones where the epsilon-argmax tests of the match
    kernels allow.  So the device's own row_nn / col_nn name the mutual pairs (min_sim = 0 lies far below every mutual
    similarity, which is asserted), their f64 similarities fill the list, and the restatement's integer stage must give the
    device's model, inlier and match counts exactly; the standalone stage on that list gives the restatement's mask exactly.
    The device sums its own similarities, each within e of the f64 one (e = l u sum |q g|; plus the e4m3 MFMA's truncation), so
    the score is within sum e + gamma_L (sum |sim| + sum e) of the f64 sum over the inliers."""
    from vpr_amd import ops
    rng = np.random.default_rng(n + 1)
    B, kc, l, n_local, tol = 2, 3, 128, 4, 1
    x = ref.unit(rng.standard_normal((B, n, l)))
    y = ref.unit(rng.standard_normal((n_local, n, l)))
    y[3] = ref.unit(np.roll(x[0].reshape(gw, gw, l), (-1, -2), (0, 1)).reshape(n, l) + 0.02 * ref.unit(rng.standard_normal((n, l))))
    to = lambda a: torch.from_numpy(a).to(torch.bfloat16) if kind == "bf16" else ops.quantize_patch_fp8(torch.from_numpy(a.astype(np.float32)).to(dev)).cpu()
    q, g = to(x), to(y)
    q64, g64 = (ref.f64(q), ref.f64(g)) if kind == "bf16" else (ref8.decode(q), ref8.decode(g))
    idx = torch.from_numpy(rng.integers(0, n_local, (B, kc)).astype(np.int32))
    idx[0, 0] = 3
    cand = idx.numpy()
    got = run(dev, q, idx, g, gw, gw, tol, 0, None, 0.0)
    gam = ref.gamma(refh.sum_roundings(n))
    j = np.arange(n)
    for b in range(B):
        for t in range(kc):
            r, c = got["row_nn"][b, t], got["col_nn"][b, t]
            S = q64[b] @ g64[cand[b, t]].T
            e = l * ref.U * (np.abs(q64[b]) @ np.abs(g64[cand[b, t]]).T)
            if kind == "e4m3":
                e = e + ref8.mfma_truncation(q64[b], g64[cand[b, t]])
            assert (r >= 0).all() and (c >= 0).all()
            mutual = r[c] == j
            assert (S[c, j][mutual] > 0.05).all() and (e[c, j] < 0.01).all()   # min_sim = 0 decides nothing
            partner = np.where(mutual, c, -1).astype(np.int32)
            sim = np.where(mutual, S[c, j], 0.0)
            v = mref.verify(partner, sim.astype(np.float32), n, gw, gw, tol)
            assert got["pair_matches"][b, t] == v["matches"] and got["pair_inliers"][b, t] == v["inliers"]
            assert got["pair_model"][b, t].tolist() == list(v["model"])
            alone = run_verify(dev, partner[None], sim.astype(np.float32)[None], n, gw, gw, tol)
            assert np.array_equal(alone["inlier_mask"][0], v["mask"]) and alone["inliers"][0] == v["inliers"] and alone["model"][0].tolist() == list(v["model"])
            inl = v["mask"].astype(bool)
            exact, esum = sim[inl].sum(), e[c, j][inl].sum()             # the device sums its own similarities, each within e of S
            assert abs(float(got["pair_score"][b, t]) - exact) <= esum + gam * (np.abs(sim[inl]).sum() + esum)
    # wrap-around of np.roll: the shifted image's columns that still lie on the grid agree on one shift: scale 1, no rotation
    assert got["idx"][0, 0] == 3 and got["pair_inliers"][0, 0] >= (gw - 2) * (gw - 1)
    assert mref.scale_rotation(got["pair_model"][0, 0]) == (1.0, 0.0)


# ---------------------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gw,matches_true", [(16, 100), (23, 225), (37, 625)])
def test_recipe_the_zoomed_view_beats_the_block_distractor(dev, kind, gw, matches_true):
    from vpr_amd import ops
    n = gw * gw
    ms = 1.5 * mref.unit_sim(kind)
    idx = torch.tensor([[0, 1]], dtype=torch.int32)
    for seed in (0, 1):
        qc, gc = mref.recipe_codes(seed, gw)
        q, g = mref.two_hot(qc[None], kind), mref.two_hot(gc, kind)
        plain = run_plain(dev, kind, q, idx, g, 0, None, ms, hires=True)
        assert plain["idx"][0].tolist() == [0, 1] and plain["matches"][0].tolist() == [n, matches_true]      # the distractor first
        shift = run_spatial(dev, q, idx, g, gw, 1, ms)
        assert shift["idx"][0].tolist() == [0, 1] and shift["inliers"][0, 1] == 36 < 64 <= shift["inliers"][0, 0]    # ... and again
        got = run(dev, q, idx, g, gw, gw, 1, 0, None, ms)
        assert got["idx"][0].tolist() == [1, 0] and got["inliers"][0, 0] == matches_true > 73 >= got["inliers"][0, 1]
        assert got["pair_inliers"][0, 1] == got["pair_matches"][0, 1] == matches_true and got["pair_matches"][0, 0] == n
        h, cs, ct, re_, im, n2g = got["pair_model"][0, 1].tolist()
        assert 1.25 <= re_ / n2g <= 1.75 and abs(im) <= re_ / 4
        scale, rot = ops.similarity_model_scale_rotation(got["pair_model"][0, 1])
        assert 1.25 <= scale <= 1.8 and abs(rot) <= 15
        assert_equal_bits(got, mref.local_rerank_similarity(q, idx, g, gw, gw, 1, 0, None, ms), ALL)


# -------------------------------------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("kind", KINDS)
def test_torch_ops_and_sharded_merge(dev, kind):
    """torch.ops.vpr.local_rerank_similarity / similarity_verify are the wrappers; R hand-made shards scored apart and merged
    (vpr_topk_merge) give the single shard's answer."""
    from vpr_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vpr.*)
    rng = np.random.default_rng(31)
    B, kc, n, gw, N = 3, 12, 289, 17, 17
    q, g = similarity_gallery(rng, kind, B, n, gw, n, gw, N)
    idx = torch.stack([torch.from_numpy(rng.permutation(N)[:kc].astype(np.int32)) for _ in range(B)])
    ms = 1.5 * mref.unit_sim(kind)
    want = mref.local_rerank_similarity(q, idx, g, gw, gw, 1, 0, 6, ms)
    v, i, m = torch.ops.vpr.local_rerank_similarity(q.to(dev), idx.to(dev), g.to(dev), gw, gw, 1, 0, 6, ms)
    assert_equal_bits(dict(vals=v.cpu().numpy(), idx=i.cpu().numpy(), inliers=m.cpu().numpy()), want, MAIN)
    for R in (2, 3):
        vs, is_ = [], []
        for r in range(R):
            lo, hi = N * r // R, N * (r + 1) // R
            sv, si, _ = ops.local_rerank_similarity(q.to(dev), idx.to(dev), g[lo:hi].contiguous().to(dev), gw, gw, 1, lo, 6, ms)
            vs.append(sv)
            is_.append(si)
        mv, mi = ops.topk_merge(torch.stack(vs), torch.stack(is_))
        assert np.array_equal(mi.cpu().numpy(), want["idx"]) and np.array_equal(mv.cpu().numpy(), want["vals"])
    partner, sim = mixed_lists(rng, n, gw, n, gw)
    out = torch.ops.vpr.similarity_verify(torch.from_numpy(partner).to(dev), torch.from_numpy(sim).to(dev), n, gw, gw, 2)
    assert_equal_bits(dict(zip(VERIFY, (t.cpu().numpy() for t in out))), mref.verify_batch(partner, sim, n, gw, gw, 2), VERIFY)


def place_gallery(dev, seed, kind="bf16", N=96, D=128, B=4, gw=17, **kw):
    """B places seen four times each: one view is the query zoomed by 3/2, one the block distractor (mref.similarity_places); as
    a ShardedGallery(local_hires=True, local_grid=gw).  Returns (gallery, queries, their local features, rows of the zoomed
    views, rows of the distractors)."""
    from vpr_amd.retrieval import ShardedGallery
    rows, local, q, ql, true, distractor = mref.similarity_places(seed, N, D, B, gw, kind)
    sg = ShardedGallery(rows.to(dev), N, local_feats=local.to(dev), local_hires=True, local_grid=gw, **kw)
    return sg, q.to(dev), ql.to(dev), true, distractor


@pytest.mark.parametrize("kind", KINDS)
def test_search_local_reranked_with_the_similarity_model(dev, kind):
    gw = 17
    sg, q, ql, true, distractor = place_gallery(dev, 2, kind)
    k, kc, ms = 4, 16, 1.5 * mref.unit_sim(kind)
    v, i = sg.search_local_reranked(q, k, kc, ql, ms, spatial_tol=1, spatial_model="similarity")
    _, ci = sg.search(q, kc)
    want = mref.local_rerank_similarity(ql.cpu(), ci.cpu(), sg.local_feats.cpu(), gw, gw, 1, 0, k, ms)
    assert np.array_equal(i.cpu().numpy(), want["idx"]) and np.array_equal(bits(v).cpu().numpy(), want["vals"].view(np.int32))
    assert np.array_equal(i[:, 0].cpu().numpy(), true)
    for kw in (dict(spatial_tol=1), dict(spatial_tol=1, spatial_model="shift"), {}):       # the shift vote and the plain call: the distractor
        _, pi = sg.search_local_reranked(q, k, kc, ql, ms, **kw)
        assert np.array_equal(pi[:, 0].cpu().numpy(), distractor)
    for a, b in zip(sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=ms, spatial_tol=1, spatial_model="similarity"), (v, i)):
        assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="name spatial_tol"):
        sg.search_local_reranked(q, k, kc, ql, ms, spatial_model="similarity")


def test_one_rank_collective_path_equals_local_path(rccl_one_rank):
    dev = rccl_one_rank
    local, q, ql, _, _ = place_gallery(dev, 4)
    coll, _, _, _, _ = place_gallery(dev, 4, force_collectives=True)
    assert coll.collective and not local.collective
    kw = dict(spatial_tol=1, spatial_model="similarity")
    for a, b in zip(local.search_local_reranked(q, 5, 16, ql, 1.5, **kw), coll.search_local_reranked(q, 5, 16, ql, 1.5, **kw)):
        assert torch.equal(bits(a), bits(b))
    kw = dict(local_rerank=16, q_local_feats=ql, min_sim=1.5, spatial_tol=0, spatial_model="similarity")
    for a, b in zip(local.search_local_queries(q, 5, **kw), coll.search_local_queries(q, 5, **kw)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_similarity_rerank_equals_eager(rccl_one_rank, kind):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    B, k, kc, ms = 4, 5, 16, 1.5 * mref.unit_sim(kind)
    sg, q0, ql0, true, _ = place_gallery(dev, 6, kind, gw=23)
    gr = GraphedRetrieval(sg, B, k, local_rerank=kc, min_sim=ms, spatial_tol=1, spatial_model="similarity")
    assert gr.q_feats.shape == (B, 529, mref.L) and gr.q_feats.dtype == (torch.bfloat16 if kind == "bf16" else torch.uint8)
    for seed, (q, ql) in enumerate(((q0, ql0), (q0.roll(3, 0).contiguous(), ql0.roll(3, 0).contiguous()))):
        v_g, i_g = gr(q, ql)
        v_g, i_g = v_g.clone(), i_g.clone()
        v_e, i_e = sg.search_local_reranked(q, k, kc, ql, ms, spatial_tol=1, spatial_model="similarity")
        assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e)), seed
    assert np.array_equal(i_g[:, 0].cpu().numpy(), np.roll(true, 3))
    gr.close()


def test_retrieval_scores_with_the_similarity_model(dev, tmp_path, monkeypatch):
    """calculate_retrieval_scores(local_rerank=, spatial_tol=1, spatial_model="similarity") on generated images at 224 px (a
    16 x 16 grid): the result is retrieval_metrics, by hand, of search_local_reranked(spatial_model="similarity") on the same
    descriptor and local-feature batches."""
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, gallery as G, modules
    from vpr_amd.retrieval import ShardedGallery
    rng = np.random.default_rng(21)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g, px = 12, 224
    gnames = [f"img_{i:04d}.png" for i in range(n_g)]
    imgs = [rng.integers(0, 256, (px, px, 3), dtype=np.uint8) for _ in range(n_g)]
    for n, im in zip(gnames, imgs):
        Image.fromarray(im).save(gdir / n)
    lat, lon, ang = 219000 + 100.0 * np.arange(n_g), 143000 + 50.0 * np.arange(n_g), (17.0 * np.arange(n_g)) % 360
    pd.DataFrame({"filename": gnames, "timestamp": "t", "latitude": lat, "longitude": lon, "angle": ang,
                  "Region_ID": np.arange(n_g) // 5}).to_csv(tmp_path / "labels_train.csv", index=False)
    src = [3, 11, 0, 7]
    vnames = [f"img_{i:04d}.png" for i in range(len(src))]
    for n, s in zip(vnames, src):
        noisy = np.clip(imgs[s].astype(np.int16) + rng.integers(-3, 4, imgs[s].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(vdir / n)
    pd.DataFrame({"filename": vnames, "timestamp": "t", "latitude": lat[src] + 3.0, "longitude": lon[src] - 4.0,
                  "angle": (ang[src] + 5.0) % 360, "Region_ID": np.array(src) // 5}).to_csv(tmp_path / "labels_val.csv", index=False)
    torch.manual_seed(1)
    ext = modules.DinoV2Salad("vit_small", img_size=px)
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    assert evaluate.build_gallery_from_images(ext, str(tmp_path / "labels_train.csv"), str(gdir), str(tmp_path / "gal"), batch_size=4,
                                              keep_local=True, graph=False, image_size=px) == n_g
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None, **kw):
        seen.append((q_local.clone(), k, self.local_grid, {n: (v.clone() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}))
        return plain_search(self, q_local, k, expand, **kw)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run_ = lambda **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "labels_val.csv"), str(vdir), k=5,
                                                            tau=10.0, batch_size=4, verbose=False, graph=False, image_size=px, **kw)
    with pytest.raises(ValueError, match="name spatial_tol"):
        run_(local_rerank=8, spatial_model="similarity")
    got = run_(local_rerank=8, min_sim=0.5, spatial_tol=1, spatial_model="similarity")
    assert all(set(kw) == {"local_rerank", "q_local_feats", "min_sim", "spatial_tol", "spatial_model"} and kw["spatial_model"] == "similarity"
               and kw["spatial_tol"] == 1 and grid == 16 for *_, grid, kw in seen) and seen
    shard = G.load_gallery_shard(str(tmp_path / "gal"), dev, load_local=True)
    sg = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True, local_feats=shard.local, local_grid=16)
    batches = [sg.search_local_reranked(d16, k, 8, kw["q_local_feats"], 0.5, spatial_tol=1, spatial_model="similarity") for d16, k, _, kw in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    top = idx.cpu().numpy()
    assert top[:, 0].tolist() == src and got["topk_indices"].tobytes() == top.tobytes()
    assert got["topk_scores"].tobytes() == vals.cpu().numpy().tobytes()
    assert (got["topk_scores"][:, 0] > 128).all()            # the same image up to noise: the matches sit at one shift
    labels = shard.labels
    pose = labels[top[:, 0]][:, :3]
    assert np.allclose(got["pose"], pose)
    tq = df[["latitude", "longitude"]].to_numpy(dtype=np.float64)
    near = lambda rows, b: np.hypot(*(labels[rows][:, :2] - tq[b]).T) <= 10.0
    assert got["recall_at_1_tau"] == np.mean([near(top[b, :1], b).any() for b in range(len(src))]) == 1.0
    assert got["recall_at_5_tau"] == np.mean([near(top[b], b).any() for b in range(len(src))])
    assert got["recall_at_1_region"] == np.mean([labels[top[b, 0], 3] == df["Region_ID"][b] for b in range(len(src))]) == 1.0
    err = np.abs((pose[:, 2] - df["angle"].to_numpy() + 180) % 360 - 180)
    assert abs(got["maae"] - err.mean()) < 1e-9 and abs(err.mean() - 5.0) < 1e-9
