"""GPU: local-feature re-ranking for up to 1369 patches per image (include/vpr_amd_local_hires.h), both element types, against
the f64 restatements (tests/local_match_ref.py, tests/local_match_fp8_ref.py, which have no patch limit) and the stated order of
the score's sum (tests/local_match_hires_ref.py): bit for bit on integer features across every chunk, row-block and column-block
seam of the kernel; bit for bit against the 256-patch calls where both apply; the order pin; epsilon-argmaxes on Gaussian unit
features; a planted permutation that puts a best match into every (row block, column chunk) combination; the edges of the
contract; bit-identity across batch, position, padding, runs, optional outputs and graph replay; and the wiring through the
modules, the sharded and graphed searches and the evaluation."""
import ctypes

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ALL = ("row_nn", "col_nn", "pair_matches", "pair_score", "vals", "idx", "matches")
S1 = 2.0 ** -16         # the e4m3 similarity of two bytes of value 1
KINDS = ("bf16", "e4m3")
OP = {"bf16": "local_rerank_hires", "e4m3": "local_rerank_fp8_hires"}
OP256 = {"bf16": "local_rerank", "e4m3": "local_rerank_fp8"}


def run(dev, kind, q, idx, g, base=0, k=None, min_sim=0.0, debug=True, op=None):
    from vpr_amd import ops
    out = getattr(ops, op or OP[kind])(q.to(dev), idx.to(dev), g.to(dev), base, k, min_sim, debug=debug)
    torch.cuda.synchronize()
    res = dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy())
    if debug:
        res.update({f: getattr(out[3], f).cpu().numpy() for f in out[3]._fields})
    return res


def restate(kind, q, idx, g, base=0, k=None, min_sim=0.0):
    return (ref.local_rerank if kind == "bf16" else ref8.local_rerank_fp8)(q, idx, g, base, k, min_sim)


def int_features(kind, rng, *shape):
    """Entries -2 .. 2: bf16 holds them; the e4m3 store holds them as byte values (the features v * 2^-8)."""
    v = rng.integers(-2, 3, shape).astype(np.float32)
    return torch.from_numpy(v).to(torch.bfloat16) if kind == "bf16" else torch.from_numpy(ref8.encode_ints(v))


def unit_features(dev, kind, x):
    """f64 unit rows -> bf16, or their e4m3 store through the device quantiser."""
    from vpr_amd import ops
    if kind == "bf16":
        return torch.from_numpy(x).to(torch.bfloat16)
    return ops.quantize_patch_fp8(torch.from_numpy(x.astype(np.float32)).to(dev)).cpu()


def values(kind, t):
    return ref.f64(t) if kind == "bf16" else ref8.decode(t)


def candidates(rng, B, kc, n_local, base):
    """Mostly rows of the shard (duplicates included), some padding and foreign rows."""
    idx = rng.integers(base, base + n_local, (B, kc))
    other = rng.choice(np.array([-1, base - 1, base + n_local, I32_MIN, I32_MAX, -7]), (B, kc))
    return torch.from_numpy(np.where(rng.random((B, kc)) < 0.2, other, idx).astype(np.int32))


def assert_equal_bits(got, want, fields):
    for f in fields:
        a, b = got[f], want[f]
        assert a.shape == b.shape and a.dtype == b.dtype, f
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (f, np.argwhere(a.view(np.int32) != b.view(np.int32))[:5])


# ------------------------------------------------------------------------------------------------ integer features
# The kernel's seams: column chunks of 256 columns (128 where a feature row exceeds 256 bytes: bf16 l > 128), row blocks of 256
# rows, blocks of 256 columns in the sum, tiles of 32 everywhere.  So every multiple of 128 up to 1280 is an edge: the issue's
# list {1, 31, 33, 127, 128, 129, 255, 256, 257, 288, 383, 385, 511, 512, 513, 529, 1024, 1369} and, around the edges it lacks,
# {639, 640, 641, 767, 768, 769, 895, 896, 897, 1023, 1025, 1151, 1152, 1153, 1279, 1280, 1281}.
NS = [1, 31, 33, 127, 128, 129, 255, 256, 257, 288, 383, 385, 511, 512, 513, 529, 1024, 1369,
      639, 640, 641, 767, 768, 769, 895, 896, 897, 1023, 1025, 1151, 1152, 1153, 1279, 1280, 1281]
PAIRS = [(257, 1), (1, 257), (529, 256), (256, 529), (1369, 65), (65, 1369), (1369, 1369)] + \
        [(NS[i], NS[(i + 11) % len(NS)]) for i in range(len(NS))]          # every n on either side, n_q != n_g


def int_shapes():
    """(B, kc, k_out, n_q, n_g, l index): l, B, kc and k_out cycle with different periods so that every value meets small and
    large images; the large B x kc products ride on the smaller pairs.  l index 0 = the narrowest width (32 bf16, 64 e4m3)."""
    out = []
    for t, (n_q, n_g) in enumerate(PAIRS):
        big = n_q * n_g > 600 * 600
        B, kc = (1, (1, 5)[t % 2]) if big else ((1, 3)[t % 2], (5, 1)[(t // 2) % 2])
        out.append((B, kc, (1, kc)[(t // 3) % 2], n_q, n_g, t % 3))
    out.append((1, 128, 128, 257, 257, 0))                                 # the longest candidate list
    out.append((3, 128, 1, 257, 33, 1))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,kc,k,n_q,n_g,li", int_shapes())
def test_integer_features_bit_for_bit(dev, kind, B, kc, k, n_q, n_g, li):
    """Entries in -2 .. 2: |S| <= 4 l <= 1024 (times 2^-16 for e4m3) and a score <= 1369 * 1024 < 2^24 are exact in f32
    whatever the order of the sums.  Full of ties: the lowest-index rule across every seam, and the padding masks."""
    l = ((32, 128, 256) if kind == "bf16" else (64, 128, 256))[li]
    rng = np.random.default_rng(B * 1000 + kc * 7 + n_q + n_g + l)
    n_local, base = 4, 5
    q, g = int_features(kind, rng, B, n_q, l), int_features(kind, rng, n_local, n_g, l)
    idx = candidates(rng, B, kc, n_local, base)
    idx[0, 0] = base + 1                                                   # at least one live pair
    unit_s = 1.0 if kind == "bf16" else S1
    for min_sim in (0.0, 3.0 * unit_s):
        got = run(dev, kind, q, idx, g, base, k, min_sim)
        want = restate(kind, q, idx, g, base, k, min_sim)
        assert_equal_bits(got, want, ALL)
    assert (want["pair_matches"] > 0).any() or n_q * n_g == 1


# ----------------------------------------------------------------------------------- equality with the 256-patch calls
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_q,n_g", [(1, 1), (33, 256), (256, 33), (196, 196), (256, 256), (1, 196), (196, 1), (33, 33)])
def test_at_256_patches_and_below_every_output_equals_the_existing_call(dev, kind, n_q, n_g):
    rng = np.random.default_rng(n_q * 300 + n_g)
    B, kc, n_local, base, l = 3, 6, 5, 2, (128 if (n_q + n_g) % 2 else 64)
    idx = candidates(rng, B, kc, n_local, base)
    gauss = (unit_features(dev, kind, ref.unit(rng.standard_normal((B, n_q, l)))),
             unit_features(dev, kind, ref.unit(rng.standard_normal((n_local, n_g, l)))))
    ints = (int_features(kind, rng, B, n_q, l), int_features(kind, rng, n_local, n_g, l))
    for q, g in (gauss, ints):
        for k, min_sim in ((None, 0.0), (1, 0.1 if q is gauss[0] else 2.0 * (1.0 if kind == "bf16" else S1))):
            new = run(dev, kind, q, idx, g, base, k, min_sim)
            old = run(dev, kind, q, idx, g, base, k, min_sim, op=OP256[kind])
            assert_equal_bits(new, old, ALL)
    assert np.isfinite(new["pair_score"]).any()


# ------------------------------------------------------------------------------------------------------ the order pin
def test_score_is_summed_in_the_stated_order(dev):
    """Integers in -16 .. 16 at l = 256, n = 1369, the image = the query's patches permuted: every S is exact, every column is
    matched, the sum passes 2^24 and rounds.  pair_score must be the numpy f32 emulation of the stated order, bit for bit, given
    the restatement's exact matched similarities; tests/test_local_match_hires_cpu.py shows that a plain ascending sum gives
    other bits on this input."""
    q, g = refh.order_pin_input()
    contrib, p = refh.matched_contrib(q[0], g[0])
    want = refh.score_in_stated_order(contrib)
    got = run(dev, "bf16", q, torch.zeros((1, 1), dtype=torch.int32), g)
    assert np.array_equal(got["row_nn"][0, 0], p["row_nn"]) and np.array_equal(got["col_nn"][0, 0], p["col_nn"])
    assert got["pair_matches"][0, 0] == p["matches"] == refh.ORDER_PIN_N and float(want) > 2.0 ** 24
    assert got["pair_score"].view(np.int32)[0, 0] == want.view(np.int32), (got["pair_score"][0, 0], want)
    assert got["vals"].view(np.int32)[0, 0] == want.view(np.int32)


# ---------------------------------------------------------------------------------------------- Gaussian unit features
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,kc,n_q,n_g,l", [(2, 3, 257, 257, 64), (1, 3, 529, 529, 128), (1, 2, 1369, 1369, 128), (1, 2, 1369, 300, 256)])
def test_gaussian_unit_features_are_epsilon_argmaxes(dev, kind, B, kc, n_q, n_g, l):
    """The assertions of tests/test_local_match_gpu.py (bf16: e[i][j] = l 2^-24 sum_d |q g|) and of
    tests/test_local_match_fp8_gpu.py (e4m3: e + t, t = local_match_fp8_ref.mfma_truncation), with L = 10 + ceil(n_g / 256)
    roundings in the score's sum: every device choice is an epsilon-argmax, no row or column left out; the match count is
    integer logic on the device's own neighbours; the score is within sum_matched e + gamma_L sum_matched |S| of the f64 sum.
    A mutual pair within its own slack of min_sim may fall either way on the device and is counted and summed as undecided,
    as the e4m3 test does, here for both elements: among the hundreds of mutual pairs of two random images of 529 or 1369
    patches, whose similarities crowd between 0.2 and 0.35, one within 1e-5 of 0.25 is an ordinary event (the bf16 test's
    stronger premise, that no pair comes that close, holds only for its few small images)."""
    rng = np.random.default_rng(n_q + n_g + l)
    n_local = 4
    q = unit_features(dev, kind, ref.unit(rng.standard_normal((B, n_q, l))))
    g = unit_features(dev, kind, ref.unit(rng.standard_normal((n_local, n_g, l))))
    g[3, : min(n_g, n_q)] = q[0, : min(n_g, n_q)]                          # one image shares the first query's patches
    idx = torch.from_numpy(rng.integers(0, n_local, (B, kc)).astype(np.int32))
    idx[0, 0] = 3
    q64, g64, cand = values(kind, q), values(kind, g), idx.numpy()
    gam = ref.gamma(refh.sum_roundings(n_g))
    worst, slack = 0.0, {}
    for min_sim in (0.0, 0.25):
        got = run(dev, kind, q, idx, g, 0, None, min_sim)
        ms = float(np.float32(min_sim))
        for b in range(B):
            for t in range(kc):
                key = (b, cand[b, t])
                if key not in slack:
                    S = q64[b] @ g64[cand[b, t]].T
                    e = l * ref.U * (np.abs(q64[b]) @ np.abs(g64[cand[b, t]]).T)
                    if kind == "e4m3":
                        e = e + ref8.mfma_truncation(q64[b], g64[cand[b, t]])
                    slack[key] = (S, e, (S - e).max(1), (S - e).max(0))
                S, e, row_floor, col_floor = slack[key]
                r, c = got["row_nn"][b, t], got["col_nn"][b, t]
                assert (r >= 0).all() and (r < n_g).all() and (c >= 0).all() and (c < n_q).all()
                i, j = np.arange(n_q), np.arange(n_g)
                assert (S[i, r] + e[i, r] >= row_floor).all()
                assert (S[c, j] + e[c, j] >= col_floor).all()
                mutual = r[c] == j
                und = mutual & (np.abs(S[c, j] - ms) <= e[c, j])             # within its own slack of min_sim: either way
                m = mutual & (S[c, j] > ms + e[c, j])
                assert m.sum() <= got["pair_matches"][b, t] <= m.sum() + und.sum()
                exact = S[c, j][m].sum()
                bound = e[c, j][m | und].sum() + gam * np.abs(S[c, j][m | und]).sum()
                score = float(got["pair_score"][b, t])
                assert exact + S[c, j][und].clip(None, 0).sum() - bound <= score <= exact + S[c, j][und].clip(0).sum() + bound, \
                    (b, t, score, exact, bound, und.sum())
                if bound > 0 and not und.any():
                    worst = max(worst, abs(score - exact) / bound)
        if min_sim == 0.25:
            assert got["pair_matches"][0, 0] >= min(n_q, n_g) and got["idx"][0, 0] == 3
    print(f"{OP[kind]} score error, largest share of its bound at ({n_q}, {n_g}, {l}): {worst:.4f}")


# ------------------------------------------------------------------------------------------- the planted permutation
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [529, 1369])
def test_planted_permutation_comes_back_first_with_every_patch_matched(dev, kind, n):
    """ref.recipe: the true image (last of 21) holds the query's patches permuted plus noise.  It comes back first with all n
    patches matched, and row_nn of that pair is the inverse permutation: a best match in every (row block, column chunk)."""
    seed, l = 3, 128
    q, gal = ref.recipe(seed, n, l)
    rng = np.random.default_rng(seed)                                      # the recipe's own draws, in its order
    rng.standard_normal((n, l))
    perm = rng.permutation(n)                                              # true[j] = q[perm[j]] + noise
    if kind == "e4m3":
        q, gal = unit_features(dev, kind, q.double().numpy()), unit_features(dev, kind, gal.double().numpy())
    N = gal.shape[0]
    idx = torch.arange(N, dtype=torch.int32)[None]                         # the true image at the last position of the list
    got = run(dev, kind, q, idx, gal, 0, None, 0.0)
    assert got["idx"][0, 0] == N - 1 and got["matches"][0, 0] == n and 0.99 * n <= got["vals"][0, 0] <= 1.004 * n
    assert np.array_equal(got["col_nn"][0, N - 1], perm) and np.array_equal(got["row_nn"][0, N - 1][perm], np.arange(n))
    blocks = {(int(i) // 256, int(j) // 128) for j, i in enumerate(perm)}
    assert len(blocks) == ((n + 255) // 256) * ((n + 127) // 128)          # every (row block, column chunk of either width)
    assert got["pair_score"][0, :N - 1].max() < got["vals"][0, 0] / 2
    hard = run(dev, kind, q, idx, gal, 0, None, 0.6)
    assert (hard["pair_score"][0, :N - 1] == 0).all() and (hard["pair_matches"][0, :N - 1] == 0).all()
    assert hard["idx"][0, 0] == N - 1 and hard["matches"][0, 0] == n
    assert hard["idx"][0, 1:].tolist() == list(range(N - 1))               # all-zero scores: by ascending index


# -------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("kind", KINDS)
def test_edges(dev, kind):
    rng = np.random.default_rng(17)
    n_q, n_g, l, base, n_local = 300, 300, 64, 100, 6
    q, g = int_features(kind, rng, 4, n_q, l), int_features(kind, rng, n_local, n_g, l)
    bad_cols, bad_rows = [3, 9, 255, 256, 299], [5, 6, 255, 256, 288]       # on both sides of the chunk / block seam at 256
    if kind == "bf16":
        nan, inf = float("nan"), float("inf")
        g[1] = nan                                                         # never named by a live index: never read
        g[2, 3], g[2, 9, 5], g[2, 255, 0], g[2, 256, 1], g[2, 299, 63] = nan, nan, inf, -inf, nan
        q[1, 5], q[1, 6, 2], q[1, 255, 7], q[1, 256], q[1, 288, 1] = inf, nan, nan, -inf, inf
    else:
        g[1] = 0x7F
        g[2, 3], g[2, 9, 5], g[2, 255, 0], g[2, 256, 1], g[2, 299, 63] = 0x7F, 0xFF, 0x7F, 0xFF, 0x7F    # NaN bytes of either sign
        q[1, 5], q[1, 6, 2], q[1, 255, 7], q[1, 256], q[1, 288, 1] = 0xFF, 0x7F, 0x7F, 0xFF, 0x7F
    g[4, 200:] = 0                                                         # zero feature rows
    q[3] = 0                                                               # an all-zero query: every S is 0, ties everywhere
    idx = torch.tensor([[102, -1, I32_MIN, I32_MAX, 99, 106, 102, 100, 104, 1, 2],
                        [105, 102, 102, 104, -1, -1, 103, 100, 106, 99, 0],
                        [-1, I32_MIN, I32_MAX, 99, 106, 1, 2, 3, 4, 5, -7],         # an all-padding query
                        [104, 100, 103, 105, 102, 104, -1, -1, -1, -1, -1]], dtype=torch.int32)
    assert not (idx == 101).any()
    for k in (1, 11):
        got = run(dev, kind, q, idx, g, base, k, 0.0)
        want = restate(kind, q, idx, g, base, k, 0.0)
        assert_equal_bits(got, want, ALL)
    assert np.isfinite(got["pair_score"][idx.numpy() == 102]).all()
    t = got["col_nn"][0, 0]
    assert (t[bad_cols] == -1).all() and not np.isin(got["row_nn"][0, 0], bad_cols).any()
    assert (got["row_nn"][1, 1][bad_rows] == -1).all() and not np.isin(got["col_nn"][1, 1], bad_rows).any()
    assert (got["vals"][2] == -np.inf).all() and (got["idx"][2] == -1).all() and (got["matches"][2] == 0).all()
    assert got["idx"][0].tolist().count(102) == 2                          # duplicates: scored as often as they occur
    assert got["idx"][3].tolist() == [100, 102, 103, 104, 104, 105, -1, -1, -1, -1, -1] and (got["vals"][3, :6] == 0).all()
    # a shard that owns nothing of the list, and min_sim above every similarity
    none = run(dev, kind, q, idx, g, 1000, 3, 0.0)
    assert (none["idx"] == -1).all() and (none["vals"] == -np.inf).all() and (none["pair_score"] == -np.inf).all()
    assert (none["row_nn"] == -1).all() and (none["col_nn"] == -1).all() and (none["pair_matches"] == 0).all()
    high = run(dev, kind, q, idx, g, base, 11, 1e6)
    assert (high["pair_matches"] == 0).all() and (high["matches"] == 0).all()
    assert_equal_bits(high, restate(kind, q, idx, g, base, 11, 1e6), ALL)


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_call_leaves_its_outputs_untouched(dev, kind):
    """Device pointers, every output filled with a sentinel: a call the library refuses (1370 patches on either side, a NaN
    min_sim, a width off the granule, a short workspace) returns its status and writes nothing."""
    from vpr_amd import _lib, ops
    lib = _lib.lib()
    entry = getattr(lib, "vpr_hires_local_rerank" if kind == "bf16" else "vpr_hires_patch_rerank_fp8")
    B, kc, n, l = 2, 3, 1370, 64
    es = 2 if kind == "bf16" else 1
    feats = torch.zeros(B * n * l * es, dtype=torch.uint8, device=dev)
    idx = torch.zeros((B, kc), dtype=torch.int32, device=dev)
    outs = [torch.full((B * kc * n,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(7)]
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n_q=300, n_g=300, l=l, min_sim=0.0, ws_bytes=4096):
        return entry(p(feats), n_q, p(idx), B, kc, p(feats), n_g, l, B, 0, min_sim, kc, *[p(o) for o in outs], p(ws), ws_bytes, ops._stream())

    unsupported, invalid = -2, -1
    assert lib.vpr_hires_local_workspace_bytes(B, kc) <= 4096
    for kw, status in ((dict(n_q=1370), unsupported), (dict(n_g=1370), unsupported), (dict(n_q=0), unsupported),
                       (dict(min_sim=float("nan")), invalid), (dict(min_sim=float("nan"), n_g=1370), invalid),
                       (dict(l=48), unsupported), (dict(l=32 if kind == "e4m3" else 16), unsupported), (dict(ws_bytes=16), unsupported)):
        assert call(**kw) == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A5A5A5A).all()) for o in outs) and bool((ws == 0xA5).all())
    assert call() == 0                                                     # and the same pointers with a supported shape run
    torch.cuda.synchronize()
    assert not bool((outs[0] == 0x5A5A5A5A).all())


# -------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("kind", KINDS)
def test_bit_identical_across_batch_position_padding_runs_outputs_and_graph_replay(dev, kind):
    from vpr_amd import ops
    rng = np.random.default_rng(23)
    B, kc, n_q, n_g, l, n_local, base = 5, 6, 529, 529, 64, 7, 40
    q = unit_features(dev, kind, ref.unit(rng.standard_normal((B, n_q, l))))
    g = unit_features(dev, kind, ref.unit(rng.standard_normal((n_local, n_g, l))))
    idx = candidates(rng, B, kc, n_local, base)
    full = run(dev, kind, q, idx, g, base, 4, 0.05)
    again = run(dev, kind, q, idx, g, base, 4, 0.05)
    assert_equal_bits(again, full, ALL)                                    # across runs
    plain = run(dev, kind, q, idx, g, base, 4, 0.05, debug=False)          # without the optional outputs
    assert_equal_bits(plain, full, ("vals", "idx", "matches"))
    perm = torch.from_numpy(rng.permutation(B))
    moved = run(dev, kind, q[perm], idx[perm], g, base, 4, 0.05)           # across position in the batch
    assert_equal_bits({f: moved[f][np.argsort(perm.numpy())] for f in ALL}, full, ALL)
    for b in (0, 2, 4):                                                    # across B
        one = run(dev, kind, q[b:b + 1], idx[b:b + 1], g, base, 4, 0.05)
        assert_equal_bits(one, {f: full[f][b:b + 1] for f in ALL}, ALL)
    pad = torch.cat([idx, torch.full((B, 7), -1, dtype=torch.int32)], 1)   # across trailing padding (another grid, too)
    padded = run(dev, kind, q, pad, g, base, 4, 0.05)
    assert_equal_bits(padded, full, ("vals", "idx", "matches"))
    assert_equal_bits({f: padded[f][:, :kc] for f in ("pair_score", "pair_matches", "row_nn", "col_nn")}, full,
                      ("pair_score", "pair_matches", "row_nn", "col_nn"))
    # under graph replay, with new inputs copied into the captured tensors
    call = getattr(ops, OP[kind])
    qd, id_, gd = q.to(dev), idx.to(dev), g.to(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        call(qd, id_, gd, base, 4, 0.05)                                   # warm-up: workspace, LDS opt-in
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(qd, id_, gd, base, 4, 0.05)
    for order in (perm, torch.arange(B)):
        qd.copy_(q[order])
        id_.copy_(idx[order])
        graph.replay()
        torch.cuda.synchronize()
        eager = run(dev, kind, q[order], idx[order], g, base, 4, 0.05, debug=False)
        assert_equal_bits(dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy()), eager,
                          ("vals", "idx", "matches"))


# -------------------------------------------------------------------------------------------------------------- wiring
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", KINDS)
def test_torch_op_and_sharded_merge(dev, kind):
    """torch.ops.vpr.local_rerank[_fp8]_hires is the wrapper; R hand-made shards at n = 300 scored apart and merged
    (vpr_topk_merge) give the single shard's answer."""
    from vpr_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vpr.*)
    rng = np.random.default_rng(31)
    B, kc, n, l, N = 3, 12, 300, 64, 17
    q, g = int_features(kind, rng, B, n, l), int_features(kind, rng, N, n, l)
    idx = torch.stack([torch.from_numpy(rng.permutation(N)[:kc].astype(np.int32)) for _ in range(B)])
    ms = 2.0 * (1.0 if kind == "bf16" else S1)
    want = restate(kind, q, idx, g, 0, 6, ms)
    v, i, m = getattr(torch.ops.vpr, OP[kind])(q.to(dev), idx.to(dev), g.to(dev), 0, 6, ms)
    assert_equal_bits(dict(vals=v.cpu().numpy(), idx=i.cpu().numpy(), matches=m.cpu().numpy()), want, ("vals", "idx", "matches"))
    for R in (2, 3):
        vs, is_ = [], []
        for r in range(R):
            lo, hi = N * r // R, N * (r + 1) // R
            sv, si, _ = getattr(ops, OP[kind])(q.to(dev), idx.to(dev), g[lo:hi].contiguous().to(dev), lo, 6, ms)
            vs.append(sv)
            is_.append(si)
        mv, mi = ops.topk_merge(torch.stack(vs), torch.stack(is_))
        assert np.array_equal(mi.cpu().numpy(), want["idx"]) and np.array_equal(mv.cpu().numpy(), want["vals"])


@pytest.fixture(scope="module")
def rccl_one_rank(dev):
    import os
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dev
    dist.destroy_process_group()


def place_gallery(dev, seed, kind="bf16", N=96, D=128, B=4, n=300, l=64, **kw):
    """ref.places as a ShardedGallery(local_hires=True) with local features of `kind`; returns (gallery, queries, their bf16 local
    features, true rows)."""
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    rows, local, q, ql, true = ref.places(seed, N, D, B, n, l)
    local = local.to(dev)
    if kind == "e4m3":
        local = ops.quantize_patch_fp8(local)
    return ShardedGallery(rows.to(dev), N, local_feats=local, local_hires=True, **kw), q.to(dev), ql.to(dev), true


@pytest.mark.parametrize("kind", KINDS)
def test_search_local_reranked_at_300_patches(dev, kind):
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    sg, q, ql, true = place_gallery(dev, 2, kind)
    k, kc = 4, 16
    v, i = sg.search_local_reranked(q, k, kc, ql, 0.3)
    _, ci = sg.search(q, kc)
    ql_kind = ql if kind == "bf16" else ops.quantize_patch_fp8(ql)
    want = restate(kind, ql_kind.cpu(), ci.cpu(), sg.local_feats.cpu(), 0, k, 0.3)
    assert np.array_equal(i[:, 0].cpu().numpy(), true) and np.array_equal(i.cpu().numpy()[:, 0], want["idx"][:, 0])
    if kind == "bf16":                                                     # the e4m3 MFMA's slack may swap near-equal tails
        assert np.array_equal(i.cpu().numpy(), want["idx"])
        assert np.abs(v.cpu().numpy() - want["vals"]).max() <= 300 * 64 * ref.U * 2 + 300 * ref.gamma(refh.sum_roundings(300)) * 1.01
    assert not np.array_equal(ci[:, 0].cpu().numpy(), true)
    for a, b in zip(sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=0.3), (v, i)):
        assert torch.equal(bits(a), bits(b))
    closed = ShardedGallery(sg.rows, sg.n_total, local_feats=sg.local_feats)      # without the opt-in: refused as always
    with pytest.raises(ValueError, match="at most 256 patches"):
        closed.search_local_reranked(q, k, kc, ql, 0.3)


def test_one_rank_collective_path_equals_local_path(rccl_one_rank):
    dev = rccl_one_rank
    local, q, ql, _ = place_gallery(dev, 4)
    coll, _, _, _ = place_gallery(dev, 4, force_collectives=True)
    assert coll.collective and not local.collective
    for a, b in zip(local.search_local_reranked(q, 5, 16, ql, 0.2), coll.search_local_reranked(q, 5, 16, ql, 0.2)):
        assert torch.equal(bits(a), bits(b))
    kw = dict(local_rerank=16, q_local_feats=ql, min_sim=0.2)
    for a, b in zip(local.search_local_queries(q, 5, **kw), coll.search_local_queries(q, 5, **kw)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_local_rerank_at_529_patches_equals_eager(rccl_one_rank, kind):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    B, k, kc = 4, 5, 16
    sg, q0, ql0, _ = place_gallery(dev, 6, kind, n=529, l=64)
    gr = GraphedRetrieval(sg, B, k, local_rerank=kc, min_sim=0.2)
    assert gr.q_feats.shape == (B, 529, 64) and gr.q_feats.dtype == (torch.bfloat16 if kind == "bf16" else torch.uint8)
    _, q1, ql1, _ = place_gallery(dev, 7, kind, n=529, l=64)
    for seed, (q, ql) in enumerate(((q0, ql0), (q0.roll(3, 0).contiguous(), ql0.roll(3, 0).contiguous()), (q1, ql1))):
        v_g, i_g = gr(q, ql)
        v_g, i_g = v_g.clone(), i_g.clone()
        v_e, i_e = sg.search_local_reranked(q, k, kc, ql, 0.2)
        assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e)), seed
    gr.close()


LOCAL_FEATURES_GATE = 2 * 0.001306      # tests/test_local_match_gpu.py: the same arithmetic per patch, so its measured gate applies


def test_features_want_local_hires_at_vit_small_322(dev):
    from vpr_amd.modules import DinoV2Salad
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small", img_size=322).to(dev).to(torch.bfloat16).eval()
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    ext.aggregator.pack()
    x = torch.randn(2, 3, 322, 322, device=dev).to(torch.bfloat16)
    d, d16 = ext.features(x, want_bf16=True)
    d, d16 = d.clone(), d16.clone()
    e, e16, local = ext.features(x, want_bf16=True, want_local=True, hires=True)
    assert torch.equal(bits(d), bits(e)) and torch.equal(d16.view(torch.int16), e16.view(torch.int16))
    f, local8 = ext.features(x, want_local="fp8", hires=True)
    assert torch.equal(bits(f), bits(d))
    assert local.shape == (2, 529, 128) and local.dtype == torch.bfloat16 and local8.shape == (2, 529, 128) and local8.dtype == torch.uint8
    tokens = ext.backbone(x, split=True).patch
    assert tokens.dtype == torch.bfloat16 and tokens.shape == (2, 529, 384)
    assert torch.equal(ext.aggregator.local_features(tokens, hires=True).view(torch.int16), local.view(torch.int16))
    assert torch.equal(ext.aggregator.local_features(tokens, fp8=True, hires=True), local8)
    # at 256 tokens and below the keyword changes nothing
    assert torch.equal(ext.aggregator.local_features(tokens[:, :256].contiguous(), hires=True).view(torch.int16),
                       ext.aggregator.local_features(tokens[:, :256].contiguous()).view(torch.int16))
    c = ext.aggregator.cluster_features
    w = lambda conv: conv.weight.detach().reshape(conv.weight.shape[0], -1).to(torch.bfloat16).float()
    with torch.no_grad():
        h = torch.relu(tokens.float().reshape(-1, 384) @ w(c[0]).T + c[0].bias.float())
        o = h @ w(c[3]).T + c[3].bias.float()
        want = (o / o.norm(dim=1, keepdim=True)).view(2, 529, 128)
    diff = float((local.float() - want).abs().max())
    print(f"features(want_local=True, hires=True) at 322 px vs the f32 MLP, largest element difference: {diff:.6f}")
    assert torch.allclose(local.float().norm(dim=2), torch.ones(2, 529, device=dev), atol=4e-3)
    assert diff <= LOCAL_FEATURES_GATE
    dec = torch.from_numpy(ref8.decode(local8.cpu())).float()
    assert float((dec - want.cpu()).abs().max()) <= LOCAL_FEATURES_GATE + 2.0 ** -5      # + half an e4m3 step at 1: 2^-4 / 2
    with pytest.raises(ValueError, match="at most 256"):
        ext.features(x, want_local=True)                                   # without the opt-in: refused as always


def test_retrieval_scores_with_local_rerank_at_322_px(dev, tmp_path, monkeypatch):
    """The pattern of tests/test_local_match_gpu.py::test_retrieval_scores_with_local_rerank at image_size 322 (529 patches):
    generated images, a gallery kept with its local features under local_hires; the result is retrieval_metrics, by hand, of
    search_local_reranked on the same descriptor and local-feature batches."""
    import os
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, gallery as G, modules
    from vpr_amd.retrieval import ShardedGallery
    rng = np.random.default_rng(21)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g, px = 12, 322
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
    train = (ext, str(tmp_path / "labels_train.csv"), str(gdir))
    with pytest.raises(ValueError, match="at most 256"):
        evaluate.build_gallery_from_images(*train, str(tmp_path / "closed"), batch_size=4, keep_local=True, graph=False, image_size=px)
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "gal"), batch_size=4, keep_local=True, local_hires=True,
                                              graph=False, image_size=px) == n_g
    assert os.path.exists(tmp_path / "gal" / G.LOCAL_FILE)
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None, **kw):
        seen.append((q_local.clone(), k, expand, {n: (v.clone() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}))
        return plain_search(self, q_local, k, expand, **kw)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run_ = lambda **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "labels_val.csv"), str(vdir), k=5,
                                                            tau=10.0, batch_size=4, verbose=False, graph=False, image_size=px, **kw)
    res = run_()
    assert all(kw == {} for *_, kw in seen) and res["topk_indices"][:, 0].tolist() == src
    with pytest.raises(ValueError, match="at most 256"):
        run_(local_rerank=8)                                               # without the opt-in: refused as always
    del seen[:]
    got = run_(local_rerank=8, min_sim=0.5, local_hires=True)
    assert all(set(kw) == {"local_rerank", "q_local_feats", "min_sim"} and kw["local_rerank"] == 8 and kw["min_sim"] == 0.5 for *_, kw in seen)
    assert all(kw["q_local_feats"].shape[1:] == (529, 128) for *_, kw in seen)
    shard = G.load_gallery_shard(str(tmp_path / "gal"), dev, load_local=True)
    assert shard.local.shape == (n_g, 529, 128) and shard.local.dtype == torch.bfloat16
    sg = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True, local_feats=shard.local, local_hires=True)
    batches = [sg.search_local_reranked(d16, k, 8, kw["q_local_feats"], 0.5) for d16, k, _, kw in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    top = idx.cpu().numpy()
    assert top[:, 0].tolist() == src and got["topk_indices"].tobytes() == top.tobytes()
    assert got["topk_scores"].tobytes() == vals.cpu().numpy().tobytes() and got["topk_scores"].tobytes() != res["topk_scores"].tobytes()
    assert (got["topk_scores"][:, 0] > 264).all()            # local scores: most of the 529 patches match at similarity ~1
    # the metrics by hand: top-1 label transfer, recalls from the lists
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
