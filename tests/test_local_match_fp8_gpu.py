"""GPU: the e4m3 form of local-feature re-ranking (include/vpr_amd_patch_fp8.h) against its restatement
(tests/local_match_fp8_ref.py): the quantiser byte for byte; the lane-to-K pairing of the block-scaled MFMA on one-hot
features; bit for bit on integer features and against the bf16 form on the same integers; as epsilon-argmaxes on Gaussian unit
features through the device quantiser; the edges of the contract with NaN bytes; bit-identity across batch, position, padding,
runs, optional outputs and graph replay; the recipe; and the wiring through the modules, the sharded and graphed searches and the
evaluation."""
import ctypes

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_ref as ref

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ALL = ("row_nn", "col_nn", "pair_matches", "pair_score", "vals", "idx", "matches")
S1 = 2.0 ** -16         # the similarity of two bytes of value 1


def run(dev, q, idx, g, base=0, k=None, min_sim=0.0, debug=True, op="local_rerank_fp8"):
    from vpr_amd import ops
    out = getattr(ops, op)(q.to(dev), idx.to(dev), g.to(dev), base, k, min_sim, debug=debug)
    torch.cuda.synchronize()
    res = dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy())
    if debug:
        res.update({f: getattr(out[3], f).cpu().numpy() for f in out[3]._fields})
    return res


def int_values(rng, *shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


def int_bytes(v):
    return torch.from_numpy(ref8.encode_ints(v))


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


# ------------------------------------------------------------------------------------------------------ the quantiser
def test_quantiser_every_bf16_pattern_and_the_f32_edges(dev):
    from vpr_amd import ops
    bits = torch.arange(65536, dtype=torch.int32).to(torch.uint16).view(torch.bfloat16)      # one launch
    got = ops.quantize_patch_fp8(bits.to(dev)).cpu().numpy()
    want = ref8.quantize(bits)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    edges = ref8.f32_edges()
    got = ops.quantize_patch_fp8(torch.from_numpy(edges).to(dev)).cpu().numpy()
    want = ref8.quantize(edges)
    assert np.array_equal(got, want), [(float(e), hex(g), hex(w)) for e, g, w in zip(edges, got, want) if g != w][:8]
    # the same values as bf16 where bf16 holds them: a bf16 input is exact in f32
    as_bf = torch.from_numpy(edges).to(torch.bfloat16)
    assert np.array_equal(ops.quantize_patch_fp8(as_bf.to(dev)).cpu().numpy(), ref8.quantize(as_bf))
    x = torch.from_numpy(edges[:60]).view(3, 4, 5)
    assert ops.quantize_patch_fp8(x.to(dev)).shape == (3, 4, 5) and ops.quantize_patch_fp8(torch.empty(0, 7, device=dev)).shape == (0, 7)


@pytest.mark.parametrize("bf16", [False, True])
def test_quantiser_counts_positions_and_alignment(dev, bf16):
    """Counts around the 16-element vector group and a count with a tail after many groups; the same values at every offset of
    the input and of the output (both the vector path, when the two offsets agree modulo 16 bytes, and the scalar one): a byte
    depends on its value only, and nothing outside [0, count) of the output is written."""
    from vpr_amd import ops
    rng = np.random.default_rng(3)
    pool = np.concatenate([ref8.f32_edges(), rng.standard_normal(5000).astype(np.float32) * 0.3])
    src = torch.from_numpy(rng.choice(pool, 4099 + 64).astype(np.float32))
    if bf16:
        src = src.to(torch.bfloat16)
    want = ref8.quantize(src)
    es = src.element_size()
    x = src.to(dev)
    for count in (1, 15, 16, 17, 4099):
        assert np.array_equal(ops.quantize_patch_fp8(x[:count].contiguous()).cpu().numpy(), want[:count]), count
    out = torch.empty(4099 + 64 + 32, dtype=torch.uint8, device=dev)
    # (count, offset of x in elements, offset of out in bytes): the vector path needs x + head 16-byte aligned where out + head is
    for count, xoff, ooff in ((4099, 0, 0), (4099, 1, 0), (4099, 4, 16), (4099, 3, 15), (4099, 7, 15), (4099, 5, 7), (4099, 8, 0),
                              (17, 5, 7), (16, 8, 16), (15, 2, 1), (1, 63, 31), (33, 3, 13), (40, 15, 15)):
        out.fill_(0xA5)
        ops._call("vpr_patch_quantize_fp8", ctypes.c_void_p(x.data_ptr() + xoff * es), int(bf16), count,
                  ctypes.c_void_p(out.data_ptr() + ooff), ops._stream())
        got = out.cpu().numpy()
        assert np.array_equal(got[ooff:ooff + count], want[xoff:xoff + count]), (count, xoff, ooff)
        assert (got[:ooff] == 0xA5).all() and (got[ooff + count:] == 0xA5).all(), (count, xoff, ooff)


# ------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("l", [64, 128, 192, 256])
def test_one_hot_features_pair_the_same_k_on_both_operands(dev, l):
    """Query row d holds one nonzero byte at position d, candidate row d' one at d' (n = l): S must be diagonal, with the
    candidate's value on it.  A lane-to-K assignment that differs between the A and the B operand of the block-scaled MFMA
    moves the nonzeros off the diagonal or drops them."""
    vals = np.array([1, 2, -1.5, 0.5], dtype=np.float32)[np.arange(l) % 4]         # the candidate's byte at d' (asymmetric)
    q = np.zeros((1, l, l), dtype=np.float32)
    g = np.zeros((2, l, l), dtype=np.float32)
    q[0, np.arange(l), np.arange(l)] = 1
    g[1, np.arange(l), np.arange(l)] = vals
    idx = torch.tensor([[1]], dtype=torch.int32)
    got = run(dev, int_bytes(q), idx, int_bytes(g), 0, None, -1.0)
    # a row whose diagonal entry is negative has its argmax at the first zero instead: column 0 (1 for row 0 is positive)
    want = ref8.local_rerank_fp8(int_bytes(q), idx, int_bytes(g), 0, None, -1.0)
    assert_equal_bits(got, want, ALL)
    pos = vals > 0
    assert np.array_equal(got["row_nn"][0, 0][pos], np.arange(l)[pos]) and np.array_equal(got["col_nn"][0, 0][pos], np.arange(l)[pos])
    assert got["pair_matches"][0, 0] >= pos.sum() and got["pair_score"][0, 0] > 0
    # and the transposed roles: the nonzero values on the query side
    got = run(dev, int_bytes(g[1:]), torch.tensor([[0]], dtype=torch.int32), int_bytes(q), 0, None, -1.0)
    want = ref8.local_rerank_fp8(int_bytes(g[1:]), torch.tensor([[0]], dtype=torch.int32), int_bytes(q), 0, None, -1.0)
    assert_equal_bits(got, want, ALL)
    assert np.array_equal(got["row_nn"][0, 0][pos], np.arange(l)[pos])


# (B, kc, k_out, n_q, n_g, l): every n in {1, 31, 32, 33, 64, 65, 196, 255, 256} on both sides with n_q != n_g included, every l,
# every B, every kc, k_out in {1, kc}; the large B x kc products ride on small images, the large images on small lists
SHAPES = [(1, 1, 1, 1, 1, 64), (3, 7, 1, 31, 33, 64), (3, 8, 8, 32, 32, 128), (3, 9, 9, 33, 31, 64), (1, 7, 7, 64, 65, 128),
          (1, 8, 1, 65, 64, 256), (3, 9, 9, 196, 196, 128), (1, 7, 7, 255, 256, 256), (1, 8, 8, 256, 255, 192), (1, 9, 1, 256, 256, 256),
          (37, 64, 64, 31, 32, 64), (37, 128, 128, 1, 33, 64), (3, 128, 1, 33, 1, 128), (1, 64, 64, 196, 255, 64), (3, 1, 1, 256, 196, 192),
          (1, 9, 9, 64, 256, 192)]


@pytest.mark.parametrize("B,kc,k,n_q,n_g,l", SHAPES)
def test_integer_features_bit_for_bit(dev, B, kc, k, n_q, n_g, l):
    """Byte values in -2 .. 2: the accumulator is an integer of magnitude <= 4 l <= 1024, S = 2^-16 of it and a score
    (<= 256 * 1024 * 2^-16) are exact in f32 whatever the order of the sums."""
    rng = np.random.default_rng(B * 1000 + kc * 7 + n_q + n_g + l)
    n_local, base = 11, 5
    q, g = int_bytes(int_values(rng, B, n_q, l)), int_bytes(int_values(rng, n_local, n_g, l))
    idx = candidates(rng, B, kc, n_local, base)
    for min_sim in (0.0, 3.0 * S1):
        got = run(dev, q, idx, g, base, k, min_sim)
        want = ref8.local_rerank_fp8(q, idx, g, base, k, min_sim)
        assert_equal_bits(got, want, ALL)
    assert (want["pair_matches"] > 0).any() or n_q * n_g == 1


@pytest.mark.parametrize("B,kc,n_q,n_g,l", [(3, 9, 65, 33, 64), (2, 8, 256, 196, 128), (1, 7, 31, 255, 192), (2, 5, 196, 256, 256)])
def test_the_bf16_form_on_the_same_integers_gives_the_same_bits(dev, B, kc, n_q, n_g, l):
    """The shared epilogue: on the same integer values the e4m3 op's outputs are the bf16 op's, bit for bit, once the bf16
    scores are multiplied by 2^-16 (exact) and min_sim is scaled likewise."""
    rng = np.random.default_rng(n_q + n_g + l)
    n_local, base = 9, 3
    qv, gv = int_values(rng, B, n_q, l), int_values(rng, n_local, n_g, l)
    idx = candidates(rng, B, kc, n_local, base)
    for m in (0.0, 2.0):
        a = run(dev, int_bytes(qv), idx, int_bytes(gv), base, None, m * S1)
        b = run(dev, torch.from_numpy(qv).to(torch.bfloat16), idx, torch.from_numpy(gv).to(torch.bfloat16), base, None, m, op="local_rerank")
        for f in ("vals", "pair_score"):
            b[f] = (b[f] * np.float32(S1)).astype(np.float32)             # -inf stays -inf
        assert_equal_bits(a, b, ALL)


GAUSS = [(2, 5, 256, 256, 128), (3, 4, 196, 255, 64), (2, 3, 33, 65, 256), (2, 8, 64, 31, 192)]


@pytest.mark.parametrize("B,kc,n_q,n_g,l", GAUSS)
def test_gaussian_unit_features_are_epsilon_argmaxes(dev, B, kc, n_q, n_g, l):
    """Unit features through the device quantiser (checked against the restatement on the way).
    The bf16 test's bounds, for f32 accumulation of exact products — e[i][j] = l 2^-24 sum_d |a b| on the decoded bytes, the score
    within sum_matched e + gamma_10 sum_matched |S| — do NOT hold for the block-scaled MFMA: measured on an MI355X the score
    error reaches 1.065 of that bound at (256, 256, 128) and 2.13 of it at (196, 255, 64), on the image that shares the query's
    patches (all products of a matched pair positive, every loss to the same side).  The power-of-two probes of
    scripts/mfma_e4m3_probe.py (profiles/mfma_e4m3_probe.txt) show why: inside a step the products are aligned in groups of 8
    consecutive k to the group's largest product and cut, towards zero, 13 bits below it; beside a product 2^16 in its group a
    product 2^2 vanishes, in any other group or step it arrives down to 2^-11.  The bound that follows
    (local_match_fp8_ref.mfma_truncation) adds t[i][j] = 7 * 2^-13 * sum_groups max_k |a b| to e: every device choice must be an
    (e + t)-argmax, no row or column left out; given the device's own neighbours the match count is integer logic; the score is
    within sum_matched (e + t) + gamma_10 sum_matched |S| of the f64 sum.  Both shares are printed."""
    from vpr_amd import ops
    rng = np.random.default_rng(n_q + n_g + l)
    n_local = 7
    qf = torch.from_numpy(ref.unit(rng.standard_normal((B, n_q, l))).astype(np.float32))
    gf = torch.from_numpy(ref.unit(rng.standard_normal((n_local, n_g, l))).astype(np.float32))
    q, g = ops.quantize_patch_fp8(qf.to(dev)).cpu(), ops.quantize_patch_fp8(gf.to(dev)).cpu()
    assert np.array_equal(q.numpy(), ref8.quantize(qf)) and np.array_equal(g.numpy(), ref8.quantize(gf))
    g[3, : min(n_g, n_q)] = q[0, : min(n_g, n_q)]                          # one image shares the first query's patches
    idx = torch.from_numpy(rng.integers(0, n_local, (B, kc)).astype(np.int32))
    idx[0, 0] = 3
    q64, g64, cand = ref8.decode(q), ref8.decode(g), idx.numpy()
    worst_arg, worst, worst_f32 = 0.0, 0.0, 0.0
    slack = {}                                                             # e + t of a pair: the same for both min_sim
    for min_sim in (0.0, 0.25):
        got = run(dev, q, idx, g, 0, None, min_sim)
        for b in range(B):
            for t in range(kc):
                S = q64[b] @ g64[cand[b, t]].T
                if (b, cand[b, t]) not in slack:
                    slack[b, cand[b, t]] = (l * ref.U * (np.abs(q64[b]) @ np.abs(g64[cand[b, t]]).T),
                                            ref8.mfma_truncation(q64[b], g64[cand[b, t]]))
                e32, trunc = slack[b, cand[b, t]]
                e = e32 + trunc
                r, c = got["row_nn"][b, t], got["col_nn"][b, t]
                assert (r >= 0).all() and (r < n_g).all() and (c >= 0).all() and (c < n_q).all()
                i, j = np.arange(n_q), np.arange(n_g)
                assert (S[i, r] + e[i, r] >= (S - e).max(1)).all()
                assert (S[c, j] + e[c, j] >= (S - e).max(0)).all()
                worst_arg = max(worst_arg, float(((S.max(1) - S[i, r]) / (e[i, r] + e[i, S.argmax(1)])).max()),
                                float(((S.max(0) - S[c, j]) / (e[c, j] + e[S.argmax(0), j])).max()))
                mutual = r[c] == j
                # a mutual pair within its own slack of min_sim may fall either way on the device: it is counted and summed as
                # undecided (the slack of the e4m3 MFMA is wide enough to meet such pairs among a few thousand)
                ms = float(np.float32(min_sim))
                und = mutual & (np.abs(S[c, j] - ms) <= e[c, j])
                m = mutual & (S[c, j] > ms + e[c, j])
                assert m.sum() <= got["pair_matches"][b, t] <= m.sum() + und.sum()
                exact = S[c, j][m].sum()
                bound = e[c, j][m | und].sum() + ref.gamma(ref.SUM_ROUNDINGS) * np.abs(S[c, j][m | und]).sum()
                score = float(got["pair_score"][b, t])
                assert exact + S[c, j][und].clip(None, 0).sum() - bound <= score <= exact + S[c, j][und].clip(0).sum() + bound, \
                    (b, t, score, exact, bound, und.sum())
                if bound > 0 and not und.any():
                    err = abs(score - exact)
                    worst = max(worst, err / bound)
                    worst_f32 = max(worst_f32, err / (e32[c, j][m].sum() + ref.gamma(ref.SUM_ROUNDINGS) * np.abs(S[c, j][m]).sum()))
        if min_sim == 0.25:
            assert got["pair_matches"][0, 0] >= min(n_q, n_g) and got["idx"][0, 0] == 3
    print(f"local_rerank_fp8 at ({n_q}, {n_g}, {l}): largest share of the argmax slack {worst_arg:.4f}, of the score bound {worst:.4f}, "
          f"of the score bound for exact products in f32 {worst_f32:.4f}")


@pytest.mark.parametrize("n,l", [(64, 64), (256, 128)])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recipe_true_image_comes_back_first(dev, seed, n, l):
    from vpr_amd import ops
    q, gal = ref.recipe(seed, n, l)
    q8, gal8 = ops.quantize_patch_fp8(q.to(dev)).cpu(), ops.quantize_patch_fp8(gal.to(dev)).cpu()
    assert np.array_equal(gal8.numpy(), ref8.quantize(gal))
    N = gal.shape[0]
    idx = torch.arange(N, dtype=torch.int32)[None]                         # the true image at the last position of the list
    got = run(dev, q8, idx, gal8, 0, None, 0.0)
    assert got["idx"][0, 0] == N - 1 and got["matches"][0, 0] == n and 0.99 * n <= got["vals"][0, 0] <= 1.004 * n
    most = n / 2 + 3 * np.sqrt(n)
    assert got["pair_matches"][0, :N - 1].max() <= most
    assert got["pair_score"][0, :N - 1].max() <= most * np.sqrt(2 * np.log(20 * n * n) / l) < 0.99 * n
    if l == 128:
        hard = run(dev, q8, idx, gal8, 0, None, 0.6)
        assert (hard["pair_score"][0, :N - 1] == 0).all() and (hard["pair_matches"][0, :N - 1] == 0).all()
        assert hard["idx"][0, 0] == N - 1 and hard["matches"][0, 0] == n
        assert hard["idx"][0, 1:].tolist() == list(range(N - 1))           # all-zero scores: by ascending index


def test_edges(dev):
    from vpr_amd import _lib, ops
    rng = np.random.default_rng(17)
    n_q, n_g, l, base, n_local = 40, 37, 64, 100, 6
    q, g = int_bytes(int_values(rng, 4, n_q, l)), int_bytes(int_values(rng, n_local, n_g, l))
    g[1] = 0x7F                                                            # never named by a live index: never read
    g[2, 3], g[2, 9, 5], g[2, 11, 0], g[2, 12, 63] = 0x7F, 0xFF, 0x7F, 0xFF  # a live image with NaN bytes (either sign) in some rows
    g[4, 20:] = 0                                                          # zero feature rows
    q[1, 5], q[1, 6, 2] = 0xFF, 0x7F                                       # and a query with such rows
    q[3] = 0                                                               # an all-zero query: every S is 0, ties everywhere
    idx = torch.tensor([[102, -1, I32_MIN, I32_MAX, 99, 106, 102, 100, 104, 1, 2],
                        [105, 102, 102, 104, -1, -1, 103, 100, 106, 99, 0],
                        [-1, I32_MIN, I32_MAX, 99, 106, 1, 2, 3, 4, 5, -7],         # an all-padding query
                        [104, 100, 103, 105, 102, 104, -1, -1, -1, -1, -1]], dtype=torch.int32)
    assert not (idx == 101).any()
    for k in (1, 11):
        got = run(dev, q, idx, g, base, k, 0.0)
        want = ref8.local_rerank_fp8(q, idx, g, base, k, 0.0)
        assert_equal_bits(got, want, ALL)
    assert np.isfinite(got["pair_score"][idx.numpy() == 102]).all()
    t = got["col_nn"][0, 0]
    assert t[3] == -1 and t[9] == -1 and t[11] == -1 and t[12] == -1 and not (got["row_nn"][0, 0][:, None] == [3, 9, 11, 12]).any()
    assert (got["row_nn"][1, 1][[5, 6]] == -1).all()
    assert (got["vals"][2] == -np.inf).all() and (got["idx"][2] == -1).all() and (got["matches"][2] == 0).all()
    assert got["idx"][0].tolist().count(102) == 2                          # duplicates: scored as often as they occur
    assert got["idx"][3].tolist() == [100, 102, 103, 104, 104, 105, -1, -1, -1, -1, -1] and (got["vals"][3, :6] == 0).all()
    # a shard that owns nothing of the list, and min_sim above every similarity
    none = run(dev, q, idx, g, 1000, 3, 0.0)
    assert (none["idx"] == -1).all() and (none["vals"] == -np.inf).all() and (none["pair_score"] == -np.inf).all()
    high = run(dev, q, idx, g, base, 11, 1e6)
    assert (high["pair_matches"] == 0).all() and (high["matches"] == 0).all()
    assert_equal_bits(high, ref8.local_rerank_fp8(q, idx, g, base, 11, 1e6), ALL)
    # a refused call (a width the e4m3 form does not take; k_out beyond kc) leaves every output as it was
    qd, id_, gd = q.to(dev), idx.to(dev), g.to(dev)
    outs = [torch.full((4 * 11 * 40,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(7)]
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for l_arg, k_arg, status in ((32, 3, -2), (96, 3, -2), (64, 12, -1), (64, 0, -1)):
        st = _lib.lib().vpr_patch_rerank_fp8(ptr(qd), n_q, ptr(id_), 4, 11, ptr(gd), n_g, l_arg, n_local, base, 0.0, k_arg,
                                             *[ptr(o) for o in outs], ptr(ws), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        assert st == status and all((o == 0x5A5A5A5A).all() for o in outs) and (ws == 0x5A).all(), (l_arg, k_arg)


def test_bit_identical_across_batch_position_padding_runs_and_outputs(dev):
    from vpr_amd import ops
    rng = np.random.default_rng(23)
    B, kc, n_q, n_g, l, n_local, base = 9, 10, 70, 67, 192, 13, 40
    q = ref8.quantize_t(torch.from_numpy(ref.unit(rng.standard_normal((B, n_q, l))).astype(np.float32)))
    g = ref8.quantize_t(torch.from_numpy(ref.unit(rng.standard_normal((n_local, n_g, l))).astype(np.float32)))
    idx = candidates(rng, B, kc, n_local, base)
    full = run(dev, q, idx, g, base, 4, 0.05)
    again = run(dev, q, idx, g, base, 4, 0.05)
    assert_equal_bits(again, full, ALL)                                    # across runs
    plain = run(dev, q, idx, g, base, 4, 0.05, debug=False)                # without the optional outputs
    assert_equal_bits(plain, full, ("vals", "idx", "matches"))
    perm = torch.from_numpy(rng.permutation(B))
    moved = run(dev, q[perm], idx[perm], g, base, 4, 0.05)                 # across position in the batch
    assert_equal_bits({f: moved[f][np.argsort(perm.numpy())] for f in ALL}, full, ALL)
    for b in (0, 4, 8):                                                    # across B
        one = run(dev, q[b:b + 1], idx[b:b + 1], g, base, 4, 0.05)
        assert_equal_bits(one, {f: full[f][b:b + 1] for f in ALL}, ALL)
    pad = torch.cat([idx, torch.full((B, 7), -1, dtype=torch.int32)], 1)   # across trailing padding (another grid, too)
    padded = run(dev, q, pad, g, base, 4, 0.05)
    assert_equal_bits(padded, full, ("vals", "idx", "matches"))
    assert_equal_bits({f: padded[f][:, :kc] for f in ("pair_score", "pair_matches", "row_nn", "col_nn")}, full,
                      ("pair_score", "pair_matches", "row_nn", "col_nn"))
    # under graph replay, with new inputs copied into the captured tensors
    qd, id_, gd = q.to(dev), idx.to(dev), g.to(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.local_rerank_fp8(qd, id_, gd, base, 4, 0.05)                   # warm-up: workspace, LDS opt-in
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.local_rerank_fp8(qd, id_, gd, base, 4, 0.05)
    for order in (perm, torch.arange(B)):
        qd.copy_(q[order])
        id_.copy_(idx[order])
        graph.replay()
        torch.cuda.synchronize()
        eager = run(dev, q[order], idx[order], g, base, 4, 0.05, debug=False)
        assert_equal_bits(dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy()), eager,
                          ("vals", "idx", "matches"))


def test_torch_ops_and_sharded_merge(dev):
    """torch.ops.vpr.local_rerank_fp8 / patch_quantize_fp8 are the wrappers; R hand-made shards scored apart and merged
    (vpr_topk_merge) give the single shard's answer."""
    from vpr_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vpr.*)
    rng = np.random.default_rng(31)
    B, kc, n, l, N = 5, 12, 50, 64, 23
    qv, gv = int_values(rng, B, n, l) * np.float32(2.0 ** -8), int_values(rng, N, n, l) * np.float32(2.0 ** -8)
    q, g = torch.ops.vpr.patch_quantize_fp8(torch.from_numpy(qv).to(dev)), torch.ops.vpr.patch_quantize_fp8(torch.from_numpy(gv).to(dev))
    assert np.array_equal(q.cpu().numpy(), ref8.quantize(qv)) and q.dtype == torch.uint8
    idx = torch.stack([torch.from_numpy(rng.permutation(N)[:kc].astype(np.int32)) for _ in range(B)])
    want = ref8.local_rerank_fp8(q.cpu(), idx, g.cpu(), 0, 6, 2.0 * S1)
    v, i, m = torch.ops.vpr.local_rerank_fp8(q, idx.to(dev), g, 0, 6, 2.0 * S1)
    assert_equal_bits(dict(vals=v.cpu().numpy(), idx=i.cpu().numpy(), matches=m.cpu().numpy()), want, ("vals", "idx", "matches"))
    for R in (2, 3):
        vs, is_ = [], []
        for r in range(R):
            lo, hi = N * r // R, N * (r + 1) // R
            sv, si, _ = ops.local_rerank_fp8(q, idx.to(dev), g[lo:hi].contiguous(), lo, 6, 2.0 * S1)
            vs.append(sv)
            is_.append(si)
        mv, mi = ops.topk_merge(torch.stack(vs), torch.stack(is_))
        assert np.array_equal(mi.cpu().numpy(), want["idx"]) and np.array_equal(mv.cpu().numpy(), want["vals"])


# -------------------------------------------------------------------------------------------------- integration
def bits(t):
    return t.contiguous().view(torch.int32)


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


def place_gallery(dev, seed, N=512, D=128, B=8, n=20, l=64, **kw):
    """ref.places as a bf16 ShardedGallery whose local features are the e4m3 store; returns (gallery, queries, their local
    features bf16, the same as bytes, true rows)."""
    from vpr_amd.retrieval import ShardedGallery
    rows, local, q, ql, true = ref.places(seed, N, D, B, n, l)
    sg = ShardedGallery(rows.to(dev), N, local_feats=ref8.quantize_t(local).to(dev), **kw)
    return sg, q.to(dev), ql.to(dev), ref8.quantize_t(ql).to(dev), true


def test_search_local_reranked_on_an_e4m3_gallery(dev):
    sg, q, ql, ql8, true = place_gallery(dev, 2)
    assert sg.local_feats.dtype == torch.uint8
    k, kc = 4, 16
    v, i = sg.search_local_reranked(q, k, kc, ql, 0.3)                      # bf16 features: quantised at entry
    _, ci = sg.search(q, kc)
    want = ref8.local_rerank_fp8(ql8.cpu(), ci.cpu(), sg.local_feats.cpu(), 0, k, 0.3)
    assert np.array_equal(i.cpu().numpy(), want["idx"]) and np.array_equal(i[:, 0].cpu().numpy(), true)
    # 20 matched pairs of unit features: sum |a b| <= 1.01 bounds both the f32 term and the MFMA's truncation term of each S
    assert np.abs(v.cpu().numpy() - want["vals"]).max() <= 20 * 1.01 * (64 * ref.U + 7 * ref8.MFMA_WINDOW + ref.gamma(ref.SUM_ROUNDINGS))
    assert not np.array_equal(ci[:, 0].cpu().numpy(), true)
    for feats in (ql, ql8):                                                # uint8 features: the same bits
        for a, b in zip(sg.search_local_reranked(q, k, kc, feats, 0.3), (v, i)):
            assert torch.equal(bits(a), bits(b))
        for a, b in zip(sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=feats, min_sim=0.3), (v, i)):
            assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="local_rerank and rerank"):
        sg.search_local_queries(q, k, rerank=kc, local_rerank=kc, q_local_feats=ql)


def test_one_rank_collective_path_equals_local_path(rccl_one_rank):
    dev = rccl_one_rank
    local, q, ql, ql8, _ = place_gallery(dev, 4)
    coll, *_ = place_gallery(dev, 4, force_collectives=True)
    assert coll.collective and not local.collective
    for feats in (ql, ql8):
        for a, b in zip(local.search_local_reranked(q, 5, 16, feats, 0.2), coll.search_local_reranked(q, 5, 16, feats, 0.2)):
            assert torch.equal(bits(a), bits(b))
        kw = dict(local_rerank=16, q_local_feats=feats, min_sim=0.2)
        for a, b in zip(local.search_local_queries(q, 5, **kw), coll.search_local_queries(q, 5, **kw)):
            assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("collective", [False, True])
def test_graphed_local_rerank_equals_eager(rccl_one_rank, collective):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    B, k, kc = 8, 5, 16
    sg, q0, ql0, ql80, _ = place_gallery(dev, 6, force_collectives=collective)
    gr = GraphedRetrieval(sg, B, k, local_rerank=kc, min_sim=0.2)
    assert gr.q_feats.shape == ql0.shape and gr.q_feats.dtype == torch.uint8
    _, q1, ql1, ql81, _ = place_gallery(dev, 7)
    for seed, (q, ql, ql8) in enumerate(((q0, ql0, ql80), (q0.roll(3, 0).contiguous(), ql0.roll(3, 0).contiguous(), ql80.roll(3, 0).contiguous()),
                                         (q1, ql1, ql81))):
        v_e, i_e = sg.search_local_reranked(q, k, kc, ql, 0.2)
        for feats in (ql, ql8):                                            # bf16: quantised into the static input; uint8: copied
            v_g, i_g = gr(q, feats)
            assert torch.equal(gr.q_feats, ql8)
            assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e)), seed
    gr.close()


def test_features_want_local_fp8_at_vit_small(dev):
    from vpr_amd import ops
    from vpr_amd.modules import DinoV2Salad
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    ext.aggregator.pack()
    x = torch.randn(3, 3, 224, 224, device=dev).to(torch.bfloat16)
    d, d16 = ext.features(x, want_bf16=True)
    d, d16 = d.clone(), d16.clone()
    e, e16, local8 = ext.features(x, want_bf16=True, want_local="fp8")
    assert torch.equal(bits(d), bits(e)) and torch.equal(d16.view(torch.int16), e16.view(torch.int16))   # the default call's, bit for bit
    e1, local81 = ext.features(x, want_local="fp8")
    assert torch.equal(bits(e1), bits(d)) and torch.equal(local81, local8)
    assert local8.shape == (3, 256, 128) and local8.dtype == torch.uint8
    _, _, local = ext.features(x, want_bf16=True, want_local=True)
    assert local.dtype == torch.bfloat16
    tokens = ext.backbone(x, split=True).patch
    agg = ext.aggregator
    assert torch.equal(agg.local_features(tokens, fp8=True), local8) and torch.equal(agg.local_features(tokens).view(torch.int16), local.view(torch.int16))
    # the f32 normalised MLP output, by the module's own two GEMMs: the bytes are its one-rounding quantisation, not the bf16's
    w = agg._packed
    h = ops.gemm_nt_bf16(tokens.reshape(-1, 384).contiguous(), w.w1_sc[agg.hidden:], w.b1_sc[agg.hidden:], relu=True, out_dtype=torch.bfloat16)
    f = ops.gemm_nt_bf16(h, w.w2_c, w.b2_c)
    assert f.dtype == torch.float32
    norm = f.norm(dim=1, keepdim=True)
    f = torch.where(norm > 0, f / norm, torch.zeros_like(f)).view(3, 256, 128)
    assert torch.equal(f.to(torch.bfloat16).view(torch.int16), local.view(torch.int16))
    assert np.array_equal(local8.cpu().numpy(), ref8.quantize(f.cpu()))
    through_bf16 = (local8.cpu().numpy() != ref8.quantize(local.cpu())).mean()
    print(f"bytes a bf16 stop would change: {through_bf16:.4f}")
    assert through_bf16 > 0
    # within one e4m3 spacing of the bf16 values (half a spacing from the e4m3 rounding, under 2^-9 relative from the bf16 one)
    a, b = ref8.decode(local8.cpu()), local.cpu().double().numpy()
    mag = np.maximum(np.abs(a), np.abs(b))
    spacing = np.where(mag < 2.0 ** -14, 2.0 ** -17, 2.0 ** (np.floor(np.log2(np.maximum(mag, 2.0 ** -30))) - 3))
    assert (np.abs(a - b) <= spacing).all()
    small = DinoV2Salad("vit_small", img_size=322)
    with pytest.raises(ValueError, match="at most 256"):
        small.features(torch.zeros(1, 3, 322, 322), want_local="fp8")    # refused before anything runs: a CPU tensor is fine


def test_retrieval_scores_on_a_gallery_kept_in_e4m3(dev, tmp_path, monkeypatch):
    """Generated images, a gallery kept with keep_local="fp8": 32 KB of local features per image; calculate_retrieval_scores(
    local_rerank=) matches on them and equals retrieval_metrics, by hand, of search_local_reranked on the same batches."""
    import os
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, gallery as G, modules
    from vpr_amd.retrieval import ShardedGallery
    rng = np.random.default_rng(21)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g = 20
    gnames = [f"img_{i:04d}.png" for i in range(n_g)]
    imgs = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(n_g)]
    for n, im in zip(gnames, imgs):
        Image.fromarray(im).save(gdir / n)
    lat, lon, ang = 219000 + 100.0 * np.arange(n_g), 143000 + 50.0 * np.arange(n_g), (17.0 * np.arange(n_g)) % 360
    pd.DataFrame({"filename": gnames, "timestamp": "t", "latitude": lat, "longitude": lon, "angle": ang,
                  "Region_ID": np.arange(n_g) // 5}).to_csv(tmp_path / "labels_train.csv", index=False)
    src = [3, 11, 0, 19, 7, 12]
    vnames = [f"img_{i:04d}.png" for i in range(len(src))]
    for n, s in zip(vnames, src):
        noisy = np.clip(imgs[s].astype(np.int16) + rng.integers(-3, 4, imgs[s].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(vdir / n)
    pd.DataFrame({"filename": vnames, "timestamp": "t", "latitude": lat[src] + 3.0, "longitude": lon[src] - 4.0,
                  "angle": (ang[src] + 5.0) % 360, "Region_ID": np.array(src) // 5}).to_csv(tmp_path / "labels_val.csv", index=False)
    torch.manual_seed(1)
    ext = modules.DinoV2Salad("vit_small")
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    train = (ext, str(tmp_path / "labels_train.csv"), str(gdir))
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "gal8"), batch_size=8, keep_local="fp8", graph=False) == n_g
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "gal"), batch_size=8, keep_local=True, graph=False) == n_g
    assert os.path.exists(tmp_path / "gal8" / G.LOCAL_FP8_FILE) and not os.path.exists(tmp_path / "gal8" / G.LOCAL_FILE)
    stored = np.load(tmp_path / "gal8" / G.LOCAL_FP8_FILE)
    assert stored.dtype == np.uint8 and stored.shape == (n_g, 256, 128) and stored[0].nbytes == 32768      # 32 KB per image
    assert np.array_equal(np.load(tmp_path / "gal8" / "descriptors.npy"), np.load(tmp_path / "gal" / "descriptors.npy"))
    apart = np.abs(ref8.decode(stored) - torch.from_numpy(np.load(tmp_path / "gal" / G.LOCAL_FILE)).view(torch.bfloat16).double().numpy())
    assert apart.max() <= 2.0 ** -4                                        # one e4m3 spacing below 1
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None, **kw):
        seen.append((q_local.clone(), k, expand, {n: (v.clone() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}))
        return plain_search(self, q_local, k, expand, **kw)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run_ = lambda gal="gal8", **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / gal), str(tmp_path / "labels_val.csv"),
                                                                        str(vdir), k=5, tau=10.0, batch_size=4, verbose=False, graph=False, **kw)
    got = run_(local_rerank=8, min_sim=0.5)
    assert all(set(kw) == {"local_rerank", "q_local_feats", "min_sim"} and kw["q_local_feats"].dtype == torch.uint8 for *_, kw in seen)
    shard = G.load_gallery_shard(str(tmp_path / "gal8"), dev, load_local=True)
    assert shard.local.shape == (n_g, 256, 128) and shard.local.dtype == torch.uint8
    sg = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True, local_feats=shard.local)
    batches = [plain_search(sg, d16, k, local_rerank=8, q_local_feats=kw["q_local_feats"], min_sim=0.5) for d16, k, _, kw in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    top = idx.cpu().numpy()
    assert top[:, 0].tolist() == src and got["topk_indices"].tobytes() == top.tobytes()
    assert got["topk_scores"].tobytes() == vals.cpu().numpy().tobytes()
    assert (got["topk_scores"][:, 0] > 128).all()            # local scores: most of the 256 patches match at similarity ~1
    base = run_("gal", local_rerank=8, min_sim=0.5)          # the bf16 gallery of the same images: the same first places
    assert base["topk_indices"][:, 0].tolist() == src
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
