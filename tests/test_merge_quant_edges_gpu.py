"""vpr_topk_merge (every multi-GPU step) and vpr_quantize_fp8_rows (every fp8 gallery) against oracle/knn.py at their
edges: values, indices, bytes and scales are compared exactly.

Merge contract (include/vpr_amd.h): (value desc, index asc) over the live entries of all shards; idx < 0 is padding
whatever its value; fewer than k live entries leave a (-inf, -1) tail; +0.0 sorts above -0.0; NaN is out of contract;
k <= 128 and shards * k <= 4096, anything larger is refused.
Quantiser contract: scale = max|x| / 448 in f32 (1 for a zero row), byte = e4m3 RNE of the f32 quotient x / scale."""
import pytest
import torch

from oracle import knn as oknn

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _merge_both(dev, vals, idxs):
    from vpr_amd import ops
    ov, oi = ops.topk_merge(vals.to(dev), idxs.to(dev))
    rv, ri = oknn.topk_merge(vals, idxs)
    ov, oi = ov.cpu(), oi.cpu()
    assert torch.equal(oi, ri), (oi, ri)
    assert torch.equal(ov.view(torch.int32), rv.view(torch.int32)), (ov, rv)         # bits: +0.0 and -0.0 differ
    return ov, oi


def _lists(R, B, k, g, levels=5, pad_frac=0.0):
    """[R, B, k] lists with many equal values (few levels), unique global indices per query in a shuffled order (so the
    lower index of a tie sits in any shard), and a share of padding entries carrying +inf."""
    vals = torch.randint(0, levels, (R, B, k), generator=g).float() * 0.25 - 0.5
    idxs = torch.stack([torch.randperm(R * k, generator=g).view(R, k) + 1000 * b for b in range(B)], 1).to(torch.int32)
    if pad_frac:
        pad = torch.rand(R, B, k, generator=g) < pad_frac
        idxs[pad] = -1
        vals[pad] = float("inf")
    return vals, idxs


def test_merge_ties_across_and_inside_shards(dev):
    # equal values across shards, the lower global index in the LATER shard; equal values inside one list
    vals = torch.tensor([[[0.5, 0.5, 0.25]], [[0.5, 0.25, 0.25]], [[0.5, 0.5, -1.0]]])
    idxs = torch.tensor([[[90, 70, 40]], [[50, 60, 10]], [[5, 80, 7]]], dtype=torch.int32)
    ov, oi = _merge_both(dev, vals, idxs)
    assert oi.tolist() == [[5, 50, 70]] and ov.tolist() == [[0.5, 0.5, 0.5]]


def test_merge_padding_and_short_lists(dev):
    inf = float("inf")
    # padding carries +inf: the value of a negative index is ignored
    vals = torch.tensor([[[inf, 0.1, inf]], [[0.3, inf, 0.2]]])
    idxs = torch.tensor([[[-1, 4, -7]], [[9, -1, 2]]], dtype=torch.int32)
    ov, oi = _merge_both(dev, vals, idxs)
    assert oi.tolist() == [[9, 2, 4]]
    # fewer than k live entries: (-inf, -1) tail; a live entry that holds -inf stays ahead of it
    vals = torch.tensor([[[0.75, inf, inf, inf]], [[NEG_INF, inf, inf, inf]]])
    idxs = torch.tensor([[[3, -1, -1, -1]], [[8, -1, -1, -1]]], dtype=torch.int32)
    ov, oi = _merge_both(dev, vals, idxs)
    assert oi.tolist() == [[3, 8, -1, -1]] and ov.tolist() == [[0.75, NEG_INF, NEG_INF, NEG_INF]]
    # all padding
    vals = torch.full((3, 2, 5), inf)
    idxs = torch.full((3, 2, 5), -1, dtype=torch.int32)
    ov, oi = _merge_both(dev, vals, idxs)
    assert bool((oi == -1).all()) and bool((ov == NEG_INF).all())


def test_merge_signed_zeros_follow_the_key_order(dev):
    """+0.0 and -0.0 with different indices: not a tie — the packed key orders +0.0 first whatever the indices (the select
    kernels share the key, and bench.py pins their outputs bit for bit, so the contract is the key's order)."""
    vals = torch.tensor([[[-0.0, 0.0, -1.0]], [[0.0, -0.0, -0.0]]])
    idxs = torch.tensor([[[1, 30, 2]], [[20, 3, 0]]], dtype=torch.int32)
    ov, oi = _merge_both(dev, vals, idxs)
    assert oi.tolist() == [[20, 30, 0]]
    assert torch.signbit(ov).tolist() == [[False, False, True]]


@pytest.mark.parametrize("R,k", [(1, 1), (255, 1), (256, 1), (257, 1), (4096, 1), (36, 7), (37, 7), (585, 7), (3, 85), (1, 64),
                                  (4, 64), (64, 64), (1, 128), (2, 128), (32, 128)])
def test_merge_sizes_and_query_stride(dev, R, k):
    """shards * k at 1, 255, 256, 257 (the 256-thread stride of the key load) and 4096 (the capacity), k at 1, 7, 64 (the
    last k of the 64-group path) and 128; B = 3 queries with different data each; with and without padding."""
    g = torch.Generator().manual_seed(R * 131 + k)
    for pad in (0.0, 0.3, 0.97):
        _merge_both(dev, *_lists(R, 3, k, g, pad_frac=pad))
    vals, idxs = _lists(R, 3, k, g, levels=1 << 20)                      # (almost) no ties
    _merge_both(dev, vals, idxs)


def test_merge_refuses_what_it_cannot_hold(dev):
    from vpr_amd import _lib, ops
    L = _lib.lib()
    for R, k in ((4097, 1), (1, 129), (33, 128)):
        vals = torch.zeros(R, 2, k, device=dev)
        idxs = torch.zeros(R, 2, k, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError):
            ops.topk_merge(vals, idxs)
        ov = torch.full((2, k), 7.0, device=dev)
        oi = torch.full((2, k), 7, dtype=torch.int32, device=dev)
        assert L.vpr_topk_merge(ops._ptr(vals), ops._ptr(idxs), R, 2, k, ops._ptr(ov), ops._ptr(oi), ops._stream()) == -2
        torch.cuda.synchronize()
        assert bool((ov == 7.0).all()) and bool((oi == 7).all())


# ------------------------------------------------------------------------------------------------ fp8 row quantiser
def _quant_both(dev, x):
    from vpr_amd import ops
    q, s = ops.quantize_fp8_rows(x.to(dev))
    rq, rs = oknn.quantize_fp8_rows(x)
    q, s = q.cpu(), s.cpu()
    assert torch.equal(s.view(torch.int32), rs.view(torch.int32)), (s, rs)
    bad = (q != rq).nonzero()
    assert bad.numel() == 0, [(int(r), int(c), float(x[r, c]), int(q[r, c]), int(rq[r, c])) for r, c in bad[:8].tolist()]
    return q, s


def _half_spacing_e4m3(y: torch.Tensor) -> torch.Tensor:
    """Half the spacing of e4m3 numbers at |y| <= 448: 2^(e - 3) / 2 with e = floor(log2 |y|), at least -6 (subnormals)."""
    e = (torch.frexp(y.abs().clamp_min(2.0 ** -6)).exponent - 1).clamp_min(-6)
    return torch.ldexp(torch.ones_like(y), e - 4)


def _check_dequant(x, q, s):
    xd, sd = x.double(), s.double()[:, None]
    deq = q.view(torch.float8_e4m3fn).double() * sd
    y = xd / sd
    tol = sd * (_half_spacing_e4m3(y) + 2.0 ** -23 * y.abs())          # + the f32 rounding of the quotient
    assert bool(((deq - xd).abs() <= tol).all())


TIE_VALUES = [448.0, 17.0, 19.0, 21.0, 200.0, 208.0, 216.0, 232.0, 240.0, 248.0, 272.0, 304.0, 432.0, 1.0625, 1.1875,
              2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 13 * 2.0 ** -10, 15 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -9, 2.0 ** -6,
              2.0 ** -6 - 2.0 ** -10, 0.0]


def test_quantize_rounding_ties_at_scale_one(dev):
    """max = 448 exactly: scale 1.0, and the other entries sit on e4m3 ties of every kind — normal range (17, 19, 208 ± 8,
    240 ± 8, ...), subnormal range (odd multiples of 2^-10), halfway to zero (2^-10 -> 0) — with both signs and their f32
    neighbours on either side; a negative maximum; -0.0 -> 0x80."""
    base = torch.tensor(TIE_VALUES)
    up = torch.nextafter(base, torch.full_like(base, 1e9))
    down = torch.nextafter(base, torch.full_like(base, -1e9)).clamp_min(0)
    up[0] = 448.0                                                        # nothing above the maximum
    row = torch.cat([base, -base, up, -up, down, -down])
    row = torch.cat([row, torch.zeros((-row.numel()) % 4)])
    neg_max = row.clone()
    neg_max[0] = neg_max[2 * len(TIE_VALUES)] = 440.0                    # both +448 entries lowered: the maximum is a -448
    assert neg_max.max().item() < 448.0 and neg_max.min().item() == -448.0
    x = torch.stack([row, neg_max])
    q, s = _quant_both(dev, x)
    assert s.tolist() == [1.0, 1.0]
    n = len(TIE_VALUES)
    f = q.view(torch.float8_e4m3fn).float()
    assert f[0, :n].tolist()[:6] == [448.0, 16.0, 20.0, 20.0, 192.0, 208.0]
    assert f[0, n - 1 - 9:n - 1 - 4].tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, 6 * 2.0 ** -9, 2.0 ** -6]     # 1, 3, 5, 13, 15 x 2^-10
    assert int(q[0, 2 * n - 1]) == 0x80 and int(q[0, n - 1]) == 0x00     # -0.0 keeps its sign
    assert int(q[1, n]) == 0xFE                                          # -448
    _check_dequant(x, q, s)


def test_quantize_ties_under_scales_that_are_no_power_of_two(dev):
    """max = 448 c with c = 3, 5, 0.7 (scale = c up to its f32 rounding) and entries c x (a tie value): where c x tie is an
    f32 value the IEEE quotient x / scale lands exactly on the tie, while x * (1 / scale) is off by an ulp for about half of
    them and rounds the other way.  Bytes are compared with the oracle (which divides), and at least 20 entries per row must
    sit exactly on a tie for the row to mean something."""
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, 25.0, 27.0, 29.0, 31.0, 34.0, 38.0, 42.0, 46.0, 50.0, 54.0, 58.0, 62.0, 68.0, 76.0,
                         84.0, 92.0, 100.0, 108.0, 116.0, 124.0, 136.0, 152.0, 168.0, 184.0, 200.0, 216.0, 232.0, 248.0, 272.0, 304.0,
                         336.0, 368.0, 400.0, 432.0, 8.5, 9.5, 10.5, 11.5, 12.5, 13.5, 14.5, 15.5, 2.0 ** -10, 3 * 2.0 ** -10])
    rows = []
    for c in (3.0, 5.0, 0.7):
        row = torch.cat([torch.tensor([448.0]), ties, -ties]) * c
        rows.append(torch.cat([row, torch.zeros((-row.numel()) % 4)]))
    x = torch.stack(rows)
    q, s = _quant_both(dev, x)
    y = x / s[:, None]                                                   # the IEEE f32 quotients
    on_tie = (y.abs()[:, 1:1 + 2 * ties.numel()] == torch.cat([ties, ties])).sum(1)
    assert (on_tie >= 20).all(), on_tie
    recip = (x * (1.0 / s)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert (recip != q).any(), "no entry tells a reciprocal multiply from the quotient"
    _check_dequant(x, q, s)


def test_quantize_zero_rows_single_nonzero_and_large_rows(dev):
    x = torch.zeros(4, 8)
    x[1, 5] = -3.25e-3                      # a single non-zero: scale |v| / 448, byte -448
    x[2] = torch.tensor([3e38, -3e38, 1e38, 1e30, 0.0, -0.0, 2.9e38, 1.0])
    x[3, 0], x[3, 3] = -0.0, -0.0           # zero row with negative zeros
    q, s = _quant_both(dev, x)
    assert s[0].item() == 1.0 and not q[0].any()
    assert q[1].tolist() == [0, 0, 0, 0, 0, 0xFE, 0, 0]
    assert s[3].item() == 1.0 and q[3].tolist() == [0x80, 0, 0, 0x80, 0, 0, 0, 0]
    assert q[2, 0].item() == 0x7E and q[2, 1].item() == 0xFE and torch.isfinite(s).all()
    _check_dequant(x[:3], q[:3], s[:3])


def test_quantize_denormal_row(dev):
    """max|x| = 1e-40: the scale itself is an f32 denormal.  The contract (include/vpr_amd.h) is plain IEEE f32 arithmetic with
    denormals kept — scale = fl(max / 448), byte = e4m3 RNE of fl(x / scale) — which is what the oracle computes."""
    x = torch.zeros(2, 8)
    x[0] = torch.tensor([1e-40, -1e-40, 5e-41, 2.5e-41, 1e-42, 1e-45, 0.0, -7e-41])
    x[1] = torch.tensor([1e-38, 1e-40, -3e-39, 1e-45, 0.0, 0.0, 0.0, 0.0])
    q, s = _quant_both(dev, x)
    print("denormal rows: scales", s.tolist(), "bytes", q.tolist())
    assert (s > 0).all()


@pytest.mark.parametrize("D", [4, 1020, 1024, 1028, 8448])
@pytest.mark.parametrize("rows", [1, 3])
def test_quantize_row_lengths(dev, D, rows):
    """D around the 1024-element stride of the row loops; every row with its own scale."""
    g = torch.Generator().manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) * torch.tensor([1.0, 1e-3, 50.0])[:rows, None]
    x[0, D - 1] = 9.0                        # the maximum in the last element: a loop that stops short gets the scale wrong
    q, s = _quant_both(dev, x)
    _check_dequant(x, q, s)


def test_quantize_refusals(dev):
    from vpr_amd import ops
    with pytest.raises(RuntimeError):
        ops.quantize_fp8_rows(torch.zeros(2, 6, device=dev))                # D % 4
    base = torch.zeros(2 * 8 + 4, device=dev)
    mis = base[1:17].view(2, 8)                                              # 4 bytes off a 16-byte boundary
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError):
        ops.quantize_fp8_rows(mis)
