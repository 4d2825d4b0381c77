"""GPU: vpr_rerank_rows (include/vpr_amd_rerank.h) through ops.rerank_rows / torch.ops.vpr.rerank_rows, ShardedGallery.
search_reranked / search_expanded(rerank=) / search_local_queries(rerank=), GraphedRetrieval(rerank=), the pipeline and
evaluate.calculate_retrieval_scores(rerank=).

Reference: f64 dot products of the stored (bf16 / f32) values, formed with torch in f64 — every product of two stored values
is exact in f64 for bf16 operands and has 2^-53 relative error otherwise, nothing beside the f32 bound below.

Bound on a written score (derived, not tuned): the kernel's sum is a tree of f32 additions of fmaf-rounded partial sums whose
longest path from a product to the result holds L = VPR_RERANK_ROUNDINGS(D, rows_are_f32) roundings (the header's order), so
    |s - exact| <= gamma_L * sum_d |q_d r_d|,   gamma_L = L u / (1 - L u),  u = 2^-24.
Measured on MI355X over the grids of the first two tests: worst |err| / bound = 0.2245 (under 0.02 at D = 8448)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
KCS = (1, 2, 63, 64, 65, 128)
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module", autouse=True)
def registered_ops(dev):
    from vpr_amd import torch_ops  # noqa: F401  registers torch.ops.vpr.*


def bits(t):
    return t.contiguous().view(torch.int32)


def gamma(D, rows_f32):
    from vpr_amd import _lib
    L = _lib.rerank_roundings(D, rows_f32)
    u = 2.0 ** -24
    return L * u / (1 - L * u)


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


# ---------------------------------------------------------------------------------------------------- reference
def exact_scores(q, rows):
    """q [B, D], rows [B, n, D] or [n, D] as stored -> (f64 scores [B, n], A = sum_d |q_d r_d| [B, n]) on the device."""
    q64, r64 = q.double(), rows.double()
    if r64.dim() == 2:
        return q64 @ r64.T, q64.abs() @ r64.abs().T
    return torch.einsum("bd,bnd->bn", q64, r64), torch.einsum("bd,bnd->bn", q64.abs(), r64.abs())


def reference(S, idx, n_local, index_base, k, per_query=False):
    """S f64 [B, n] (numpy; column = local row, or with per_query the candidate's own local row b * n + col), idx int [B, kc]
    -> (score f64 [B, k], idx [B, k], position in the input [B, k]) by (numeric before NaN, f64 score desc, index asc, position)."""
    B, kc = idx.shape
    sv, si, sp = np.full((B, k), -np.inf), np.full((B, k), -1, dtype=np.int64), np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        rel = idx[b].astype(np.int64) - index_base
        live = np.nonzero((rel >= 0) & (rel < n_local))[0]
        col = rel[live] - (b * S.shape[1] if per_query else 0)
        s = S[b, col]
        order = sorted(range(len(live)), key=lambda t: (bool(np.isnan(s[t])), 0.0 if np.isnan(s[t]) else -s[t], int(idx[b, live[t]]),
                                                        int(live[t])))[:k]
        for pos, t in enumerate(order):
            sv[b, pos], si[b, pos], sp[b, pos] = s[t], idx[b, live[t]], live[t]
    return sv, si, sp


# ------------------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module")
def worst_ratio():
    seen = {"worst": 0.0}
    yield seen
    print(f"\nrerank: worst |err| / bound over the module = {seen['worst']:.4f}")


@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("D", [64, 192, 8448])
@pytest.mark.parametrize("qd", ["bf16", "f32"])
@pytest.mark.parametrize("rd", ["bf16", "f32"])
def test_scores_within_the_derived_bound(dev, rd, qd, D, B, worst_ratio):
    """i.i.d. unit rows (150 of them at index_base 1000), kc in KCS x k_out in {1, kc}: every written value is within gamma_L A
    of the f64 score of the index written beside it; the list is non-increasing; where it differs from the f64 order (gaps
    may fall under the bound here) the reference's index scores within 2 x bound of the k-th."""
    g = torch.Generator(device=dev).manual_seed(10000 * D + 100 * B + 10 * (rd == "f32") + (qd == "f32"))
    n, base = 150, 1000
    rows = unit(torch.randn(n, D, device=dev, generator=g, dtype=torch.float64)).to(DTYPES[rd])
    q = unit(torch.randn(B, D, device=dev, generator=g, dtype=torch.float64) / D ** 0.5 + 0.5 * rows[:B].double()).to(DTYPES[qd])
    S_t, A_t = exact_scores(q, rows)
    S, A = S_t.cpu().numpy(), A_t.cpu().numpy()
    gam = gamma(D, rd == "f32")
    rng = np.random.default_rng(D + B)
    for kc in KCS:
        idx = np.stack([rng.permutation(n)[:kc] for _ in range(B)]).astype(np.int32) + base
        idx_t = torch.from_numpy(idx).to(dev)
        for k in sorted({1, kc}):
            v, i = torch.ops.vpr.rerank_rows(q, idx_t, rows, base, k)
            assert v.shape == i.shape == (B, k) and v.dtype == torch.float32 and i.dtype == torch.int32
            v, i = v.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)
            assert (i >= base).all() and (i < base + n).all()
            for b in range(B):                               # distinct candidates, each at most once
                assert len(set(i[b].tolist())) == k and set(i[b].tolist()) <= set(idx[b].tolist())
            ex = np.take_along_axis(S, i - base, 1)
            bound = gam * np.take_along_axis(A, i - base, 1)
            ratio = float((np.abs(v - ex) / bound).max())
            worst_ratio["worst"] = max(worst_ratio["worst"], ratio)
            print(f"rows {rd} q {qd} D={D} B={B} kc={kc} k={k}: max |err| / bound = {ratio:.4f}")
            assert ratio <= 1.0, (kc, k, ratio)
            assert (np.diff(v, axis=1) <= 0).all()
            rv, ri, _ = reference(S, idx, n, base, k)
            # computed scores within beta of the exact ones put, at every position, an exact score within 2 beta of the
            # reference's score of that position (the k-th included)
            for b, pos in zip(*np.nonzero(ri != i)):
                beta = gam * A[b, idx[b].astype(np.int64) - base].max()
                assert abs(ex[b, pos] - rv[b, pos]) <= 2 * beta, (kc, k, b, pos)


# -------------------------------------------------------------------------------------------------------- order
def gapped(dev, B, D, n, seed, step=2e-3, top=0.9):
    """Per query b, n rows s_j q_b + sqrt(1 - s_j^2) n_j with n_j a unit vector orthogonal to q_b and the s_j a shuffled grid
    `step` apart below `top`: f64 q [B, D], rows [B, n, D]."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = unit(torch.randn(B, D, device=dev, generator=g, dtype=torch.float64))
    noise = torch.randn(B, n, D, device=dev, generator=g, dtype=torch.float64)
    noise = unit(noise - (noise * q[:, None, :]).sum(-1, keepdim=True) * q[:, None, :])
    s = top - step * torch.stack([torch.randperm(n, device=dev, generator=g) for _ in range(B)]).double()
    return q, s[..., None] * q[:, None, :] + (1 - s * s).sqrt()[..., None] * noise


@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("D", [64, 192, 8448])
@pytest.mark.parametrize("qd", ["bf16", "f32"])
@pytest.mark.parametrize("rd", ["bf16", "f32"])
def test_order_equals_the_f64_order_on_gapped_rows(dev, rd, qd, D, B, worst_ratio):
    """128 gapped rows per query (global row = base + 128 b + j): after rounding to the stored dtype, consecutive f64 scores are
    more than 4 x the bound apart (asserted), so the index lists must equal the f64 reference exactly — every kc, every k_out."""
    n, base = 128, 77
    q64, rows64 = gapped(dev, B, D, n, 7 * D + B)
    q, rows = q64.to(DTYPES[qd]), rows64.to(DTYPES[rd])
    S_t, A_t = exact_scores(q, rows)
    S, A = S_t.cpu().numpy(), A_t.cpu().numpy()
    gam = gamma(D, rd == "f32")
    flat = rows.view(B * n, D)
    rng = np.random.default_rng(3 * D + B)
    for kc in KCS:
        pick = np.stack([rng.permutation(n)[:kc] for _ in range(B)])
        idx = (pick + n * np.arange(B)[:, None] + base).astype(np.int32)
        # the precondition, on the candidates of this list: sorted f64 scores more than 4 x bound apart
        s_c, a_c = np.take_along_axis(S, pick, 1), np.take_along_axis(A, pick, 1)
        order = np.argsort(-s_c, axis=1, kind="stable")
        s_s, b_s = np.take_along_axis(s_c, order, 1), gam * np.take_along_axis(a_c, order, 1)
        if kc > 1:
            assert (s_s[:, :-1] - s_s[:, 1:] > 4 * np.maximum(b_s[:, :-1], b_s[:, 1:])).all(), kc
        idx_t = torch.from_numpy(idx).to(dev)
        for k in sorted({1, kc}):
            v, i = torch.ops.vpr.rerank_rows(q, idx_t, flat, base, k)
            rv, ri, _ = reference(S, idx, B * n, base, k, per_query=True)
            assert np.array_equal(i.cpu().numpy().astype(np.int64), ri), (kc, k)
            ratio = float((np.abs(v.cpu().numpy().astype(np.float64) - rv) / b_s[:, :k]).max())
            worst_ratio["worst"] = max(worst_ratio["worst"], ratio)
            assert ratio <= 1.0, (kc, k, ratio)


@pytest.mark.parametrize("rd", ["bf16", "f32"])
def test_identical_rows_come_out_in_ascending_index_order(dev, rd):
    D, n, base = 192, 40, 300
    g = torch.Generator(device=dev).manual_seed(5)
    rows = unit(torch.randn(n, D, device=dev, generator=g)).to(DTYPES[rd])
    rows[[3, 9, 17, 30]] = rows[12].clone()                  # five indices, one row: the same score bit for bit
    rows[[25, 1]] = rows[38].clone()
    q = unit(rows[12].float() + 0.6 * rows[38].float() + 0.02 * torch.randn(2, D, device=dev, generator=g)).to(torch.bfloat16)
    idx = torch.tensor([[30, 5, 17, 12, 38, 9, 1, 3, 25, 20], [1, 25, 38, 3, 9, 12, 17, 30, 7, 8]], dtype=torch.int32, device=dev) + base
    v, i = torch.ops.vpr.rerank_rows(q, idx, rows, base, 10)
    v, i = v.cpu(), (i.cpu() - base).tolist()
    for b in range(2):
        assert i[b][:5] == [3, 9, 12, 17, 30] and i[b][5:8] == [1, 25, 38], i[b]
        assert len(set(bits(v[b, :5]).tolist())) == 1 and len(set(bits(v[b, 5:8]).tolist())) == 1
    # a duplicated INDEX is scored and emitted as often as it occurs
    dup = torch.tensor([[7, 12, 7, 38, 7, 20]], dtype=torch.int32, device=dev) + base
    v, i = torch.ops.vpr.rerank_rows(q[:1], dup, rows, base)
    got = (i.cpu()[0] - base).tolist()
    assert sorted(got) == [7, 7, 7, 12, 20, 38] and got[0] == 12 and got[1] == 38
    at = [p for p, x in enumerate(got) if x == 7]
    assert at == list(range(at[0], at[0] + 3)) and len(set(bits(v.cpu()[0, at]).tolist())) == 1


# ----------------------------------------------------------------------------------- cross-check against knn_topk
@pytest.mark.parametrize("D", [192, 8448])
def test_rerank_of_a_bf16_search_returns_its_order(dev, D):
    """Fine rows = the bf16 rows that were searched, bf16 queries, gapped rows: vpr_knn_topk's values are the f32 roundings of
    the exact scores, so re-ranking its list returns the same index order and values within the bound of its values."""
    from vpr_amd import ops
    B, n, k = 3, 64, 64
    q64, rows64 = gapped(dev, B, D, n, 900 + D)
    g = torch.Generator(device=dev).manual_seed(9)
    filler = unit(torch.randn(200, D, device=dev, generator=g, dtype=torch.float64))
    perm = torch.randperm(B * n + 200, device=dev, generator=g)
    gal = torch.cat([rows64.view(B * n, D), filler])[perm].to(torch.bfloat16).contiguous()
    q = q64.to(torch.bfloat16)
    kv, ki = ops.knn_topk(q, gal, k, index_base=40)
    v, i = ops.rerank_rows(q, ki, gal, index_base=40)
    assert torch.equal(i, ki)
    _, A = exact_scores(q, gal)
    bound = gamma(D, False) * torch.gather(A, 1, (ki - 40).long())
    assert ((v.double() - kv.double()).abs() <= bound).all()
    v10, i10 = ops.rerank_rows(q, ki, gal, index_base=40, k=10)
    assert torch.equal(i10, ki[:, :10]) and torch.equal(bits(v10), bits(v[:, :10]))


# ----------------------------------------------------------------------------------------------- hostile indices
@pytest.mark.parametrize("rd", ["bf16", "f32"])
def test_hostile_indices_are_never_dereferenced(dev, rd):
    """A 20-row shard at index_base 500, cut out of a NaN-filled buffer; every row no live index names is NaN as well, so a
    wrong dereference shows in the output."""
    D, n, base, kc = 192, 20, 500, 16
    g = torch.Generator(device=dev).manual_seed(13)
    big = torch.full((n + 16, D), float("nan"), device=dev, dtype=DTYPES[rd])
    rows = big[8:8 + n]
    named = [0, 19, 4, 7, 11]                                # first and last owned row among them
    rows[named] = unit(torch.randn(len(named), D, device=dev, generator=g)).to(DTYPES[rd])
    nan_row = 13                                             # live, and NaN: after the numeric scores, before the padding
    q = unit(torch.randn(5, D, device=dev, generator=g)).to(torch.bfloat16)
    lists = [
        [-1, I32_MIN, I32_MAX, base - 1, base + n, base + 0, base + 19, base + 4, -1, base + 7, base + nan_row, base + 11, 0, n, base + n + 5, base + 4],
        [base + nan_row, -1, base + 19, I32_MAX, base + nan_row, I32_MIN, base - 1, base + n] + [-1] * 8,
        [-1, I32_MIN, I32_MAX, base - 1, base + n, 0, 1, 19, base + 1000, -7, base - 500, 2 * base, -base, I32_MAX - 1, I32_MIN + 1, -1],
        [base + 11] + [-1] * 15,
        [base + nan_row, base + 0, -1, base + 19] + [-1] * 12,
    ]
    idx = np.array(lists, dtype=np.int64).astype(np.int32)
    S, A = (t.cpu().numpy() for t in exact_scores(q, rows))
    for k in (1, 5, kc):
        v, i = torch.ops.vpr.rerank_rows(q, torch.from_numpy(idx).to(dev), rows, base, k)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        rv, ri, _ = reference(S, idx, n, base, k)
        assert np.array_equal(i, ri), k
        want_v = np.where(np.isnan(rv), -np.inf, rv)
        finite = np.isfinite(want_v)
        assert np.array_equal(np.isfinite(v), finite) and (v[~finite] == -np.inf).all()
        assert (np.abs(v[finite] - want_v[finite]) <= gamma(D, rd == "f32") * 1.01).all()      # A <= |q| |r| <= 1.01
    # spelled out for k = kc
    assert i[0].tolist()[:7] == ri[0].tolist()[:7] and i[0, 6] == base + nan_row and v[0, 6] == -np.inf and np.isfinite(v[0, :6]).all()
    assert (i[0, 7:] == -1).all() and (v[0, 7:] == -np.inf).all()
    assert i[1].tolist()[:3] == [base + 19, base + nan_row, base + nan_row] and (i[1, 3:] == -1).all() and np.isfinite(v[1, 0])
    assert (i[2] == -1).all() and (v[2] == -np.inf).all()                      # no live candidate: all padding
    assert i[3, 0] == base + 11 and (i[3, 1:] == -1).all()
    assert i[4].tolist()[:3] == [ri[4, 0], ri[4, 1], base + nan_row] and v[4, 2] == -np.inf and (i[4, 3:] == -1).all()
    # the output is a list vpr_topk_merge takes (distinct indices: queries 2-4): merging it with an empty shard's list
    # changes nothing, the NaN-scored row included
    sub = torch.from_numpy(idx[2:]).to(dev)
    v_t, i_t = torch.ops.vpr.rerank_rows(q[2:], sub, rows, base, kc)
    empty = torch.ops.vpr.rerank_rows(q[2:], sub, rows, 10 ** 6, kc)
    assert (empty[1] == -1).all() and (empty[0] == float("-inf")).all()
    mv, mi = torch.ops.vpr.topk_merge(torch.stack([empty[0], v_t]), torch.stack([empty[1], i_t]))
    assert torch.equal(mi, i_t) and torch.equal(bits(mv), bits(v_t))


# -------------------------------------------------------------------------------------------------- determinism
def test_a_query_does_not_depend_on_its_batch_padding_or_run(dev):
    from vpr_amd import _lib, ops
    D, n, base, kc = 8448, 300, 64, 10
    g = torch.Generator(device=dev).manual_seed(21)
    rows = unit(torch.randn(n, D, device=dev, generator=g)).to(torch.bfloat16)
    q = unit(torch.randn(37, D, device=dev, generator=g)).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(n, device=dev, generator=g)[:kc] for _ in range(37)]).to(torch.int32) + base
    v, i = ops.rerank_rows(q, idx, rows, base)
    for _ in range(2):                                       # repeated calls
        v2, i2 = ops.rerank_rows(q, idx, rows, base)
        assert torch.equal(i2, i) and torch.equal(bits(v2), bits(v))
    for sel in ([0], [36], [5, 0, 36], list(range(36, -1, -1))):               # B and the position in the batch
        s = torch.tensor(sel, device=dev)
        vs, is_ = ops.rerank_rows(q[s].contiguous(), idx[s].contiguous(), rows, base)
        assert torch.equal(is_, i[s]) and torch.equal(bits(vs), bits(v[s]))
    for pad_to, where in ((11, "back"), (64, "back"), (65, "front"), (128, "mixed")):   # kc padding beyond the live entries
        pad = torch.full((37, pad_to - kc), -1, dtype=torch.int32, device=dev)
        if where == "mixed":
            pad[:, ::3] = base + n + 5                       # rows another shard owns
        wide = torch.cat([idx, pad], 1) if where != "front" else torch.cat([pad, idx], 1)
        if where == "mixed":
            wide = wide[:, torch.randperm(pad_to, device=dev, generator=g)]
        vp, ip = ops.rerank_rows(q, wide.contiguous(), rows, base)
        assert torch.equal(ip[:, :kc], i) and torch.equal(bits(vp[:, :kc]), bits(v))
        assert (ip[:, kc:] == -1).all() and (vp[:, kc:] == float("-inf")).all()
    vf, i_f = ops.rerank_rows(q.float(), idx, rows, base)     # the query's dtype does not enter the order of the sum
    assert torch.equal(i_f, i) and torch.equal(bits(vf), bits(v))
    # graph replay equals the eager op
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    q_buf, idx_buf = torch.zeros_like(q), torch.full_like(idx, -1)
    with torch.cuda.stream(side):
        ops.rerank_rows(q_buf, idx_buf, rows, base, 5)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gv, gi = ops.rerank_rows(q_buf, idx_buf, rows, base, 5)
    for shift in (0, 7):
        q_buf.copy_(q.roll(shift, 0)), idx_buf.copy_(idx.roll(shift, 0))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(gi, i.roll(shift, 0)[:, :5]) and torch.equal(bits(gv), bits(v.roll(shift, 0)[:, :5]))
    del graph
    ops.drop_stream_caches(side.cuda_stream)
    # a refused call (workspace one byte short) leaves poisoned outputs untouched
    need = _lib.lib().vpr_rerank_workspace_bytes(37, kc)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    pv = torch.full((37, kc), 123.0, device=dev)
    pi = torch.full((37, kc), 456, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.lib().vpr_rerank_rows(P(q), 0, P(idx), 37, D, kc, P(rows), 0, n, base, kc, P(pv), P(pi), P(ws), need - 1,
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert st == -2 and (pv == 123.0).all() and (pi == 456).all()
    with pytest.raises(RuntimeError, match="vpr_rerank_rows"):
        ops.rerank_rows(q, idx, rows, base, ws=ws[:need - 16])
    vw, iw = ops.rerank_rows(q, idx, rows, base, ws=ws)
    assert torch.equal(iw, i) and torch.equal(bits(vw), bits(v))


# ------------------------------------------------------------------------------------------ the point of the feature
def near_duplicates(seed, N=1024, D=128, B=16, group=12, noise=0.04):
    """Groups of `group` near-duplicates — unit(q + noise * N(0, I)) — around each query among i.i.d. unit rows, shuffled:
    fine rows bf16 [N, D], queries bf16 [B, D] (host)."""
    rng = np.random.default_rng(seed)
    un = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    q = un(rng.standard_normal((B, D)))
    rows = un(rng.standard_normal((N, D)))
    rows[:B * group] = un(np.repeat(q, group, 0) + noise * rng.standard_normal((B * group, D)))
    rows = rows[rng.permutation(N)]
    return torch.from_numpy(rows).to(torch.bfloat16), torch.from_numpy(q).to(torch.bfloat16)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("tier", ["e4m3", "pca"])
def test_reranking_restores_the_fine_top1(dev, tier, seed):
    """e4m3: an e4m3 gallery of D = 128 with its bf16 rows as the fine tier.  pca: D_in = 192 rows projected to d = 64 (fitted
    on the gallery) as the coarse tier, the D_in-wide rows as the fine tier; the caller's queries are the fine queries."""
    from oracle import knn as oknn
    from vpr_amd import ops
    from vpr_amd.projection import fit_projection
    from vpr_amd.retrieval import ShardedGallery
    N, B, kc = 1024, 16, 16
    fine, q = near_duplicates(seed, N, 128 if tier == "e4m3" else 192, B)
    exact = q.double() @ fine.double().T
    top = exact.argmax(1)
    best2 = exact.topk(2, dim=1).values
    assert (best2[:, 0] - best2[:, 1] > 2 * gamma(fine.shape[1], False)).all()   # the fine top-1 is decided beyond the f32 bound
    fine_d, q_d = fine.to(dev), q.to(dev)
    if tier == "e4m3":
        g8, gs = ops.quantize_fp8_rows(fine_d.float())
        sg = ShardedGallery(g8, N, scales=gs, fine_rows=fine_d)
        q8, qs = oknn.quantize_fp8_rows(q.float())
        _, ci = oknn.knn_topk_fp8(q8, qs, g8.cpu(), gs.cpu(), kc)
    else:
        p = fit_projection(fine_d, 64)
        coarse = p.apply(fine_d)
        sg = ShardedGallery(coarse, N, projection=p, fine_rows=fine_d)
        _, ci = oknn.knn_topk(p.apply(q_d).cpu(), coarse.cpu(), kc)
    # on the CPU oracle: the coarse order is wrong at the top for at least 2 of the 16, and the right row is a candidate
    assert int((ci[:, 0].long() != top).sum()) >= 2
    assert (ci.long() == top[:, None]).any(1).all()
    v1, i1 = sg.search(q_d, 1)
    assert not torch.equal(i1[:, 0].long().cpu(), top)                           # the plain search does not return it
    for k in (1, 5):
        v, i = sg.search_reranked(q_d, k, kc)
        assert torch.equal(i[:, 0].long().cpu(), top)
        assert ((v[:, 0].double().cpu() - best2[:, 0]).abs() <= 1.01 * gamma(fine.shape[1], False)).all()
    assert sg.uncertified_queries() == 0


# -------------------------------------------------------------------------------------------------- integration
@pytest.fixture(scope="module")
def rccl_one_rank(dev):
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


def two_tier(dev, seed, N=1024, D=128, B=16, **kw):
    """The near-duplicate gallery as an e4m3 ShardedGallery with bf16 fine rows; returns (gallery, queries, fine rows)."""
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    fine, q = near_duplicates(seed, N, D, B)
    fine, q = fine.to(dev), q.to(dev)
    g8, gs = ops.quantize_fp8_rows(fine.float())
    return ShardedGallery(g8, N, scales=gs, fine_rows=fine, **kw), q, fine


@pytest.mark.parametrize("R", [2, 3])
def test_merge_of_per_shard_reranks_equals_the_union_reference(dev, R):
    """One gapped gallery (24 rows per query + filler, D = 128) cut at uneven boundaries: per shard an e4m3 search for kc, the
    re-rank of its list on its own fine rows, then vpr_topk_merge — against the f64 order over the union of the shards' lists."""
    from vpr_amd import ops
    B, D, per, kc, k = 5, 128, 24, 12, 8
    q64, rows64 = gapped(dev, B, D, per, 50 + R, step=4e-3)
    g = torch.Generator(device=dev).manual_seed(R)
    filler = unit(torch.randn(93, D, device=dev, generator=g, dtype=torch.float64))
    all64 = torch.cat([rows64.view(B * per, D), filler])
    N = all64.shape[0]
    fine = all64[torch.randperm(N, device=dev, generator=g)].to(torch.bfloat16).contiguous()
    q = q64.to(torch.bfloat16)
    g8, gs = ops.quantize_fp8_rows(fine.float())
    q8, qs = ops.quantize_fp8_rows(q.float())
    cuts = [0, 31, N] if R == 2 else [0, 100, 107, N]        # uneven; one shard shorter than kc
    vs, is_, union = [], [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _, ci = ops.knn_topk_fp8(q8, qs, g8[lo:hi].contiguous(), gs[lo:hi].contiguous(), kc, lo)
        v, i = torch.ops.vpr.rerank_rows(q, ci, fine[lo:hi], lo, k)
        vs.append(v), is_.append(i), union.append(ci)
    mv, mi = torch.ops.vpr.topk_merge(torch.stack(vs), torch.stack(is_))
    S_t, A_t = exact_scores(q, fine)
    S, A = S_t.cpu().numpy(), A_t.cpu().numpy()
    cand = torch.cat(union, 1).cpu().numpy()
    rv, ri, _ = reference(S, cand, N, 0, k + 1)
    bound = gamma(D, False) * np.take_along_axis(A, np.maximum(ri, 0), 1)
    assert (ri >= 0).all() and (rv[:, :-1] - rv[:, 1:] > 4 * np.maximum(bound[:, :-1], bound[:, 1:])).all()
    assert np.array_equal(mi.cpu().numpy(), ri[:, :k])
    assert (np.abs(mv.cpu().numpy() - rv[:, :k]) <= bound[:, :k]).all()
    assert np.array_equal(ri[:, 0], S.argmax(1))             # and the union holds the fine top-1 of the whole gallery


def test_one_rank_collective_path_equals_local_path(rccl_one_rank):
    dev = rccl_one_rank
    local, q, fine = two_tier(dev, 4)
    coll, _, _ = two_tier(dev, 4, force_collectives=True)
    assert coll.collective and not local.collective
    for a, b in zip(local.search_reranked(q, 5, 16), coll.search_reranked(q, 5, 16)):
        assert torch.equal(bits(a), bits(b))
    for kw in (dict(rerank=16), dict(rerank=16, expand=(4, 1.0))):
        for a, b in zip(local.search_local_queries(q, 5, **kw), coll.search_local_queries(q, 5, **kw)):
            assert torch.equal(bits(a), bits(b))
    assert torch.equal(local.search_local_queries(q, 5, rerank=16)[1], local.search_reranked(q, 5, 16)[1])


def test_search_expanded_reranks_its_last_search_on_the_original_queries(dev):
    sg, q, fine = two_tier(dev, 5)
    k, kc = 6, 16
    v1, i1 = sg.search(q, k)
    e = sg.expand(q, v1, i1, 4, 2.0, 1.0)
    assert not torch.equal(e, q)
    _, ci = sg.search(e, kc)                                 # the last search, for kc
    want_v, want_i = torch.ops.vpr.rerank_rows(q, ci, fine, 0, k)                # ... re-ranked by hand on the caller's queries
    got_v, got_i = sg.search_expanded(q, k, 4, alpha=2.0, rerank=kc)
    assert torch.equal(got_i, want_i) and torch.equal(bits(got_v), bits(want_v))
    other_v, _ = torch.ops.vpr.rerank_rows(e, ci, fine, 0, k)                    # not on the expanded ones
    assert not torch.equal(bits(other_v), bits(got_v))
    plain = sg.search_expanded(q, k, 4, alpha=2.0)           # rerank None: as ever
    want = sg.search(e, k)
    assert torch.equal(plain[1], want[1]) and torch.equal(bits(plain[0]), bits(want[0]))


@pytest.mark.parametrize("collective", [False, True])
def test_graphed_two_tier_retrieval_equals_eager(rccl_one_rank, collective):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    N, B, k, kc = 1024, 16, 5, 16
    rng = np.random.default_rng(3)
    labels = np.stack([2e5 + rng.normal(0, 900, N), 1.4e5 + rng.normal(0, 1100, N), rng.uniform(0, 360, N),
                       rng.integers(0, 6, N).astype(np.float64)], 1)
    scaler = [2e5, 1.4e5, 900.0, 1100.0]
    sg, q0, _ = two_tier(dev, 6, force_collectives=collective)
    gr = GraphedRetrieval(sg, B, k, labels=labels, mode="weighted", temperature=0.05, scaler=scaler, rerank=kc)
    both = GraphedRetrieval(sg, B, k, expand=(4, 2.0), rerank=kc)
    plain = GraphedRetrieval(sg, B, k)
    assert sg.uncertified_queries() == 0
    for seed, q in enumerate((q0, q0.roll(3, 0).contiguous(), near_duplicates(7)[1].to(dev))):
        v_g, i_g = gr(q)
        v_g, i_g, p64, p4 = v_g.clone(), i_g.clone(), gr.pose64.clone(), gr.pose4.clone()
        v_e, i_e = sg.search_reranked(q, k, kc)
        assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e)), seed
        e64, e4, _, _ = torch.ops.vpr.retrieval_pose(v_e, i_e, gr.labels, "weighted", 0.05, None, 0.0, scaler)
        assert torch.equal(p64, e64) and torch.equal(p4, e4), seed
        v_b, i_b = both(q)
        v_x, i_x = sg.search_expanded(q, k, 4, alpha=2.0, rerank=kc)
        assert torch.equal(i_b, i_x) and torch.equal(bits(v_b), bits(v_x)), seed
        v_p, i_p = plain(q)
        v_1, i_1 = sg.search(q, k)
        assert torch.equal(i_p, i_1) and torch.equal(bits(v_p), bits(v_1)), seed
    assert not torch.equal(i_1, i_e)                         # the coarse order is not the fine one
    gr.close(), both.close(), plain.close()


def test_pipeline_with_rerank_equals_its_stages(dev):
    """ViT-S, as smoke() builds it, over an e4m3 gallery of noisy copies of the step's own descriptors: the eager and the graph
    path return the same bits, and both equal search_reranked on the step's bf16 descriptor."""
    import torch.nn as nn
    from vpr_amd import ops
    from vpr_amd.modules import DinoV2Salad, FusedGeoPoseHead
    from vpr_amd.pipeline import VPRGeoPosePipeline
    from vpr_amd.retrieval import ShardedGallery
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    ext.backbone.fold_layerscale()
    pos = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    ang = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    head = FusedGeoPoseHead(pos, ang, normalize=True)
    n, B, k, kc = 400, 2, 5, 16
    images = torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16)
    _, d16 = ext.features(images, want_bf16=True)
    g = torch.Generator(device=dev).manual_seed(2)
    fine = unit(torch.randn(n, 8448, device=dev, generator=g))
    fine[:24] = unit(d16.float().repeat_interleave(12, 0) + 0.45 * torch.randn(24, 8448, device=dev, generator=g) / 8448 ** 0.5)
    fine = fine.to(torch.bfloat16)
    g8, gs = ops.quantize_fp8_rows(fine.float())
    labels = np.stack([np.arange(n) * 10.0, np.arange(n) * 5.0, np.arange(n) % 360 * 1.0, np.arange(n) // 50 * 1.0], 1)
    mk = lambda: ShardedGallery(g8, n, scales=gs, fine_rows=fine)
    want_v, want_i = mk().search_reranked(d16, k, kc)
    outs = []
    for kw in (dict(), dict(graph_retrieval=True)):
        pipe = VPRGeoPosePipeline(ext, head, mk(), k, labels=labels, rerank=kc, **kw)
        for _ in range(2):
            out = pipe.step(images)
        torch.cuda.synchronize()
        assert torch.equal(out.topk_indices, want_i) and torch.equal(bits(out.topk_scores), bits(want_v)), kw
        rp = torch.ops.vpr.retrieval_pose(want_v, want_i, torch.from_numpy(labels).to(dev), "top1", 0.01, None, 0.0, None)[1]
        assert torch.equal(bits(out.retrieval_pose), bits(rp)), kw
        outs.append(out)
    for name in ("descriptors", "topk_scores", "topk_indices", "pose", "retrieval_pose"):
        assert torch.equal(getattr(outs[0], name), getattr(outs[1], name)), name
    base = VPRGeoPosePipeline(ext, head, mk(), k).step(images)                   # rerank None: the coarse search, as ever
    cv, ci = mk().search(d16, k)
    assert torch.equal(base.topk_indices, ci) and torch.equal(bits(base.topk_scores), bits(cv))


def test_retrieval_scores_with_rerank(dev, tmp_path, monkeypatch):
    """Generated images, an e4m3 gallery kept with its fine descriptors: rerank=None gives the coarse numbers; with rerank the
    result is retrieval_metrics of search_reranked on the same descriptor batches."""
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
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "gal"), batch_size=8, fp8=True, keep_fine=True, graph=False) == n_g
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "bare"), batch_size=8, fp8=True, graph=False) == n_g
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "bf16"), batch_size=8, keep_fine=True, graph=False) == n_g
    assert os.path.exists(tmp_path / "gal" / G.FINE_FILE) and not os.path.exists(tmp_path / "bare" / G.FINE_FILE)
    assert not os.path.exists(tmp_path / "bf16" / G.FINE_FILE)                   # a bf16 gallery is its own fine tier
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None, **kw):
        seen.append((q_local.clone(), k, expand, kw))
        return plain_search(self, q_local, k, expand, **kw)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run = lambda gal="gal", **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / gal), str(tmp_path / "labels_val.csv"),
                                                                      str(vdir), k=5, tau=10.0, batch_size=4, verbose=False, graph=False, **kw)
    res = run()
    assert all(kw == {} for *_, kw in seen) and res["topk_indices"][:, 0].tolist() == src
    assert run("bare")["topk_scores"].tobytes() == res["topk_scores"].tobytes()  # the file changes nothing until it is asked for
    with pytest.raises(ValueError, match="keep_fine"):
        run("bare", rerank=8)
    del seen[:]
    got = run(rerank=8)
    assert all(kw == {"rerank": 8} for *_, kw in seen)
    shard = G.load_gallery_shard(str(tmp_path / "gal"), dev, load_fine=True)
    assert shard.fine.shape == (n_g, 8448) and shard.fine.dtype == torch.bfloat16
    sg = ShardedGallery(shard.rows, shard.n_total, scales=shard.scales, exact_fallback=True, fine_rows=shard.fine)
    batches = [sg.search_reranked(d16, k, 8) for d16, k, _, _ in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    want = evaluate.retrieval_metrics(vals, idx, shard.labels, df[["latitude", "longitude"]].to_numpy(dtype=np.float64),
                                      df["Region_ID"].to_numpy(), df["angle"].to_numpy(dtype=np.float64), 10.0, "top1")
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[key].tobytes() == w.tobytes(), key
        else:
            assert got[key] == w, key
    assert got["topk_indices"][:, 0].tolist() == src and got["topk_scores"].tobytes() != res["topk_scores"].tobytes()
    # the fine scores are those of the bf16 gallery's own search of the same queries, to the f32 bound
    own = run("bf16")
    assert np.abs(got["topk_scores"][:, 0].astype(np.float64) - own["topk_scores"][:, 0]).max() <= 2 * gamma(8448, False)
    two = run("bf16", rerank=8)                              # a bf16 gallery re-ranks on its own rows
    assert two["topk_indices"][:, 0].tolist() == src
