"""GPU: vpr_query_expand / vpr_query_expand_finish (include/vpr_amd_expand.h) through torch.ops.vpr.query_expand[_finish],
ops.query_expand, ShardedGallery.expand / search_expanded, GraphedRetrieval(expand=...), gallery.augment_gallery and
evaluate.calculate_retrieval_scores(query_expansion=...).

Reference: `reference()` below restates the header's contract in numpy f64, with the kernel's own f32 weights
w_j = float32(pow(float64(vals_j), alpha)) (0 for a score that is not positive) and f64 everywhere else: the row values
(bf16, or scale * e4m3) are exact in f64.

Bound on out_f32, with A_d = |q_weight q_d| + sum_j |w_j row_j,d| and s the f64 sum:
    |out_f32[b, d] - ref| <= 2^-23 (n_use + R + 4) A_d / ||s||  +  2^-17 |ref|
  first term: one rounding per product, per add, per weight * scale product and per shard add, each u = 2^-24 of a partial
  sum that A_d bounds, with a factor 2; second term: the f32 norm of D <= 8448 squares in any reduction order (at most a few
  dozen u along any path of the tree, halved by the square root) plus the reciprocal, the square root and the final product.
out_bf16 is the round-to-nearest-even of out_f32 bit for bit; a query whose sum is zero or not finite comes back as q."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1
ALPHA_QW = [(0.0, 0.0), (1.0, 1.0), (3.0, 0.0), (0.0, 1.0), (1.0, 0.0), (3.0, 1.0)]


@pytest.fixture(scope="module", autouse=True)
def registered_ops(dev):
    from vpr_amd import torch_ops  # noqa: F401  registers torch.ops.vpr.*


# ------------------------------------------------------------------------------------------------------- inputs
def unit_rows(rng, n, D):
    g = rng.standard_normal((n, D))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def as_shard(dev, rows64, fp8):
    """f64 rows -> (device rows, device scales or None, the exact f64 values the kernel sees)."""
    from vpr_amd import ops
    x = torch.from_numpy(rows64).to(dev)
    if not fp8:
        r = x.to(torch.bfloat16)
        return r, None, r.double().cpu().numpy()
    r8, sc = ops.quantize_fp8_rows(x.float().contiguous())
    seen = r8.view(torch.float8_e4m3fn).float().double() * sc.double()[:, None]
    return r8, sc, seen.cpu().numpy()


def make_lists(rng, B, k, n_rows, lo=0.2, hi=0.9):
    """Descending positive scores; neighbours are distinct rows while the gallery has enough of them."""
    vals = np.sort(rng.uniform(lo, hi, (B, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    idx = np.stack([rng.permutation(n_rows)[:k] if k <= n_rows else rng.integers(0, n_rows, k) for _ in range(B)]).astype(np.int32)
    return vals, idx


def noisy_queries(rng, seen, idx, n_use, noise=0.3):
    """Each query = a noisy copy of the mean of the neighbours it will use, so the expanded sum is not small; bf16."""
    D = seen.shape[1]
    q = np.stack([seen[idx[b, :n_use]].mean(0) for b in range(idx.shape[0])])
    q = q / np.linalg.norm(q, axis=1, keepdims=True) + noise * rng.standard_normal(q.shape) / np.sqrt(D)
    return torch.from_numpy(q / np.linalg.norm(q, axis=1, keepdims=True)).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- reference
def weights_f32(vals, alpha):
    v = vals.astype(np.float64)
    with np.errstate(all="ignore"):
        w = np.power(np.where(vals > 0, v, 1.0), alpha)
    return np.where(vals > 0, w, 0.0).astype(np.float32)


def reference(q, vals, idx, seen, n_use, alpha, q_weight, index_base=0):
    """q bf16 [B, D] (host), vals / idx numpy [B, k], seen f64 [N, D] = the rows as the kernel sees them, global row r of the
    gallery at seen[r - index_base].  Returns ref [B, D] (q where the sum is zero or not finite), A [B, D], ||s|| [B], ok [B]."""
    q64 = q.double().numpy()
    N = seen.shape[0]
    rel = idx[:, :n_use].astype(np.int64) - index_base
    live = (rel >= 0) & (rel < N)
    w = np.where(live, weights_f32(vals[:, :n_use], alpha), np.float32(0)).astype(np.float64)
    s, A = q_weight * q64, np.abs(q_weight * q64)
    with np.errstate(all="ignore"):
        for b in range(q64.shape[0]):
            use = np.nonzero(w[b] != 0)[0]
            if len(use):
                g = seen[rel[b, use]]
                s[b] = s[b] + w[b, use] @ g
                A[b] = A[b] + np.abs(w[b, use]) @ np.abs(g)
        norm = np.sqrt((s * s).sum(1))
        ok = np.isfinite(norm) & (norm > 0)
        ref = np.where(ok[:, None], s / norm[:, None], q64)
    return ref, A, norm, ok


def check(out_f32, out_bf16, q, ref, A, norm, ok, n_use, R, what=""):
    out = out_f32.double().cpu().numpy()
    assert torch.equal(out_bf16, out_f32.to(torch.bfloat16)), what             # RNE of out_f32, bit for bit
    if (~ok).any():                                                             # fallback rows: q itself
        kept = torch.from_numpy(~ok)
        assert torch.equal(out_bf16.cpu()[kept].view(torch.int16), q[kept].view(torch.int16)), what
        assert np.array_equal(out[~ok], q.double().numpy()[~ok]), what
    if ok.any():
        with np.errstate(all="ignore"):
            bound = 2.0 ** -23 * (n_use + R + 4) * A / norm[:, None] + 2.0 ** -17 * np.abs(ref)
        err = np.abs(out - ref)
        worst = float((err[ok] / np.maximum(bound[ok], 1e-300)).max())
        print(f"{what}: max err / bound = {worst:.3f}")
        assert worst <= 1.0, (what, worst)
        assert np.abs(np.linalg.norm(out[ok], axis=1) - 1.0).max() < 2.0 ** -16, what   # unit rows


def run_one(dev, q, vals, idx, shard, index_base, n_use, alpha, q_weight):
    """Single shard through the two torch ops; returns (out_f32, out_bf16)."""
    rows, sc, _ = shard
    part = torch.ops.vpr.query_expand(q.to(dev), torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev), rows, sc,
                                      index_base, n_use, alpha, q_weight, True)
    return torch.ops.vpr.query_expand_finish(part[None].contiguous(), q.to(dev))


# -------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("D", [64, 192, 8448])
@pytest.mark.parametrize("fp8", [False, True])
def test_numerics_against_f64(dev, fp8, D, B):
    """k in {1, 10, 64, 128} x n_use in {1, k}, each with the next two of the six (alpha, q_weight) pairs in rotation; a
    40-row shard at index_base 1000."""
    rng = np.random.default_rng(1000 * D + 10 * B + fp8)
    n_rows, base = 40, 1000
    shard = as_shard(dev, unit_rows(rng, n_rows, D), fp8)
    turn = 0
    for k in (1, 10, 64, 128):
        for n_use in sorted({1, k}):
            vals, idx = make_lists(rng, B, k, n_rows)
            q = noisy_queries(rng, shard[2], idx, n_use)
            for _ in range(2):
                alpha, qw = ALPHA_QW[turn % 6]
                turn += 1
                o32, o16 = run_one(dev, q, vals, idx + base, shard, base, n_use, alpha, qw)
                ref, A, norm, ok = reference(q, vals, idx + base, shard[2], n_use, alpha, qw, index_base=base)
                assert ok.all()
                check(o32, o16, q, ref, A, norm, ok, n_use, 1, f"fp8={fp8} D={D} B={B} k={k} n_use={n_use} alpha={alpha} qw={qw}")
    # the one-call form (partial in the cached workspace, finish in the same call) is the same two kernels
    from vpr_amd import ops
    a32, a16 = ops.query_expand(q.to(dev), torch.from_numpy(vals).to(dev), torch.from_numpy(idx + base).to(dev), shard[0], shard[1],
                                base, n_use, alpha, qw, True, finish=True)
    assert torch.equal(a32, o32) and torch.equal(a16, o16)


@pytest.mark.parametrize("fp8", [False, True])
def test_foreign_indices_are_never_read_and_the_weight_rules(dev, fp8):
    """idx holding -1, index_base + n_local, INT32_MAX, index_base - 1 and rows of other shards: nothing is added for them.
    The shard is the tail of its allocation and the rows before it are NaN, so a read one row before or after the shard
    would not give the reference's numbers.  Scores that are negative, zero or NaN weigh 0 (their rows hold Inf here: a 0
    weight must not meet them), and columns j >= n_use are ignored (they point at the Inf rows, with large scores)."""
    rng = np.random.default_rng(7 + fp8)
    D, B, k, n_use, base, n_local, n_before = 192, 37, 10, 6, 500, 24, 8
    rows64 = unit_rows(rng, n_before + n_local, D)
    whole = as_shard(dev, rows64, fp8)
    seen = whole[2][n_before:].copy()
    poison = [n_local - 1, n_local - 2]                                  # two rows only dead neighbours point at
    if fp8:
        whole[0][:n_before] = 0x7f                                       # e4m3 NaN bytes in front of the shard
        whole[1][[n_before + p for p in poison]] = float("inf")
    else:
        whole[0][:n_before] = float("nan")
        whole[0][[n_before + p for p in poison]] = float("inf")
    seen[poison] = np.inf
    shard = (whole[0][n_before:], None if whole[1] is None else whole[1][n_before:], seen)
    assert shard[0].data_ptr() + shard[0].numel() * shard[0].element_size() == \
        whole[0].data_ptr() + whole[0].numel() * whole[0].element_size()          # the shard ends where its allocation ends
    vals, idx = make_lists(rng, B, k, n_local - 2)
    idx += base
    foreign = [-1, base + n_local, I32_MAX, base - 1, 0, base + n_local + 3, -I32_MAX - 1]
    for b in range(B):
        for j in rng.permutation(n_use)[:b % 4]:                         # up to three foreign neighbours among the used ones
            idx[b, j] = foreign[int(rng.integers(0, len(foreign)))]
        idx[b, n_use:] = base + poison[b % 2]                            # ignored columns
        vals[b, n_use:] = 50.0
    for b, (j, v) in enumerate([(0, 0.0), (1, -0.3), (2, -0.0), (3, float("nan")), (4, -np.inf)]):
        vals[b + 5, j], idx[b + 5, j] = v, base + poison[0]              # weight 0 on a local row full of Inf
    idx[20, :n_use] = foreign[:n_use]                                    # a query with no local neighbour at all
    q = noisy_queries(rng, shard[2], np.where((idx >= base) & (idx < base + n_local - 2), idx - base, 0), n_use)
    for alpha, qw in ((1.0, 1.0), (3.0, 0.0), (0.0, 1.0)):
        o32, o16 = run_one(dev, q, vals, idx, shard, base, n_use, alpha, qw)
        ref, A, norm, ok = reference(q, vals, idx, shard[2], n_use, alpha, qw, index_base=base)
        assert ok.sum() >= B - 1 and ok[20] == (qw != 0)
        check(o32, o16, q, ref, A, norm, ok, n_use, 1, f"foreign fp8={fp8} alpha={alpha} qw={qw}")


@pytest.mark.parametrize("fp8", [False, True])
def test_fallback_to_the_query(dev, fp8):
    rng = np.random.default_rng(17 + fp8)
    D, B, k, n_rows = 8448, 5, 10, 30
    whole = as_shard(dev, unit_rows(rng, n_rows, D), fp8)
    vals, idx = make_lists(rng, B, k, n_rows - 2)
    q = noisy_queries(rng, whole[2], idx, k)
    # all neighbours dead and q_weight = 0: the output is q exactly
    dead = np.full_like(idx, -1)
    o32, o16 = run_one(dev, q, vals, dead, whole, 0, k, 3.0, 0.0)
    assert torch.equal(o16.cpu().view(torch.int16), q.view(torch.int16)) and torch.equal(o32.cpu(), q.float())
    o32, o16 = run_one(dev, q, np.zeros_like(vals), idx, whole, 0, k, 3.0, 0.0)            # every weight zero
    assert torch.equal(o16.cpu().view(torch.int16), q.view(torch.int16)) and torch.equal(o32.cpu(), q.float())
    # Inf / NaN in a contributing row: q for that query only, its batch neighbours keep their bits
    clean32, clean16 = run_one(dev, q, vals, idx, whole, 0, k, 1.0, 1.0)
    for victim, row, value, col in ((1, n_rows - 1, float("inf"), 8447), (3, n_rows - 2, float("nan"), 5000)):
        rows = whole[0].clone()
        sc = None if whole[1] is None else whole[1].clone()
        if fp8 and value != value:
            rows[row, col] = 0x7f                                                          # the e4m3 NaN byte
        elif fp8:
            sc[row] = value                                                                # e4m3 has no Inf: the scale carries it
        else:
            rows[row, col] = value
        idx2 = idx.copy()
        idx2[victim, 4] = row
        o32, o16 = run_one(dev, q, vals, idx2, (rows, sc, None), 0, k, 1.0, 1.0)
        others = [b for b in range(B) if b != victim]
        assert torch.equal(o16[victim].cpu().view(torch.int16), q[victim].view(torch.int16))
        assert torch.equal(o32[victim].cpu(), q[victim].float())
        assert torch.equal(o32[others], clean32[others]) and torch.equal(o16[others], clean16[others])
        assert not torch.equal(clean16[victim].cpu().view(torch.int16), q[victim].view(torch.int16))


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("fp8", [False, True])
def test_sharded_partials_sum_to_the_whole(dev, fp8, R):
    """One gallery cut into R shards at uneven boundaries, add_query on shard 0 only, partials stacked in shard order: within
    the bound (with that R) of the unsharded f64 result — a neighbour counted twice or not at all would miss it by far."""
    rng = np.random.default_rng(31 * R + fp8)
    D, B, k, n_use, N = 192, 37, 10, 10, 61
    whole = as_shard(dev, unit_rows(rng, N, D), fp8)
    cuts = [0] + sorted(rng.choice(np.arange(1, N), R - 1, replace=False).tolist()) + [N]
    vals, idx = make_lists(rng, B, k, N)
    idx[::5, 7:] = -1                                                    # short lists too
    q = noisy_queries(rng, whole[2], np.where(idx >= 0, idx, 0), 7)
    qd, vd, idd = q.to(dev), torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    for alpha, qw in ((3.0, 1.0), (1.0, 0.0)):
        parts, counted = [], np.zeros_like(idx)
        for r in range(R):
            lo, hi = cuts[r], cuts[r + 1]
            rows = whole[0][lo:hi].contiguous()
            sc = None if whole[1] is None else whole[1][lo:hi].contiguous()
            parts.append(torch.ops.vpr.query_expand(qd, vd, idd, rows, sc, lo, n_use, alpha, qw, r == 0))
            counted += (idx >= lo) & (idx < hi)
        assert np.array_equal(counted, (idx >= 0).astype(counted.dtype))     # the shards partition the live neighbours
        o32, o16 = torch.ops.vpr.query_expand_finish(torch.stack(parts), qd)
        ref, A, norm, ok = reference(q, vals, idx, whole[2], n_use, alpha, qw)
        assert ok.all()
        check(o32, o16, q, ref, A, norm, ok, n_use, R, f"shards R={R} fp8={fp8} alpha={alpha}")
        if R > 1:                                                       # a shard's partial alone is not the answer
            assert not torch.equal(torch.ops.vpr.query_expand_finish(parts[0][None].contiguous(), qd)[0], o32)


@pytest.mark.parametrize("D", [192, 8448])
@pytest.mark.parametrize("fp8", [False, True])
def test_a_query_depends_on_its_own_row_only(dev, fp8, D):
    rng = np.random.default_rng(5 * D + fp8)
    B, k, n_rows = 37, 10, 33
    shard = as_shard(dev, unit_rows(rng, n_rows, D), fp8)
    vals, idx = make_lists(rng, B, k, n_rows)
    q = noisy_queries(rng, shard[2], idx, k)
    o32, o16 = run_one(dev, q, vals, idx, shard, 0, k, 3.0, 1.0)
    again32, again16 = run_one(dev, q, vals, idx, shard, 0, k, 3.0, 1.0)
    assert torch.equal(o32, again32) and torch.equal(o16, again16)           # two runs, the same bits
    for b in (range(B) if D == 192 else (0, 17, 36)):
        s32, s16 = run_one(dev, q[b:b + 1], vals[b:b + 1], idx[b:b + 1], shard, 0, k, 3.0, 1.0)
        assert torch.equal(s32[0], o32[b]) and torch.equal(s16[0], o16[b]), b
    perm = rng.permutation(B)                                                # any position in the batch
    at = torch.from_numpy(perm)
    p32, p16 = run_one(dev, q[at], vals[perm], idx[perm], shard, 0, k, 3.0, 1.0)
    assert torch.equal(p32, o32[at.to(dev)]) and torch.equal(p16, o16[at.to(dev)])


@pytest.mark.parametrize("fp8", [False, True])
def test_closed_form_second_pass(dev, fp8):
    """q = e0; rows r0 = (e0 + e1) / sqrt 2, r1 = e3, r2 = (e1 + e4) / sqrt 2, r3 = e5, then further basis vectors.  The plain
    search gives [0, 1] (the zeros tie, the lower index wins); expanded with n_use = 1, alpha = 1, q_weight = 1 the query is
    (1.5 e0 + 0.5 e1) / sqrt 2.5, and the second search gives [0, 2] with scores 2 / sqrt 5 and 1 / (2 sqrt 5).
    D = 64 for bf16 rows; the e4m3 search takes D % 128 == 0, so that shard has D = 128 (the same vectors, zero-extended).
    Tolerance: the first row (whose score is the weight), the expanded query and the row it is scored against are each
    rounded once to bf16 (8 significant bits, 2^-8 relative) before the second score is formed — three roundings, under
    2^-6; for the e4m3 engine the expanded query is quantised to 4 significant bits, 2^-4 relative on its smaller component,
    which carries the whole second score."""
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    D, N = (128, 8) if fp8 else (64, 8)
    rows = torch.zeros(N, D, dtype=torch.float64)
    h = 0.5 ** 0.5
    rows[0, 0] = rows[0, 1] = rows[2, 1] = rows[2, 4] = h
    rows[1, 3] = rows[3, 5] = 1.0
    for r in range(4, N):
        rows[r, r + 2] = 1.0
    q = torch.zeros(1, D, dtype=torch.bfloat16, device=dev)
    q[0, 0] = 1.0
    if fp8:
        r8, sc = ops.quantize_fp8_rows(rows.float().to(dev))
        sg = ShardedGallery(r8, N, scales=sc)
    else:
        sg = ShardedGallery(rows.to(dev).to(torch.bfloat16), N)
    v, i = sg.search(q, 2)
    assert i.tolist() == [[0, 1]] and v[0, 1] == 0.0 and abs(float(v[0, 0]) - h) < 2.0 ** -8
    v2, i2 = sg.search_expanded(q, 2, 1, alpha=1.0, q_weight=1.0)
    tol = 2.0 ** -4 if fp8 else 2.0 ** -6
    assert i2.tolist() == [[0, 2]]
    for got, want in zip(v2[0].tolist(), (2 / 5 ** 0.5, 1 / (2 * 5 ** 0.5))):
        print(f"fp8={fp8}: score {got} against {want}")
        assert abs(got - want) <= tol * want


def _clustered(dev, N, D, B, seed, noise=0.5):
    """A gallery of noisy copies of N // 8 centres (so neighbours score well above 0) and queries near some of its rows."""
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(max(N // 8, 1), D, device=dev, generator=g)
    gal = centres.repeat_interleave(8, 0)[:N] + noise * torch.randn(N, D, device=dev, generator=g)
    gal = torch.nn.functional.normalize(gal, dim=1)
    pos = torch.randint(0, N, (B,), device=dev, generator=g)
    q = torch.nn.functional.normalize(gal[pos] + 0.3 * torch.randn(B, D, device=dev, generator=g) / D ** 0.5, dim=1)
    return gal, q.to(torch.bfloat16)


def _gallery(gal, fp8, **kw):
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    if fp8:
        g8, gs = ops.quantize_fp8_rows(gal)
        return ShardedGallery(g8, gal.shape[0], 0, 1, scales=gs, **kw)
    return ShardedGallery(gal.to(torch.bfloat16), gal.shape[0], 0, 1, **kw)


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


@pytest.mark.parametrize("fp8", [False, True])
def test_search_expanded_is_search_of_expand_of_search(dev, fp8):
    gal, q = _clustered(dev, 3000, 8448, 16, 40 + fp8)
    sg = _gallery(gal, fp8)
    v1, i1 = sg.search(q, 10)
    e = sg.expand(q, v1, i1, 5, 2.0, 0.5)
    assert e.dtype == torch.bfloat16 and e.shape == q.shape and not torch.equal(e, q)
    want_v, want_i = sg.search(e, 10)
    got_v, got_i = sg.search_expanded(q, 10, 5, alpha=2.0, q_weight=0.5)
    assert torch.equal(got_i, want_i) and torch.equal(got_v, want_v)
    assert not torch.equal(got_v, v1)                                        # the second pass is another search
    v3, i3 = sg.search(sg.expand(e, want_v, want_i, 5, 2.0, 0.5), 10)        # rounds = 2: expand the expanded query again
    r_v, r_i = sg.search_expanded(q, 10, 5, alpha=2.0, q_weight=0.5, rounds=2)
    assert torch.equal(r_i, i3) and torch.equal(r_v, v3)
    # against the restatement: the expanded query is the bf16 rounding of a vector within the bound
    seen = (sg.rows.view(torch.float8_e4m3fn).float().double() * sg.scales.double()[:, None] if fp8 else sg.rows.double()).cpu().numpy()
    ref, A, norm, ok = reference(q.cpu(), v1.cpu().numpy(), i1.cpu().numpy(), seen, 5, 2.0, 0.5)
    bound = 2.0 ** -23 * (5 + 1 + 4) * A / norm[:, None] + 2.0 ** -17 * np.abs(ref)
    assert ok.all() and (np.abs(e.double().cpu().numpy() - ref) <= bound + 2.0 ** -8 * (np.abs(ref) + bound)).all()      # + one rounding to bf16


@pytest.mark.parametrize("fp8", [False, True])
def test_collective_path_equals_local_path(rccl_one_rank, fp8):
    dev = rccl_one_rank
    gal, q = _clustered(dev, 3000, 8448, 16, 50 + fp8)
    local, coll = _gallery(gal, fp8), _gallery(gal, fp8, force_collectives=True)
    assert coll.collective and not local.collective
    v1, i1 = local.search(q, 10)
    e_l, e_c = local.expand(q, v1, i1, 10, 3.0, 1.0), coll.expand(q, v1, i1, 10, 3.0, 1.0)
    assert torch.equal(e_l, e_c)
    for a, b in zip(local.search_expanded(q, 10, 10), coll.search_expanded(q, 10, 10)):
        assert torch.equal(a, b)
    for a, b in zip(local.search_local_queries(q, 10, (4, 1.0)), coll.search_local_queries(q, 10, {"n_use": 4, "alpha": 1.0})):
        assert torch.equal(a, b)


@pytest.mark.parametrize("collective", [False, True])
@pytest.mark.parametrize("fp8", [False, True])
def test_graphed_two_pass_retrieval_equals_eager(rccl_one_rank, fp8, collective):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    N, B, k = 4000, 16, 10
    gal, _ = _clustered(dev, N, 8448, B, 60 + fp8)
    rng = np.random.default_rng(3)
    labels = np.stack([2e5 + rng.normal(0, 900, N), 1.4e5 + rng.normal(0, 1100, N), rng.uniform(0, 360, N),
                       rng.integers(0, 6, N).astype(np.float64)], 1)
    sg = _gallery(gal, fp8, force_collectives=collective)
    expand = {"n_use": 5, "alpha": 3.0, "q_weight": 1.0}
    gr = GraphedRetrieval(sg, B, k, labels=labels, mode="weighted", temperature=0.05, scaler=[2e5, 1.4e5, 900.0, 1100.0],
                          expand=expand)
    plain = GraphedRetrieval(sg, B, k)                                       # no expand: today's one-pass graph
    assert sg.uncertified_queries() == 0                                     # the warm-ups are not searches
    for trial in range(3):
        g = torch.Generator(device=dev).manual_seed(300 + trial)
        pos = torch.randint(0, N, (B,), device=dev, generator=g)
        q = torch.nn.functional.normalize(gal[pos] + 0.004 * torch.randn(B, 8448, device=dev, generator=g), dim=1).to(torch.bfloat16)
        v_g, i_g = gr(q)
        v_g, i_g, p64, p4 = v_g.clone(), i_g.clone(), gr.pose64.clone(), gr.pose4.clone()
        v_e, i_e = sg.search_expanded(q, k, **expand)
        assert torch.equal(i_g, i_e) and torch.equal(v_g, v_e), trial
        e64, e4, _, _ = torch.ops.vpr.retrieval_pose(v_e, i_e, gr.labels, "weighted", 0.05, None, 0.0, [2e5, 1.4e5, 900.0, 1100.0])
        assert torch.equal(p64, e64) and torch.equal(p4, e4), trial
        v_p, i_p = plain(q)
        v_1, i_1 = sg.search(q, k)
        assert torch.equal(i_p, i_1) and torch.equal(v_p, v_1), trial
        assert not torch.equal(v_1, v_e)
    gr.close(), plain.close()


@pytest.mark.parametrize("fp8", [False, True])
def test_augment_gallery(dev, fp8):
    """96 rows, batch 40: two full batches and a last one of 16 rows padded with 24 copies of row 0.  The restatement takes
    the top-k lists of the same padded batches (the search is the tested kNN; its lists are the expansion's input)."""
    from vpr_amd import gallery as G, ops
    N, D, n_use, alpha, batch = 96, 256, 5, 3.0, 40
    gal, _ = _clustered(dev, N, D, 1, 70 + fp8, noise=0.6)
    sg = _gallery(gal, fp8)
    got = G.augment_gallery(sg, n_use, alpha, batch)
    seen_t = sg.rows.view(torch.float8_e4m3fn).float() * sg.scales[:, None] if fp8 else sg.rows.float()
    seen = seen_t.double().cpu().numpy()
    queries = seen_t.to(torch.bfloat16)
    ref = np.empty((N, D))
    bound = np.empty((N, D))
    for lo in range(0, N, batch):
        sel = torch.zeros(batch, dtype=torch.long, device=dev)
        sel[:min(batch, N - lo)] = torch.arange(lo, min(lo + batch, N), device=dev)
        qb = queries[sel].contiguous()
        v, i = sg.search(qb, n_use)
        assert (i[:, 0] == sel.to(torch.int32)).all()                        # every row finds itself first
        r, A, norm, ok = reference(qb.cpu(), v.cpu().numpy(), i.cpu().numpy(), seen, n_use, alpha, 0.0)
        assert ok.all()
        m = min(batch, N - lo)
        ref[lo:lo + m] = r[:m]
        bound[lo:lo + m] = (2.0 ** -23 * (n_use + 1 + 4) * A / norm[:, None] + 2.0 ** -17 * np.abs(r))[:m]
    bf16_bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)                   # one rounding to bf16 (8 significant bits)
    if not fp8:
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N, D)
        out = got.double().cpu().numpy()
        assert (np.abs(out - ref) <= bf16_bound).all()
        assert np.abs(np.linalg.norm(out, axis=1) - 1.0).max() <= 2.0 ** -8
        assert not torch.equal(got, sg.rows)
    else:
        g8, gs = got
        assert g8.dtype == torch.uint8 and tuple(g8.shape) == (N, D) and gs.dtype == torch.float32 and tuple(gs.shape) == (N,)
        out = (g8.view(torch.float8_e4m3fn).float().double() * gs.double()[:, None]).cpu().numpy()
        # the restatement quantised the same way: f64 -> bf16 -> quantize_fp8_rows.  Where got and want round a value to
        # different bf16 neighbours, the e4m3 codes may differ by one step: half a step each side of the bf16 value, i.e.
        # 2^-4 relative for normal codes and 2^-10 of the scale (half the subnormal step 2^-9) below them.
        w8, ws = ops.quantize_fp8_rows(torch.from_numpy(ref).to(dev).to(torch.bfloat16).float())
        want = (w8.view(torch.float8_e4m3fn).float().double() * ws.double()[:, None]).cpu().numpy()
        step = np.maximum(2.0 ** -4 * np.abs(ref), 2.0 ** -10 * gs.double().cpu().numpy()[:, None]) + bf16_bound
        assert (np.abs(out - ref) <= step).all()
        assert (out == want).mean() > 0.95 and (np.abs(out - want) <= 2 * step).all()
        assert np.abs(np.linalg.norm(out, axis=1) - 1.0).max() <= 2.0 ** -4
    assert sg.uncertified_queries() == 0


def test_retrieval_scores_with_query_expansion(dev, tmp_path, monkeypatch):
    """The end-to-end case of test_golden_gpu.py::test_retrieval_evaluation_entry_points (bf16 gallery): query_expansion=None
    gives its numbers; with expansion the result is retrieval_metrics of search_expanded on the same descriptor batches."""
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
    assert evaluate.build_gallery_from_images(ext, str(tmp_path / "labels_train.csv"), str(gdir), str(tmp_path / "gal"), batch_size=8) == n_g
    seen = []                                                                # the descriptor batches the evaluation searched
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None):
        seen.append((q_local.clone(), k, expand))
        return plain_search(self, q_local, k, expand)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run = lambda **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "labels_val.csv"), str(vdir),
                                                           k=5, tau=10.0, batch_size=4, verbose=False, **kw)
    res = run(query_expansion=None)
    assert all(e is None for _, _, e in seen)
    assert res["topk_indices"][:, 0].tolist() == src
    assert np.allclose(res["pose"][:, 0], lat[src]) and np.allclose(res["pose"][:, 1], lon[src]) and np.allclose(res["pose"][:, 2], ang[src])
    assert res["final_loss"] == pytest.approx(0.5 * (9.0 + 16.0)) and res["maae"] == pytest.approx(5.0)
    assert res["recall_at_1_tau"] == 1.0 and res["recall_at_1_region"] == 1.0 and res["uncertified_queries"] == 0
    default = run()
    assert default["topk_scores"].tobytes() == res["topk_scores"].tobytes() and default["final_loss"] == res["final_loss"]
    del seen[:]
    expansion = {"n_use": 3, "alpha": 2.0, "q_weight": 1.0}
    got = run(query_expansion=expansion)
    shard = G.load_gallery_shard(str(tmp_path / "gal"), dev)
    sg = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True)
    batches = [sg.search_expanded(d16, k, **expansion) for d16, k, _ in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    want = evaluate.retrieval_metrics(vals, idx, shard.labels, df[["latitude", "longitude"]].to_numpy(dtype=np.float64),
                                      df["Region_ID"].to_numpy(), df["angle"].to_numpy(dtype=np.float64), 10.0, "top1")
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[key].tobytes() == w.tobytes(), key
        else:
            assert got[key] == w, key
    assert got["topk_scores"].tobytes() != res["topk_scores"].tobytes()                  # the second pass is another search
