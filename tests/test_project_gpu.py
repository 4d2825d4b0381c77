"""GPU: vpr_project_rows (include/vpr_amd_project.h) through ops.project_rows / torch.ops.vpr.project_rows against an f64
restatement on the same bf16 operands, on both routes; then the retrieval wiring on recipe R: fit_projection ->
project_gallery -> ShardedGallery(projection=) -> GraphedRetrieval / VPRGeoPosePipeline / the evaluation entry points.

Bounds (u = 2^-24, the f32 unit rounding of the arithmetic contract of vpr_amd.h):
  delta_j = 1.1 u (D + 66) (|c_j| + sum_k |x_k P_jk|): every product is exact, so z_j is an f32 sum of D + 1 terms in some order
  with up to 64 slabs.  normalize = 0: |out - ref| <= delta_j.
  normalize = 1: |out_j - ref_j| <= 1.25 [delta_j / |z| + |ref_j| (|delta|_2 / |z| + (d + 16) u)] — first order in delta / |z|,
  which the test asserts to be at most 2^-6 on its own inputs before it uses the bound.
"""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DS, DOUTS = (64, 192, 8448), (64, 128, 512)
ROWS = (1, 3, 64, 65, 127, 128, 129, 257)          # the route boundary is 128: both sides of it, and of the 64-row tile
MAX_ROWS = max(ROWS)
WORST = {}                                        # (normalize) -> largest error / tolerance seen, printed for DESIGN.md §3.7


@pytest.fixture(scope="module", autouse=True)
def registered_ops(dev):
    from vpr_amd import torch_ops  # noqa: F401  registers torch.ops.vpr.*


# ------------------------------------------------------------------------------------------------------- inputs
_CASES = {}


def case(dev, D, d):
    """Operands of one (D, d), made once and never changed: P bf16 with orthonormal-ish rows (N(0, 1/D) entries), c f32, x bf16
    [MAX_ROWS, D] unit rows that lie mostly in the span of P (a random combination of its rows plus half as much noise), as
    descriptors lie in the span of their principal axes — so |z| is of order 1.  With them the f64 restatement:
    z = c + x P^T, A = |c| + |x| |P|^T, both from the bf16 values."""
    key = (D, d)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * D + d)
        P = torch.from_numpy(rng.standard_normal((d, D)) / np.sqrt(D)).to(torch.bfloat16)
        c = torch.from_numpy(0.02 * rng.standard_normal(d)).to(torch.float32)
        x = (rng.standard_normal((MAX_ROWS, d)) / np.sqrt(d)) @ P.double().numpy() + 0.5 * rng.standard_normal((MAX_ROWS, D)) / np.sqrt(D)
        x = torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(torch.bfloat16)
        x64, P64, c64 = x.double().numpy(), P.double().numpy(), c.double().numpy()
        z = c64 + x64 @ P64.T
        A = np.abs(c64) + np.abs(x64) @ np.abs(P64).T
        _CASES[key] = dict(x=x.to(dev), P=P.to(dev), c=c.to(dev), z=z, A=A)
    return _CASES[key]


def tolerances(z, A, D, d, normalize):
    """(reference, elementwise tolerance) of the f32 output for the rows of z / A."""
    delta = 1.1 * U32 * (D + 66) * A
    if not normalize:
        return z, delta
    norm = np.linalg.norm(z, axis=1, keepdims=True)
    dn = np.linalg.norm(delta, axis=1, keepdims=True)
    assert (dn <= 2.0 ** -6 * norm).all(), "the first-order bound needs |delta| <= 2^-6 |z| on the test's own inputs"
    ref = z / norm
    return ref, 1.25 * (delta / norm + np.abs(ref) * (dn / norm + (d + 16) * U32))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_bf16(o16, o32, ref, tol):
    """out_bf16 is the RNE bf16 of out_f32 bit for bit.  Against the reference: rounding is monotone, so it lies between
    bf16(ref - tol) and bf16(ref + tol) — it IS bf16(ref) wherever ref is further than the f32 tolerance from a bf16 rounding
    boundary (there the two ends coincide), and one of the two neighbours elsewhere."""
    assert torch.equal(bits(o16), bits(o32.to(torch.bfloat16)))
    rnd = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().numpy()
    slack = 2.0 ** -40 * np.abs(ref)               # the reference's own f64 rounding
    lo, hi = rnd(ref - tol - slack), rnd(ref + tol + slack)
    got = o16.double().cpu().numpy()
    assert ((lo <= got) & (got <= hi)).all()
    forced = lo == hi
    assert (got[forced] == rnd(ref)[forced]).all()
    return float(forced.mean())


# ------------------------------------------------------------------------------------------------ against f64
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", DOUTS)
@pytest.mark.parametrize("D", DS)
def test_against_f64(dev, D, d, rows):
    from vpr_amd import _lib, ops
    k = case(dev, D, d)
    assert ops.project_route(rows, D, d) == (0 if rows <= _lib.PROJECT_STREAM_MAX_ROWS else 1)
    x = k["x"][:rows].contiguous()
    for normalize in (0, 1):
        o32, o16 = ops.project_rows(x, k["P"], k["c"], bool(normalize), want_f32=True, want_bf16=True)
        assert o32.shape == o16.shape == (rows, d) and o32.dtype == torch.float32 and o16.dtype == torch.bfloat16
        ref, tol = tolerances(k["z"][:rows], k["A"][:rows], D, d, normalize)
        err = np.abs(o32.double().cpu().numpy() - ref)
        ratio = float((err / tol).max())
        WORST[normalize] = max(WORST.get(normalize, 0.0), ratio)
        print(f"D={D} d={d} rows={rows} normalize={normalize}: worst error / tolerance {ratio:.4f} (so far {WORST[normalize]:.4f})")
        assert (err <= tol).all()
        check_bf16(o16, o32, ref, tol)
        if normalize:
            assert np.abs(np.linalg.norm(o32.double().cpu().numpy(), axis=1) - 1.0).max() <= (d + 16) * U32
        only16 = ops.project_rows(x, k["P"], k["c"], bool(normalize))                     # either output may be absent
        only32 = ops.project_rows(x, k["P"], k["c"], bool(normalize), want_f32=True, want_bf16=False)
        assert only16[0] is None and only32[1] is None
        assert torch.equal(bits(only16[1]), bits(o16)) and torch.equal(bits(only32[0]), bits(o32))
        t32, t16 = torch.ops.vpr.project_rows(x, k["P"], k["c"], bool(normalize))
        assert torch.equal(bits(t32), bits(o32)) and torch.equal(bits(t16), bits(o16))


# -------------------------------------------------------------------- row independence, reproducibility, strides
@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("D", [192, 8448])
def test_a_row_depends_on_itself_and_the_route_only(dev, D, d):
    from vpr_amd import _lib, ops
    k = case(dev, D, d)
    bound = _lib.PROJECT_STREAM_MAX_ROWS
    run = lambda x: ops.project_rows(x, k["P"], k["c"], True, want_f32=True)
    x = k["x"]
    for full, others in ((bound, (1, 3, 64, 65, bound - 1)), (MAX_ROWS, (bound + 1, 200))):     # route 0, then route 1
        route = ops.project_route(full, D, d)
        w32, w16 = run(x[:full].contiguous())
        a32, a16 = run(x[:full].contiguous())
        assert torch.equal(bits(a32), bits(w32)) and torch.equal(bits(a16), bits(w16))           # run to run
        for rows in others:
            assert ops.project_route(rows, D, d) == route
            g32, g16 = run(x[:rows].contiguous())                                                # its bits do not depend on rows
            assert torch.equal(bits(g32), bits(w32[:rows])) and torch.equal(bits(g16), bits(w16[:rows]))
        lo = 37 if route == 0 else 3                                                             # nor on its position
        g32, _ = run(x[lo:full].contiguous())
        assert torch.equal(bits(g32), bits(w32[lo:]))
        perm = torch.randperm(full, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        g32, g16 = run(x[:full][perm].contiguous())
        assert torch.equal(bits(g32), bits(w32[perm])) and torch.equal(bits(g16), bits(w16[perm]))
        padded = torch.full((full, D + 8), 3.0, dtype=torch.bfloat16, device=dev)                # nor on x_stride
        padded[:, :D] = x[:full]
        view = padded[:, :D]
        assert view.stride(0) == D + 8 and not view.is_contiguous()
        g32, g16 = run(view)
        assert torch.equal(bits(g32), bits(w32)) and torch.equal(bits(g16), bits(w16))


def test_tall_inputs_go_through_in_chunks(dev, monkeypatch):
    """A chunk boundary (and a route change between the chunks) leaves every row's bits to its route: 300 rows in chunks of
    140 are two route-1 calls and a route-0 call of 20 rows."""
    from vpr_amd import ops
    k = case(dev, 192, 128)
    x = torch.cat([k["x"], k["x"][:43]]).contiguous()
    w0 = ops.project_rows(x[280:], k["P"], k["c"], True, want_f32=True)[0]
    w1 = ops.project_rows(x, k["P"], k["c"], True, want_f32=True)[0]
    monkeypatch.setattr(ops, "PROJECT_CHUNK_ROWS", 140)
    g32, g16 = ops.project_rows(x, k["P"], k["c"], True, want_f32=True)
    assert torch.equal(bits(g32[:280]), bits(w1[:280])) and torch.equal(bits(g32[280:]), bits(w0))
    assert torch.equal(bits(g16), bits(g32.to(torch.bfloat16)))


# ------------------------------------------------------------------------------------------------ special rows
@pytest.mark.parametrize("rows", [66, 130])
def test_zero_and_infinite_rows(dev, rows):
    from vpr_amd import ops
    D, d = 192, 128
    k = case(dev, D, d)
    x = k["x"][:rows].clone()
    zero_c = torch.zeros_like(k["c"])
    clean = ops.project_rows(x, k["P"], zero_c, True, want_f32=True)
    x[5] = 0
    x[64, 7] = float("inf")
    x[rows - 1, D - 1] = float("-inf")
    x[9, 3] = float("nan")
    g32, g16 = ops.project_rows(x, k["P"], zero_c, True, want_f32=True)
    bad = [5, 64, rows - 1, 9]
    for r in bad:                                   # +0, every bit
        assert (bits(g32[r]) == 0).all() and (bits(g16[r]) == 0).all(), r
    keep = torch.ones(rows, dtype=torch.bool, device=dev)
    keep[bad] = False
    assert torch.equal(bits(g32[keep]), bits(clean[0][keep])) and torch.equal(bits(g16[keep]), bits(clean[1][keep]))
    # with a bias the all-zero row is c normalised; without normalisation non-finite values pass through
    b32, _ = ops.project_rows(x[5:6].contiguous(), k["P"], k["c"], True, want_f32=True)
    c64 = k["c"].double().cpu().numpy()
    assert np.abs(b32.double().cpu().numpy()[0] - c64 / np.linalg.norm(c64)).max() <= (d + 16) * U32
    raw, _ = ops.project_rows(x, k["P"], zero_c, False, want_f32=True)
    assert not torch.isfinite(raw[64]).all() and torch.isfinite(raw[keep]).all() and (bits(raw[5]) == 0).all()


@pytest.mark.parametrize("rows", [70, 131])
@pytest.mark.parametrize("D,d", [(64, 64), (192, 128), (8448, 512)])
def test_sums_that_are_exact(dev, D, d, rows):
    """Small integers: every product and every partial sum is an integer below 2^24, so any f32 order gives the f64 answer."""
    from vpr_amd import ops
    rng = np.random.default_rng(D + d + rows)
    x = rng.integers(-3, 4, (rows, D))
    P = rng.integers(-3, 4, (d, D))
    c = rng.integers(-50, 51, d)
    want = (c + x @ P.T).astype(np.float64)
    assert np.abs(x).astype(np.int64).dot(np.abs(P).T).max() + 50 < 2 ** 24
    g32, g16 = ops.project_rows(torch.from_numpy(x).to(dev).to(torch.bfloat16), torch.from_numpy(P).to(dev).to(torch.bfloat16),
                                torch.from_numpy(c).to(dev).to(torch.float32), False, want_f32=True)
    assert (g32.double().cpu().numpy() == want).all()
    assert torch.equal(bits(g16), bits(g32.to(torch.bfloat16)))


def test_too_small_workspace_is_refused_and_outputs_untouched(dev):
    from vpr_amd import _lib
    L = _lib.lib()
    D, d = 192, 128
    k = case(dev, D, d)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rows in (64, 200):
        need = L.vpr_project_workspace_bytes(rows, D, d)
        ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        o32 = torch.full((rows, d), 7.0, dtype=torch.float32, device=dev)
        o16 = torch.full((rows, d), 7.0, dtype=torch.bfloat16, device=dev)
        x = k["x"][:rows].contiguous()
        args = lambda n: (ctypes.c_void_p(x.data_ptr()), D, rows, D, ctypes.c_void_p(k["P"].data_ptr()), ctypes.c_void_p(k["c"].data_ptr()),
                          d, 1, ctypes.c_void_p(o32.data_ptr()), ctypes.c_void_p(o16.data_ptr()), ctypes.c_void_p(ws.data_ptr()), n, stream)
        assert L.vpr_project_rows(*args(need - 1)) == -3
        torch.cuda.synchronize()
        assert (o32 == 7.0).all() and (o16 == 7.0).all() and (ws == 0).all()
        assert L.vpr_project_rows(*args(need)) == 0
        torch.cuda.synchronize()
        assert not (o32 == 7.0).any() and torch.equal(bits(o16), bits(o32.to(torch.bfloat16)))


@pytest.mark.parametrize("rows", [64, 200])
def test_graph_replay_equals_eager(dev, rows):
    from vpr_amd import ops
    k = case(dev, 8448, 512)
    x = torch.zeros((rows, 8448), dtype=torch.bfloat16, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.project_rows(x, k["P"], k["c"], True, want_f32=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g32, g16 = ops.project_rows(x, k["P"], k["c"], True, want_f32=True)
    for lo in (0, 31):
        x.copy_(k["x"][lo:lo + rows])
        graph.replay()
        torch.cuda.synchronize(dev)
        e32, e16 = ops.project_rows(k["x"][lo:lo + rows].contiguous(), k["P"], k["c"], True, want_f32=True)
        assert torch.equal(bits(g32), bits(e32)) and torch.equal(bits(g16), bits(e16))
    ops.drop_stream_caches(side.cuda_stream)


# ------------------------------------------------------------------------------------------ retrieval, recipe R
def recipe_r(seed, N=2048, D=384, latent=160, n_query=64):
    """Recipe R: rows = normalise(latent(160, std 2^(-i/64)) . U^T + 0.25 N(0, I) offset + 0.01 noise) in bf16; queries =
    distinct gallery rows + 0.005 noise, renormalised, bf16.  Returns (rows bf16 [N, D], queries bf16 [64, D], planted [64])."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((D, latent)))[0]
    lam = 2.0 ** (-np.arange(latent) / 64.0)
    offset = 0.25 * rng.standard_normal(D)
    x = (rng.standard_normal((N, latent)) * lam) @ U.T + offset + 0.01 * rng.standard_normal((N, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    rows = torch.from_numpy(x).to(torch.bfloat16)
    planted = rng.choice(N, size=n_query, replace=False)
    q = rows[planted].double().numpy() + 0.005 * rng.standard_normal((n_query, D))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return rows, torch.from_numpy(q).to(torch.bfloat16), planted


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).double().numpy()


def top1_and_margin(q, g):
    s = q @ g.T
    order = np.argsort(-s, axis=1)
    first, second = np.take_along_axis(s, order[:, :1], 1)[:, 0], np.take_along_axis(s, order[:, 1:2], 1)[:, 0]
    return order[:, 0], first - second


@pytest.fixture(scope="module")
def recipe(dev):
    """Recipe R (seed 0) and the facts of its f64 restatement: the full-width search and the search after PCA to d in
    {64, 128}, whitened or not, with bf16 rounding of operands and outputs, recover every planted row as top-1; in the
    projected spaces, the ones the device path searches, the top-1 / top-2 margin is at least 0.38."""
    rows, q, planted = recipe_r(0)
    X, Q = rows.double().numpy(), q.double().numpy()
    top, margin = top1_and_margin(Q, X)
    assert (top == planted).all()                   # (margin 0.378 with this order of the generator's draws)
    mean = X.mean(0)
    w, v = np.linalg.eigh(np.cov(X, rowvar=False))
    w, v = w[::-1], v[:, ::-1]
    for d in (64, 128):
        for whiten in (False, True):
            M = v[:, :d].T / (np.sqrt(w[:d] + 1e-6 * w[0])[:, None] if whiten else 1.0)
            P = bf16_round(M.astype(np.float32))
            c = (-(P @ mean)).astype(np.float32).astype(np.float64)
            proj = lambda a: bf16_round((lambda z: z / np.linalg.norm(z, axis=1, keepdims=True))(a @ P.T + c))
            top, margin = top1_and_margin(proj(Q), proj(X))
            assert (top == planted).all() and margin.min() >= 0.38, (d, whiten)
    return rows.to(dev), q.to(dev), torch.from_numpy(planted).to(dev)


@pytest.fixture(scope="module")
def fits(recipe):
    from vpr_amd.projection import fit_projection
    rows = recipe[0]
    return {(d, wh): fit_projection(rows, d, whiten=wh) for d in (64, 128) for wh in (False, True)}


def projected_gallery(recipe, fits, d, whiten, fp8, **kw):
    from vpr_amd import gallery as G
    from vpr_amd.retrieval import ShardedGallery
    p = fits[(d, whiten)]
    g, sc = G.project_gallery(recipe[0], p, fp8=fp8)
    assert g.shape == (recipe[0].shape[0], d) and g.dtype == (torch.uint8 if fp8 else torch.bfloat16) and (sc is not None) == fp8
    return ShardedGallery(g, g.shape[0], scales=sc, projection=p, **kw), p


@pytest.mark.parametrize("d,whiten,fp8", [(64, False, False), (64, True, False), (128, False, False), (128, True, False),
                                          (128, False, True), (128, True, True)])
def test_device_path_recovers_every_planted_row(recipe, fits, d, whiten, fp8):
    rows, q, planted = recipe
    sg, p = projected_gallery(recipe, fits, d, whiten, fp8)
    assert sg.query_width == 384 and p.n_fit == 2048
    v, i = sg.search(q, 2)
    assert (i[:, 0] == planted.to(torch.int32)).all()
    print(f"d={d} whiten={whiten} fp8={fp8}: smallest top-1 / top-2 margin on the device {float((v[:, 0] - v[:, 1]).min()):.3f}")
    # D_in-wide queries are projected first; d-wide ones are taken as they are: the same bits
    qp = p.apply(q)
    assert qp.shape == (64, d) and qp.dtype == torch.bfloat16
    v2, i2 = sg.search(qp, 2)
    assert torch.equal(i, i2) and torch.equal(bits(v), bits(v2))
    with pytest.raises(ValueError, match="wide"):
        sg.search(q[:, :256].contiguous(), 2)


@pytest.mark.parametrize("fp8", [False, True])
def test_search_expanded_works_in_the_projected_space(recipe, fits, fp8):
    rows, q, _ = recipe
    sg, p = projected_gallery(recipe, fits, 128, True, fp8)
    qp = p.apply(q)
    v1, i1 = sg.search(qp, 10)
    e = sg.expand(qp, v1, i1, 5, 2.0, 1.0)
    assert e.shape == (64, 128) and e.dtype == torch.bfloat16
    want_v, want_i = sg.search(e, 10)
    for queries in (q, qp):
        got_v, got_i = sg.search_expanded(queries, 10, 5, alpha=2.0, q_weight=1.0)
        assert torch.equal(got_i, want_i) and torch.equal(bits(got_v), bits(want_v))
    assert not torch.equal(bits(want_v), bits(v1))


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


def test_local_queries_travel_projected(rccl_one_rank, recipe, fits, monkeypatch):
    from vpr_amd.retrieval import ShardedGallery
    rows, q, planted = recipe
    local, p = projected_gallery(recipe, fits, 64, True, False)
    coll, _ = projected_gallery(recipe, fits, 64, True, False, force_collectives=True)
    assert coll.collective and not local.collective
    gathered = []
    plain_gather = ShardedGallery.gather_queries

    def spy(self, q_local):
        gathered.append(tuple(q_local.shape))
        return plain_gather(self, q_local)

    monkeypatch.setattr(ShardedGallery, "gather_queries", spy)
    for expand in (None, (4, 1.0)):
        want = local.search_local_queries(q, 5, expand)
        got = coll.search_local_queries(q, 5, expand)
        for a, b in zip(got, want):
            assert torch.equal(bits(a), bits(b))
    assert gathered and all(s == (64, 64) for s in gathered)          # d-wide rows travel
    assert (want[1][:, 0] == planted.to(torch.int32)).all()


@pytest.mark.parametrize("collective", [False, True])
def test_graphed_retrieval_with_projection_equals_eager(rccl_one_rank, recipe, fits, collective):
    from vpr_amd.retrieval import GraphedRetrieval
    rows, q, planted = recipe
    N, B, k = rows.shape[0], 16, 5
    rng = np.random.default_rng(3)
    labels = np.stack([2e5 + rng.normal(0, 900, N), 1.4e5 + rng.normal(0, 1100, N), rng.uniform(0, 360, N),
                       rng.integers(0, 6, N).astype(np.float64)], 1)
    scaler = [2e5, 1.4e5, 900.0, 1100.0]
    sg, p = projected_gallery(recipe, fits, 128, True, False, force_collectives=collective)
    gr = GraphedRetrieval(sg, B, k, labels=labels, mode="weighted", temperature=0.05, scaler=scaler)
    two = GraphedRetrieval(sg, B, k, expand=(4, 2.0))
    assert gr.q.shape == (B, 384) and two.q.shape == (B, 384)        # the static buffer has the input width
    assert sg.uncertified_queries() == 0
    for lo in (0, 16, 48):
        qb = q[lo:lo + B].contiguous()
        v_g, i_g = gr(qb)
        v_g, i_g, p64, p4 = v_g.clone(), i_g.clone(), gr.pose64.clone(), gr.pose4.clone()
        v_e, i_e = sg.search(qb, k)
        assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e))
        assert (i_g[:, 0] == planted[lo:lo + B].to(torch.int32)).all()
        e64, e4, _, _ = torch.ops.vpr.retrieval_pose(v_e, i_e, gr.labels, "weighted", 0.05, None, 0.0, scaler)
        assert torch.equal(p64, e64) and torch.equal(p4, e4)
        v_t, i_t = two(qb)
        v_x, i_x = sg.search_expanded(qb, k, 4, alpha=2.0)
        assert torch.equal(i_t, i_x) and torch.equal(bits(v_t), bits(v_x))
    gr.close(), two.close()


def test_pipeline_on_a_projected_gallery(dev):
    """ViT-S, as smoke() builds it: the head sees the full f32 descriptor, the retrieval leg the projected bf16 one."""
    import torch.nn as nn
    from vpr_amd.modules import DinoV2Salad, FusedGeoPoseHead
    from vpr_amd.pipeline import VPRGeoPosePipeline
    from vpr_amd.projection import DescriptorProjection
    from vpr_amd.retrieval import ShardedGallery
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    ext.backbone.fold_layerscale()
    pos = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    ang = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    head = FusedGeoPoseHead(pos, ang, normalize=True)
    n, B, k, d = 500, 2, 5, 64
    g = torch.Generator().manual_seed(4)
    proj = DescriptorProjection(torch.randn(d, 8448, generator=g) / 8448 ** 0.5, 0.01 * torch.randn(8448, generator=g).double(),
                                torch.ones(d, dtype=torch.float64), whiten=False)
    gal = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(dev).to(torch.bfloat16)
    rng = np.random.default_rng(8)
    labels = np.stack([2e5 + rng.normal(0, 900, n), 1.4e5 + rng.normal(0, 1100, n), rng.uniform(0, 360, n),
                       rng.integers(0, 6, n).astype(np.float64)], 1)
    images = torch.randn(B, 3, 224, 224, device=dev).to(torch.bfloat16)
    with torch.no_grad():
        desc, desc16 = ext.features(images, want_bf16=True)
        want_pose = head(desc)
    sg = ShardedGallery(gal, n, projection=proj)
    want_v, want_i = ShardedGallery(gal, n).search(proj.apply(desc16), k)
    want_r = torch.ops.vpr.retrieval_pose(want_v, want_i, torch.from_numpy(labels).to(dev), "top1", 0.01, None, 0.0, None)[1]
    for kw in (dict(), dict(graph_retrieval=True)):
        pipe = VPRGeoPosePipeline(ext, head, sg, k, labels=labels, **kw)
        for _ in range(2):
            out = pipe.step(images)
        torch.cuda.synchronize()
        assert out.descriptors.shape == (B, 8448) and torch.equal(out.descriptors, desc) and torch.equal(out.pose, want_pose)
        assert torch.equal(out.topk_indices, want_i) and torch.equal(bits(out.topk_scores), bits(want_v)), kw
        assert torch.equal(out.retrieval_pose, want_r), kw


def test_evaluation_entry_points_with_a_projection(dev, tmp_path, monkeypatch):
    """build_gallery_from_images(projection=64) fits on the gallery's own descriptors, stores 64-wide rows and the projection;
    calculate_retrieval_scores picks it up: its result is retrieval_metrics of the stored gallery searched by hand with the
    query descriptors it saw, projected."""
    import json
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, gallery as G, modules
    from vpr_amd.retrieval import ShardedGallery
    rng = np.random.default_rng(21)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g = 72                                                                 # more rows than d = 64
    gnames = [f"img_{i:04d}.png" for i in range(n_g)]
    imgs = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(n_g)]
    for n, im in zip(gnames, imgs):
        Image.fromarray(im).save(gdir / n)
    lat, lon, ang = 219000 + 100.0 * np.arange(n_g), 143000 + 50.0 * np.arange(n_g), (17.0 * np.arange(n_g)) % 360
    pd.DataFrame({"filename": gnames, "timestamp": "t", "latitude": lat, "longitude": lon, "angle": ang,
                  "Region_ID": np.arange(n_g) // 5}).to_csv(tmp_path / "labels_train.csv", index=False)
    src = [3, 11, 0, 19, 70, 42]
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
    gal_dir = str(tmp_path / "gal")
    assert evaluate.build_gallery_from_images(ext, str(tmp_path / "labels_train.csv"), str(gdir), gal_dir, batch_size=8,
                                              projection=64, whiten=False) == n_g
    meta = json.load(open(os.path.join(gal_dir, "meta.json")))
    assert meta["version"] == 1 and meta["d"] == 64 and meta["n"] == n_g and os.path.exists(os.path.join(gal_dir, "projection.npz"))
    shard = G.load_gallery_shard(gal_dir, dev)
    proj = shard.projection
    assert shard.rows.shape == (n_g, 64) and proj.d == 64 and proj.d_in == 8448 and proj.n_fit == n_g and not proj.whiten
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None):
        seen.append((q_local.clone(), k))
        return plain_search(self, q_local, k, expand)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    got = evaluate.calculate_retrieval_scores(ext, gal_dir, str(tmp_path / "labels_val.csv"), str(vdir), k=5, tau=10.0,
                                              batch_size=4, verbose=False)
    assert seen and all(q.shape[1] == 8448 for q, _ in seen)                 # full-width descriptors in, projected inside
    monkeypatch.setattr(ShardedGallery, "search_local_queries", plain_search)
    by_hand = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True)                      # no projection: d-wide queries
    batches = [by_hand.search(proj.apply(q), k) for q, k in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    want = evaluate.retrieval_metrics(vals, idx, shard.labels, df[["latitude", "longitude"]].to_numpy(dtype=np.float64),
                                      df["Region_ID"].to_numpy(), df["angle"].to_numpy(dtype=np.float64), 10.0, "top1")
    for key, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[key].tobytes() == w.tobytes(), key
        else:
            assert got[key] == w, key
