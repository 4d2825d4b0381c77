"""CPU: the descriptor-projection extension of the C ABI (include/vpr_amd_project.h) — header, binding table and exported
symbols agree, the older tables are what they were, every refusal comes back with its status before a device is touched, the
torch op has a fake implementation, the wrappers refuse what they cannot take; projection.fit_projection against an f64 numpy
restatement (mean, np.cov, eigh) on CPU tensors; the gallery format with and without projection.npz."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


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


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_project.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    for name, (restype, argtypes) in _lib.PROJECT_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    assert len(_lib.PROJECT_PROTOTYPES["vpr_project_rows"][1]) == 13
    bound = int(re.search(r"#define VPR_PROJECT_STREAM_MAX_ROWS (\d+)", code).group(1))
    assert bound == _lib.PROJECT_STREAM_MAX_ROWS
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert len(_lib.EXPAND_PROTOTYPES["vpr_query_expand"][1]) == 18 and len(_lib.EXPAND_PROTOTYPES["vpr_query_expand_finish"][1]) == 8
    assert len(_lib.EXTENSION_PROTOTYPES["vpr_retrieval_pose"][1]) == 16
    new = set(_lib.PROJECT_PROTOTYPES)
    assert not new & set(_lib.PROTOTYPES) and not new & set(_lib.EXTENSION_PROTOTYPES) and not new & set(_lib.EXPAND_PROTOTYPES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert "vpr_project" not in main and re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)
    for other in ("vpr_amd_retrieval.h", "vpr_amd_expand.h"):
        assert "vpr_project" not in open(os.path.join(ROOT, "include", other)).read()


def test_refusals_come_back_without_a_device(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    big = 1 << 40

    def call(x=p, stride=None, rows=1, D=64, P=p, c=p, d=64, normalize=1, o32=p, o16=p, ws=p, ws_bytes=big):
        return lib.vpr_project_rows(x, D if stride is None else stride, rows, D, P, c, d, normalize, o32, o16, ws, ws_bytes, null)

    for kw in (dict(x=null), dict(P=null), dict(c=null), dict(ws=null), dict(o32=null, o16=null), dict(rows=-1), dict(D=-64),
               dict(d=-64), dict(normalize=2), dict(normalize=-1), dict(stride=56), dict(D=128, stride=64), dict(rows=0, x=null)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(D=0), dict(D=96), dict(D=63), dict(d=0), dict(d=96), dict(d=32), dict(d=4160), dict(d=8192), dict(stride=68),
               dict(stride=100), dict(x=odd), dict(P=odd), dict(c=odd), dict(o32=odd), dict(o16=odd), dict(ws=odd),
               dict(o32=null, o16=odd), dict(rows=200, D=8448, d=512, stride=8452)):
        assert call(**kw) == UNSUPPORTED, kw
    # the shape part of the status is what vpr_project_route answers (a function of rows, D, d only)
    for rows, D, d in ((-1, 64, 64), (1, -64, 64), (1, 64, -64)):
        assert lib.vpr_project_route(rows, D, d) == INVALID == call(rows=rows, D=D, d=d, stride=max(D, 64))
    for rows, D, d in ((1, 0, 64), (1, 96, 64), (1, 63, 64), (1, 64, 0), (1, 64, 96), (1, 64, 4160), (300, 8448, 8192)):
        assert lib.vpr_project_route(rows, D, d) == UNSUPPORTED == call(rows=rows, D=D, d=d, stride=max(D, 64))
        assert lib.vpr_project_workspace_bytes(rows, D, d) == 0
    # workspace: one byte short is refused, on both routes
    for rows, D, d in ((1, 64, 64), (64, 8448, 512), (128, 8448, 512), (129, 8448, 512), (65536, 8448, 4096)):
        need = lib.vpr_project_workspace_bytes(rows, D, d)
        assert need > 0 and call(rows=rows, D=D, d=d, ws_bytes=need - 1) == WORKSPACE
        assert call(rows=rows, D=D, d=d, ws_bytes=0) == WORKSPACE
    # what the rules leave alone: rows = 0 launches nothing, either output may be absent, the largest legal sizes
    assert call(rows=0) == 0 and call(rows=0, o32=null) == 0 and call(rows=0, o16=null, normalize=0) == 0
    assert call(rows=0, D=8448, d=4096, stride=8456, ws_bytes=0) == 0


def test_route_and_workspace_queries(lib):
    from vpr_amd import _lib
    bound = _lib.PROJECT_STREAM_MAX_ROWS
    for D, d in ((64, 64), (192, 128), (8448, 512), (8448, 2048), (8448, 4096), (128, 64)):
        assert [lib.vpr_project_route(r, D, d) for r in (0, 1, 64, bound, bound + 1, 4097, 65536, 1 << 20)] == [0, 0, 0, 0, 1, 1, 1, 1]
        sizes = [lib.vpr_project_workspace_bytes(r, D, d) for r in sorted(set(range(0, 300)) | set(range(max(bound - 100, 0), bound + 300)))]
        sizes += [lib.vpr_project_workspace_bytes(r, D, d) for r in (4096, 30000, 65535, 65536, 65537, 300000, 1 << 20)]
        assert sizes[0] == 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (D, d)    # monotone in rows
        assert lib.vpr_project_workspace_bytes(1 << 20, D, d) >= (1 << 20) * d * 4         # one f32 slab on the tiled route
    # the serving shape: 8 output tiles x 33 slices of 8 K-steps = 33 slabs of [rows, 512] f32
    assert lib.vpr_project_workspace_bytes(64, 8448, 512) == 33 * 64 * 512 * 4
    for D, d in ((64, 64), (8448, 64), (8448, 4096), (64 * 1000, 64), (64 * 1000, 4096)):  # never more than 64 slabs
        assert lib.vpr_project_workspace_bytes(1, D, d) <= 64 * d * 4


def test_fake_op_gives_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "project_rows" in torch_ops.OPS
    schema = str(torch.ops.vpr.project_rows.default._schema)
    assert schema.startswith("vpr::project_rows(") and "bool normalize=True" in schema
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        x, P, c = mk(37, 8448, dtype=torch.bfloat16), mk(512, 8448, dtype=torch.bfloat16), mk(512, dtype=torch.float32)
        for args in ((x, P, c), (x, P, c, False)):
            o32, o16 = torch.ops.vpr.project_rows(*args)
            assert o32.shape == o16.shape == (37, 512) and o32.dtype == torch.float32 and o16.dtype == torch.bfloat16
            assert o32.device.type == "cuda"


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    from vpr_amd.projection import DescriptorProjection
    from vpr_amd.retrieval import ShardedGallery
    rows, D, d = 3, 128, 64
    x, P, c = torch.zeros(rows, D, dtype=torch.bfloat16), torch.zeros(d, D, dtype=torch.bfloat16), torch.zeros(d)
    proj = DescriptorProjection(torch.zeros(d, D), torch.zeros(D, dtype=torch.float64), torch.ones(d, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.project_rows(x, P, c)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.project_rows(x, P, c)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        proj.apply(x)
    with pytest.raises(ValueError, match="projection maps to 64"):
        ShardedGallery(torch.zeros(4, 128, dtype=torch.bfloat16), 4, projection=proj)
    sg = ShardedGallery(torch.zeros(4, d, dtype=torch.bfloat16), 4, projection=proj)
    assert sg.query_width == D and sg.project_queries(torch.zeros(2, d, dtype=torch.bfloat16)).shape == (2, d)
    with pytest.raises(ValueError, match="queries are 192 wide"):
        sg.search(torch.zeros(2, 192, dtype=torch.bfloat16), 1)
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    for bad, match in (((x.float(), P, c), "x: expected dtype"), ((x, P.float(), c), "P: expected dtype"),
                       ((x, P, c.double()), "c: expected dtype"), ((x[0], P, c), "x: expected 2 dims"),
                       ((x, P[0], c), "P: expected 2 dims"), ((x, P, c[None]), "c: expected 1 dims"),
                       ((x[:, :64], P[:, :64], c), "contiguous"), ((x, P[:, :64].contiguous(), c), "disagree on D"),
                       ((x, P, c[:32]), "disagree on d"), ((x[:, ::2], P[:, :64].contiguous(), c), "column stride"),
                       ((torch.zeros(rows, D + 4, dtype=torch.bfloat16)[:, :D], P, c), "multiple of 8")):
        with pytest.raises(RuntimeError, match=match):
            ops.project_rows(*bad)
    for kw, match in ((dict(want_f32=False, want_bf16=False), "at least one"),
                      (dict(out=(torch.zeros(rows, d + 64), None)), r"\[rows, d\]"),
                      (dict(out=(None, torch.zeros(rows, d))), "out_bf16: expected dtype"), (dict(out=(None, None)), "at least one")):
        with pytest.raises(RuntimeError, match=match):
            ops.project_rows(x, P, c, **kw)


# ---------------------------------------------------------------------------------------------- fit_projection
@pytest.fixture(scope="module")
def fitted():
    """Recipe R, seed 0, with its f64 numpy reference (mean, np.cov, eigh) and the fits under test, computed once."""
    from vpr_amd.projection import fit_projection
    rows, _, _ = recipe_r(0)
    X = rows.double().numpy()
    mean = X.mean(0)
    w, v = np.linalg.eigh(np.cov(X, rowvar=False))
    w, v = w[::-1], v[:, ::-1]
    fits = {(d, wh): fit_projection(rows, d, whiten=wh) for d in (64, 128) for wh in (False, True)}
    return rows, X, mean, w, v, fits


def test_fit_matches_the_f64_reference(fitted):
    rows, X, mean, w, v, fits = fitted
    for (d, wh), p in fits.items():
        assert p.matrix.shape == (d, X.shape[1]) and p.matrix.dtype == torch.float32
        assert p.mean.dtype == p.eigenvalues.dtype == torch.float64 and p.n_fit == X.shape[0] and p.whiten == wh
        np.testing.assert_allclose(p.mean.numpy(), mean, rtol=0, atol=1e-14)
        lam = p.eigenvalues.numpy()
        assert np.all(np.diff(lam) <= 0)
        assert np.max(np.abs(lam - w[:d]) / w[:d]) <= 1e-9
        if not wh:       # the rank-d projector is well defined whatever the signs; unit rows in f32 (entries ~ D^-1/2, d of them)
            U = p.matrix.double().numpy()
            assert np.max(np.abs(U.T @ U - v[:, :d] @ v[:, :d].T)) <= 1e-8


def test_fit_sign_convention_whitening_and_bias(fitted):
    rows, X, mean, w, v, fits = fitted
    for (d, wh), p in fits.items():
        M = p.matrix.numpy()
        big = np.argmax(np.abs(M), axis=1)                   # first index of the largest magnitude
        assert np.all(M[np.arange(d), big] > 0)
        P16, c = p.host_operands()
        assert P16.dtype == torch.bfloat16 and torch.equal(P16, p.matrix.to(torch.bfloat16))
        ref_c = (-(P16.double().numpy() @ p.mean.numpy())).astype(np.float32)      # formed in f64, rounded once
        assert c.dtype == torch.float32 and np.array_equal(c.numpy(), ref_c)
        if wh:
            lam = p.eigenvalues.numpy()
            Z = (X - mean) @ p.matrix.double().numpy().T
            expect = np.diag(lam / (lam + p.eps_rel * lam[0]))
            assert np.max(np.abs(np.cov(Z, rowvar=False) - expect)) <= 1e-4
            scale = 1.0 / np.sqrt(w[:d] + 1e-6 * w[0])
            unit = M / scale[:, None]
            np.testing.assert_allclose(np.linalg.norm(unit, axis=1), 1.0, rtol=0, atol=1e-6)
        else:
            np.testing.assert_allclose(np.linalg.norm(M, axis=1), 1.0, rtol=0, atol=1e-6)


def test_fit_subsampling_dtype_and_refusals(fitted):
    from vpr_amd.projection import fit_projection, subsample_rows
    rows = fitted[0]
    N = rows.shape[0]
    sel = subsample_rows(N, 500)
    assert sel.numel() == 500 and sel[0] == 0 and torch.all(sel[1:] > sel[:-1]) and sel[-1] < N
    assert torch.equal(sel, (torch.arange(500) * N) // 500) and torch.equal(subsample_rows(100, 500), torch.arange(100))
    a = fit_projection(rows, 64, max_rows=500, chunk=128)
    b = fit_projection(rows, 64, max_rows=500, chunk=4096)
    c = fit_projection(rows[sel], 64)                        # the subsample is those rows, and nothing else
    assert a.n_fit == b.n_fit == c.n_fit == 500
    assert torch.equal(a.matrix, fit_projection(rows, 64, max_rows=500, chunk=128).matrix)          # deterministic
    assert torch.allclose(a.eigenvalues, b.eigenvalues, rtol=1e-12, atol=0) and torch.allclose(a.eigenvalues, c.eigenvalues, rtol=1e-12, atol=0)
    # f32 descriptors are used at their bf16 values
    noisy = rows.float() * (1 + 2.0 ** -12)
    assert torch.equal(noisy.to(torch.bfloat16), rows)
    assert torch.equal(fit_projection(noisy, 64).matrix, fitted[5][(64, True)].matrix)
    for kw in (dict(d=448), dict(d=100), dict(d=0), dict(d=64, max_rows=64), dict(d=128, max_rows=100)):
        with pytest.raises(ValueError):
            fit_projection(rows, **kw)
    with pytest.raises(ValueError):
        fit_projection(rows[:64], 64)
    with pytest.raises(ValueError):
        fit_projection(rows.double(), 64)
    with pytest.raises(ValueError):
        fit_projection(rows[0], 64)


def test_fit_with_fewer_rows_than_columns(fitted):
    """n < D goes through the n x n form of the eigenproblem: the same eigenvalues and the same rank-d projector."""
    from vpr_amd.projection import fit_projection
    rows = fitted[0][:200]
    X = rows.double().numpy()
    w, v = np.linalg.eigh(np.cov(X, rowvar=False))
    w, v = w[::-1], v[:, ::-1]
    p = fit_projection(rows, 64, whiten=False)
    lam, U = p.eigenvalues.numpy(), p.matrix.double().numpy()
    assert p.n_fit == 200 and np.max(np.abs(lam - w[:64]) / w[:64]) <= 1e-9
    assert np.max(np.abs(U.T @ U - v[:, :64] @ v[:, :64].T)) <= 1e-8
    M = p.matrix.numpy()
    assert np.all(M[np.arange(64), np.argmax(np.abs(M), axis=1)] > 0)
    with pytest.raises(ValueError, match="span fewer"):
        fit_projection(rows[:3].repeat(30, 1), 64)           # 90 rows of rank 2


def test_save_load_round_trips_bit_for_bit(fitted, tmp_path):
    from vpr_amd.projection import DescriptorProjection
    for key, p in fitted[5].items():
        path = str(tmp_path / f"p{key[0]}{int(key[1])}.npz")
        p.save(path)
        with np.load(path, allow_pickle=False) as z:         # arrays and scalars only
            assert set(z.files) == {"matrix", "mean", "eigenvalues", "whiten", "eps_rel", "n_fit"}
            assert z["matrix"].dtype == np.float32 and z["mean"].dtype == z["eigenvalues"].dtype == np.float64
        q = DescriptorProjection.load(path)
        assert torch.equal(q.matrix, p.matrix) and torch.equal(q.mean, p.mean) and torch.equal(q.eigenvalues, p.eigenvalues)
        assert (q.whiten, q.eps_rel, q.n_fit) == (p.whiten, p.eps_rel, p.n_fit)
        assert all(torch.equal(a, b) for a, b in zip(q.host_operands(), p.host_operands()))


def test_gallery_round_trip_with_and_without_projection(fitted, tmp_path):
    from vpr_amd import gallery as G
    p = fitted[5][(64, True)]
    N = 40
    rng = np.random.default_rng(1)
    labels = rng.standard_normal((N, 4))
    wide = fitted[0][:N].contiguous()
    narrow = torch.from_numpy(rng.standard_normal((N, 64))).to(torch.bfloat16)
    plain, proj = str(tmp_path / "plain"), str(tmp_path / "proj")
    G.save_gallery(plain, wide, labels)
    G.save_gallery(proj, narrow, labels, projection=p)
    assert not os.path.exists(os.path.join(plain, "projection.npz")) and os.path.exists(os.path.join(proj, "projection.npz"))
    metas = [json.load(open(os.path.join(d, "meta.json"))) for d in (plain, proj)]
    for meta, width in zip(metas, (384, 64)):                # what an older loader reads
        assert meta["version"] == 1 and meta["d"] == width and meta["n"] == N and meta["dtype"] == "bf16"
        assert set(meta) == {"version", "n", "d", "dtype", "label_columns"}
    a = G.load_gallery_shard(plain, torch.device("cpu"))
    b = G.load_gallery_shard(proj, torch.device("cpu"), rank=1, world=2)
    assert a.projection is None and torch.equal(a.rows, wide)
    assert torch.equal(b.rows, narrow[20:]) and b.index_base == 20
    assert torch.equal(b.projection.matrix, p.matrix) and torch.equal(b.projection.mean, p.mean) and b.projection.d_in == 384
    assert G.sharded_gallery_from(a).projection is None and G.sharded_gallery_from(b, 1, 2).projection is b.projection
    with pytest.raises(ValueError, match="projection maps to 64"):
        G.save_gallery(str(tmp_path / "bad"), wide, labels, projection=p)
    with pytest.raises(ValueError, match="d % 128"):
        G.project_gallery(wide, p, fp8=True)
    G.save_gallery(proj, narrow, labels)                     # written over without one: the stale file goes
    assert G.load_gallery_shard(proj, torch.device("cpu")).projection is None
