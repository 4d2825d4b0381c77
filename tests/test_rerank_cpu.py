"""CPU: the two-tier retrieval extension of the C ABI (include/vpr_amd_rerank.h) — header, binding table and exported symbols
agree, the older tables are what they were, every refusal comes back with its status before a device is touched, the workspace
query is monotone, the torch op has a fake implementation, the wrappers refuse what they cannot take; the gallery format with
and without fine_descriptors.npy; ShardedGallery.search_reranked on an injected CPU engine (oracle searches, an f64 re-rank
written here) over hand-made shards against the f64 top-k over the union of the shards' coarse candidates."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_rerank.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    for name, (restype, argtypes) in _lib.RERANK_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    assert len(_lib.RERANK_PROTOTYPES["vpr_rerank_rows"][1]) == 16
    const = lambda n: int(re.search(rf"#define {n} (\d+)", code).group(1))
    assert const("VPR_RERANK_MAX_KC") == _lib.RERANK_MAX_KC == 128 and const("VPR_RERANK_MAX_D") == _lib.RERANK_MAX_D >= 16384
    assert const("VPR_RERANK_CHUNK_BF16") == 8 and const("VPR_RERANK_CHUNK_F32") == 4
    # L: the macro of the header, evaluated as C would, is the binding's rerank_roundings and the formula of the comment
    m = re.search(r"#define VPR_RERANK_ROUNDINGS\(D, rows_are_f32\)\s*\\\s*\n\s*\(\(rows_are_f32\) \? (.*?) : (.*?)\)\s*\n", code)
    as_py = lambda expr, D: eval(expr.replace("/", "//"), {"D": D})
    for D in (64, 128, 192, 256, 448, 512, 576, 8448, 16384):
        for f32, E in ((False, 8), (True, 4)):
            L = -(-D // (64 * E)) + int(np.log2(E)) + 6
            assert as_py(m.group(2 - f32), D) == _lib.rerank_roundings(D, f32) == L, (D, f32)
    assert _lib.rerank_roundings(8448, False) == 26 and _lib.rerank_roundings(8448, True) == 41
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    assert len(_lib.EXPAND_PROTOTYPES["vpr_query_expand"][1]) == 18 and len(_lib.EXPAND_PROTOTYPES["vpr_query_expand_finish"][1]) == 8
    assert len(_lib.EXTENSION_PROTOTYPES["vpr_retrieval_pose"][1]) == 16 and len(_lib.PROJECT_PROTOTYPES["vpr_project_rows"][1]) == 13
    assert len(_lib.PROTOTYPES) == 61
    new = set(_lib.RERANK_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES):
        assert not new & set(older)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert "vpr_rerank" not in main and re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)
    for other in ("vpr_amd_retrieval.h", "vpr_amd_expand.h", "vpr_amd_project.h"):
        assert "vpr_rerank" not in open(os.path.join(ROOT, "include", other)).read()


def test_refusals_come_back_without_a_device(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    odd2 = ctypes.c_void_p(p.value + 2)                      # not even 4-byte aligned
    big = 1 << 40

    def call(q=p, qf=0, idx=p, B=1, D=64, kc=10, rows=p, rf=0, n_local=5, base=0, k=3, vals=p, out=p, ws=p, ws_bytes=big):
        return lib.vpr_rerank_rows(q, qf, idx, B, D, kc, rows, rf, n_local, base, k, vals, out, ws, ws_bytes, null)

    for kw in (dict(q=null), dict(idx=null), dict(rows=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1),
               dict(D=-64), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2), dict(kc=0, k=0),
               dict(qf=2), dict(qf=-1), dict(rf=2), dict(rf=-1), dict(B=0, q=null), dict(kc=200, k=201)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(kc=129, k=1), dict(kc=129, k=129), dict(D=0), dict(D=96), dict(D=63), dict(D=16384 + 64), dict(D=1 << 20),
               dict(q=odd), dict(rows=odd), dict(ws=odd), dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(ws_bytes=0)):
        assert call(**kw) == UNSUPPORTED, kw
    for B, kc in ((1, 1), (1, 10), (64, 64), (37, 128), (100000, 128)):                # workspace: one byte short is refused
        need = lib.vpr_rerank_workspace_bytes(B, kc)
        assert need >= 4 * B * kc and call(B=B, kc=kc, k=1, ws_bytes=need - 1) == UNSUPPORTED
    # what the rules leave alone: B = 0 launches nothing; both dtypes; the largest legal sizes; element-aligned lists
    assert call(B=0) == 0 and call(B=0, qf=1, rf=1) == 0 and call(B=0, D=16384, kc=128, k=128) == 0
    assert call(B=0, idx=odd, vals=odd, out=odd) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
    assert call(B=0, ws_bytes=lib.vpr_rerank_workspace_bytes(0, 10)) == 0


def test_workspace_query_is_monotone(lib):
    w = lib.vpr_rerank_workspace_bytes
    for kc in (1, 2, 63, 64, 65, 128):
        sizes = [w(B, kc) for B in list(range(0, 300)) + [4096, 65536, 1 << 20]]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), kc
    for B in (0, 1, 3, 37, 64, 5000):
        sizes = [w(B, kc) for kc in range(1, 129)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), B
    assert w(64, 64) == 64 * 64 * 4 and w(1 << 20, 128) == (1 << 20) * 128 * 4
    for B, kc in ((-1, 10), (1, 0), (1, -3), (1, 129), (64, 1000), (-5, 200)):
        assert w(B, kc) == 0, (B, kc)


def test_fake_op_gives_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "rerank_rows" in torch_ops.OPS
    schema = str(torch.ops.vpr.rerank_rows.default._schema)
    assert schema.startswith("vpr::rerank_rows(") and "Int index_base=0" in schema and "Int? k=None" in schema
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        idx = mk(37, 64, dtype=torch.int32)
        for qd in (torch.bfloat16, torch.float32):
            for rd in (torch.bfloat16, torch.float32):
                q, rows = mk(37, 8448, dtype=qd), mk(500, 8448, dtype=rd)
                for args, k in (((q, idx, rows), 64), ((q, idx, rows, 1000), 64), ((q, idx, rows, 0, 10), 10), ((q, idx, rows, 7, 1), 1)):
                    v, i = torch.ops.vpr.rerank_rows(*args)
                    assert v.shape == i.shape == (37, k) and v.dtype == torch.float32 and i.dtype == torch.int32
                    assert v.device.type == "cuda"


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    from vpr_amd.retrieval import ShardedGallery
    B, D, kc, n = 2, 64, 4, 5
    q, i, rows = torch.zeros(B, D, dtype=torch.bfloat16), torch.zeros(B, kc, dtype=torch.int32), torch.zeros(n, D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.rerank_rows(q, i, rows)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.rerank_rows(q, i, rows)
    # ShardedGallery: the fine rows are checked against the shard, and search_reranked against its limits
    coarse = torch.zeros(n, D, dtype=torch.uint8)
    with pytest.raises(ValueError, match="fine_rows must be"):
        ShardedGallery(coarse, n, scales=torch.ones(n), fine_rows=rows[:4])
    with pytest.raises(ValueError, match="fine_rows must be"):
        ShardedGallery(coarse[:2], n, 0, 2, scales=torch.ones(2), fine_rows=rows)        # the whole gallery's, not the shard's
    with pytest.raises(ValueError, match="bf16 or f32"):
        ShardedGallery(coarse, n, scales=torch.ones(n), fine_rows=rows.double())
    sg = ShardedGallery(coarse, n, scales=torch.ones(n), fine_rows=rows.float())
    with pytest.raises(ValueError, match="at most 64"):
        sg.search_reranked(q, 3, 65)
    with pytest.raises(ValueError, match="at most 64"):
        sg.search_reranked(q, 1, 0)
    with pytest.raises(ValueError, match="1..kc"):
        sg.search_reranked(q, 5, 4)
    with pytest.raises(ValueError, match="wide"):
        sg.search_reranked(q, 2, 4, q_fine=torch.zeros(B, 2 * D, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="disagree on B"):
        sg.search_reranked(q, 2, 4, q_fine=torch.zeros(B + 1, D, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="no fine_rows"):
        ShardedGallery(coarse, n, scales=torch.ones(n)).search_reranked(q, 2, 4)
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    for bad, match in (((q.double(), i, rows), "q: expected dtype"), ((q.half(), i, rows), "q: expected dtype"),
                       ((q, i.long(), rows), "idx: expected dtype"), ((q, i, rows.double()), "rows: expected dtype"),
                       ((q, i, rows.to(torch.uint8)), "rows: expected dtype"), ((q[0], i, rows), "q: expected 2 dims"),
                       ((q, i[0], rows), "idx: expected 2 dims"), ((q, i, rows[0]), "rows: expected 2 dims"),
                       ((q, i[:, :2], rows), "contiguous"), ((q[:, :32], i, rows), "contiguous"),
                       ((q[:1], i, rows), "disagree on B"), ((q, i, torch.zeros(n, 2 * D, dtype=torch.bfloat16)), "disagree on D"),
                       ((q, torch.zeros(B, 129, dtype=torch.int32), rows), "1..128 candidates"),
                       ((q, torch.zeros(B, 0, dtype=torch.int32), rows), "1..128 candidates")):
        with pytest.raises(RuntimeError, match=match):
            ops.rerank_rows(*bad)
    for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(k=-1), "k must be")):
        with pytest.raises(RuntimeError, match=match):
            ops.rerank_rows(q, i, rows, **kw)


# ------------------------------------------------------------------------------------------------- gallery format
def test_gallery_round_trip_with_and_without_fine_rows(tmp_path):
    from vpr_amd import gallery as G
    rng = np.random.default_rng(5)
    N, D, d = 41, 128, 64
    fine = torch.from_numpy(rng.standard_normal((N, D))).to(torch.bfloat16)
    coarse = torch.from_numpy(rng.integers(0, 256, (N, d), dtype=np.uint8))
    scales = torch.from_numpy(rng.uniform(0.001, 0.01, N).astype(np.float32))
    labels = rng.standard_normal((N, 4))
    plain, two = str(tmp_path / "plain"), str(tmp_path / "two")
    G.save_gallery(plain, coarse, labels, scales=scales)
    G.save_gallery(two, coarse, labels, scales=scales, fine=fine)
    assert not os.path.exists(os.path.join(plain, G.FINE_FILE)) and os.path.exists(os.path.join(two, G.FINE_FILE))
    stored = np.load(os.path.join(two, "fine_descriptors.npy"))
    assert stored.dtype == np.uint16 and stored.shape == (N, D) and np.array_equal(stored, fine.view(torch.uint16).numpy())
    for path in (plain, two):                                # what an older loader reads: meta.json does not change
        meta = json.load(open(os.path.join(path, "meta.json")))
        assert set(meta) == {"version", "n", "d", "dtype", "label_columns"}
        assert meta["version"] == 1 and meta["d"] == d and meta["n"] == N and meta["dtype"] == "fp8_e4m3"
    cpu = torch.device("cpu")
    a = G.load_gallery_shard(plain, cpu)
    b = G.load_gallery_shard(two, cpu)                       # load_fine defaults to False: as ever
    assert a.fine is None and b.fine is None and torch.equal(b.rows, coarse)
    assert G.sharded_gallery_from(b).fine_rows is None
    for rank, world in ((0, 1), (0, 3), (1, 3), (2, 3)):
        s = G.load_gallery_shard(two, cpu, rank, world, load_fine=True)
        lo, hi = N * rank // world, N * (rank + 1) // world
        assert s.index_base == lo and s.fine.dtype == torch.bfloat16 and torch.equal(s.fine, fine[lo:hi])
        assert torch.equal(s.rows, coarse[lo:hi]) and torch.equal(s.scales, scales[lo:hi])
        sg = G.sharded_gallery_from(s, rank, world)
        assert sg.fine_rows is s.fine and sg.index_base == lo
    with pytest.raises(ValueError, match="no fine_descriptors.npy"):
        G.load_gallery_shard(plain, cpu, load_fine=True)
    for bad in (fine[:40], fine.float(), fine[0]):
        with pytest.raises(ValueError, match="fine must be"):
            G.save_gallery(str(tmp_path / "bad"), coarse, labels, scales=scales, fine=bad)
    G.save_gallery(two, coarse, labels, scales=scales)       # written over without them: the stale file goes
    assert not os.path.exists(os.path.join(two, G.FINE_FILE))
    assert G.load_gallery_shard(two, cpu).fine is None
    fields = [f.name for f in G.GalleryShard.__dataclass_fields__.values()]
    assert fields[-1] == "fine" and fields[:8] == ["rows", "scales", "labels", "n_total", "index_base", "dtype", "labels_dev", "projection"]


# ---------------------------------------------------------------------------------- search_reranked, CPU engine
def f32_key(v32):
    bits = v32.view(np.int32).astype(np.int64)
    return np.where(bits >= 0, bits, -(bits & 0x7fffffff) - 1)


def rerank_f64(q, idx, rows, index_base, k):
    """The contract of include/vpr_amd_rerank.h with f64 sums: q [B, D], idx int32 [B, kc], rows [n, D] (torch, any float dtype)
    -> (vals f32 [B, k], idx int32 [B, k]): live candidates by (f32 of the f64 score desc, index asc), NaN scores after the
    numeric ones as -inf, the rest (-inf, -1)."""
    q64, r64, cand = q.double().numpy(), rows.double().numpy(), idx.numpy().astype(np.int64)
    B, kc = cand.shape
    vals, out = np.full((B, k), -np.inf, dtype=np.float32), np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        rel = cand[b] - index_base
        live = np.nonzero((rel >= 0) & (rel < r64.shape[0]))[0]
        with np.errstate(all="ignore"):
            s = (r64[rel[live]] @ q64[b]).astype(np.float32)
        order = sorted(range(len(live)), key=lambda t: (bool(np.isnan(s[t])), 0 if np.isnan(s[t]) else -int(f32_key(s[t:t + 1])[0]),
                                                        int(cand[b, live[t]]), int(live[t])))[:k]
        for pos, t in enumerate(order):
            vals[b, pos] = -np.inf if np.isnan(s[t]) else s[t]
            out[b, pos] = cand[b, live[t]]
    return torch.from_numpy(vals), torch.from_numpy(out)


class CpuEngine:
    """oracle/knn.py searches and merge; the re-rank is the f64 restatement above."""

    def local_topk(self, q, gallery, k, index_base, scales=None):
        from oracle import knn as oknn
        if scales is None:
            return oknn.knn_topk(q, gallery, k, index_base)
        q8, qs = oknn.quantize_fp8_rows(q.float())
        return oknn.knn_topk_fp8(q8, qs, gallery, scales, k, index_base)

    def merge(self, vals, idxs):
        from oracle import knn as oknn
        return oknn.topk_merge(vals, idxs)

    def rerank(self, q, idx, rows, index_base, k, ws=None):
        return rerank_f64(q, idx, rows, index_base, k)


def near_duplicates(seed, N, D, B, group=6, noise=0.04):
    """Groups of `group` near-duplicates (noise `noise`) around each query, the rest i.i.d. unit rows, shuffled: fine rows bf16
    [N, D], queries bf16 [B, D]."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    q = unit(rng.standard_normal((B, D)))
    rows = unit(rng.standard_normal((N, D)))
    rows[:B * group] = unit(np.repeat(q, group, 0) + noise * unit(rng.standard_normal((B * group, D))))
    rows = rows[rng.permutation(N)]
    return torch.from_numpy(rows).to(torch.bfloat16), torch.from_numpy(q).to(torch.bfloat16)


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("coarse", ["fp8", "bf16_half"])
def test_search_reranked_is_the_fine_topk_of_the_coarse_union(monkeypatch, R, coarse):
    """Shards of N = 83 rows at the uneven cuts of shard_bounds; the collective is replaced by a stack of every rank's list."""
    from oracle import knn as oknn
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, kc, k = 83, 128, 6, 8, 5
    fine, q = near_duplicates(11 + R, N, D, B)
    if coarse == "fp8":
        c_rows, c_scales = oknn.quantize_fp8_rows(fine.float())
        q_coarse = q
    else:                                                    # a narrower coarse tier: the first half of the columns
        c_rows, c_scales, q_coarse = fine[:, :D // 2].contiguous(), None, q[:, :D // 2].contiguous()
    eng = CpuEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(c_rows[lo:hi], N, r, R, engine=eng, scales=None if c_scales is None else c_scales[lo:hi],
                                     fine_rows=fine[lo:hi], force_collectives=R == 1 and coarse == "fp8"))
    sizes = [s.rows.shape[0] for s in shards]
    assert sum(sizes) == N and (R < 3 or len(set(sizes)) > 1)
    sent = {}

    def record(v, i, world, group=None):                     # first pass: what each rank would send
        sent[rank] = (v.clone(), i.clone())
        return torch.stack([v] * world), torch.stack([i] * world)

    def stacked(v, i, world, group=None):                    # second pass: every rank receives all of them, in rank order
        assert torch.equal(v, sent[rank][0]) and torch.equal(i, sent[rank][1])
        return torch.stack([sent[r][0] for r in range(world)]), torch.stack([sent[r][1] for r in range(world)])

    results = []
    for fn in (record, stacked):
        monkeypatch.setattr(retrieval, "all_gather_topk", fn)
        results = []
        for rank, sg in enumerate(shards):
            results.append(sg.search_reranked(q_coarse, k, kc, q_fine=q))
            if not sg.collective:
                sent[rank] = results[-1]
    # reference: the union of the shards' coarse top-kc, by f64 fine score
    union = []
    for r, sg in enumerate(shards):
        _, ci = eng.local_topk(q_coarse, sg.rows, kc, sg.index_base, *([] if sg.scales is None else [sg.scales]))
        assert (ci >= 0).all() and sent[r][1].shape == (B, k)
        union.append(ci)
    want_v, want_i = rerank_f64(q, torch.cat(union, 1), fine, 0, k)
    for v, i in results:                                     # the same on every rank
        assert torch.equal(i, want_i) and torch.equal(v, want_v)
    # the point: the fine order differs from the coarse one somewhere, and the answer is the fine top-1 of the whole gallery
    exact = (q.double() @ fine.double().T)
    assert torch.equal(want_i[:, 0].long(), exact.argmax(1))
    coarse_top = eng.merge(torch.stack([eng.local_topk(q_coarse, s.rows, k, s.index_base, *([] if s.scales is None else [s.scales]))[0] for s in shards]),
                           torch.stack([eng.local_topk(q_coarse, s.rows, k, s.index_base, *([] if s.scales is None else [s.scales]))[1] for s in shards]))[1]
    assert not torch.equal(coarse_top, want_i)
    if R == 1 and coarse == "bf16_half":                     # q_fine None: q_all is the fine query and must have its width
        with pytest.raises(ValueError, match="wide"):
            shards[0].search_reranked(q_coarse, k, kc)
        same = ShardedGallery(fine, N, engine=eng, fine_rows=fine.float()).search_reranked(q, k, kc)
        assert torch.equal(same[1], rerank_f64(q, eng.local_topk(q, fine, kc, 0)[1], fine, 0, k)[1])
