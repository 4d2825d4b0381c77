"""CPU: the local-feature re-ranking extension of the C ABI (include/vpr_amd_local.h) — header, binding table and exported
symbols agree, the older tables are what they were, every refusal comes back with its status in the stated order before a
device is touched and leaves the outputs alone, the workspace query is monotone, the torch op has a fake implementation and
exports, the wrappers refuse what they cannot take; the f64 restatement of the contract (tests/local_match_ref.py) checked on
hand-made matrices and on the recipe the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import local_match_ref as ref

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
    header = open(os.path.join(ROOT, "include", "vpr_amd_local.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LOCAL_PROTOTYPES) == {"vpr_local_workspace_bytes", "vpr_local_rerank"}
    for name, (restype, argtypes) in _lib.LOCAL_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    assert len(_lib.LOCAL_PROTOTYPES["vpr_local_rerank"][1]) == 22
    const = lambda n: int(re.search(rf"#define {n} (\d+)", code).group(1))
    assert const("VPR_LOCAL_MAX_N") == _lib.LOCAL_MAX_N == 256 and const("VPR_LOCAL_MAX_L") == _lib.LOCAL_MAX_L == 256
    assert const("VPR_LOCAL_MAX_KC") == _lib.LOCAL_MAX_KC == _lib.RERANK_MAX_KC == 128
    assert const("VPR_LOCAL_SUM_ROUNDINGS") == _lib.LOCAL_SUM_ROUNDINGS == ref.SUM_ROUNDINGS == 6 + 4
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    assert set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    assert set(_lib.SALAD_STAGES_PROTOTYPES) == {"vpr_salad_stage_outputs"}
    assert set(_lib.SALAD_ANYRES_PROTOTYPES) == {"vpr_salad_sinkhorn_aggregate_n", "vpr_salad_aggregate_n", "vpr_salad_aggregate_f32_n"}
    assert set(_lib.SALAD_HIRES_PROTOTYPES) == {"vpr_salad_sinkhorn_aggregate_hires", "vpr_salad_aggregate_hires",
                                                "vpr_salad_aggregate_f32_hires"}
    assert len(_lib.RERANK_PROTOTYPES["vpr_rerank_rows"][1]) == 16 and len(_lib.PROTOTYPES) == 61
    new = set(_lib.LOCAL_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
                  _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES):
        assert not new & set(older)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert "vpr_local" not in main and re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_local.h":
            assert "vpr_local" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_refusals_come_back_without_a_device_and_write_nothing(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 8192)()
    ctypes.memset(buf, 0xA5, 8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    odd2 = ctypes.c_void_p(p.value + 2)                      # not even 4-byte aligned
    big = 1 << 40
    nan = float("nan")

    def call(q=p, n_q=16, idx=p, B=1, kc=10, g=p, n_g=16, l=32, n_local=5, base=0, min_sim=0.0, k=3, vals=p, out=p, mt=p,
             ps=null, pm=null, rn=null, cn=null, ws=p, ws_bytes=big):
        st = lib.vpr_local_rerank(q, n_q, idx, B, kc, g, n_g, l, n_local, base, min_sim, k, vals, out, mt, ps, pm, rn, cn, ws,
                                  ws_bytes, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and B == 0) writes nothing"
        return st

    for kw in (dict(q=null), dict(idx=null), dict(g=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1), dict(n_q=-1),
               dict(n_g=-5), dict(l=-32), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2),
               dict(kc=0, k=0), dict(min_sim=nan), dict(B=0, q=null),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(kc=200, k=201), dict(q=null, l=48), dict(k=0, n_q=300), dict(min_sim=nan, ws_bytes=0), dict(base=-1, q=odd),
               dict(n_local=-1, kc=129, k=1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(kc=129, k=1), dict(kc=129, k=129), dict(n_q=0), dict(n_g=0), dict(n_q=257), dict(n_g=257), dict(n_g=1 << 20),
               dict(l=0), dict(l=16), dict(l=48), dict(l=288), dict(l=1 << 20), dict(q=odd), dict(g=odd), dict(ws=odd),
               dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(mt=odd2), dict(ps=odd2), dict(pm=odd2), dict(rn=odd2), dict(cn=odd2),
               dict(ws_bytes=0),
               # double faults: a shape or alignment fault together with a short workspace is still UNSUPPORTED
               dict(l=48, ws_bytes=0), dict(q=odd, ws_bytes=0), dict(n_q=257, l=48)):
        assert call(**kw) == UNSUPPORTED, kw
    for B, kc in ((1, 1), (1, 10), (64, 64), (37, 128), (100000, 128)):                # workspace: one byte short is refused
        need = lib.vpr_local_workspace_bytes(B, kc)
        assert need >= 8 * B * kc and call(B=B, kc=kc, k=1, ws_bytes=need - 1) == UNSUPPORTED
    # what the rules leave alone: B = 0 launches nothing; the largest legal sizes; element-aligned lists; no matches_out
    assert call(B=0) == 0 and call(B=0, n_q=256, n_g=256, l=256, kc=128, k=128) == 0 and call(B=0, n_q=1, n_g=1, l=32, kc=1, k=1) == 0
    assert call(B=0, idx=odd, vals=odd, out=odd, mt=null) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
    assert call(B=0, ps=p, pm=p, rn=p, cn=p, min_sim=float("inf")) == 0 and call(B=0, min_sim=-float("inf")) == 0
    assert call(B=0, ws_bytes=lib.vpr_local_workspace_bytes(0, 10)) == 0
    for l in range(32, 257, 32):
        assert call(B=0, l=l) == 0


def test_workspace_query_is_monotone(lib):
    w = lib.vpr_local_workspace_bytes
    for kc in (1, 2, 63, 64, 65, 128):
        sizes = [w(B, kc) for B in list(range(0, 300)) + [4096, 65536, 1 << 20]]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), kc
    for B in (0, 1, 3, 37, 64, 5000):
        sizes = [w(B, kc) for kc in range(1, 129)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), B
    assert w(64, 64) == 2 * 64 * 64 * 4
    for B, kc in ((-1, 10), (1, 0), (1, -3), (1, 129), (64, 1000), (-5, 200)):
        assert w(B, kc) == 0, (B, kc)


def test_fake_op_gives_shapes_and_dtypes_and_exports():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "local_rerank" in torch_ops.OPS
    schema = str(torch.ops.vpr.local_rerank.default._schema)
    assert schema.startswith("vpr::local_rerank(") and "int index_base=0" in schema.replace("Int", "int")
    assert "k=None" in schema and "float min_sim=0" in schema.replace("Float", "float")
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        idx = mk(37, 64, dtype=torch.int32)
        q, g = mk(37, 256, 128, dtype=torch.bfloat16), mk(500, 196, 128, dtype=torch.bfloat16)
        for args, k in (((q, idx, g), 64), ((q, idx, g, 1000), 64), ((q, idx, g, 0, 10), 10), ((q, idx, g, 7, 1, 0.5), 1)):
            v, i, m = torch.ops.vpr.local_rerank(*args)
            assert v.shape == i.shape == m.shape == (37, k) and v.device.type == "cuda"
            assert v.dtype == torch.float32 and i.dtype == torch.int32 and m.dtype == torch.int32

    class Rerank(torch.nn.Module):
        def forward(self, q, idx, g):
            v, i, m = torch.ops.vpr.local_rerank(q, idx, g, 3, 5, 0.25)
            return v * 2, i, m

    ep = torch.export.export(Rerank(), (torch.zeros(4, 64, 32, dtype=torch.bfloat16), torch.zeros(4, 8, dtype=torch.int32),
                                        torch.zeros(9, 50, 32, dtype=torch.bfloat16)))
    assert "vpr.local_rerank" in str(ep.graph)
    assert [tuple(n.meta["val"].shape) for n in ep.graph.nodes if n.op == "output" for n in n.args[0]] == [(4, 5)] * 3


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, n, l, kc, N = 2, 16, 32, 4, 5
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    q, i, g = bf(B, n, l), torch.zeros(B, kc, dtype=torch.int32), bf(N, n, l)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.local_rerank(q, i, g)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.local_rerank(q, i, g)
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    for bad, match in (((q.float(), i, g), "q_local: expected dtype"), ((q, i, g.float()), "g_local: expected dtype"),
                       ((q.view(torch.uint16), i, g), "q_local: expected dtype"), ((q, i.long(), g), "idx: expected dtype"),
                       ((q[0], i, g), "q_local: expected 3 dims"), ((q, i[0], g), "idx: expected 2 dims"), ((q, i, g[0]), "g_local: expected 3 dims"),
                       ((q, i[:, :2], g), "contiguous"), ((q[:, :, :16], i, g), "contiguous"),
                       ((q[:1], i, g), "disagree on B"), ((q, i, bf(N, n, 64)), "disagree on l"),
                       ((bf(B, n, 48), i, bf(N, n, 48)), "multiple of 32"), ((bf(B, n, 288), i, bf(N, n, 288)), "multiple of 32"),
                       ((bf(B, 257, l), i, g), "q_local must hold 1..256 patches"), ((q, i, bf(N, 257, l)), "g_local must hold 1..256 patches"),
                       ((bf(B, 0, l), i, g), "q_local must hold 1..256 patches"),
                       ((q, torch.zeros(B, 129, dtype=torch.int32), g), "1..128 candidates"),
                       ((q, torch.zeros(B, 0, dtype=torch.int32), g), "1..128 candidates")):
        with pytest.raises(RuntimeError, match=match):
            ops.local_rerank(*bad)
    for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(k=-1), "k must be"),
                      (dict(min_sim=float("nan")), "min_sim must be")):
        with pytest.raises(RuntimeError, match=match):
            ops.local_rerank(q, i, g, **kw)


# ------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_on_hand_made_matrices():
    S = np.array([[1., 5., 5., 0.],
                  [7., 5., 2., 0.],
                  [7., 1., 2., 0.]])
    fin = np.ones_like(S, dtype=bool)
    r, c = ref.nearest(S, fin)
    assert r.tolist() == [1, 0, 0] and c.tolist() == [1, 0, 0, 0]            # ties go to the lowest index
    m = ref.matched_columns(S, r, c, 0.0)
    assert m.tolist() == [True, True, False, False]                         # column 3: c = 0, but r(0) = 1
    assert ref.matched_columns(S, r, c, 6.0).tolist() == [True, False, False, False]
    fin[1, 0] = fin[2, 0] = False                                           # "no similarity" is never a neighbour
    r, c = ref.nearest(S, fin)
    assert r.tolist() == [1, 1, 2] and c.tolist() == [0, 0, 0, 0]
    fin[:, 3] = False
    fin[0, :] = False
    r, c = ref.nearest(S, fin)
    assert r.tolist() == [-1, 1, 2] and c.tolist() == [-1, 1, 1, -1]
    # NaN / Inf operands: columns 1 and 2 hold no similarity at all, match nothing, and the score stays finite
    q = torch.eye(4, 32)[:3].to(torch.bfloat16)
    g = torch.eye(4, 32).to(torch.bfloat16)
    g[1, 5], g[2, 2] = float("nan"), float("inf")
    p = ref.pair(q, g, 0.0)
    assert p["row_nn"].tolist() == [0, 0, 0] and p["col_nn"].tolist() == [0, -1, -1, 0] and p["matches"] == 1 and p["score"] == 1.0
    # the order: score desc by bit pattern, index asc, duplicates as often as they occur, (-inf, -1, 0) tail
    scores = np.array([2., 3., 2., 0., -0., 3.], dtype=np.float32)
    v, i, mt = ref.order(scores, np.arange(6), np.array([9, 4, 7, 1, 0, 4]), np.array([1, 1, 1, 1, 1, 1], bool), 6)
    assert i.tolist() == [4, 4, 7, 9, 1, 0] and mt.tolist() == [1, 5, 2, 0, 3, 4]
    v, i, mt = ref.order(scores, np.arange(6), np.array([9, 4, 7, 1, 0, 4]), np.array([1, 0, 0, 1, 0, 0], bool), 4)
    assert i.tolist() == [9, 1, -1, -1] and mt.tolist() == [0, 3, 0, 0] and v.tolist() == [2., 0., -np.inf, -np.inf]


@pytest.mark.parametrize("n,l", [(64, 32), (256, 128)])
def test_recipe_separates_the_true_image(n, l):
    """The recipe of the GPU tests: the true image matches every patch at similarity ~1; a distractor of random unit features
    keeps a fraction of chance mutual neighbours at the similarity of the best of n random directions in l dimensions
    (~ sqrt(2 ln n / l): 0.51 at (64, 32), 0.29 at (256, 128))."""
    q, gal = ref.recipe(3, n, l)
    idx = torch.arange(gal.shape[0], dtype=torch.int32)[None]
    out = ref.local_rerank(q, idx, gal, 0, None, 0.0)
    true = gal.shape[0] - 1
    print("true", out["pair_matches"][0, true], out["pair_score"][0, true], "distractors", out["pair_matches"][0, :true].max(),
          out["pair_score"][0, :true].max())
    assert out["idx"][0, 0] == true and out["matches"][0, 0] == n
    # noise of norm 0.02 costs 2e-4 of the cosine, the bf16 rounding of both sides at most 2^-8 more
    assert 0.995 * n <= out["vals"][0, 0] <= 1.004 * n
    # a column of an i.i.d. n x n matrix is a mutual maximum with probability n / (2 n - 1) ~ 1/2: n / 2 matches, standard
    # deviation below sqrt(n) / 2, so six of them is 3 sqrt(n); no similarity of n * n * 20 random pairs in l dimensions
    # passes sqrt(2 ln(20 n^2) / l) (the Gaussian tail of a coordinate of a random unit vector, union bound)
    most = n / 2 + 3 * np.sqrt(n)
    assert out["pair_matches"][0, :true].max() <= most
    assert out["pair_score"][0, :true].max() <= most * np.sqrt(2 * np.log(20 * n * n) / l) < 0.995 * n
    if l == 128:
        hard = ref.local_rerank(q, idx, gal, 0, None, 0.6)
        assert (hard["pair_score"][0, :true] == 0).all() and (hard["pair_matches"][0, :true] == 0).all()
        assert hard["idx"][0, 0] == true and hard["matches"][0, 0] == n


# ------------------------------------------------------------------------------------------------- gallery format
def test_gallery_round_trip_with_and_without_local_features(tmp_path):
    from vpr_amd import gallery as G
    rng = np.random.default_rng(5)
    N, D, n, l = 23, 128, 9, 32
    rows = torch.from_numpy(rng.standard_normal((N, D))).to(torch.bfloat16)
    local = torch.from_numpy(rng.standard_normal((N, n, l))).to(torch.bfloat16)
    labels = rng.standard_normal((N, 4))
    plain, two = str(tmp_path / "plain"), str(tmp_path / "two")
    G.save_gallery(plain, rows, labels)
    G.save_gallery(two, rows, labels, local=local)
    assert G.LOCAL_FILE == "local_features.npy" and "local_features.npy" in G.__doc__
    assert not os.path.exists(os.path.join(plain, G.LOCAL_FILE)) and os.path.exists(os.path.join(two, G.LOCAL_FILE))
    stored = np.load(os.path.join(two, "local_features.npy"))
    assert stored.dtype == np.uint16 and stored.shape == (N, n, l) and np.array_equal(stored, local.view(torch.uint16).numpy())
    cpu = torch.device("cpu")
    a, b = G.load_gallery_shard(plain, cpu), G.load_gallery_shard(two, cpu)      # load_local defaults to False: as ever
    assert a.local is None and b.local is None and torch.equal(b.rows, rows)
    assert G.sharded_gallery_from(b).local_feats is None
    for rank, world in ((0, 1), (0, 3), (1, 3), (2, 3)):
        s = G.load_gallery_shard(two, cpu, rank, world, load_local=True)
        lo, hi = N * rank // world, N * (rank + 1) // world
        assert s.index_base == lo and s.local.dtype == torch.bfloat16 and torch.equal(s.local, local[lo:hi]) and s.fine is None
        sg = G.sharded_gallery_from(s, rank, world)
        assert sg.local_feats is s.local and sg.fine_rows is None
    with pytest.raises(ValueError, match="no local_features.npy"):
        G.load_gallery_shard(plain, cpu, load_local=True)
    for bad in (local[:20], local.float(), local[0], local[:, 0]):
        with pytest.raises(ValueError, match="local must be"):
            G.save_gallery(str(tmp_path / "bad"), rows, labels, local=bad)
    G.save_gallery(two, rows, labels)                        # written over without them: the stale file goes
    assert not os.path.exists(os.path.join(two, G.LOCAL_FILE)) and G.load_gallery_shard(two, cpu).local is None


# ------------------------------------------------------------------------ search_local_reranked, CPU engine
class CpuEngine:
    """oracle/knn.py searches and merge; the local re-rank is the f64 restatement."""

    def local_topk(self, q, gallery, k, index_base, scales=None):
        from oracle import knn as oknn
        return oknn.knn_topk(q, gallery, k, index_base)

    def merge(self, vals, idxs):
        from oracle import knn as oknn
        return oknn.topk_merge(vals, idxs)

    def local_rerank(self, q_local_feats, idx, local_feats, index_base, k, min_sim=0.0):
        out = ref.local_rerank(q_local_feats, idx, local_feats, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["matches"])


@pytest.mark.parametrize("R", [1, 2, 3])
def test_search_local_reranked_is_the_local_topk_of_the_coarse_union(monkeypatch, R):
    """Shards of N = 83 rows at the uneven cuts of shard_bounds; the collective is replaced by a stack of every rank's list."""
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, n, l, kc, k = 83, 64, 5, 12, 32, 8, 5
    rows, local, q, ql, true = ref.places(11 + R, N, D, B, n, l)
    eng = CpuEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(rows[lo:hi], N, r, R, engine=eng, local_feats=local[lo:hi], force_collectives=R == 1))
    sent = {}

    def record(v, i, world, group=None):                     # first pass: what each rank would send
        sent[rank] = (v.clone(), i.clone())
        return torch.stack([v] * world), torch.stack([i] * world)

    def stacked(v, i, world, group=None):                    # second pass: every rank receives all of them, in rank order
        assert torch.equal(v, sent[rank][0]) and torch.equal(i, sent[rank][1])
        return torch.stack([sent[r][0] for r in range(world)]), torch.stack([sent[r][1] for r in range(world)])

    for fn in (record, stacked):
        monkeypatch.setattr(retrieval, "all_gather_topk", fn)
        results = []
        for rank, sg in enumerate(shards):
            results.append(sg.search_local_reranked(q, k, kc, ql, 0.3))
    union = torch.cat([eng.local_topk(q, sg.rows, kc, sg.index_base)[1] for sg in shards], 1)
    want = ref.local_rerank(ql, union, local, 0, k, 0.3)
    for v, i in results:                                     # the same on every rank
        assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy().view(np.int32), want["vals"].view(np.int32))
    # the point: the global descriptors cannot tell a place's views apart, the patches can
    assert np.array_equal(want["idx"][:, 0], true) and (want["matches"][:, 0] == n).all()
    coarse = eng.merge(*[torch.stack(t) for t in zip(*[eng.local_topk(q, sg.rows, k, sg.index_base) for sg in shards])])[1]
    assert not np.array_equal(coarse[:, 0].numpy(), true)


def test_sharded_wrappers_refuse_what_they_cannot_take():
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    N, D, B, n, l = 6, 64, 2, 5, 32
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    rows, local, q, ql = bf(N, D), bf(N, n, l), bf(B, D), bf(B, n, l)
    with pytest.raises(ValueError, match="local_feats must be"):
        ShardedGallery(rows, N, local_feats=local[:4])
    with pytest.raises(ValueError, match="local_feats must be"):
        ShardedGallery(rows, N, local_feats=local[:, 0])
    with pytest.raises(ValueError, match="local_feats must be"):
        ShardedGallery(rows[:3], N, 0, 2, local_feats=local)  # the whole gallery's, not the shard's
    with pytest.raises(ValueError, match="local_feats: bf16"):
        ShardedGallery(rows, N, local_feats=local.float())
    sg = ShardedGallery(rows, N, engine=CpuEngine(), local_feats=local, fine_rows=rows)
    for args, match in (((q, 3, 65, ql), "at most 64"), ((q, 1, 0, ql), "at most 64"), ((q, 5, 4, ql), "1..kc"),
                        ((q, 2, 4, bf(B, n, 64)), "wide"), ((q, 2, 4, bf(B + 1, n, l)), "disagree on B"),
                        ((q, 2, 4, ql.float()), "must be bf16"), ((q, 2, 4, ql[0]), "must be bf16"), ((q, 2, 4, None), "must be bf16"),
                        ((q, 2, 4, bf(B, 257, l)), "at most 256 patches")):
        with pytest.raises(ValueError, match=match):
            sg.search_local_reranked(*args)
    with pytest.raises(ValueError, match="no local_feats"):
        ShardedGallery(rows, N, engine=CpuEngine()).search_local_reranked(q, 2, 4, ql)
    # both kinds of second stage at once, by name
    for call in (lambda: sg.search_gathered(q, 2, rerank=4, local_rerank=4, q_local_feats=ql),
                 lambda: sg.search_local_queries(q, 2, None, 4, local_rerank=4, q_local_feats=ql)):
        with pytest.raises(ValueError, match="local_rerank and rerank"):
            call()
    with pytest.raises(ValueError, match="does not combine with expand"):
        sg.search_gathered(q, 2, (2, 3.0), local_rerank=4, q_local_feats=ql)
    with pytest.raises(ValueError, match="needs q_local_feats"):
        sg.search_local_queries(q, 2, local_rerank=4)
    with pytest.raises(ValueError, match="neither with rerank nor with expand"):
        GraphedRetrieval(sg, B, 2, rerank=4, local_rerank=4)
    with pytest.raises(ValueError, match="needs a gallery with local_feats"):
        GraphedRetrieval(ShardedGallery(rows, N, engine=CpuEngine()), B, 2, local_rerank=4)
    # SaladAggregator.local_features: more than 256 tokens is refused by name, before anything runs
    from vpr_amd.modules import SaladAggregator
    agg = SaladAggregator(64, hidden=64)
    with pytest.raises(ValueError, match="at most 256"):
        agg.local_features(torch.zeros(1, 257, 64))
    with pytest.raises(ValueError, match="patch tokens"):
        agg.local_features(torch.zeros(1, 16, 32))
    feats = agg.local_features(torch.cat([torch.randn(2, 15, 64), torch.zeros(2, 1, 64)], 1))
    assert feats.shape == (2, 16, 128) and feats.dtype == torch.bfloat16
    assert torch.allclose(feats.float().norm(dim=2), torch.ones(2, 16), atol=4e-3)


def _two_rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    N, D, B, n, l, kc, k = 83, 64, 3, 12, 32, 8, 5
    rows, local, q_all, ql_all, true = ref.places(41, N, D, world * B, n, l)
    lo, hi = shard_bounds(N, rank, world)
    eng = CpuEngine()
    sg = ShardedGallery(rows[lo:hi], N, rank, world, engine=eng, local_feats=local[lo:hi])
    mine = slice(rank * B, (rank + 1) * B)
    v, i = sg.search_local_queries(q_all[mine].contiguous(), k, local_rerank=kc, q_local_feats=ql_all[mine].contiguous(), min_sim=0.3)
    union = torch.cat([eng.local_topk(q_all, rows[slice(*shard_bounds(N, r, world))], kc, shard_bounds(N, r, world)[0])[1]
                       for r in range(world)], 1)
    want = ref.local_rerank(ql_all, union, local, 0, k, 0.3)
    ret[rank] = bool(np.array_equal(i.numpy(), want["idx"][mine]) and np.array_equal(v.numpy(), want["vals"][mine])
                     and np.array_equal(i[:, 0].numpy(), true[mine]))
    dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_gloo_ranks_get_their_own_rows_of_the_local_reranked_search():
    import torch.multiprocessing as mp
    world = 2
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_two_rank_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}
