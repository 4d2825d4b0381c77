"""CPU: the extension include/vpr_amd_local_hires.h without a device — header, ctypes table and exported symbols agree; the older
tables are untouched; every refusal of both calls in the stated order, writing nothing; the 256-patch calls still refuse 257;
the workspace rule; fake ops and torch.export at 257, 529 and 1369 patches; the wrappers' refusals by message; the routing of
the hires keywords on an injected CPU engine that records which entry ran; and the order-pin input of the GPU test: the numpy
f32 emulation of the stated sum order gives other bits there than a plain ascending sum."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
ENTRIES = (("vpr_hires_local_rerank", 32), ("vpr_hires_patch_rerank_fp8", 64))      # (symbol, the width's granule)


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_local_hires.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header and "eleventh" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.LOCAL_HIRES_PROTOTYPES) == {"vpr_hires_local_workspace_bytes", "vpr_hires_local_rerank",
                                                            "vpr_hires_patch_rerank_fp8"}
    for name, (restype, argtypes) in _lib.LOCAL_HIRES_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    for name, _ in ENTRIES:                                  # the 22 parameters of the 256-patch calls
        assert _lib.LOCAL_HIRES_PROTOTYPES[name] == _lib.LOCAL_PROTOTYPES["vpr_local_rerank"] and len(_lib.LOCAL_HIRES_PROTOTYPES[name][1]) == 22
    assert _lib.LOCAL_HIRES_PROTOTYPES["vpr_hires_local_workspace_bytes"] == _lib.LOCAL_PROTOTYPES["vpr_local_workspace_bytes"]
    assert int(re.search(r"#define VPR_LOCAL_HIRES_MAX_N (\d+)", code).group(1)) == _lib.LOCAL_HIRES_MAX_N == refh.MAX_N == 1369 == 37 * 37
    from vpr_amd.backbone import DinoV2
    assert DinoV2("vit_small", 518).num_patches == _lib.LOCAL_HIRES_MAX_N   # = the largest token count the aggregation takes
    assert re.search(r"#define VPR_LOCAL_HIRES_SUM_ROUNDINGS\(n_g\) \(VPR_LOCAL_SUM_ROUNDINGS \+ \(\(n_g\) \+ 255\) / 256\)", code)
    for n_g, L in ((1, 11), (256, 11), (257, 12), (529, 13), (1280, 15), (1281, 16), (1369, 16)):
        assert _lib.local_hires_sum_roundings(n_g) == refh.sum_roundings(n_g) == L == 10 + -(-n_g // 256)
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
    assert set(_lib.LOCAL_PROTOTYPES) == {"vpr_local_workspace_bytes", "vpr_local_rerank"}
    assert set(_lib.SALAD_F32_STAGES_PROTOTYPES) == {"vpr_salad_f32_stage_outputs"}
    assert set(_lib.PATCH_FP8_PROTOTYPES) == {"vpr_patch_quantize_fp8", "vpr_patch_workspace_bytes_fp8", "vpr_patch_rerank_fp8"}
    assert len(_lib.PROTOTYPES) == 61 and _lib.LOCAL_MAX_N == 256 and _lib.LOCAL_MAX_KC == 128 and _lib.LOCAL_MAX_L == 256
    new = set(_lib.LOCAL_HIRES_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
                  _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES, _lib.LOCAL_PROTOTYPES,
                  _lib.SALAD_F32_STAGES_PROTOTYPES, _lib.PATCH_FP8_PROTOTYPES):
        assert not new & set(older)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_local_hires.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "vpr_hires_" not in text and "LOCAL_HIRES" not in text, other


def test_refusals_come_back_without_a_device_and_write_nothing(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 8192)()
    ctypes.memset(buf, 0xA5, 8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    odd2 = ctypes.c_void_p(p.value + 2)                      # not even 4-byte aligned
    big = 1 << 40
    nan = float("nan")
    for name, step in ENTRIES:
        entry = getattr(lib, name)

        def call(q=p, n_q=300, idx=p, B=1, kc=10, g=p, n_g=1369, l=64, n_local=5, base=0, min_sim=0.0, k=3, vals=p, out=p, mt=p,
                 ps=null, pm=null, rn=null, cn=null, ws=p, ws_bytes=big):
            st = entry(q, n_q, idx, B, kc, g, n_g, l, n_local, base, min_sim, k, vals, out, mt, ps, pm, rn, cn, ws, ws_bytes, null)
            assert bytes(buf) == b"\xa5" * 8192, "a refused call (and B == 0) writes nothing"
            return st

        for kw in (dict(q=null), dict(idx=null), dict(g=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1), dict(n_q=-1),
                   dict(n_g=-5), dict(l=-64), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2),
                   dict(kc=0, k=0), dict(min_sim=nan), dict(B=0, q=null),
                   # double faults: the invalid argument is reported ahead of what is merely unsupported
                   dict(kc=200, k=201), dict(q=null, l=48), dict(k=0, n_q=1370), dict(min_sim=nan, ws_bytes=0), dict(base=-1, q=odd),
                   dict(n_local=-1, kc=129, k=1), dict(min_sim=nan, n_g=1370), dict(idx=null, n_q=0)):
            assert call(**kw) == INVALID, (name, kw)
        for kw in (dict(kc=129, k=1), dict(kc=129, k=129), dict(n_q=0), dict(n_g=0), dict(n_q=1370), dict(n_g=1370), dict(n_g=1 << 20),
                   dict(l=0), dict(l=16), dict(l=48), dict(l=288), dict(l=320), dict(l=1 << 20), dict(q=odd), dict(g=odd), dict(ws=odd),
                   dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(mt=odd2), dict(ps=odd2), dict(pm=odd2), dict(rn=odd2), dict(cn=odd2),
                   dict(ws_bytes=0),
                   # double faults: a shape or alignment fault together with a short workspace is still UNSUPPORTED
                   dict(l=48, ws_bytes=0), dict(q=odd, ws_bytes=0), dict(n_q=1370, l=48), dict(n_q=1370, n_g=0), dict(kc=129, k=1, n_g=1370)):
            assert call(**kw) == UNSUPPORTED, (name, kw)
        if step == 64:                                       # l = 32 and 96: bf16 only
            assert call(l=32) == UNSUPPORTED and call(l=96) == UNSUPPORTED and call(l=32, n_q=1370) == UNSUPPORTED
        assert call(B=0, l=32) == (0 if step == 32 else UNSUPPORTED) and call(B=0, l=96) == (0 if step == 32 else UNSUPPORTED)
        for B, kc in ((1, 1), (1, 10), (64, 64), (37, 128), (100000, 128)):            # workspace: one byte short is refused
            need = lib.vpr_hires_local_workspace_bytes(B, kc)
            assert need >= 8 * B * kc and call(B=B, kc=kc, k=1, ws_bytes=need - 1) == UNSUPPORTED
        # what the rules leave alone: B = 0 launches nothing; the largest legal sizes on either side, independently
        assert call(B=0) == 0 and call(B=0, n_q=1369, n_g=1369, l=256, kc=128, k=128) == 0 and call(B=0, n_q=1, n_g=1, l=64, kc=1, k=1) == 0
        assert call(B=0, n_q=1369, n_g=1) == 0 and call(B=0, n_q=1, n_g=1369) == 0 and call(B=0, n_q=257, n_g=256) == 0
        assert call(B=0, idx=odd, vals=odd, out=odd, mt=null) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
        assert call(B=0, ps=p, pm=p, rn=p, cn=p, min_sim=float("inf")) == 0 and call(B=0, min_sim=-float("inf")) == 0
        assert call(B=0, ws_bytes=lib.vpr_hires_local_workspace_bytes(0, 10)) == 0
        for l in range(step, 257, step):
            assert call(B=0, l=l) == 0
    # the 256-patch calls still refuse 257 patches on either side
    for old in (lib.vpr_local_rerank, lib.vpr_patch_rerank_fp8):
        for n_q, n_g in ((257, 16), (16, 257), (1369, 1369)):
            assert old(p, n_q, p, 0, 10, p, n_g, 64, 5, 0, 0.0, 3, p, p, p, null, null, null, null, p, big, null) == UNSUPPORTED
        assert old(p, 256, p, 0, 10, p, 256, 64, 5, 0, 0.0, 3, p, p, p, null, null, null, null, p, big, null) == 0
    assert bytes(buf) == b"\xa5" * 8192


def test_workspace_query_is_monotone(lib):
    w = lib.vpr_hires_local_workspace_bytes
    for kc in (1, 2, 63, 64, 65, 128):
        sizes = [w(B, kc) for B in list(range(0, 300)) + [4096, 65536, 1 << 20]]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), kc
    for B in (0, 1, 3, 37, 64, 5000):
        sizes = [w(B, kc) for kc in range(1, 129)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), B
    for B, kc in ((-1, 10), (1, 0), (1, -3), (1, 129), (64, 1000), (-5, 200)):
        assert w(B, kc) == 0, (B, kc)


@pytest.mark.parametrize("op,dtype", [("local_rerank_hires", torch.bfloat16), ("local_rerank_fp8_hires", torch.uint8)])
def test_fake_ops_give_shapes_and_dtypes_and_export(op, dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert op in torch_ops.OPS
    fn = getattr(torch.ops.vpr, op)
    schema = str(fn.default._schema)
    assert schema.startswith(f"vpr::{op}(") and "int index_base=0" in schema.replace("Int", "int")
    assert "k=None" in schema and "float min_sim=0" in schema.replace("Float", "float")
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        idx = mk(37, 64, dtype=torch.int32)
        for n_q, n_g in ((257, 257), (529, 1369), (1369, 529), (1369, 1369)):
            q, g = mk(37, n_q, 128, dtype=dtype), mk(50, n_g, 128, dtype=dtype)
            for args, k in (((q, idx, g), 64), ((q, idx, g, 1000), 64), ((q, idx, g, 0, 10), 10), ((q, idx, g, 7, 1, 0.5), 1)):
                v, i, m = fn(*args)
                assert v.shape == i.shape == m.shape == (37, k) and v.device.type == "cuda"
                assert v.dtype == torch.float32 and i.dtype == torch.int32 and m.dtype == torch.int32

    class Rerank(torch.nn.Module):
        def forward(self, q, idx, g):
            v, i, m = fn(q, idx, g, 3, 5, 0.25)
            return v * 2, i, m

    for n in (257, 529, 1369):
        ep = torch.export.export(Rerank(), (torch.zeros(4, n, 64, dtype=dtype), torch.zeros(4, 8, dtype=torch.int32),
                                            torch.zeros(3, n, 64, dtype=dtype)))
        assert f"vpr.{op}" in str(ep.graph)
        assert [tuple(n_.meta["val"].shape) for n_ in ep.graph.nodes if n_.op == "output" for n_ in n_.args[0]] == [(4, 5)] * 3


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, n, kc, N = 2, 300, 4, 3
    for op, dtype, l, step in ((ops.local_rerank_hires, torch.bfloat16, 32, 32), (ops.local_rerank_fp8_hires, torch.uint8, 64, 64)):
        z = lambda *s: torch.zeros(*s, dtype=dtype)
        q, i, g = z(B, n, l), torch.zeros(B, kc, dtype=torch.int32), z(N, n, l)
        with monkeypatch.context() as mp:
            with pytest.raises(RuntimeError, match="GPU tensor"):
                op(q, i, g)
            with pytest.raises(RuntimeError, match="GPU tensor"):
                getattr(torch.ops.vpr, op.__name__)(q, i, g)
            # the remaining checks, with the device test answered "yes": nothing below reaches the library
            mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
            mp.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
            for bad, match in (((q.float(), i, g), "q_local: expected dtype"), ((q, i, g.float()), "g_local: expected dtype"),
                               ((q, i.long(), g), "idx: expected dtype"), ((q[0], i, g), "q_local: expected 3 dims"),
                               ((q, i[:, :2], g), "contiguous"), ((q[:1], i, g), "disagree on B"), ((q, i, z(N, n, 2 * l)), "disagree on l"),
                               ((z(B, n, 48), i, z(N, n, 48)), f"multiple of {step}"), ((z(B, n, 320), i, z(N, n, 320)), f"multiple of {step}"),
                               ((z(B, 1370, l), i, g), "q_local must hold 1..1369 patches"), ((q, i, z(N, 1370, l)), "g_local must hold 1..1369 patches"),
                               ((z(B, 0, l), i, g), "q_local must hold 1..1369 patches"),
                               ((q, torch.zeros(B, 129, dtype=torch.int32), g), "1..128 candidates"),
                               ((q, torch.zeros(B, 0, dtype=torch.int32), g), "1..128 candidates")):
                with pytest.raises(RuntimeError, match=match):
                    op(*bad)
            for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(min_sim=float("nan")), "min_sim must be")):
                with pytest.raises(RuntimeError, match=match):
                    op(q, i, g, **kw)
            # the 256-patch wrappers keep their limit and their words
            old = ops.local_rerank if dtype == torch.bfloat16 else ops.local_rerank_fp8
            with pytest.raises(RuntimeError, match="q_local must hold 1..256 patches"):
                old(z(B, 257, l), i, z(N, 16, l))
            with pytest.raises(RuntimeError, match="g_local must hold 1..256 patches"):
                old(z(B, 16, l), i, z(N, 257, l))


# ------------------------------------------------------------------------------------------------ routing, CPU engine
class RecordingEngine:
    """oracle/knn.py searches and merge; the four local re-rank entries are the f64 restatements and record their names."""

    def __init__(self):
        self.calls = []

    def local_topk(self, q, gallery, k, index_base, scales=None):
        from oracle import knn as oknn
        return oknn.knn_topk(q, gallery, k, index_base)

    def merge(self, vals, idxs):
        from oracle import knn as oknn
        return oknn.topk_merge(vals, idxs)

    def quantize_patch_fp8(self, feats):
        return ref8.quantize_t(feats)

    def _run(self, name, fn, q_local_feats, idx, local_feats, index_base, k, min_sim):
        self.calls.append((name, q_local_feats.shape[1], local_feats.shape[1]))
        out = fn(q_local_feats, idx, local_feats, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["matches"])

    def local_rerank(self, *a):
        return self._run("local_rerank", ref.local_rerank, *a)

    def local_rerank_hires(self, *a):
        return self._run("local_rerank_hires", ref.local_rerank, *a)

    def local_rerank_fp8(self, *a):
        return self._run("local_rerank_fp8", ref8.local_rerank_fp8, *a)

    def local_rerank_fp8_hires(self, *a):
        return self._run("local_rerank_fp8_hires", ref8.local_rerank_fp8, *a)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_search_local_reranked_at_300_patches_is_the_local_topk_of_the_coarse_union(monkeypatch, R):
    """Shards of N = 41 rows at the uneven cuts of shard_bounds, 300 patches per image, local_hires=True; the collective is
    replaced by a stack of every rank's list.  The hires entry runs, once per rank and pass."""
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, n, l, kc, k = 41, 64, 3, 300, 32, 6, 4
    rows, local, q, ql, true = ref.places(11 + R, N, D, B, n, l)
    eng = RecordingEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(rows[lo:hi], N, r, R, engine=eng, local_feats=local[lo:hi], force_collectives=R == 1, local_hires=True))
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
    assert eng.calls == [("local_rerank_hires", n, n)] * (2 * R)
    union = torch.cat([eng.local_topk(q, sg.rows, kc, sg.index_base)[1] for sg in shards], 1)
    want = ref.local_rerank(ql, union, local, 0, k, 0.3)
    for v, i in results:                                     # the same on every rank
        assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy().view(np.int32), want["vals"].view(np.int32))
    assert np.array_equal(want["idx"][:, 0], true) and (want["matches"][:, 0] == n).all()


def test_the_entry_follows_the_patch_counts_and_the_gallery_dtype():
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    N, D, B, l, kc, k = 9, 64, 2, 64, 4, 2
    rng = np.random.default_rng(3)
    bf = lambda *s: torch.from_numpy(ref.unit(rng.standard_normal(s))).to(torch.bfloat16)
    rows, q = bf(N, D), bf(B, D)
    for n_q, n_g, hires in ((200, 200, False), (300, 300, True), (200, 300, True), (300, 200, True), (256, 256, False), (257, 1, True),
                            (1, 257, True), (1369, 40, True)):
        local, ql = bf(N, n_g, l), bf(B, n_q, l)
        for fp8 in (False, True):
            eng = RecordingEngine()
            sg = ShardedGallery(rows, N, engine=eng, local_feats=ref8.quantize_t(local) if fp8 else local, local_hires=True)
            sg.search_local_reranked(q, k, kc, ql, 0.1)
            sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, min_sim=0.1)
            sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=0.1)
            name = "local_rerank" + ("_fp8" if fp8 else "") + ("_hires" if hires else "")
            assert eng.calls == [(name, n_q, n_g)] * 3, (n_q, n_g, fp8)
            closed = ShardedGallery(rows, N, engine=eng, local_feats=sg.local_feats)         # local_hires defaults to False
            if hires:
                for call in (lambda: closed.search_local_reranked(q, k, kc, ql, 0.1),
                             lambda: closed.search_gathered(q, k, local_rerank=kc, q_local_feats=ql),
                             lambda: closed.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql)):
                    with pytest.raises(ValueError, match="at most 256 patches"):
                        call()
            else:
                closed.search_local_reranked(q, k, kc, ql, 0.1)
                assert eng.calls[-1] == (name, n_q, n_g)
    sg = ShardedGallery(rows, N, engine=RecordingEngine(), local_feats=bf(N, 300, l), local_hires=True)
    with pytest.raises(ValueError, match="at most 1369 patches"):
        sg.search_local_reranked(q, k, kc, bf(B, 1370, l), 0.1)
    assert sg.engine.calls == []
    # both kinds of second stage at once stay refused by name
    with pytest.raises(ValueError, match="local_rerank and rerank"):
        sg.search_gathered(q, 2, rerank=4, local_rerank=4, q_local_feats=bf(B, 300, l))
    with pytest.raises(ValueError, match="does not combine with expand"):
        sg.search_gathered(q, 2, (2, 3.0), local_rerank=4, q_local_feats=bf(B, 300, l))
    with pytest.raises(ValueError, match="neither with rerank nor with expand"):
        GraphedRetrieval(sg, B, 2, rerank=4, local_rerank=4)


def test_local_features_and_features_take_hires_by_keyword():
    from vpr_amd.modules import DinoV2Salad, SaladAggregator
    torch.manual_seed(0)
    agg = SaladAggregator(64, hidden=64)
    for n in (257, 1369):
        feats = agg.local_features(torch.randn(1, n, 64), hires=True)
        assert feats.shape == (1, n, 128) and feats.dtype == torch.bfloat16
        assert torch.allclose(feats.float().norm(dim=2), torch.ones(1, n), atol=4e-3)
        with pytest.raises(ValueError, match=r"SaladAggregator\.local_features: .* at most 256"):
            agg.local_features(torch.zeros(1, n, 64))                          # without hires: refused as today
    with pytest.raises(ValueError, match=r"local_features\(hires=True\): 1370 patch tokens .* at most 1369"):
        agg.local_features(torch.zeros(1, 1370, 64), hires=True)
    with pytest.raises(ValueError, match="at most 256"):
        agg.local_features(torch.zeros(1, 1370, 64))
    tokens = torch.randn(2, 200, 64)
    assert torch.equal(agg.local_features(tokens, hires=True).view(torch.int16), agg.local_features(tokens).view(torch.int16))
    # DinoV2Salad.features: decided from the grid, before anything runs (CPU tensors of zeros are fine)
    for px, n in ((322, 529), (518, 1369)):
        ext = DinoV2Salad("vit_small", img_size=px)
        assert ext.backbone.num_patches == n
        seen = []
        ext._features = lambda x, want_bf16, events, keep=None: (keep.append(torch.zeros(x.shape[0], n, 384)), torch.zeros(x.shape[0], 8448))[1]
        ext.aggregator.local_features = lambda t, fp8=False, hires=False: (seen.append((tuple(t.shape), fp8, hires)), "local")[1]
        assert ext.features(torch.zeros(1, 3, px, px), want_local=True, hires=True)[1] == "local"
        assert ext.features(torch.zeros(1, 3, px, px), want_local="fp8", hires=True)[1] == "local"
        assert seen == [((1, n, 384), False, True), ((1, n, 384), True, True)]
        with pytest.raises(ValueError, match=r"features\(want_local=True\): .* at most 256"):
            ext.features(torch.zeros(1, 3, px, px), want_local=True)
        assert len(seen) == 2
    big = DinoV2Salad("vit_small", img_size=518)
    big.backbone.num_patches = 1370                                            # a grid the aggregation itself would refuse
    with pytest.raises(ValueError, match=r"hires=True\): 1370 patch tokens .* at most 1369"):
        big.features(torch.zeros(1, 3, 518, 518), want_local=True, hires=True)


def test_evaluation_entry_points_take_local_hires():
    import inspect
    from vpr_amd import evaluate
    for fn in (evaluate.build_gallery_from_images, evaluate.calculate_retrieval_scores):
        par = inspect.signature(fn).parameters["local_hires"]
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
        for size in ("135 KB", "68 KB", "350 KB", "175 KB"):
            assert size in fn.__doc__, (fn.__name__, size)
    assert 529 * 128 * 2 == 135424 and 529 * 128 == 67712 and 1369 * 128 * 2 == 350464 and 1369 * 128 == 175232


# ------------------------------------------------------------------------------------------------------ the order pin
def test_stated_sum_order_restated_and_told_from_an_ascending_sum():
    """The emulation on hand-made values, and the premise of the GPU order pin: on its input the stated order and a plain
    ascending f32 sum give different bits (so the device cannot pass with another order), every similarity is exact in f32 and
    the sum passes 2^24."""
    one = np.zeros(256, dtype=np.float32)
    one[0], one[32], one[64] = 2.0 ** 24, 1.0, 1.0           # lane 0 + lane 32 rounds the 1 away; the next wave's 1 then too
    assert refh.block_sum(one) == np.float32(2.0 ** 24)
    one[32], one[33], one[1] = 0.0, 1.0, 1.0                 # lanes 1 and 33 meet first: 2, which survives beside 2^24;
    assert refh.block_sum(one) == np.float32(2.0 ** 24 + 4)  # the next wave's 1 makes 2^24 + 3, a tie that goes to the even 2^24 + 4
    one[64] = 0.0
    assert refh.block_sum(one) == np.float32(2.0 ** 24 + 2)
    v = np.zeros(600, dtype=np.float32)
    v[0], v[256], v[257], v[512] = 2.0 ** 24, 1.0, 1.0, 1.0  # block 1 sums to 2 first; block 2's 1 then makes the tie 2^24 + 3 -> + 4;
    assert refh.score_in_stated_order(v) == np.float32(2.0 ** 24 + 4) and refh.ascending_sum(v) == np.float32(2.0 ** 24)   # one by one: all lost
    huge = np.full(300, np.finfo(np.float32).max, dtype=np.float32)
    assert refh.score_in_stated_order(huge) == refh.FLT_MAX and refh.score_in_stated_order(-huge) == -refh.FLT_MAX
    huge[256:] *= -1                                         # clamped block by block: no Inf - Inf
    assert refh.score_in_stated_order(huge) == 0.0
    small = np.arange(200, dtype=np.float32)                 # n_g <= 256: the rule of the 256-patch header, then +0 + x
    assert refh.score_in_stated_order(small) == refh.block_sum(np.concatenate([small, np.zeros(56, np.float32)])) == 19900.0
    q, g = refh.order_pin_input()
    assert q.shape == g.shape == (1, 1369, 256) and float(q.float().abs().max()) == 16.0
    contrib, p = refh.matched_contrib(q[0], g[0])
    assert p["matches"] == 1369 and float(np.abs(p["S"]).max()) < 2.0 ** 17
    stated, plain = refh.score_in_stated_order(contrib), refh.ascending_sum(contrib)
    exact = float(contrib.astype(np.float64).sum())
    assert exact > 2.0 ** 24 and stated.view(np.int32) != plain.view(np.int32), (stated, plain, exact)
    assert abs(float(stated) - exact) <= ref.gamma(refh.sum_roundings(1369)) * exact
