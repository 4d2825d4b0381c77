"""CPU: the extension include/vpr_amd_similarity.h without a device — header, ctypes table and exported symbols agree; the twelve
older tables are untouched and disjoint; every refusal of the three calls in the stated order, writing nothing; the workspace
rule equals the spatial one; fake ops and torch.export at 256, 529 and 1369 patches; the wrappers' refusals by message; the
routing of spatial_model on an injected CPU engine that records which entry ran, sharded R = 1, 2, 3; and the restatement's own
properties (tests/similarity_ref.py): the hypothesis index rule, the int32 bounds, the planted-similarity identity, both tie
levels of the key, the M = 1 rule, and the premise of the GPU test's recipe."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import local_match_hires_ref as refh
import local_match_ref as ref
import similarity_ref as mref
import spatial_ref as sref
from test_spatial_cpu import RecordingEngine, _buffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = {"vpr_similarity_workspace_bytes", "vpr_similarity_verify", "vpr_similarity_local_rerank"}


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_similarity.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header and "thirteenth" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SIMILARITY_PROTOTYPES) == NAMES
    for name, (restype, argtypes) in _lib.SIMILARITY_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    # the parameter list of the spatial call in its order, pair_model in the place of pair_shift
    spatial = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd_spatial.h")).read(), flags=re.S)
    plist = lambda text, name: [" ".join(p.split()) for p in re.search(rf"{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    for ours, theirs in (("vpr_similarity_local_rerank", "vpr_spatial_local_rerank"), ("vpr_similarity_verify", "vpr_spatial_verify")):
        want = [p.replace("pair_shift", "pair_model").replace("int32_t* shift", "int32_t* model") for p in plist(spatial, theirs)]
        assert plist(code, ours) == want and want != plist(spatial, theirs)
        assert _lib.SIMILARITY_PROTOTYPES[ours] == _lib.SPATIAL_PROTOTYPES[theirs]
    const = lambda n: int(re.search(rf"#define {n} (\d+)", code).group(1))
    assert const("VPR_SIM_MAX_SIDE") == _lib.SIM_MAX_SIDE == mref.MAX_SIDE == 37
    assert const("VPR_SIM_HYPOTHESES") == _lib.SIM_HYPOTHESES == mref.HYPOTHESES == 256
    assert const("VPR_SIM_MAX_SCALE") == _lib.SIM_MAX_SCALE == mref.MAX_SCALE == 2
    assert const("VPR_SIM_MAX_TOL") == _lib.SIM_MAX_TOL == mref.MAX_TOL == 8
    assert const("VPR_SIM_MAX_N") == _lib.SIM_MAX_N == mref.MAX_N == _lib.LOCAL_HIRES_MAX_N == 1369 == 37 * 37
    assert "M = 1" in header                                 # the difference from the shift vote is stated
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move
    assert re.search(r"#define VPR_AMD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "vpr_amd.h")).read())


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.LOCAL_HIRES_PROTOTYPES) == {"vpr_hires_local_workspace_bytes", "vpr_hires_local_rerank", "vpr_hires_patch_rerank_fp8"}
    assert set(_lib.SPATIAL_PROTOTYPES) == {"vpr_spatial_workspace_bytes", "vpr_spatial_verify", "vpr_spatial_local_rerank"}
    assert len(_lib.PROTOTYPES) == 61 and len(_lib.SPATIAL_PROTOTYPES["vpr_spatial_local_rerank"][1]) == 28
    older = (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
             _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES, _lib.LOCAL_PROTOTYPES,
             _lib.SALAD_F32_STAGES_PROTOTYPES, _lib.PATCH_FP8_PROTOTYPES, _lib.LOCAL_HIRES_PROTOTYPES, _lib.SPATIAL_PROTOTYPES)
    assert len(older) == 13                                  # vpr_amd.h and the twelve older extensions
    assert sum(len(t) for t in older) == 61 + 1 + 2 + 3 + 2 + 1 + 3 + 3 + 2 + 1 + 3 + 3 + 3
    for table in older:
        assert not NAMES & set(table)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_similarity.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "vpr_similarity" not in text and "VPR_SIM_" not in text, other


def test_verify_refusals_come_back_without_a_device_and_write_nothing(lib):
    null = ctypes.c_void_p(0)
    buf, p, _, odd2 = _buffers()

    def call(partner=p, sim=p, P=2, n_q=256, gw_q=16, n_g=256, gw_g=16, tol=1, score=p, inl=p, mt=p, model=p, mask=null):
        st = lib.vpr_similarity_verify(partner, sim, P, n_q, gw_q, n_g, gw_g, tol, score, inl, mt, model, mask, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and P == 0) writes nothing"
        return st

    for kw in (dict(partner=null), dict(sim=null), dict(score=null), dict(inl=null), dict(mt=null), dict(model=null), dict(P=-1),
               dict(n_q=-1), dict(n_g=-256), dict(gw_q=-1), dict(gw_g=-16), dict(tol=-1), dict(P=0, sim=null),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(tol=-1, n_q=1370, gw_q=1370), dict(gw_q=-1, tol=9), dict(partner=null, gw_g=0), dict(P=-1, n_g=1370, gw_g=1),
               dict(gw_g=-3, score=odd2), dict(tol=-1, n_q=1368, gw_q=36), dict(model=null, n_g=1368, gw_g=38)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(gw_q=0), dict(gw_g=0), dict(gw_q=15), dict(gw_g=17), dict(gw_q=257), dict(n_q=255, gw_q=16), dict(tol=9), dict(tol=1 << 20),
               dict(n_q=1368, gw_q=38), dict(n_q=1368, gw_q=36),   # a side of 38: 38 x 36 and 36 x 38
               dict(n_g=1368, gw_g=38), dict(n_g=1368, gw_g=36), dict(n_g=38, gw_g=38), dict(n_q=38, gw_q=1),
               dict(n_q=1369, gw_q=1369), dict(n_g=1369, gw_g=1), dict(n_q=1369, gw_q=37, n_g=1369, gw_g=1369),       # 1369 x 1
               dict(n_q=1370, gw_q=37), dict(n_g=1370, gw_g=10), dict(n_q=0), dict(n_g=0), dict(n_q=0, gw_q=0),
               dict(partner=odd2), dict(sim=odd2), dict(score=odd2), dict(inl=odd2), dict(mt=odd2), dict(model=odd2),
               dict(gw_q=0, tol=9), dict(n_q=1370, gw_q=0), dict(tol=9, partner=odd2), dict(n_q=38, gw_q=38, tol=9), dict(n_g=38, gw_g=1, sim=odd2)):
        assert call(**kw) == UNSUPPORTED, kw
    # what the rules leave alone (P = 0 launches nothing): the largest grids, sides of 37, 1-wide and 1-high grids, every tol
    assert call(P=0) == 0 and call(P=0, n_q=1369, gw_q=37, n_g=1369, gw_g=37, tol=8) == 0
    assert call(P=0, n_q=37, gw_q=37, n_g=37, gw_g=1) == 0 and call(P=0, n_q=1, gw_q=1, n_g=1, gw_g=1, tol=0) == 0
    assert call(P=0, n_q=74, gw_q=2, n_g=74, gw_g=37) == 0 and call(P=0, n_q=1332, gw_q=36, n_g=1332, gw_g=37) == 0
    for tol in range(9):
        assert call(P=0, tol=tol, mask=p) == 0 and call(P=0, tol=tol, mask=odd2) == 0       # bytes: no alignment asked
    assert bytes(buf) == b"\xa5" * 8192


@pytest.mark.parametrize("fp8", [0, 1])
def test_rerank_refusals_come_back_without_a_device_and_write_nothing(lib, fp8):
    """The refusals of the spatial call (tests/test_spatial_cpu.py) in their order, the side limit where it has the bin limit."""
    null = ctypes.c_void_p(0)
    buf, p, odd, odd2 = _buffers()
    big = 1 << 40
    nan = float("nan")
    step = 64 if fp8 else 32

    def call(q=p, n_q=289, idx=p, B=1, kc=10, g=p, n_g=1369, l=64, n_local=5, base=0, min_sim=0.0, k=3, vals=p, out=p, inl=p,
             ps=null, pi=null, pm=null, mo=null, rn=null, cn=null, fp8=fp8, gw_q=17, gw_g=37, tol=1, ws=p, ws_bytes=big):
        st = lib.vpr_similarity_local_rerank(q, n_q, idx, B, kc, g, n_g, l, n_local, base, min_sim, k, vals, out, inl, ps, pi, pm, mo, rn, cn,
                                             fp8, gw_q, gw_g, tol, ws, ws_bytes, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and B == 0) writes nothing"
        return st

    for kw in (dict(q=null), dict(idx=null), dict(g=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1), dict(n_q=-1),
               dict(n_g=-5), dict(l=-64), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2),
               dict(kc=0, k=0), dict(min_sim=nan), dict(B=0, q=null),
               dict(gw_q=-1), dict(gw_g=-37), dict(tol=-1), dict(fp8=2), dict(fp8=-1), dict(B=0, tol=-1),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(kc=200, k=201), dict(q=null, l=48), dict(k=0, n_q=1370), dict(min_sim=nan, ws_bytes=0), dict(base=-1, q=odd),
               dict(tol=-1, n_q=1370), dict(gw_q=-1, l=48), dict(fp8=2, tol=9), dict(gw_g=-1, q=odd), dict(tol=-1, ws_bytes=0),
               dict(fp8=2, n_q=1368, gw_q=38), dict(fp8=3, l=32), dict(min_sim=nan, gw_q=0), dict(fp8=2, ws_bytes=0)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(kc=129, k=1), dict(n_q=0), dict(n_g=0), dict(n_q=1370), dict(n_g=1370), dict(n_g=1 << 20),
               dict(l=0), dict(l=16), dict(l=48), dict(l=288), dict(l=1 << 20), dict(q=odd), dict(g=odd), dict(ws=odd),
               dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(inl=odd2), dict(ps=odd2), dict(pi=odd2), dict(pm=odd2), dict(mo=odd2),
               dict(rn=odd2), dict(cn=odd2), dict(ws_bytes=0),
               dict(gw_q=0), dict(gw_g=0), dict(gw_q=16), dict(gw_g=36), dict(gw_q=290), dict(tol=9), dict(tol=1 << 30),
               dict(n_q=1368, gw_q=38), dict(n_q=1368, gw_q=36), dict(n_g=1368, gw_g=38), dict(n_g=1368, gw_g=36),     # a side of 38
               dict(gw_g=1), dict(gw_g=1369), dict(n_q=1369, gw_q=1369),                                               # 1369 x 1
               # double faults: a shape, grid or alignment fault together with a short workspace is still UNSUPPORTED
               dict(l=48, ws_bytes=0), dict(q=odd, ws_bytes=0), dict(n_q=1370, l=48), dict(kc=129, k=1, n_g=1370),
               dict(gw_q=0, ws_bytes=0), dict(tol=9, q=odd), dict(n_q=1370, gw_q=0), dict(gw_g=36, l=48), dict(tol=9, gw_q=16),
               dict(n_q=1368, gw_q=38, ws_bytes=0), dict(n_q=1368, gw_q=38, q=odd), dict(n_g=1368, gw_g=38, tol=9)):
        assert call(**kw) == UNSUPPORTED, kw
    if fp8:                                                  # l = 32 and 96: bf16 only
        assert call(l=32) == UNSUPPORTED and call(l=96) == UNSUPPORTED
    assert call(B=0, l=32) == (UNSUPPORTED if fp8 else 0)
    for B, kc, n_g, gw_g in ((1, 1, 1369, 37), (1, 10, 1, 1), (64, 64, 529, 23), (37, 128, 256, 16), (1000, 128, 1369, 37)):
        need = lib.vpr_similarity_workspace_bytes(B, kc, n_g)  # workspace: one byte short is refused
        assert need >= 8 * B * kc * (n_g + 1) and call(B=B, kc=kc, k=1, n_g=n_g, gw_g=gw_g, ws_bytes=need - 1) == UNSUPPORTED
    # what the rules leave alone: B = 0 launches nothing; the largest legal sizes; both routes
    assert call(B=0) == 0 and call(B=0, n_q=1369, gw_q=37, l=256, kc=128, k=128, tol=8) == 0
    assert call(B=0, n_q=1, gw_q=1, n_g=1, gw_g=1, l=64, kc=1, k=1, tol=0) == 0 and call(B=0, n_q=256, gw_q=16, n_g=256, gw_g=16) == 0
    assert call(B=0, idx=odd, vals=odd, out=odd, inl=null) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
    assert call(B=0, ps=p, pi=p, pm=p, mo=p, rn=p, cn=p, min_sim=float("inf")) == 0
    assert call(B=0, ws_bytes=lib.vpr_similarity_workspace_bytes(0, 10, 1369)) == 0
    for l in range(step, 257, step):
        assert call(B=0, l=l) == 0
    assert bytes(buf) == b"\xa5" * 8192


def test_workspace_equals_the_spatial_rule(lib):
    ours, theirs = lib.vpr_similarity_workspace_bytes, lib.vpr_spatial_workspace_bytes
    rng = np.random.default_rng(0)
    cases = [(B, kc, n_g) for B in (-1, 0, 1, 3, 64, 4096, 1 << 20) for kc in (-3, 0, 1, 2, 63, 64, 128, 129)
             for n_g in (-1, 0, 1, 255, 256, 257, 529, 1369, 1370)]
    cases += [tuple(int(v) for v in c) for c in zip(rng.integers(0, 5000, 200), rng.integers(1, 129, 200), rng.integers(1, 1370, 200))]
    for c in cases:
        assert ours(*c) == theirs(*c), c
    assert ours(1, 10, 1370) == 0 and ours(1, 129, 256) == 0 and ours(-1, 10, 256) == 0 and ours(0, 1, 1) > 0
    assert ours(1 << 20, 128, 1369) >= 8 * (1 << 20) * 128 * 1369        # beyond 2^32 bytes: a size_t
    assert ours(64, 32, 529) > lib.vpr_hires_local_workspace_bytes(64, 32) + 8 * 64 * 32 * 529 - 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8])
def test_fake_ops_give_shapes_and_dtypes_and_export(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert torch_ops.OPS[-2:] == ("similarity_verify", "local_rerank_similarity")           # appended
    fn, fv = torch.ops.vpr.local_rerank_similarity, torch.ops.vpr.similarity_verify
    schema = str(fn.default._schema).replace("SymInt", "int").replace("Float", "float")
    assert schema.startswith("vpr::local_rerank_similarity(") and "int gw_q, int gw_g, int tol=1, int index_base=0" in schema
    assert "k=None" in schema and "float min_sim=0" in schema
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        idx = mk(37, 64, dtype=torch.int32)
        for n_q, gw_q, n_g, gw_g in ((256, 16, 256, 16), (529, 23, 1369, 37), (1369, 37, 529, 23), (1369, 37, 1369, 37), (256, 16, 529, 23)):
            q, g = mk(37, n_q, 128, dtype=dtype), mk(50, n_g, 128, dtype=dtype)
            for args, k in (((q, idx, g, gw_q, gw_g), 64), ((q, idx, g, gw_q, gw_g, 0, 1000), 64), ((q, idx, g, gw_q, gw_g, 8, 0, 10), 10),
                            ((q, idx, g, gw_q, gw_g, 2, 7, 1, 0.5), 1)):
                v, i, m = fn(*args)
                assert v.shape == i.shape == m.shape == (37, k) and v.device.type == "cuda"
                assert v.dtype == torch.float32 and i.dtype == torch.int32 and m.dtype == torch.int32
            out = fv(mk(5, n_g, dtype=torch.int32), mk(5, n_g, dtype=torch.float32), n_q, gw_q, gw_g, 2)
            assert [tuple(t.shape) for t in out] == [(5,), (5,), (5,), (5, 6), (5, n_g)]
            assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.int32, torch.int32, torch.uint8]
        with pytest.raises(RuntimeError, match="gw_q must be a grid width"):
            fn(mk(2, 256, 64, dtype=dtype), mk(2, 4, dtype=torch.int32), mk(3, 256, 64, dtype=dtype), 15, 16)
        with pytest.raises(RuntimeError, match="a grid side is at most 37"):
            fn(mk(2, 76, 64, dtype=dtype), mk(2, 4, dtype=torch.int32), mk(3, 256, 64, dtype=dtype), 38, 16)
        with pytest.raises(RuntimeError, match="tol must be in 0..8"):
            fv(mk(5, 256, dtype=torch.int32), mk(5, 256, dtype=torch.float32), 256, 16, 16, 9)

    class Rerank(torch.nn.Module):
        def __init__(self, gw):
            super().__init__()
            self.gw = gw

        def forward(self, q, idx, g):
            v, i, m = fn(q, idx, g, self.gw, self.gw, 1, 3, 5, 0.25)
            return v * 2, i, m

    for gw in (16, 23, 37):
        n = gw * gw
        ep = torch.export.export(Rerank(gw), (torch.zeros(4, n, 64, dtype=dtype), torch.zeros(4, 8, dtype=torch.int32),
                                              torch.zeros(3, n, 64, dtype=dtype)))
        assert "vpr.local_rerank_similarity" in str(ep.graph)
        assert [tuple(n_.meta["val"].shape) for n_ in ep.graph.nodes if n_.op == "output" for n_ in n_.args[0]] == [(4, 5)] * 3


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, n, gw, kc, N = 2, 289, 17, 4, 3
    i = torch.zeros(B, kc, dtype=torch.int32)
    for dtype, l, step in ((torch.bfloat16, 32, 32), (torch.uint8, 64, 64)):
        z = lambda *s: torch.zeros(*s, dtype=dtype)
        q, g = z(B, n, l), z(N, n, l)
        op = lambda q_, i_, g_, gw_q=gw, gw_g=gw, tol=1, **kw: ops.local_rerank_similarity(q_, i_, g_, gw_q, gw_g, tol, **kw)
        with monkeypatch.context() as mp:
            with pytest.raises(RuntimeError, match="GPU tensor"):
                op(q, i, g)
            with pytest.raises(RuntimeError, match="GPU tensor"):
                torch.ops.vpr.local_rerank_similarity(q, i, g, gw, gw)
            with pytest.raises(RuntimeError, match="GPU tensor"):
                ops.similarity_verify(torch.zeros(2, n, dtype=torch.int32), torch.zeros(2, n), n, gw, gw)
            # the remaining checks, with the device test answered "yes": nothing below reaches the library
            mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
            mp.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
            for bad, match in (((q.float(), i, g), "bf16 features or their uint8"), ((q, i, g.float()), "g_local: expected dtype"),
                               ((q, i.long(), g), "idx: expected dtype"), ((q[0], i, g), "q_local: expected 3 dims"),
                               ((q[:1], i, g), "disagree on B"), ((q, i, z(N, n, 2 * l)), "disagree on l"),
                               ((z(B, n, 48), i, z(N, n, 48)), f"multiple of {step}"),
                               ((z(B, 1370, l), i, g), "q_local must hold 1..1369 patches"), ((q, i, z(N, 1370, l)), "g_local must hold 1..1369 patches"),
                               ((q, torch.zeros(B, 129, dtype=torch.int32), g), "1..128 candidates")):
                with pytest.raises(RuntimeError, match=match):
                    op(*bad)
            for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(min_sim=float("nan")), "min_sim must be"),
                              (dict(gw_q=0), "gw_q must be a grid width"), (dict(gw_q=16), "gw_q must be a grid width"),
                              (dict(gw_g=-17), "gw_g must be a grid width"), (dict(gw_g=290), "gw_g must be a grid width"),
                              (dict(tol=-1), "tol must be in 0..8"), (dict(tol=9), "tol must be in 0..8"),
                              (dict(gw_q=289), "the query grid is 289 x 1; a grid side is at most 37"),
                              (dict(gw_g=1), "the candidate grid is 1 x 289; a grid side is at most 37")):
                with pytest.raises(RuntimeError, match=match):
                    op(q, i, g, **kw)
            part, sim = torch.zeros(2, n, dtype=torch.int32), torch.zeros(2, n)
            for args, match in (((part.long(), sim, n, gw, gw), "partner: expected dtype"), ((part, sim.double(), n, gw, gw), "sim: expected dtype"),
                                ((part, sim[:1], n, gw, gw), "one shape"), ((part[0], sim[0], n, gw, gw), "partner: expected 2 dims"),
                                ((part, sim, 1370, 37, gw), "n_q must be in 1..1369"), ((part, sim, 0, 1, gw), "n_q must be in 1..1369"),
                                ((part, sim, n, 16, gw), "gw_q must be a grid width"), ((part, sim, n, gw, 0), "gw_g must be a grid width"),
                                ((part, sim, n, gw, gw, 9), "tol must be in 0..8"), ((part, sim, 76, 38, gw), "a grid side is at most 37")):
                with pytest.raises(RuntimeError, match=match):
                    ops.similarity_verify(*args)
    assert ops.similarity_model_scale_rotation([3, 0, 5, 6, 0, 4]) == (1.5, 0.0)
    s, r = ops.similarity_model_scale_rotation(torch.tensor([0, 1, 2, 2, 2, 4]))
    assert abs(s - 2 ** 0.5 / 2) < 1e-12 and abs(r - 45.0) < 1e-12
    assert ops.similarity_model_scale_rotation([mref.I32_MIN] * 6) is None
    assert [f for f in ops.SimilarityRerankDebug._fields] == ["pair_score", "pair_inliers", "pair_matches", "pair_model", "row_nn", "col_nn"]


# ------------------------------------------------------------------------------------------------ routing, CPU engine
class SimilarityEngine(RecordingEngine):
    def local_rerank_similarity(self, q_local_feats, idx, local_feats, index_base, k, min_sim, gw_q, gw_g, tol):
        self.calls.append(("local_rerank_similarity", q_local_feats.shape[1], local_feats.shape[1], str(q_local_feats.dtype), gw_q, gw_g, tol))
        out = mref.local_rerank_similarity(q_local_feats, idx, local_feats, gw_q, gw_g, tol, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["inliers"])


@pytest.mark.parametrize("R", [1, 2, 3])
def test_similarity_search_is_the_similarity_topk_of_the_coarse_union(monkeypatch, R):
    """Shards of N = 41 rows at the uneven cuts of shard_bounds on a 16 x 16 grid; the collective is replaced by a stack of
    every rank's list.  With spatial_model="similarity" the similarity entry runs, once per rank and pass, and the merged answer
    is the restatement on the union of the shards' coarse lists: the zoomed view.  The default and "shift" reach the spatial entry
    exactly as before, and it picks the block distractor; so does the plain call."""
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, gw, kc, k = 41, 64, 3, 16, 6, 4
    n = gw * gw
    rows, local, q, ql, true, distractor = mref.similarity_places(11 + R, N, D, B, gw)
    eng = SimilarityEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(rows[lo:hi], N, r, R, engine=eng, local_feats=local[lo:hi], force_collectives=R == 1, local_grid=gw))
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
            results.append(sg.search_local_reranked(q, k, kc, ql, 1.5, spatial_tol=1, spatial_model="similarity"))
    assert eng.calls == [("local_rerank_similarity", n, n, "torch.bfloat16", gw, gw, 1)] * (2 * R)
    union = torch.cat([eng.local_topk(q, sg.rows, kc, sg.index_base)[1] for sg in shards], 1)
    want = mref.local_rerank_similarity(ql, union, local, gw, gw, 1, 0, k, 1.5)
    for v, i in results:                                     # the same on every rank
        assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy().view(np.int32), want["vals"].view(np.int32))
    assert np.array_equal(want["idx"][:, 0], true) and (want["inliers"][:, 0] == 100).all()
    shift = sref.local_rerank_spatial(ql, union, local, gw, gw, 1, 0, k, 1.5)
    plain = ref.local_rerank(ql, union, local, 0, k, 1.5)
    assert np.array_equal(shift["idx"][:, 0], distractor) and np.array_equal(plain["idx"][:, 0], distractor)
    del eng.calls[:]
    monkeypatch.setattr(retrieval, "all_gather_topk", record)
    for rank, sg in enumerate(shards):
        for kw in ({}, dict(spatial_model="shift")):
            v, i = sg.search_local_reranked(q, k, kc, ql, 1.5, spatial_tol=1, **kw)
            assert i.shape == (B, k)
    assert eng.calls == [("local_rerank_spatial", n, n, "torch.bfloat16", gw, gw, 1)] * (2 * R)


def test_the_similarity_entry_runs_when_spatial_model_names_it_and_only_then():
    from vpr_amd import evaluate
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    N, D, B, kc, k = 9, 64, 2, 4, 2
    for gw, kind in ((16, "bf16"), (16, "e4m3"), (23, "bf16"), (23, "e4m3")):
        n = gw * gw
        rows, local, q, ql, _, _ = mref.similarity_places(gw, N, D, B, gw, kind)
        ql16 = mref.two_hot(np.zeros((B, n), np.int64)) if kind == "e4m3" else ql       # bf16 queries against an e4m3 store
        eng = SimilarityEngine()
        sg = ShardedGallery(rows, N, engine=eng, local_feats=local, local_hires=True, local_grid=gw)
        dt = "torch.uint8" if kind == "e4m3" else "torch.bfloat16"
        sim = dict(spatial_model="similarity")
        sg.search_local_reranked(q, k, kc, ql16, 1.5, spatial_tol=2, **sim)
        sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=0, **sim)
        sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=8, q_grid=gw, **sim)
        assert eng.calls == [("local_rerank_similarity", n, n, dt, gw, gw, tol) for tol in (2, 0, 8)], (gw, kind)
        del eng.calls[:]
        for kw in ({}, dict(spatial_model="shift")):         # the default and "shift": the spatial entry, as before
            sg.search_local_reranked(q, k, kc, ql16, 1.5, spatial_tol=2, **kw)
            sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=0, **kw)
            sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=8, q_grid=gw, **kw)
        assert eng.calls == [("local_rerank_spatial", n, n, dt, gw, gw, tol) for tol in (2, 0, 8)] * 2
        del eng.calls[:]
        sg.search_local_reranked(q, k, kc, ql, 1.5)          # no spatial_tol: the plain entries, as before
        sg.search_local_reranked(q, k, kc, ql, 1.5, spatial_model="shift")
        name = "local_rerank" + ("_fp8" if kind == "e4m3" else "") + ("_hires" if n > 256 else "")
        assert eng.calls == [(name, n, n)] * 2
    # "similarity" without spatial_tol, and an unknown model: a ValueError by name, at every entry
    for call in (lambda **kw: sg.search_local_reranked(q, k, kc, ql, 1.5, **kw),
                 lambda **kw: sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, **kw),
                 lambda **kw: sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, **kw),
                 lambda **kw: GraphedRetrieval(sg, B, k, local_rerank=kc, **kw),
                 lambda **kw: evaluate.calculate_retrieval_scores(None, "", "", "", **kw)):
        with pytest.raises(ValueError, match='spatial_model="similarity" verifies the matches within spatial_tol patches; name spatial_tol'):
            call(spatial_model="similarity")
        with pytest.raises(ValueError, match='spatial_model must be "shift" or "similarity"'):
            call(spatial_model="affine", spatial_tol=1)
    assert eng.calls == [(name, n, n)] * 2
    # a grid side over 37: 76 patches on a grid 38 wide (legal for the shift vote: 75 x 3 bins)
    rows, local, q, _, _, _ = mref.similarity_places(5, N, D, B, 16)
    wide = ShardedGallery(rows, N, engine=eng, local_feats=mref.two_hot(np.zeros((N, 76), np.int64)), local_grid=38)
    ql76 = mref.two_hot(np.zeros((B, 76), np.int64))
    del eng.calls[:]
    with pytest.raises(ValueError, match="the query grid is 38 x 2; a grid side is at most 37"):
        wide.search_local_reranked(q, k, kc, ql76, 1.5, spatial_tol=1, spatial_model="similarity")
    assert eng.calls == []
    wide.search_local_reranked(q, k, kc, ql76, 1.5, spatial_tol=1)
    assert eng.calls == [("local_rerank_spatial", 76, 76, "torch.bfloat16", 38, 38, 1)]
    # the gallery's grid and q_grid keep their meaning
    sg16 = ShardedGallery(rows, N, engine=eng, local_feats=local, local_grid=16)
    ql8 = mref.two_hot(np.arange(B * 128).reshape(B, 128))
    del eng.calls[:]
    sg16.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, q_grid=8, spatial_model="similarity")
    assert eng.calls == [("local_rerank_similarity", 128, 256, "torch.bfloat16", 8, 16, 1)]
    with pytest.raises(ValueError, match="q_grid"):
        sg16.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, spatial_model="similarity")
    closed = ShardedGallery(rows, N, engine=eng, local_feats=local)
    with pytest.raises(ValueError, match="local_grid"):
        closed.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, q_grid=8, spatial_model="similarity")
    with pytest.raises(ValueError, match="local_grid"):
        GraphedRetrieval(closed, B, k, local_rerank=kc, spatial_tol=1, spatial_model="similarity")


def test_spatial_model_is_the_last_keyword_everywhere():
    from vpr_amd import evaluate
    from vpr_amd.retrieval import GraphedRetrieval, HipEngine, ShardedGallery
    for fn in (ShardedGallery.search_local_reranked, ShardedGallery.search_gathered, ShardedGallery.search_local_queries,
               GraphedRetrieval.__init__, evaluate.calculate_retrieval_scores):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == "spatial_model" and inspect.signature(fn).parameters["spatial_model"].default == "shift", fn
    assert list(inspect.signature(HipEngine.local_rerank_similarity).parameters) == list(inspect.signature(HipEngine.local_rerank_spatial).parameters)
    assert "vpr_amd_similarity.h" in evaluate.calculate_retrieval_scores.__doc__


# ------------------------------------------------------------------------------------- the restatement's own properties
def test_the_hypothesis_index_rule_gives_two_different_matches():
    for M in range(2, 1370):
        s, t = mref.pair_indices(M)
        assert (s != t).all() and s.min() == 0 and 0 <= t.min() and max(s.max(), t.max()) < M and (np.diff(s) >= 0).all(), M
        if M >= 256:
            assert np.unique(s).size == 256
    assert mref.pair_indices(2)[0].tolist() == [0] * 128 + [1] * 128 and mref.pair_indices(2)[1].tolist() == [1] * 128 + [0] * 128


def test_int32_bounds_hold_at_the_corners_of_a_37_x_37_grid():
    """Matches between the extreme corners: every component of the residual reaches at most 4 * 36 * 36 = 5184, its square
    sum 2 * 5184^2 < 2^31, tol^2 |dg|^2 at most 64 * 2592."""
    n, gw = 1369, 37
    corners = [0, gw - 1, n - gw, n - 1]
    worst = 0
    for a in corners:
        for b in corners:
            for c in corners:
                for d in corners:
                    for e in corners:
                        for f in corners:
                            g = np.array([[a % gw, a // gw], [b % gw, b // gw], [c % gw, c // gw]], np.int64)
                            q = np.array([[d % gw, d // gw], [e % gw, e // gw], [f % gw, f // gw]], np.int64)
                            hyp = mref.hypotheses(g, q)
                            worst = max(worst, int(mref.residuals(g, q, hyp).max()))        # asserts the bounds itself
                            assert int(hyp["n2g"].max()) * 64 <= 64 * 2592 and np.abs(hyp["re"]).max() <= 2592 and np.abs(hyp["im"]).max() <= 2592
    assert 2592 ** 2 <= worst <= 2 * 5184 ** 2 < 2 ** 31    # the stated bound is generous: the corners reach 1.25 * 2592^2


def test_planted_similarity_identity():
    """All matches under one shift (M >= 2): every hypothesis has dq = dg, every match is an inlier at any tol, the score is the
    stated-order sum over all matches — what the match kernels would have written.  Under an exact integer scale 2 likewise;
    under 3/2 and 2/3 with rounding every match is an inlier at tol 1; a list turned by 90 degrees has no admissible model."""
    rng = np.random.default_rng(0)
    for n_q, gw_q, n_g, gw_g, shift in ((256, 16, 256, 16, (2, 1)), (289, 17, 289, 17, (-3, 0)), (256, 16, 529, 23, (-7, -5)), (9, 3, 9, 3, (0, 0)),
                                        (1369, 37, 1369, 37, (35, -36)), (37, 1, 37, 1, (0, 3)), (37, 37, 37, 37, (-4, 0)), (4, 2, 4, 2, (0, 0))):
        partner, sim = sref.planted_list(rng, n_q, gw_q, n_g, gw_g, shift)
        m = int((partner >= 0).sum())
        assert m >= 2
        for tol in (0, 1, 8):
            v = mref.verify(partner, sim, n_q, gw_q, gw_g, tol)
            assert v["inliers"] == v["matches"] == m and np.array_equal(v["mask"], partner >= 0) and v["admissible"].all()
            assert v["model"][0] == 0 and v["model"][3] == v["model"][5] > 0 and v["model"][4] == 0 and (v["counts"] == m).all()
            assert v["score"].view(np.int32) == refh.score_in_stated_order(np.where(partner >= 0, sim, 0).astype(np.float32)).view(np.int32)
            assert mref.scale_rotation(v["model"]) == (1.0, 0.0)
    partner, sim = mref.planted_similarity_list(rng, 1369, 37, 256, 16, 2, 1, centre=(8, 8))      # exact: q = 2 (g - 8) + 18
    v = mref.verify(partner, sim, 1369, 37, 16, 0)
    assert v["matches"] == v["inliers"] == 256 and mref.scale_rotation(v["model"]) == (2.0, 0.0) and v["admissible"].all()
    for (num, den), grids in (((3, 2), ((256, 16), (529, 23), (1369, 37))), ((2, 3), ((256, 16), (529, 23), (1369, 37)))):
        for n, gw in grids:
            partner, sim = mref.planted_similarity_list(rng, n, gw, n, gw, num, den)
            v = mref.verify(partner, sim, n, gw, gw, 1)
            s, r = mref.scale_rotation(v["model"])
            assert v["inliers"] == v["matches"] >= (n * 3 // 8 if num > den else n) and abs(s - num / den) < 0.1 and abs(r) < 3, (num, den, n)
            assert mref.verify(partner, sim, n, gw, gw, 0)["inliers"] < v["matches"]              # the rounding shows at tol 0
    partner, sim = mref.planted_similarity_list(rng, 529, 23, 529, 23, 1, 1, rot90=True)
    v = mref.verify(partner, sim, 529, 23, 23, 8)
    assert v["matches"] == 529 and v["inliers"] == 0 and v["model"] == mref.NO_MODEL and not v["admissible"].any() and not v["mask"].any()
    assert v["score"].view(np.int32) == 0


def test_the_tie_key_the_single_match_and_junk_partners():
    n, gw = 256, 16
    j = np.arange(n)
    sim = np.ones(n, np.float32)
    # two clusters of ten, shift (0, 0) on columns 0 .. 9 and shift (1, 3) on columns 16 .. 25: hypotheses inside a cluster count
    # 10 at tol 0; equal counts: the lowest h wins, and h = 0 has s = 0 (cluster A)
    partner = np.full(n, -1, np.int32)
    partner[:10] = j[:10]
    partner[16:26] = j[16:26] + 1 + 3 * gw
    v = mref.verify(partner, sim, n, gw, gw, 0)
    inside = [h for h in range(256) if v["counts"][h] == 10]
    assert v["matches"] == 20 and v["inliers"] == 10 and v["counts"].max() == 10 and v["model"][0] == min(inside) and v["mask"][:10].all()
    a_side = [h for h in inside if mref.pair_indices(20)[0][h] < 10]
    assert a_side and [h for h in inside if h not in a_side] and min(inside) in a_side
    partner[26] = j[26] + 1 + 3 * gw                                              # one more for B: the count decides before h
    v = mref.verify(partner, sim, n, gw, gw, 0)
    assert v["inliers"] == 11 and v["mask"][16:27].all() and not v["mask"][:10].any() and v["model"][0] > min(inside)
    # M = 1: no model (the shift vote counts one inlier); M = 0 likewise
    one = np.full(n, -1, np.int32)
    one[77] = 5
    v = mref.verify(one, sim, n, gw, gw, 8)
    assert v["matches"] == 1 and v["inliers"] == 0 and v["model"] == mref.NO_MODEL and v["score"].view(np.int32) == 0
    assert sref.verify(one, sim, n, gw, gw, 8)["inliers"] == 1
    v = mref.verify(np.full(n, -1, np.int32), sim, n, gw, gw, 3)
    assert v["matches"] == 0 and v["inliers"] == 0 and v["model"] == mref.NO_MODEL
    # duplicate partners: dq = 0, not admissible
    dup = np.full(n, -1, np.int32)
    dup[[3, 200]] = 17
    v = mref.verify(dup, sim, n, gw, gw, 8)
    assert v["matches"] == 2 and v["inliers"] == 0 and v["model"] == mref.NO_MODEL
    # junk next to valid entries: decided from the value alone; a non-finite similarity is no match either
    junk = partner.copy()
    junk[100:106] = [-1, mref.I32_MIN, mref.I32_MAX, n, n + 5, -7]
    s2 = sim.copy()
    s2[0], s2[1], s2[2] = np.nan, np.inf, -np.inf
    w = mref.verify(junk, s2, n, gw, gw, 0)
    assert w["matches"] == 21 - 3 and w["inliers"] == 11 and w["mask"][100:106].sum() == 0 and w["mask"][:3].sum() == 0


@pytest.mark.parametrize("gw,matches_true", [(16, 100), (23, 225), (37, 625)])
def test_the_recipes_premise(gw, matches_true):
    """Over 20 seeds: under the similarity model at tol 1 every match of the zoomed view is an inlier and the block distractor
    stays below it; under the shift vote at tol 1 and under the plain match count the distractor is ahead."""
    n = gw * gw
    seen = dict(sim=[], shift=[])
    for seed in range(20):
        qc, gc = mref.recipe_codes(seed, gw)
        lists = [mref.code_match_list(qc, gc[t], 2.0) for t in (0, 1)]
        if seed < 2 and gw < 37:                             # the lists are what the f64 matching gives on the two-hot features
            q, g = mref.two_hot(qc), mref.two_hot(gc)
            for t in (0, 1):
                got = sref.match_list(ref.pair(ref.f64(q), ref.f64(g[t]), 1.5))
                assert np.array_equal(got[0], lists[t][0]) and np.array_equal(got[1], lists[t][1])
        (dis, true), (dis_s, true_s) = ([fn(p, s, n, gw, gw, 1) for p, s in lists] for fn in (mref.verify, sref.verify))
        assert dis["matches"] == n > true["matches"] == matches_true             # plain: the distractor is ahead
        assert dis_s["inliers"] > true_s["inliers"] == 36                        # shift vote: the distractor is ahead
        assert true["inliers"] == matches_true > dis["inliers"] and float(true["score"]) == 2 * matches_true > float(dis["score"])
        s, r = mref.scale_rotation(true["model"])
        assert 1.25 <= s <= 1.75 and abs(true["model"][4]) <= true["model"][3] / 4
        seen["sim"].append(dis["inliers"])
        seen["shift"].append(dis_s["inliers"])
    print(f"block distractor on {gw} x {gw} over 20 seeds: similarity inliers {min(seen['sim'])} .. {max(seen['sim'])}, "
          f"shift-vote inliers {min(seen['shift'])} .. {max(seen['shift'])}; zoomed view {matches_true} / 36")
    assert 64 <= min(seen["sim"]) and max(seen["sim"]) <= 73 and 64 <= min(seen["shift"])
