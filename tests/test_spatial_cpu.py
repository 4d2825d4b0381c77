"""CPU: the extension include/vpr_amd_spatial.h without a device — header, ctypes table and exported symbols agree; the eleven
older tables are untouched and disjoint; every refusal of the three calls in the stated order, writing nothing; the workspace
rule; fake ops and torch.export at 256, 529 and 1369 patches; the wrappers' refusals by message; the routing of spatial_tol on an
injected CPU engine that records which entry ran, sharded R = 1, 2, 3; and the restatement's own properties (tests/spatial_ref.py):
the planted-shift identity, both tie levels of the key, and the premise of the GPU test's recipe."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import local_match_fp8_ref as ref8
import local_match_hires_ref as refh
import local_match_ref as ref
import spatial_ref as sref

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
    header = open(os.path.join(ROOT, "include", "vpr_amd_spatial.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header and "twelfth" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SPATIAL_PROTOTYPES) == {"vpr_spatial_workspace_bytes", "vpr_spatial_verify", "vpr_spatial_local_rerank"}
    for name, (restype, argtypes) in _lib.SPATIAL_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    # the whole second stage: the 22 parameters of the hires call + pair_inliers, pair_shift + feat_is_fp8, gw_q, gw_g, tol
    assert len(_lib.SPATIAL_PROTOTYPES["vpr_spatial_local_rerank"][1]) == 22 + 2 + 4 and len(_lib.SPATIAL_PROTOTYPES["vpr_spatial_verify"][1]) == 14
    params = re.search(r"vpr_spatial_local_rerank\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert re.search(r"const void\*\s*q_local", params) and re.search(r"const void\*\s*g_local", params)
    for name in ("feat_is_fp8", "gw_q", "gw_g", "tol", "inliers_out", "pair_inliers", "pair_matches", "pair_shift", "row_nn", "col_nn"):
        assert re.search(rf"\b{name}\b", params), name
    const = lambda n: int(re.search(rf"#define {n} (\d+)", code).group(1))
    assert const("VPR_SPATIAL_MAX_BINS") == _lib.SPATIAL_MAX_BINS == sref.MAX_BINS == 5329 == 73 * 73 == (37 + 37 - 1) ** 2
    assert const("VPR_SPATIAL_MAX_TOL") == _lib.SPATIAL_MAX_TOL == sref.MAX_TOL == 8
    assert const("VPR_SPATIAL_MAX_N") == _lib.SPATIAL_MAX_N == sref.MAX_N == _lib.LOCAL_HIRES_MAX_N == 1369
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move
    assert re.search(r"#define VPR_AMD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "vpr_amd.h")).read())


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
    assert set(_lib.LOCAL_HIRES_PROTOTYPES) == {"vpr_hires_local_workspace_bytes", "vpr_hires_local_rerank", "vpr_hires_patch_rerank_fp8"}
    assert len(_lib.PROTOTYPES) == 61 and len(_lib.LOCAL_PROTOTYPES["vpr_local_rerank"][1]) == 22
    assert _lib.LOCAL_HIRES_PROTOTYPES["vpr_hires_local_rerank"] == _lib.LOCAL_PROTOTYPES["vpr_local_rerank"]
    new = set(_lib.SPATIAL_PROTOTYPES)
    older = (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
             _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES, _lib.LOCAL_PROTOTYPES,
             _lib.SALAD_F32_STAGES_PROTOTYPES, _lib.PATCH_FP8_PROTOTYPES, _lib.LOCAL_HIRES_PROTOTYPES)
    assert len(older) == 12                                  # vpr_amd.h and the eleven older extensions
    for table in older:
        assert not new & set(table)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_spatial.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "vpr_spatial" not in text and "VPR_SPATIAL" not in text, other


def _buffers():
    buf = (ctypes.c_char * 8192)()
    ctypes.memset(buf, 0xA5, 8192)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    return buf, p, ctypes.c_void_p(p.value + 8), ctypes.c_void_p(p.value + 2)


def test_verify_refusals_come_back_without_a_device_and_write_nothing(lib):
    null = ctypes.c_void_p(0)
    buf, p, _, odd2 = _buffers()

    def call(partner=p, sim=p, P=2, n_q=256, gw_q=16, n_g=256, gw_g=16, tol=1, score=p, inl=p, mt=p, shift=p, mask=null):
        st = lib.vpr_spatial_verify(partner, sim, P, n_q, gw_q, n_g, gw_g, tol, score, inl, mt, shift, mask, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and P == 0) writes nothing"
        return st

    for kw in (dict(partner=null), dict(sim=null), dict(score=null), dict(inl=null), dict(mt=null), dict(shift=null), dict(P=-1),
               dict(n_q=-1), dict(n_g=-256), dict(gw_q=-1), dict(gw_g=-16), dict(tol=-1), dict(P=0, sim=null),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(tol=-1, n_q=1370, gw_q=1370), dict(gw_q=-1, tol=9), dict(partner=null, gw_g=0), dict(P=-1, n_g=1370, gw_g=1),
               dict(gw_g=-3, score=odd2)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(gw_q=0), dict(gw_g=0), dict(gw_q=15), dict(gw_g=17), dict(gw_q=257), dict(n_q=255, gw_q=16), dict(tol=9), dict(tol=1 << 20),
               dict(n_q=1369, gw_q=37, n_g=1369, gw_g=1),          # 37 x 37 against a grid 1 wide and 1369 high: 37 x 1405 bins
               dict(n_q=1369, gw_q=37, n_g=1369, gw_g=1369),       # ... and against one 1369 wide and 1 high: 1405 x 37
               dict(n_q=1369, gw_q=37, n_g=1360, gw_g=68),         # 37 x 37 against 68 x 20: 104 x 56 = 5824 bins
               dict(n_q=1370, gw_q=37), dict(n_g=1370, gw_g=10), dict(n_q=0), dict(n_g=0), dict(n_q=0, gw_q=0),
               dict(partner=odd2), dict(sim=odd2), dict(score=odd2), dict(inl=odd2), dict(mt=odd2), dict(shift=odd2),
               dict(gw_q=0, tol=9), dict(n_q=1370, gw_q=0), dict(tol=9, partner=odd2)):
        assert call(**kw) == UNSUPPORTED, kw
    assert (37 + 1 - 1) * (37 + 1369 - 1) == 51985 > 5329
    # what the rules leave alone (P = 0 launches nothing): the largest grids, 1-wide and 1-high grids, every tol, the mask
    assert call(P=0) == 0 and call(P=0, n_q=1369, gw_q=37, n_g=1369, gw_g=37, tol=8) == 0
    assert call(P=0, n_q=1369, gw_q=37, n_g=1332, gw_g=36) == 0 and call(P=0, n_q=1369, gw_q=37, n_g=1360, gw_g=40) == 0   # 5256, 5320 bins
    assert call(P=0, n_q=1, gw_q=1, n_g=1, gw_g=1, tol=0) == 0 and call(P=0, n_q=40, gw_q=1, n_g=40, gw_g=40) == 0
    assert call(P=0, n_q=1369, gw_q=1369, n_g=1369, gw_g=1369) == 0 and call(P=0, n_q=1369, gw_q=1, n_g=1369, gw_g=1) == 0
    for tol in range(9):
        assert call(P=0, tol=tol, mask=p) == 0 and call(P=0, tol=tol, mask=odd2) == 0       # bytes: no alignment asked
    assert bytes(buf) == b"\xa5" * 8192


@pytest.mark.parametrize("fp8", [0, 1])
def test_rerank_refusals_come_back_without_a_device_and_write_nothing(lib, fp8):
    """The refusals of the hires calls (tests/test_local_match_hires_cpu.py) in their order, with the new ones appended to their
    groups: gw / tol negative and feat_is_fp8 outside 0 / 1 with the invalid arguments; the grid faults after kc, n and l and
    before the alignment and the workspace."""
    null = ctypes.c_void_p(0)
    buf, p, odd, odd2 = _buffers()
    big = 1 << 40
    nan = float("nan")
    step = 64 if fp8 else 32

    def call(q=p, n_q=289, idx=p, B=1, kc=10, g=p, n_g=1369, l=64, n_local=5, base=0, min_sim=0.0, k=3, vals=p, out=p, inl=p,
             ps=null, pi=null, pm=null, sh=null, rn=null, cn=null, fp8=fp8, gw_q=17, gw_g=37, tol=1, ws=p, ws_bytes=big):
        st = lib.vpr_spatial_local_rerank(q, n_q, idx, B, kc, g, n_g, l, n_local, base, min_sim, k, vals, out, inl, ps, pi, pm, sh, rn, cn,
                                          fp8, gw_q, gw_g, tol, ws, ws_bytes, null)
        assert bytes(buf) == b"\xa5" * 8192, "a refused call (and B == 0) writes nothing"
        return st

    for kw in (dict(q=null), dict(idx=null), dict(g=null), dict(vals=null), dict(out=null), dict(ws=null), dict(B=-1), dict(n_q=-1),
               dict(n_g=-5), dict(l=-64), dict(kc=-1, k=1), dict(n_local=-1), dict(base=-1), dict(k=0), dict(k=11), dict(k=-2),
               dict(kc=0, k=0), dict(min_sim=nan), dict(B=0, q=null),
               dict(gw_q=-1), dict(gw_g=-37), dict(tol=-1), dict(fp8=2), dict(fp8=-1), dict(B=0, tol=-1),
               # double faults: the invalid argument is reported ahead of what is merely unsupported
               dict(kc=200, k=201), dict(q=null, l=48), dict(k=0, n_q=1370), dict(min_sim=nan, ws_bytes=0), dict(base=-1, q=odd),
               dict(n_local=-1, kc=129, k=1), dict(min_sim=nan, n_g=1370), dict(idx=null, n_q=0),
               dict(tol=-1, n_q=1370), dict(gw_q=-1, l=48), dict(fp8=2, tol=9), dict(gw_g=-1, q=odd), dict(tol=-1, ws_bytes=0),
               dict(fp8=3, l=32), dict(min_sim=nan, gw_q=0)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(kc=129, k=1), dict(kc=129, k=129), dict(n_q=0), dict(n_g=0), dict(n_q=1370), dict(n_g=1370), dict(n_g=1 << 20),
               dict(l=0), dict(l=16), dict(l=48), dict(l=288), dict(l=320), dict(l=1 << 20), dict(q=odd), dict(g=odd), dict(ws=odd),
               dict(idx=odd2), dict(vals=odd2), dict(out=odd2), dict(inl=odd2), dict(ps=odd2), dict(pi=odd2), dict(pm=odd2), dict(sh=odd2),
               dict(rn=odd2), dict(cn=odd2), dict(ws_bytes=0),
               dict(gw_q=0), dict(gw_g=0), dict(gw_q=16), dict(gw_g=36), dict(gw_q=290), dict(tol=9), dict(tol=1 << 30),
               dict(n_q=1369, gw_q=37, gw_g=1),                    # 37 x 37 against 1 x 1369: 51 985 bins
               dict(n_q=1369, gw_q=37, gw_g=1369),
               # double faults: a shape, grid or alignment fault together with a short workspace is still UNSUPPORTED
               dict(l=48, ws_bytes=0), dict(q=odd, ws_bytes=0), dict(n_q=1370, l=48), dict(n_q=1370, n_g=0), dict(kc=129, k=1, n_g=1370),
               dict(gw_q=0, ws_bytes=0), dict(tol=9, q=odd), dict(n_q=1370, gw_q=0), dict(gw_g=36, l=48), dict(tol=9, gw_q=16)):
        assert call(**kw) == UNSUPPORTED, kw
    if fp8:                                                  # l = 32 and 96: bf16 only
        assert call(l=32) == UNSUPPORTED and call(l=96) == UNSUPPORTED and call(l=32, n_q=1370) == UNSUPPORTED
    assert call(B=0, l=32) == (UNSUPPORTED if fp8 else 0) and call(B=0, l=96) == (UNSUPPORTED if fp8 else 0)
    for B, kc, n_g, gw_g in ((1, 1, 1369, 37), (1, 10, 1, 1), (64, 64, 529, 23), (37, 128, 256, 16), (1000, 128, 1369, 37)):
        need = lib.vpr_spatial_workspace_bytes(B, kc, n_g)  # workspace: one byte short is refused
        assert need >= 8 * B * kc * (n_g + 1) and call(B=B, kc=kc, k=1, n_g=n_g, gw_g=gw_g, ws_bytes=need - 1) == UNSUPPORTED
        assert need > lib.vpr_hires_local_workspace_bytes(B, kc)
    # what the rules leave alone: B = 0 launches nothing; the largest legal sizes; both routes
    assert call(B=0) == 0 and call(B=0, n_q=1369, gw_q=37, l=256, kc=128, k=128, tol=8) == 0
    assert call(B=0, n_q=1, gw_q=1, n_g=1, gw_g=1, l=64, kc=1, k=1, tol=0) == 0 and call(B=0, n_q=256, gw_q=16, n_g=256, gw_g=16) == 0
    assert call(B=0, idx=odd, vals=odd, out=odd, inl=null) == 0 and call(B=0, n_local=0, base=2 ** 31 - 1) == 0
    assert call(B=0, ps=p, pi=p, pm=p, sh=p, rn=p, cn=p, min_sim=float("inf")) == 0 and call(B=0, min_sim=-float("inf")) == 0
    assert call(B=0, ws_bytes=lib.vpr_spatial_workspace_bytes(0, 10, 1369)) == 0
    for l in range(step, 257, step):
        assert call(B=0, l=l) == 0
    assert bytes(buf) == b"\xa5" * 8192


def test_workspace_query_is_monotone(lib):
    w = lib.vpr_spatial_workspace_bytes
    for kc, n_g in ((1, 1), (2, 256), (63, 257), (64, 529), (128, 1369)):
        sizes = [w(B, kc, n_g) for B in list(range(0, 300)) + [4096, 65536, 1 << 20]]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (kc, n_g)
    for B, n_g in ((0, 1), (1, 256), (3, 529), (64, 1369), (5000, 1369)):
        sizes = [w(B, kc, n_g) for kc in range(1, 129)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), (B, n_g)
    for B, kc in ((0, 1), (1, 10), (64, 64), (4096, 128)):
        sizes = [w(B, kc, n_g) for n_g in range(1, 1370)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), (B, kc)
        assert sizes[-1] >= lib.vpr_hires_local_workspace_bytes(B, kc) + 8 * max(B, 1) * kc * 1369
    for B, kc, n_g in ((-1, 10, 256), (1, 0, 256), (1, -3, 256), (1, 129, 256), (1, 10, 0), (1, 10, -1), (1, 10, 1370), (64, 1000, 1370)):
        assert w(B, kc, n_g) == 0, (B, kc, n_g)
    assert w(1 << 20, 128, 1369) >= 8 * (1 << 20) * 128 * 1369      # beyond 2^32 bytes: a size_t


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8])
def test_fake_ops_give_shapes_and_dtypes_and_export(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "spatial_verify" in torch_ops.OPS and "local_rerank_spatial" in torch_ops.OPS
    fn, fv = torch.ops.vpr.local_rerank_spatial, torch.ops.vpr.spatial_verify
    schema = str(fn.default._schema).replace("SymInt", "int").replace("Float", "float")
    assert schema.startswith("vpr::local_rerank_spatial(") and "int gw_q, int gw_g, int tol=1, int index_base=0" in schema
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
            assert [tuple(t.shape) for t in out] == [(5,), (5,), (5,), (5, 2), (5, n_g)]
            assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.int32, torch.int32, torch.uint8]
        with pytest.raises(RuntimeError, match="gw_q must be a grid width"):
            fn(mk(2, 256, 64, dtype=dtype), mk(2, 4, dtype=torch.int32), mk(3, 256, 64, dtype=dtype), 15, 16)
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
        assert "vpr.local_rerank_spatial" in str(ep.graph)
        assert [tuple(n_.meta["val"].shape) for n_ in ep.graph.nodes if n_.op == "output" for n_ in n_.args[0]] == [(4, 5)] * 3


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, n, gw, kc, N = 2, 289, 17, 4, 3
    i = torch.zeros(B, kc, dtype=torch.int32)
    for dtype, l, step in ((torch.bfloat16, 32, 32), (torch.uint8, 64, 64)):
        z = lambda *s: torch.zeros(*s, dtype=dtype)
        q, g = z(B, n, l), z(N, n, l)
        op = lambda q_, i_, g_, gw_q=gw, gw_g=gw, tol=1, **kw: ops.local_rerank_spatial(q_, i_, g_, gw_q, gw_g, tol, **kw)
        with monkeypatch.context() as mp:
            with pytest.raises(RuntimeError, match="GPU tensor"):
                op(q, i, g)
            with pytest.raises(RuntimeError, match="GPU tensor"):
                torch.ops.vpr.local_rerank_spatial(q, i, g, gw, gw)
            with pytest.raises(RuntimeError, match="GPU tensor"):
                ops.spatial_verify(torch.zeros(2, n, dtype=torch.int32), torch.zeros(2, n), n, gw, gw)
            # the remaining checks, with the device test answered "yes": nothing below reaches the library
            mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
            mp.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
            for bad, match in (((q.float(), i, g), "bf16 features or their uint8"), ((q, i, g.float()), "g_local: expected dtype"),
                               ((q, i, g.view(torch.int8) if dtype == torch.uint8 else g.view(torch.int16)), "g_local: expected dtype"),
                               ((q, i.long(), g), "idx: expected dtype"), ((q[0], i, g), "q_local: expected 3 dims"),
                               ((q, i[:, :2], g), "contiguous"), ((q[:1], i, g), "disagree on B"), ((q, i, z(N, n, 2 * l)), "disagree on l"),
                               ((z(B, n, 48), i, z(N, n, 48)), f"multiple of {step}"), ((z(B, n, 320), i, z(N, n, 320)), f"multiple of {step}"),
                               ((z(B, 1370, l), i, g), "q_local must hold 1..1369 patches"), ((q, i, z(N, 1370, l)), "g_local must hold 1..1369 patches"),
                               ((q, torch.zeros(B, 129, dtype=torch.int32), g), "1..128 candidates")):
                with pytest.raises(RuntimeError, match=match):
                    op(*bad)
            for kw, match in ((dict(k=0), "k must be"), (dict(k=kc + 1), "k must be"), (dict(min_sim=float("nan")), "min_sim must be"),
                              (dict(gw_q=0), "gw_q must be a grid width"), (dict(gw_q=16), "gw_q must be a grid width"),
                              (dict(gw_g=-17), "gw_g must be a grid width"), (dict(gw_g=290), "gw_g must be a grid width"),
                              (dict(tol=-1), "tol must be in 0..8"), (dict(tol=9), "tol must be in 0..8"),
                              (dict(gw_q=289, gw_g=1), "span 83521 shift bins, more than 5329")):
                with pytest.raises(RuntimeError, match=match):
                    op(q, i, g, **kw)
            part, sim = torch.zeros(2, n, dtype=torch.int32), torch.zeros(2, n)
            for args, match in (((part.long(), sim, n, gw, gw), "partner: expected dtype"), ((part, sim.double(), n, gw, gw), "sim: expected dtype"),
                                ((part, sim[:1], n, gw, gw), "one shape"), ((part[0], sim[0], n, gw, gw), "partner: expected 2 dims"),
                                ((part, sim, 1370, 37, gw), "n_q must be in 1..1369"), ((part, sim, 0, 1, gw), "n_q must be in 1..1369"),
                                ((part, sim, n, 16, gw), "gw_q must be a grid width"), ((part, sim, n, gw, 0), "gw_g must be a grid width"),
                                ((part, sim, n, gw, gw, 9), "tol must be in 0..8"), ((part, sim, n, 1, 289), "shift bins")):
                with pytest.raises(RuntimeError, match=match):
                    ops.spatial_verify(*args)


# ------------------------------------------------------------------------------------------------ routing, CPU engine
class RecordingEngine:
    """oracle/knn.py searches and merge; the local re-rank entries are the restatements and record their names."""

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

    def local_rerank_spatial(self, q_local_feats, idx, local_feats, index_base, k, min_sim, gw_q, gw_g, tol):
        self.calls.append(("local_rerank_spatial", q_local_feats.shape[1], local_feats.shape[1], str(q_local_feats.dtype), gw_q, gw_g, tol))
        out = sref.local_rerank_spatial(q_local_feats, idx, local_feats, gw_q, gw_g, tol, index_base, k, min_sim)
        return torch.from_numpy(out["vals"]), torch.from_numpy(out["idx"]), torch.from_numpy(out["inliers"])


@pytest.mark.parametrize("R", [1, 2, 3])
def test_spatial_search_is_the_spatial_topk_of_the_coarse_union(monkeypatch, R):
    """Shards of N = 41 rows at the uneven cuts of shard_bounds on a 17 x 17 grid; the collective is replaced by a stack of
    every rank's list.  With spatial_tol the spatial entry runs, once per rank and pass, and the merged answer is the
    restatement on the union of the shards' coarse lists; without it the plain entries run as before."""
    from vpr_amd import retrieval
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    N, D, B, gw, kc, k = 41, 64, 3, 17, 6, 4
    n = gw * gw
    rows, local, q, ql, true, scrambled = sref.spatial_places(11 + R, N, D, B, gw)
    eng = RecordingEngine()
    shards = []
    for r in range(R):
        lo, hi = shard_bounds(N, r, R)
        shards.append(ShardedGallery(rows[lo:hi], N, r, R, engine=eng, local_feats=local[lo:hi], force_collectives=R == 1, local_hires=True,
                                     local_grid=gw))
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
            results.append(sg.search_local_reranked(q, k, kc, ql, 1.5, spatial_tol=1))
    assert eng.calls == [("local_rerank_spatial", n, n, "torch.bfloat16", gw, gw, 1)] * (2 * R)
    union = torch.cat([eng.local_topk(q, sg.rows, kc, sg.index_base)[1] for sg in shards], 1)
    want = sref.local_rerank_spatial(ql, union, local, gw, gw, 1, 0, k, 1.5)
    for v, i in results:                                     # the same on every rank
        assert np.array_equal(i.numpy(), want["idx"]) and np.array_equal(v.numpy().view(np.int32), want["vals"].view(np.int32))
    assert np.array_equal(want["idx"][:, 0], true) and (want["inliers"][:, 0] == (gw - 2) * (gw - 1)).all()
    plain = ref.local_rerank(ql, union, local, 0, k, 1.5)    # without the verification the scrambled view wins
    assert np.array_equal(plain["idx"][:, 0], scrambled) and (plain["matches"][:, 0] == n).all()
    del eng.calls[:]
    monkeypatch.setattr(retrieval, "all_gather_topk", record)
    for rank, sg in enumerate(shards):
        sg.search_local_reranked(q, k, kc, ql, 1.5)
    assert eng.calls == [("local_rerank_hires", n, n)] * R


def test_the_spatial_entry_runs_when_spatial_tol_is_given_and_only_then():
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    N, D, B, kc, k = 9, 64, 2, 4, 2
    for gw, kind in ((16, "bf16"), (16, "e4m3"), (23, "bf16"), (23, "e4m3")):
        n = gw * gw
        rows, local, q, ql, _, _ = sref.spatial_places(gw, N, D, B, gw, kind)
        ql16 = sref.two_hot(np.zeros((B, n), np.int64)) if kind == "e4m3" else ql       # bf16 queries against an e4m3 store
        eng = RecordingEngine()
        sg = ShardedGallery(rows, N, engine=eng, local_feats=local, local_hires=True, local_grid=gw)
        assert sg.local_grid == gw
        dt = "torch.uint8" if kind == "e4m3" else "torch.bfloat16"
        sg.search_local_reranked(q, k, kc, ql16, 1.5, spatial_tol=2)
        sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=0)
        sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5, spatial_tol=8, q_grid=gw)
        assert eng.calls == [("local_rerank_spatial", n, n, dt, gw, gw, tol) for tol in (2, 0, 8)], (gw, kind)
        del eng.calls[:]
        sg.search_local_reranked(q, k, kc, ql, 1.5)          # no spatial_tol: the plain entries, as before
        sg.search_gathered(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5)
        sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=1.5)
        name = "local_rerank" + ("_fp8" if kind == "e4m3" else "") + ("_hires" if n > 256 else "")
        assert eng.calls == [(name, n, n)] * 3
    # queries on another grid than the gallery's: q_grid names it
    rows, local, q, _, _, _ = sref.spatial_places(5, N, D, B, 16)
    eng = RecordingEngine()
    sg = ShardedGallery(rows, N, engine=eng, local_feats=local, local_grid=16)
    ql8 = sref.two_hot(np.arange(B * 128).reshape(B, 128))
    sg.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, q_grid=8)
    assert eng.calls == [("local_rerank_spatial", 128, 256, "torch.bfloat16", 8, 16, 1)]
    with pytest.raises(ValueError, match="q_grid"):
        sg.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1)
    with pytest.raises(ValueError, match="gw_q must be a grid width"):
        sg.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, q_grid=7)
    with pytest.raises(ValueError, match="tol must be in 0..8"):
        sg.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=9, q_grid=8)
    with pytest.raises(ValueError, match="q_grid is the queries' grid of a spatial search"):
        sg.search_local_reranked(q, k, kc, ql8, 1.5, q_grid=8)
    with pytest.raises(ValueError, match="at most 256 patches"):                    # local_hires stays the opt-in beyond 256
        sg.search_local_reranked(q, k, kc, sref.two_hot(np.zeros((B, 289), np.int64)), 1.5, spatial_tol=1, q_grid=17)
    # a gallery without a grid refuses a spatial search and names the keyword
    closed = ShardedGallery(rows, N, engine=eng, local_feats=local)
    assert closed.local_grid is None
    for call in (lambda: closed.search_local_reranked(q, k, kc, ql8, 1.5, spatial_tol=1, q_grid=8),
                 lambda: closed.search_gathered(q, k, local_rerank=kc, q_local_feats=ql8, spatial_tol=1),
                 lambda: closed.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql8, spatial_tol=1),
                 lambda: GraphedRetrieval(closed, B, k, local_rerank=kc, spatial_tol=1)):
        with pytest.raises(ValueError, match="local_grid"):
            call()
    assert len(eng.calls) == 1
    with pytest.raises(ValueError, match="spatial_tol verifies the matches of local_rerank"):
        sg.search_gathered(q, k, spatial_tol=1)
    with pytest.raises(ValueError, match="spatial_tol verifies the matches of local_rerank"):
        GraphedRetrieval(sg, B, k, spatial_tol=1)
    for bad in (0, 15, 257, -16):
        with pytest.raises(ValueError, match="local_grid"):
            ShardedGallery(rows, N, engine=eng, local_feats=local, local_grid=bad)
    with pytest.raises(ValueError, match="local_grid"):
        ShardedGallery(rows, N, engine=eng, local_grid=16)


def test_evaluation_and_graph_entry_points_take_spatial_tol():
    from vpr_amd import evaluate
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    par = inspect.signature(evaluate.calculate_retrieval_scores).parameters["spatial_tol"]
    assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY and "image_size // 14" in evaluate.calculate_retrieval_scores.__doc__
    assert inspect.signature(GraphedRetrieval.__init__).parameters["spatial_tol"].default is None
    assert inspect.signature(ShardedGallery.__init__).parameters["local_grid"].default is None
    for fn in (ShardedGallery.search_local_reranked, ShardedGallery.search_gathered, ShardedGallery.search_local_queries):
        assert inspect.signature(fn).parameters["spatial_tol"].default is None and inspect.signature(fn).parameters["q_grid"].default is None


# ------------------------------------------------------------------------------------- the restatement's own properties
def test_planted_shift_identity():
    """A list whose matches all share one shift: at every tol the dominant shift is that shift, every match is an inlier, and
    the score is the stated-order sum over all matches — what the match kernels would have written."""
    rng = np.random.default_rng(0)
    for n_q, gw_q, n_g, gw_g, shift in ((256, 16, 256, 16, (2, 1)), (289, 17, 289, 17, (-3, 0)), (256, 16, 529, 23, (-7, -5)), (9, 3, 9, 3, (0, 0)),
                                        (1, 1, 1, 1, (0, 0)), (1369, 37, 1369, 37, (36, -36)), (40, 1, 40, 1, (0, 3)), (40, 40, 40, 40, (-4, 0))):
        partner, sim = sref.planted_list(rng, n_q, gw_q, n_g, gw_g, shift)
        m = int((partner >= 0).sum())
        assert m > 0
        for tol in (0, 1, 8):
            v = sref.verify(partner, sim, n_q, gw_q, gw_g, tol)
            assert v["shift"] == shift and v["inliers"] == v["matches"] == m and np.array_equal(v["mask"], partner >= 0)
            assert v["score"].view(np.int32) == refh.score_in_stated_order(np.where(partner >= 0, sim, 0).astype(np.float32)).view(np.int32)
            assert v["votes"].sum() == m and v["votes"].max() == m
    # tol >= max(W, H) - 1: the window of every bin covers all bins, so every match is an inlier whatever the list
    partner = rng.integers(-1, 9, 9).astype(np.int32)
    v = sref.verify(partner, np.ones(9, np.float32), 9, 3, 3, 4)
    assert v["inliers"] == v["matches"] == int((partner >= 0).sum()) and (v["support"] == v["matches"]).all()


def test_the_tie_key_and_junk_partners():
    n, gw = 256, 16
    j = np.arange(n)
    # two clusters of equal support and equal votes: the lower bin wins.  Cluster A: shift (0, 0) on columns 0 .. 9;
    # cluster B: shift (1, 0) on columns 16 .. 25 (the partner is the column's right-hand neighbour)
    partner = np.full(n, -1, np.int32)
    partner[:10] = j[:10]
    partner[16:26] = j[16:26] + 1
    sim = np.ones(n, np.float32)
    v = sref.verify(partner, sim, n, gw, gw, 0)
    assert v["shift"] == (0, 0) and v["inliers"] == 10 and v["matches"] == 20          # bin ascending: dx = 0 before dx = 1
    partner[32] = j[32] + 1                                                       # one more vote for B
    assert sref.verify(partner, sim, n, gw, gw, 0)["shift"] == (1, 0)
    # equal support, unequal own votes: at tol 1 the bins (0, 0) and (1, 0) and their neighbours all see the 21 matches;
    # the key's second part picks the bin with more votes of its own, (1, 0), although (-1, *) and (0, *) come first by index
    v = sref.verify(partner, sim, n, gw, gw, 1)
    assert v["shift"] == (1, 0) and v["inliers"] == 21 and (v["support"] == 21).sum() > 2
    partner[48] = j[48]                                                           # 11 : 11 votes again: back to the lower bin
    v = sref.verify(partner, sim, n, gw, gw, 1)
    assert v["shift"] == (0, 0) and v["inliers"] == 22
    # junk next to valid entries: decided from the value alone; a non-finite similarity is no match either
    junk = partner.copy()
    junk[100:106] = [-1, sref.I32_MIN, sref.I32_MAX, n, n + 5, -7]
    s2 = sim.copy()
    s2[0], s2[1], s2[2] = np.nan, np.inf, -np.inf
    w = sref.verify(junk, s2, n, gw, gw, 1)
    assert w["matches"] == 22 - 3 and w["shift"] == (1, 0) and w["mask"][100:106].sum() == 0 and w["mask"][:3].sum() == 0
    # a window clipped at each border of the bin plane: one match in a corner bin; at tol 8 its window reaches 8 bins inwards
    for partner_0, col, shift in ((0, n - 1, (-15, -15)), (n - 1, 0, (15, 15)), (gw - 1, n - gw, (15, -15)), (n - gw, gw - 1, (-15, 15))):
        one = np.full(n, -1, np.int32)
        one[col] = partner_0
        v = sref.verify(one, sim, n, gw, gw, 8)
        assert v["matches"] == v["inliers"] == 1 and (v["support"] == 1).sum() == 81
        assert v["shift"] == shift                                                # the bin's own vote decides among the 81
    empty = sref.verify(np.full(n, -1, np.int32), sim, n, gw, gw, 3)
    assert empty["shift"] == (sref.I32_MIN, sref.I32_MIN) and empty["inliers"] == empty["matches"] == 0
    assert empty["score"].view(np.int32) == 0                                     # +0


@pytest.mark.parametrize("gw,matches_true", [(16, 210), (23, 462)])
def test_the_recipes_premise(gw, matches_true):
    """Over 20 seeds: the plain match count ranks the scrambled image (every one of the n patches matched) above the true
    one ((gw - 2)(gw - 1) matches under the shift (2, 1)); the scrambled image reaches at most 6 inliers at tol 0, 19 at tol 1
    and 39 at tol 2, the true one keeps all of its matches at the shift (2, 1)."""
    n = gw * gw
    assert (gw - 2) * (gw - 1) == matches_true < n
    worst = {0: 0, 1: 0, 2: 0}
    for seed in range(20):
        qc, gc = sref.recipe_codes(seed, gw)
        q, g = sref.two_hot(qc), sref.two_hot(gc)
        pairs = [ref.pair(ref.f64(q), ref.f64(g[t]), 1.5) for t in (0, 1)]
        assert pairs[0]["matches"] == n and pairs[1]["matches"] == matches_true and pairs[0]["score"] == 2 * n > pairs[1]["score"]
        for tol in (0, 1, 2):
            dis, true = (sref.verify(*sref.match_list(p), n, gw, gw, tol) for p in pairs)
            worst[tol] = max(worst[tol], dis["inliers"])
            assert true["inliers"] == matches_true and true["shift"] == (2, 1) and float(true["score"]) == 2 * matches_true
    print(f"scrambled image on {gw} x {gw}, most inliers over 20 seeds at tol 0 / 1 / 2: {worst[0]} / {worst[1]} / {worst[2]}")
    assert worst[0] <= 6 and worst[1] <= 19 and worst[2] <= 39
    # the same through the e4m3 store: the same integers, the similarities scaled by 2^-16
    q8, g8 = sref.two_hot(qc, "e4m3"), sref.two_hot(gc, "e4m3")
    out = sref.local_rerank_spatial(q8[None], torch.tensor([[0, 1]], dtype=torch.int32), g8, gw, gw, 1, 0, None, 1.5 * 2.0 ** -16)
    assert out["idx"][0].tolist() == [1, 0] and out["inliers"][0, 0] == matches_true and out["pair_shift"][0, 1].tolist() == [2, 1]
    assert float(out["vals"][0, 0]) == 2 * matches_true * 2.0 ** -16 and out["pair_matches"][0].tolist() == [n, matches_true]
