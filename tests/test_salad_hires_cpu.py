"""CPU: the high-resolution SALAD extension of the C ABI (include/vpr_amd_salad_hires.h, 65 .. 1369 patch tokens) — header,
binding table and exported symbols agree, the older tables and VPR_SALAD_MAX_N are what they were, every refusal comes back
before a device is touched and in the order the header states, the two torch ops trace with fake tensors, SaladAggregator
sends each token count to the op it belongs to, and DinoV2Salad carries 448 / 518 px to the backbone."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
M, L, T, HID = 64, 128, 256, 512
NEW = {"vpr_salad_sinkhorn_aggregate_hires", "vpr_salad_aggregate_hires", "vpr_salad_aggregate_f32_hires"}
OLDER_HEADERS = ("vpr_amd.h", "vpr_amd_retrieval.h", "vpr_amd_expand.h", "vpr_amd_project.h", "vpr_amd_rerank.h",
                 "vpr_amd_salad_stages.h", "vpr_amd_salad_anyres.h")


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def _declared(header_name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header_name)).read(), flags=re.S)
    return code, set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_salad_hires.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    assert "vpr_salad_sinkhorn_aggregate_hires" in re.sub(r"\s*\*\s*", " ", header.split("present iff")[1]).split(";")[0]
    code, declared = _declared("vpr_amd_salad_hires.h")
    assert declared == set(_lib.SALAD_HIRES_PROTOTYPES) == NEW
    any_code, _ = _declared("vpr_amd_salad_anyres.h")
    params = lambda text, name: re.sub(r"\s+", " ", re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)).strip()
    for name, twin, arity in (("vpr_salad_sinkhorn_aggregate_hires", "vpr_salad_sinkhorn_aggregate_n", 13),
                              ("vpr_salad_aggregate_hires", "vpr_salad_aggregate_n", 19),
                              ("vpr_salad_aggregate_f32_hires", "vpr_salad_aggregate_f32_n", 19)):
        restype, argtypes = _lib.SALAD_HIRES_PROTOTYPES[name]
        fn = getattr(lib, name)                               # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype == ctypes.c_int and fn.argtypes == argtypes and len(argtypes) == arity
        assert (restype, argtypes) == _lib.SALAD_ANYRES_PROTOTYPES[twin]
        assert params(code, name) == params(any_code, twin)   # the header's parameter list is the _n call's, word for word
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6     # an additive extension: the version does not move


def test_constants():
    from vpr_amd import _lib
    hires = open(os.path.join(ROOT, "include", "vpr_amd_salad_hires.h")).read()
    anyres = open(os.path.join(ROOT, "include", "vpr_amd_salad_anyres.h")).read()
    assert re.search(r"#define VPR_SALAD_HIRES_MAX_N 1369\b", hires) and _lib.SALAD_HIRES_MAX_N == 1369 == 37 * 37
    assert re.search(r"#define VPR_SALAD_MAX_N 576\b", anyres) and _lib.SALAD_MAX_N == 576
    assert "VPR_SALAD_MAX_N" not in re.sub(r"/\*.*?\*/", "", hires, flags=re.S)       # it defines its own limit only


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    assert set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    assert set(_lib.SALAD_STAGES_PROTOTYPES) == {"vpr_salad_stage_outputs"}
    assert set(_lib.SALAD_ANYRES_PROTOTYPES) == {"vpr_salad_sinkhorn_aggregate_n", "vpr_salad_aggregate_n", "vpr_salad_aggregate_f32_n"}
    assert len(_lib.PROTOTYPES) == 61
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES,
                  _lib.RERANK_PROTOTYPES, _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES):
        assert not NEW & set(older)
    for other in OLDER_HEADERS:
        assert not NEW & _declared(other)[1], other
    assert re.search(r"#define VPR_AMD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "vpr_amd.h")).read())


def _weights_struct(p, null=None):
    from vpr_amd import _lib
    vals = [None if i == null else p.value for i in range(10)] + [None, None]
    return _lib.SaladWeightsC(*vals)


def _stage(lib, p, n, B=2, m=M, l=L, t=T, iters=3, scores=None, feats=None, out=0):
    return lib.vpr_salad_sinkhorn_aggregate_hires(p if scores is None else scores, p if feats is None else feats, p, B, n, m, l, t, 1.0,
                                                  iters, p if out == 0 else out, None, None)


def _one_call(lib, p, n, ws_bytes, B=2, C=128, m=M, l=L, t=T, hidden=HID, iters=3, w=None, patch=None, stride=None, ws=0, out=0):
    w = w if w is not None else _weights_struct(p)
    return lib.vpr_salad_aggregate_hires(p if patch is None else patch, n * C if stride is None else stride, p, C, B, n, C,
                                         ctypes.byref(w), 1.0, m, l, t, hidden, iters, p if out == 0 else out, None,
                                         p if ws == 0 else ws, ws_bytes, None)


def _one_call_f32(lib, p, n, ws_bytes, B=2, C=128, m=M, l=L, t=T, hidden=HID, iters=3, patch=None, stride=None, ws=0, out=0, null=None):
    from vpr_amd import _lib
    w = _lib.SaladWeightsF32C(*[None if i == null else p.value for i in range(10)])
    return lib.vpr_salad_aggregate_f32_hires(p if patch is None else patch, n * C if stride is None else stride, p, C, B, n, C,
                                             ctypes.byref(w), 1.0, m, l, t, hidden, iters, p if out == 0 else out, None,
                                             p if ws == 0 else ws, ws_bytes, None)


def test_refusals_need_no_device_and_come_in_the_stated_order(lib):
    """Dummy non-null pointers, never dereferenced: every status below is decided before a launch (without a device a
    launch would come back as VPR_ERR_LAUNCH, and the kernels would fault on these pointers)."""
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)           # 64-byte aligned
    off4, off2 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    big = 1 << 42
    calls = (lambda n, **kw: _stage(lib, p, n, **kw), lambda n, **kw: _one_call(lib, p, n, big, **kw),
             lambda n, **kw: _one_call_f32(lib, p, n, big, **kw))
    for call in calls:
        # sinkhorn_iters < 1 ahead of everything: alone, with a bad n, with a bad B, with a wrong m
        for kw in (dict(), dict(B=0), dict(m=32)):
            assert call(1369, iters=0, **kw) == INVALID and call(1369, iters=-3, **kw) == INVALID, kw
        for n in (1, 64, 1370, 2048):
            assert call(n, iters=0) == INVALID, n
        # nulls and non-positive sizes
        for n in (0, -1):
            assert call(n) == INVALID, n
        assert call(1369, B=0) == INVALID and call(1369, B=-2) == INVALID
        assert call(1369, out=None) == INVALID
        assert call(1370, out=None) == INVALID and call(1370, B=0) == INVALID       # ... ahead of the domain
        # the domain
        for n in (1, 63, 64, 1370, 2048):
            assert call(n) == UNSUPPORTED, n
        for kw in (dict(m=32), dict(l=64), dict(t=128)):
            assert call(1369, **kw) == UNSUPPORTED and call(577, **kw) == UNSUPPORTED, kw
    for kw in (dict(C=96), dict(hidden=500)):
        assert _one_call(lib, p, 1369, big, **kw) == UNSUPPORTED and _one_call_f32(lib, p, 1369, big, **kw) == UNSUPPORTED, kw
    assert lib.vpr_salad_sinkhorn_aggregate_hires(None, p, p, 2, 1369, M, L, T, 1.0, 3, p, None, None) == INVALID
    assert lib.vpr_salad_sinkhorn_aggregate_hires(p, None, p, 2, 1369, M, L, T, 1.0, 3, p, None, None) == INVALID
    assert lib.vpr_salad_sinkhorn_aggregate_hires(p, p, None, 2, 1369, M, L, T, 1.0, 3, p, None, None) == INVALID
    assert _one_call(lib, p, 1369, big, w=_weights_struct(p, null=4)) == INVALID            # a null member of the weights
    assert _one_call_f32(lib, p, 1369, big, null=7) == INVALID
    assert _one_call(lib, p, 1369, big, ws=None) == INVALID and _one_call_f32(lib, p, 1369, big, ws=None) == INVALID
    assert _one_call(lib, p, 1369, big, C=0) == INVALID and _one_call_f32(lib, p, 1369, big, C=-64) == INVALID
    # misaligned operands: scores / feats of stage A; the patch pointer, an image stride and the workspace of the one-call forms
    assert _stage(lib, p, 1369, scores=off4) == UNSUPPORTED and _stage(lib, p, 577, feats=off4) == UNSUPPORTED
    assert _stage(lib, p, 1369, out=off2) == UNSUPPORTED
    for n in (577, 1024, 1369):
        assert _one_call(lib, p, n, big, patch=off2) == UNSUPPORTED and _one_call_f32(lib, p, n, big, patch=off4) == UNSUPPORTED
        assert _one_call(lib, p, n, big, stride=n * 128 + 4) == UNSUPPORTED and _one_call_f32(lib, p, n, big, stride=n * 128 + 2) == UNSUPPORTED
        assert _one_call(lib, p, n, big, ws=off4) == UNSUPPORTED and _one_call_f32(lib, p, n, big, ws=off4) == UNSUPPORTED
        assert _one_call(lib, p, n, big, out=off2) == UNSUPPORTED and _one_call_f32(lib, p, n, big, out=off2) == UNSUPPORTED
        # ... ahead of WORKSPACE: misaligned with a short workspace
        assert _one_call(lib, p, n, 0, patch=off2) == UNSUPPORTED and _one_call_f32(lib, p, n, 0, patch=off4) == UNSUPPORTED
        assert _one_call(lib, p, n, 16, out=off2) == UNSUPPORTED and _one_call_f32(lib, p, n, 16, stride=n * 128 + 2) == UNSUPPORTED
    # workspace one byte short; the size calls scale with n
    for n in (65, 529, 577, 1024, 1369):
        for B, C in ((1, 128), (3, 1024)):
            need = lib.vpr_salad_workspace_bytes(B, n, C, M, L, T, HID)
            assert need > 0 and _one_call(lib, p, n, need - 1, B=B, C=C) == WORKSPACE
            need32 = lib.vpr_salad_f32_workspace_bytes(B, n, C, M, L, T, HID)
            assert need32 > 0 and _one_call_f32(lib, p, n, need32 - 1, B=B, C=C) == WORKSPACE
    # the order: an unsupported shape with a short workspace is UNSUPPORTED, n = 0 INVALID, a bad iteration count INVALID
    assert _one_call(lib, p, 1370, 0) == UNSUPPORTED and _one_call(lib, p, 0, 0) == INVALID and _one_call(lib, p, 1369, 0, iters=0) == INVALID
    assert _one_call_f32(lib, p, 1370, 0) == UNSUPPORTED and _one_call_f32(lib, p, 1369, 0, iters=0) == INVALID


def test_workspace_arithmetic_at_the_largest_batch(lib):
    """B = 64 at n = 1369: B*n*2*hidden bf16 hidden activations are 179 MB, the whole plan stays exact in 64 bits and the
    row count an int; one byte short is WORKSPACE, decided without touching the pointers."""
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    B, n, C = 64, 1369, 1024
    rows = B * n
    assert rows < 2 ** 31 and rows * 2 * HID * 2 == 179_437_568
    up = lambda v: (v + 255) // 256 * 256
    want = 4096 + up(rows * 2 * HID * 2) + up(2 * rows * M * 4) + up(2 * rows * L * 4) + up(B * HID * 2) + up(B * T * 4)
    need = lib.vpr_salad_workspace_bytes(B, n, C, M, L, T, HID)
    assert need == want
    assert _one_call(lib, p, n, need - 1, B=B, C=C) == WORKSPACE
    need32 = lib.vpr_salad_f32_workspace_bytes(B, n, C, M, L, T, HID)
    assert need32 > rows * 12 * HID * 2 + rows * 6 * C * 2 > 2 ** 31          # past 32 bits: the plan is size_t throughout
    assert _one_call_f32(lib, p, n, need32 - 1, B=B, C=C) == WORKSPACE


def test_the_any_n_entries_keep_their_limit(lib):
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    from vpr_amd import _lib
    w, w32 = _weights_struct(p), _lib.SaladWeightsF32C(*[p.value] * 10)
    big = 1 << 42
    for n in (577, 1024, 1369):
        assert lib.vpr_salad_sinkhorn_aggregate_n(p, p, p, 2, n, M, L, T, 1.0, 3, p, None, None) == UNSUPPORTED
        assert lib.vpr_salad_aggregate_n(p, n * 128, p, 128, 2, n, 128, ctypes.byref(w), 1.0, M, L, T, HID, 3, p, None, p, big, None) == UNSUPPORTED
        assert lib.vpr_salad_aggregate_f32_n(p, n * 128, p, 128, 2, n, 128, ctypes.byref(w32), 1.0, M, L, T, HID, 3, p, None, p, big,
                                             None) == UNSUPPORTED
        assert lib.vpr_salad_sinkhorn_aggregate(p, p, p, 2, n, M, L, T, 1.0, 3, p, None, None) == UNSUPPORTED


def test_torch_ops_are_registered_and_trace_with_fake_tensors():
    from vpr_amd import modules, torch_ops
    from vpr_amd.backbone import SplitTokens
    assert {"salad_aggregate_hires", "salad_aggregate_f32_hires"} <= set(torch_ops.OPS)
    for name in ("salad_aggregate_hires", "salad_aggregate_f32_hires"):
        schema = str(getattr(torch.ops.vpr, name).default._schema)
        assert schema.startswith(f"vpr::{name}(") and "Tensor? cls" in schema
    agg = modules.SaladAggregator(128)
    agg.pack()
    agg.pack_f32()
    with FakeTensorMode(allow_non_fake_inputs=True):
        for n in (577, 1025, 1369):
            tok = torch.empty(2, 1 + n, 128, dtype=torch.bfloat16, device="cuda")
            d, d16 = torch.ops.vpr.salad_aggregate_hires(tok, None, torch_ops.weight_list(agg._packed), 1.0, 3)
            assert d.shape == d16.shape == (2, 8448) and d.dtype == torch.float32 and d16.dtype == torch.bfloat16
            assert d.device.type == "cuda"
            d, d16 = torch.ops.vpr.salad_aggregate_hires(tok[:, 1:].contiguous(), tok[:, 0].contiguous(),
                                                         torch_ops.weight_list(agg._packed), 1.0, 3)
            assert d.shape == d16.shape == (2, 8448)
            d, d16 = torch.ops.vpr.salad_aggregate_f32_hires(tok.float(), None, torch_ops.weight_list(agg._packed_f32), 1.0, 3)
            assert d.shape == d16.shape == (2, 8448) and d.dtype == torch.float32 and d16.dtype == torch.bfloat16
            # the module traces at these token counts, in every layout it takes
            d = agg(tok)
            assert d.shape == (2, 8448) and d.dtype == torch.float32
            d, d16 = agg(SplitTokens(tok[:, 1:].contiguous(), tok[:, 0].contiguous()), want_bf16=True)
            assert d.shape == d16.shape == (2, 8448) and d16.dtype == torch.bfloat16
            d, d16 = agg(tok.float(), want_bf16=True)
            assert d.shape == (2, 8448) and d16.dtype == torch.bfloat16


def test_the_op_exports_through_torch_export():
    """torch.export at 1369 tokens: the graph holds the call torch.ops.vpr.salad_aggregate_hires.default."""
    from vpr_amd import modules, torch_ops
    agg = modules.SaladAggregator(128)
    weights = [w.to("meta") for w in torch_ops.weight_list(agg.pack())]

    class Agg(torch.nn.Module):
        def forward(self, tokens):
            return torch.ops.vpr.salad_aggregate_hires(tokens, None, weights, 1.0, 3)

    ep = torch.export.export(Agg(), (torch.empty(2, 1370, 128, dtype=torch.bfloat16, device="meta"),), strict=False)
    targets = [n.target for n in ep.graph.nodes if n.op == "call_function"]
    assert torch.ops.vpr.salad_aggregate_hires.default in targets


class _Recorder:
    """Stands in for torch.ops.vpr inside vpr_amd.modules: notes which op was called, returns a descriptor-shaped pair."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def op(first, *rest):
            self.calls.append((name, tuple(first.shape), rest[0] is None if name.endswith(("_n", "_hires")) else None))
            return torch.zeros(first.shape[0], 8448), torch.zeros(first.shape[0], 8448, dtype=torch.bfloat16)
        return op


def test_the_aggregator_routes_by_token_count(monkeypatch):
    from vpr_amd import modules
    from vpr_amd.backbone import SplitTokens
    rec = _Recorder()
    monkeypatch.setattr(modules, "_vpr", rec)
    agg = modules.SaladAggregator(64)
    agg.pack()
    agg.pack_f32()
    bf = lambda n: torch.zeros(2, 1 + n, 64, dtype=torch.bfloat16)
    split = lambda t: SplitTokens(t[:, 1:].contiguous(), t[:, 0].contiguous())

    def names(tokens):
        del rec.calls[:]
        agg(tokens)
        assert len(rec.calls) == 1
        return rec.calls[0]

    # n = 256: the ops it calls today
    assert names(bf(256))[0] == "salad_aggregate" and names(split(bf(256)))[0] == "salad_aggregate_split"
    assert names(bf(256).float())[0] == "salad_aggregate_f32" and names(split(bf(256).float()))[0] == "salad_aggregate_f32"
    # other n <= 576: the any-n ops
    for n in (65, 529, 576):
        assert names(bf(n)) == ("salad_aggregate_n", (2, 1 + n, 64), True)
        assert names(split(bf(n))) == ("salad_aggregate_n", (2, n, 64), False)
        assert names(bf(n).float())[0] == "salad_aggregate_f32_n"
    # 577 .. 1369: the high-resolution ops, the hub layout in place or the pair
    for n in (577, 1024, 1369):
        assert names(bf(n)) == ("salad_aggregate_hires", (2, 1 + n, 64), True)
        assert names(split(bf(n))) == ("salad_aggregate_hires", (2, n, 64), False)
        assert names(bf(n).float()) == ("salad_aggregate_f32_hires", (2, 1 + n, 64), True)
        assert names(split(bf(n).float())) == ("salad_aggregate_f32_hires", (2, n, 64), False)
    # past the limit: a ValueError that names it and the image size, before any op
    for tokens in (bf(1370), split(bf(1370)), bf(1444).float()):
        del rec.calls[:]
        with pytest.raises(ValueError, match=r"\b1369\b.*\b518 px"):
            agg(tokens)
        assert rec.calls == []


def test_img_size_reaches_the_backbone_at_448_and_518():
    from vpr_amd.modules import DinoV2Salad
    ext = DinoV2Salad("vit_small", img_size=518)
    assert ext.backbone.num_patches == 1369 and ext.backbone.pos_embed.shape[1] == 1370
    assert DinoV2Salad("vit_small", img_size=448).backbone.num_patches == 1024
