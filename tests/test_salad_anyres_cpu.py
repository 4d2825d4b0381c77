"""CPU: the any-token-count SALAD extension of the C ABI (include/vpr_amd_salad_anyres.h) — header, binding table and
exported symbols agree, the older tables are what they were, every refusal comes back before a device is touched and in the
order the header states, the two torch ops trace with fake tensors, and the img_size plumbing of DinoV2Salad / evaluate
names a grid mismatch instead of failing inside the position-embedding add."""
import ctypes
import os
import re

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
M, L, T, HID = 64, 128, 256, 512
NEW = {"vpr_salad_sinkhorn_aggregate_n", "vpr_salad_aggregate_n", "vpr_salad_aggregate_f32_n"}
OLDER_HEADERS = ("vpr_amd.h", "vpr_amd_retrieval.h", "vpr_amd_expand.h", "vpr_amd_project.h", "vpr_amd_rerank.h",
                 "vpr_amd_salad_stages.h")


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_header_table_and_symbols_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_salad_anyres.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    assert "vpr_salad_sinkhorn_aggregate_n" in header.split("present iff")[1].split(";")[0]
    assert re.search(r"#define VPR_SALAD_MAX_N 576\b", header) and _lib.SALAD_MAX_N == 576
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SALAD_ANYRES_PROTOTYPES) == NEW
    for name, arity in (("vpr_salad_sinkhorn_aggregate_n", 13), ("vpr_salad_aggregate_n", 19), ("vpr_salad_aggregate_f32_n", 19)):
        restype, argtypes = _lib.SALAD_ANYRES_PROTOTYPES[name]
        fn = getattr(lib, name)                               # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype == ctypes.c_int and fn.argtypes == argtypes and len(argtypes) == arity
        params = re.search(name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == arity
    # the f32 form takes the parameter list of vpr_salad_aggregate_f32
    assert _lib.SALAD_ANYRES_PROTOTYPES["vpr_salad_aggregate_f32_n"] == _lib.PROTOTYPES["vpr_salad_aggregate_f32"]
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6     # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    assert set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    assert set(_lib.SALAD_STAGES_PROTOTYPES) == {"vpr_salad_stage_outputs"}
    assert len(_lib.PROTOTYPES) == 61
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES,
                  _lib.RERANK_PROTOTYPES, _lib.SALAD_STAGES_PROTOTYPES):
        assert not NEW & set(older)
    for other in OLDER_HEADERS:
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(name in text for name in NEW), other
    assert re.search(r"#define VPR_AMD_ABI_VERSION 6\b", open(os.path.join(ROOT, "include", "vpr_amd.h")).read())


def _weights_struct(p, null=None):
    from vpr_amd import _lib
    vals = [None if i == null else p.value for i in range(10)] + [None, None]
    return _lib.SaladWeightsC(*vals)


def _stage(lib, p, n, B=2, m=M, l=L, t=T, iters=3, scores=None):
    return lib.vpr_salad_sinkhorn_aggregate_n(p if scores is None else scores, p, p, B, n, m, l, t, 1.0, iters, p, None, None)


def _one_call(lib, p, n, ws_bytes, B=2, C=128, m=M, l=L, t=T, hidden=HID, iters=3, w=None, patch=None, stride=None):
    w = w if w is not None else _weights_struct(p)
    return lib.vpr_salad_aggregate_n(p if patch is None else patch, n * C if stride is None else stride, p, C, B, n, C, ctypes.byref(w),
                                     1.0, m, l, t, hidden, iters, p, None, p, ws_bytes, None)


def _one_call_f32(lib, p, n, ws_bytes, B=2, C=128, m=M, l=L, t=T, hidden=HID, iters=3):
    from vpr_amd import _lib
    w = _lib.SaladWeightsF32C(*[p.value] * 10)
    return lib.vpr_salad_aggregate_f32_n(p, n * C, p, C, B, n, C, ctypes.byref(w), 1.0, m, l, t, hidden, iters, p, None, p, ws_bytes, None)


def test_refusals_need_no_device_and_come_in_the_stated_order(lib):
    """Dummy non-null pointers, never dereferenced: every status below is decided before a launch (without a device a
    launch would come back as VPR_ERR_LAUNCH, and the kernels would fault on these pointers)."""
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)           # 64-byte aligned
    big = 1 << 42
    for call in (lambda n, **kw: _stage(lib, p, n, **kw), lambda n, **kw: _one_call(lib, p, n, big, **kw),
                 lambda n, **kw: _one_call_f32(lib, p, n, big, **kw)):
        for n in (0, -1):
            assert call(n) == INVALID, n
        assert call(529, B=0) == INVALID and call(529, B=-2) == INVALID and call(529, iters=0) == INVALID
        for n in (1, 63, 64, 577, 1369):
            assert call(n) == UNSUPPORTED, n
        for kw in (dict(m=32), dict(l=64), dict(t=128)):
            assert call(529, **kw) == UNSUPPORTED, kw
    for kw in (dict(C=96), dict(hidden=500)):
        assert _one_call(lib, p, 529, big, **kw) == UNSUPPORTED and _one_call_f32(lib, p, 529, big, **kw) == UNSUPPORTED, kw
    assert lib.vpr_salad_sinkhorn_aggregate_n(None, p, p, 2, 529, M, L, T, 1.0, 3, p, None, None) == INVALID
    assert lib.vpr_salad_sinkhorn_aggregate_n(p, p, p, 2, 529, M, L, T, 1.0, 3, None, None, None) == INVALID
    assert _one_call(lib, p, 529, big, w=_weights_struct(p, null=4)) == INVALID             # a null member of the weights
    # misaligned operands: scores of stage A; the patch pointer and an image stride of the one-call form
    off = ctypes.c_void_p(p.value + 4)
    assert _stage(lib, p, 529, scores=off) == UNSUPPORTED
    assert _one_call(lib, p, 529, big, patch=ctypes.c_void_p(p.value + 2)) == UNSUPPORTED
    assert _one_call(lib, p, 529, big, stride=529 * 128 + 4) == UNSUPPORTED
    # workspace one byte short, and the order: an unsupported shape with a short workspace is UNSUPPORTED, not WORKSPACE
    for n in (65, 529, 576):
        for B, C in ((1, 128), (3, 1024)):
            need = lib.vpr_salad_workspace_bytes(B, n, C, M, L, T, HID)
            assert need > 0 and _one_call(lib, p, n, need - 1, B=B, C=C) == WORKSPACE
            need32 = lib.vpr_salad_f32_workspace_bytes(B, n, C, M, L, T, HID)
            assert need32 > 0 and _one_call_f32(lib, p, n, need32 - 1, B=B, C=C) == WORKSPACE
    assert _one_call(lib, p, 577, 0) == UNSUPPORTED and _one_call(lib, p, 0, 0) == INVALID
    # the older calls keep their n = 256 domain
    assert lib.vpr_salad_sinkhorn_aggregate(p, p, p, 2, 529, M, L, T, 1.0, 3, p, None, None) == UNSUPPORTED
    assert lib.vpr_salad_stage_aggregate(2, 529, 128, 1.0, M, L, T, HID, 3, p, None, p, big, None) == UNSUPPORTED


def test_torch_ops_are_registered_and_the_aggregator_traces_at_other_token_counts():
    from vpr_amd import modules, torch_ops
    from vpr_amd.backbone import SplitTokens
    assert {"salad_aggregate_n", "salad_aggregate_f32_n"} <= set(torch_ops.OPS)
    for name in ("salad_aggregate_n", "salad_aggregate_f32_n"):
        schema = str(getattr(torch.ops.vpr, name).default._schema)
        assert schema.startswith(f"vpr::{name}(") and "Tensor? cls" in schema
    agg = modules.SaladAggregator(128)
    agg.pack()
    agg.pack_f32()
    with FakeTensorMode(allow_non_fake_inputs=True):
        for tokens_per_image in (530, 257 + 1, 66):
            tok = torch.empty(2, tokens_per_image, 128, dtype=torch.bfloat16, device="cuda")
            d = agg(tok)
            assert d.shape == (2, 8448) and d.dtype == torch.float32
            d, d16 = agg(SplitTokens(tok[:, 1:].contiguous(), tok[:, 0].contiguous()), want_bf16=True)
            assert d.shape == d16.shape == (2, 8448) and d.dtype == torch.float32 and d16.dtype == torch.bfloat16
            d, d16 = agg(tok.float(), want_bf16=True)                      # f32 tokens: the f32-accurate form
            assert d.shape == (2, 8448) and d.dtype == torch.float32 and d16.dtype == torch.bfloat16
        d, d16 = torch.ops.vpr.salad_aggregate_n(torch.empty(2, 530, 128, dtype=torch.bfloat16, device="cuda"), None,
                                                 torch_ops.weight_list(agg._packed), 1.0, 3)
        assert d.shape == (2, 8448) and d16.dtype == torch.bfloat16 and d.device.type == "cuda"


def test_img_size_reaches_the_backbone_and_evaluate_names_a_grid_mismatch(tmp_path):
    from vpr_amd import evaluate
    from vpr_amd.modules import DinoV2Salad
    ext = DinoV2Salad("vit_small", img_size=322)
    assert ext.backbone.num_patches == 529 and ext.backbone.pos_embed.shape[1] == 530
    assert DinoV2Salad("vit_small").backbone.num_patches == 256
    with pytest.raises(ValueError, match=r"image_size=224\b.*\b256\b.*\b529\b"):
        evaluate.build_gallery_from_images(ext, str(tmp_path / "none.csv"), str(tmp_path), str(tmp_path / "gal"), image_size=224)
    with pytest.raises(ValueError, match=r"image_size=336\b.*\b576\b.*\b529\b"):
        evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "none.csv"), str(tmp_path), image_size=336)
    with pytest.raises(ValueError, match=r"image_size=322\b.*\b529\b.*\b256\b"):
        evaluate.build_gallery_from_images(DinoV2Salad("vit_small"), str(tmp_path / "none.csv"), str(tmp_path), str(tmp_path / "gal"),
                                           image_size=322)
