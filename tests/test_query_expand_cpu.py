"""CPU: the query-expansion extension of the C ABI (include/vpr_amd_expand.h) — header, binding table and exported symbols
agree, the older tables are what they were, every refusal comes back with its status before a device is touched, the torch
ops have fake implementations, and the wrappers refuse what they cannot take."""
import ctypes
import os
import re

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
    header = open(os.path.join(ROOT, "include", "vpr_amd_expand.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    for name, (restype, argtypes) in _lib.EXPAND_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
        params = re.search(rf"{name}\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(params.split(",")) == len(argtypes), name
    assert len(_lib.EXPAND_PROTOTYPES["vpr_query_expand"][1]) == 18
    assert len(_lib.EXPAND_PROTOTYPES["vpr_query_expand_finish"][1]) == 8
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    new = set(_lib.EXPAND_PROTOTYPES)
    assert not new & set(_lib.PROTOTYPES) and not new & set(_lib.EXTENSION_PROTOTYPES)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert "query_expand" not in main and re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)


def test_invalid_arguments_are_rejected_without_a_device(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 8)                       # 8-byte aligned only
    nan, inf = float("nan"), float("inf")

    def expand(q=p, vals=p, idx=p, B=1, D=64, k=10, rows=p, scales=null, n_local=5, base=0, n_use=3, alpha=3.0, qw=1.0, add=1,
               partial=p, o32=null, o16=null):
        return lib.vpr_query_expand(q, vals, idx, B, D, k, rows, scales, n_local, base, n_use, alpha, qw, add, partial, o32, o16,
                                    null)

    def finish(partials=p, R=1, q=p, B=1, D=64, o32=p, o16=p):
        return lib.vpr_query_expand_finish(partials, R, q, B, D, o32, o16, null)

    for kw in (dict(q=null), dict(vals=null), dict(idx=null), dict(rows=null), dict(partial=null), dict(B=-1), dict(D=-64),
               dict(k=-1), dict(n_local=-1), dict(n_use=0), dict(n_use=11), dict(n_use=-2), dict(k=0, n_use=0),
               dict(alpha=-0.5), dict(alpha=nan), dict(qw=-1.0), dict(qw=nan), dict(add=2), dict(add=-1),
               dict(o32=p, B=-1)):
        assert expand(**kw) == INVALID, kw
    for kw in (dict(k=129, n_use=129), dict(k=129, n_use=1), dict(D=96), dict(D=63), dict(D=0), dict(q=odd), dict(rows=odd),
               dict(partial=odd), dict(o32=odd), dict(o16=odd), dict(o32=p, o16=odd)):
        assert expand(**kw) == UNSUPPORTED, kw
    for kw in (dict(partials=null), dict(q=null), dict(o32=null, o16=null), dict(B=-1), dict(D=-64), dict(R=0), dict(R=-3)):
        assert finish(**kw) == INVALID, kw
    for kw in (dict(R=65), dict(D=100), dict(D=0), dict(partials=odd), dict(q=odd), dict(o32=odd), dict(o16=odd)):
        assert finish(**kw) == UNSUPPORTED, kw
    # what the rules leave alone: B = 0 launches nothing, either output of the finish may be absent, the largest legal sizes
    assert expand(B=0) == 0 and expand(B=0, scales=p, k=128, n_use=128, alpha=0.0, qw=0.0, add=0, D=8448) == 0
    assert expand(B=0, o32=p) == 0 and expand(B=0, o16=p) == 0 and expand(B=0, alpha=inf, qw=inf, n_local=0) == 0
    assert finish(B=0) == 0 and finish(B=0, R=64, o32=null) == 0 and finish(B=0, o16=null) == 0


def test_fake_ops_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "query_expand" in torch_ops.OPS and "query_expand_finish" in torch_ops.OPS
    schema = str(torch.ops.vpr.query_expand.default._schema)
    assert schema.startswith("vpr::query_expand(") and "Tensor? scales" in schema and "bool add_query=True" in schema
    assert str(torch.ops.vpr.query_expand_finish.default._schema).startswith("vpr::query_expand_finish(")
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        q, v, i = mk(37, 8448, dtype=torch.bfloat16), mk(37, 10, dtype=torch.float32), mk(37, 10, dtype=torch.int32)
        for rows, scales in ((mk(50, 8448, dtype=torch.bfloat16), None), (mk(50, 8448, dtype=torch.uint8), mk(50, dtype=torch.float32))):
            part = torch.ops.vpr.query_expand(q, v, i, rows, scales, 100, 10)
            assert part.shape == (37, 8448) and part.dtype == torch.float32 and part.device.type == "cuda"
            part = torch.ops.vpr.query_expand(q, v, i, rows, scales, 0, 3, 1.0, 0.0, False)
            assert part.shape == (37, 8448) and part.dtype == torch.float32
        o32, o16 = torch.ops.vpr.query_expand_finish(mk(3, 37, 8448, dtype=torch.float32), q)
        assert o32.shape == o16.shape == (37, 8448) and o32.dtype == torch.float32 and o16.dtype == torch.bfloat16


def test_wrappers_refuse_what_they_cannot_take(monkeypatch):
    from vpr_amd import ops
    B, D, k, n = 2, 64, 3, 5
    q, v, i = torch.zeros(B, D, dtype=torch.bfloat16), torch.ones(B, k), torch.zeros(B, k, dtype=torch.int32)
    rows, rows8, sc = torch.zeros(n, D, dtype=torch.bfloat16), torch.zeros(n, D, dtype=torch.uint8), torch.ones(n)
    parts = torch.zeros(2, B, D)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.query_expand(q, v, i, rows)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.query_expand(q, v, i, rows, None, 0, k)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.query_expand_finish(parts, q)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.query_expand_finish(parts, q)
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    for bad, match in (((q.float(), v, i, rows), "q: expected dtype"), ((q, v.double(), i, rows), "vals: expected dtype"),
                       ((q, v, i.long(), rows), "idx: expected dtype"), ((q, v, i, rows.float()), "rows: expected dtype"),
                       ((q[0], v, i, rows), "q: expected 2 dims"), ((q, v[0], i[0], rows), "vals: expected 2 dims"),
                       ((q, v, i, rows[0]), "rows: expected 2 dims"), ((q, v, i[:, :2], rows), "contiguous"),
                       ((q, v, i[:, :2].contiguous(), rows), "shapes differ"), ((q[:1], v, i, rows), "disagree on B"),
                       ((q, v, i, rows[:, :32].contiguous()), "disagree on D"),
                       ((q, v, i, rows, sc), "scales"), ((q, v, i, rows8), "scales"), ((q, v, i, rows8, sc.double()), "scales: expected dtype"),
                       ((q, v, i, rows8, sc[:3]), "one per row")):
        with pytest.raises(RuntimeError, match=match):
            ops.query_expand(*bad)
    for kw, match in ((dict(n_use=0), "n_use"), (dict(n_use=k + 1), "n_use"), (dict(alpha=-1.0), ">= 0"),
                      (dict(q_weight=float("nan")), ">= 0"), (dict(partial=torch.zeros(B, D + 64)), r"\[B, D\]"),
                      (dict(partial=torch.zeros(B, D, dtype=torch.float64)), "partial: expected dtype")):
        with pytest.raises(RuntimeError, match=match):
            ops.query_expand(q, v, i, rows, **kw)
    for bad, match in (((parts.double(), q), "partials: expected dtype"), ((parts[0], q), "expected 3 dims"),
                       ((parts, q.float()), "q: expected dtype"), ((parts, q[:1]), "disagree")):
        with pytest.raises(RuntimeError, match=match):
            ops.query_expand_finish(*bad)


def test_expansion_params_forms():
    from vpr_amd.retrieval import expansion_params
    assert expansion_params(None) is None
    assert expansion_params((5, 2.0)) == {"n_use": 5, "alpha": 2.0, "q_weight": 1.0, "rounds": 1}
    assert expansion_params({"n_use": 3}) == {"n_use": 3, "alpha": 3.0, "q_weight": 1.0, "rounds": 1}
    assert expansion_params({"n_use": 3, "q_weight": 0, "rounds": 2})["rounds"] == 2
    for bad in ({"alpha": 1.0}, {"n_use": 3, "beta": 1}, {"n_use": 3, "rounds": 0}):
        with pytest.raises(ValueError):
            expansion_params(bad)
