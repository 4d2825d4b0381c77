"""CPU: the f32 SALAD stage-output extension of the C ABI (include/vpr_amd_salad_f32_stages.h) — header, binding table and
exported symbol agree, the older tables are what they were, every refusal comes back with the status and in the order the
three f32 aggregation entries give on the same arguments, a refused call writes nothing, and the buffers it names lie inside
vpr_salad_f32_workspace_bytes, apart from each other."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
N, M, L, T, HID = 256, 64, 128, 256, 512
NAMES = ("H", "Ht", "S", "F", "g", "A1", "cls3", "W1", "H2", "W1t", "W2s", "W2c", "W2t", "Ht2")
REQUIRED, OPTIONAL = NAMES[:9], NAMES[9:]
SENTINEL = 0x5A5A5A50


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def _outputs(lib, ws, ws_bytes, B=2, n=N, C=128, m=M, l=L, t=T, hidden=HID, want=NAMES):
    out = {k: ctypes.c_void_p(SENTINEL) for k in NAMES}
    st = lib.vpr_salad_f32_stage_outputs(ws, ws_bytes, B, n, C, m, l, t, hidden, *[ctypes.byref(out[k]) if k in want else None for k in NAMES])
    return st, {k: v.value for k, v in out.items()}


def _untouched(out):
    return all(v == SENTINEL for v in out.values())


def test_header_table_and_symbol_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_salad_f32_stages.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    assert "b2_s" in header and "cancel" in header.lower() and "2^-60, 2^60" in header and "subnormal" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SALAD_F32_STAGES_PROTOTYPES) == {"vpr_salad_f32_stage_outputs"}
    restype, argtypes = _lib.SALAD_F32_STAGES_PROTOTYPES["vpr_salad_f32_stage_outputs"]
    fn = lib.vpr_salad_f32_stage_outputs                     # exported by the built library, bound by _lib.lib()
    assert fn.restype == restype and fn.argtypes == argtypes and len(argtypes) == 9 + len(NAMES)
    params = re.search(r"vpr_salad_f32_stage_outputs\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(params.split(",")) == len(argtypes)
    assert [p.split("*")[-1].strip() for p in params.split(",")[9:]] == list(NAMES)      # the order ops.salad_f32_stage_views relies on
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
    assert len(_lib.PROTOTYPES) == 61
    new = set(_lib.SALAD_F32_STAGES_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES,
                  _lib.SALAD_STAGES_PROTOTYPES, _lib.SALAD_ANYRES_PROTOTYPES, _lib.SALAD_HIRES_PROTOTYPES, _lib.LOCAL_PROTOTYPES):
        assert not new & set(older)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "vpr_amd_salad_f32_stages.h":
            assert "vpr_salad_f32_stage_outputs" not in open(os.path.join(ROOT, "include", other)).read(), other


def _run(lib, entry, ws, ws_bytes, B=2, n=N, C=128, m=M, l=L, t=T, hidden=HID):
    """The aggregation entry on the same workspace and shape, everything else sound (dummy pointers, never dereferenced:
    each status compared below is decided before a launch)."""
    from vpr_amd import _lib
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)
    w = _lib.SaladWeightsF32C(*[p.value] * 10)
    return getattr(lib, entry)(p, n * C, p, C, B, n, C, ctypes.byref(w), 1.0, m, l, t, hidden, 3, p, None, ws, ws_bytes, None)


def test_refusals_are_those_of_the_f32_aggregation_in_its_order_and_write_nothing(lib):
    buf = (ctypes.c_char * 128)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)          # never dereferenced: the call is pointer arithmetic
    big = 1 << 42
    hires = "vpr_salad_aggregate_f32_hires"
    # argument checks
    for kw in (dict(ws=None), dict(B=0), dict(B=-3), dict(n=0), dict(n=-1), dict(C=0), dict(C=-64),
               *[dict(want=tuple(k for k in NAMES if k != name)) for name in REQUIRED]):
        kw = dict(kw)
        ws = kw.pop("ws", p)
        st, out = _outputs(lib, ws, big, **kw)
        assert st == INVALID and _untouched(out), kw
        if "want" not in kw:
            assert _run(lib, hires, ws, big, **kw) == INVALID, kw
    # domain: the widest of the three entries', so the high-resolution entry agrees on every n
    for kw in (dict(n=64), dict(n=1), dict(n=1370), dict(m=32), dict(m=128), dict(l=64), dict(t=128), dict(C=96), dict(C=1000), dict(hidden=500)):
        st, out = _outputs(lib, p, big, **kw)
        assert st == UNSUPPORTED and _untouched(out), kw
        assert _run(lib, hires, p, big, **kw) == UNSUPPORTED, kw
    for n in (65, 255, 256, 257, 576, 577, 1369):
        assert _outputs(lib, p, big, n=n)[0] == 0 and _run(lib, hires, p, 0, n=n) == WORKSPACE
    assert _run(lib, "vpr_salad_aggregate_f32", p, big, n=257) == UNSUPPORTED and _run(lib, "vpr_salad_aggregate_f32_n", p, big, n=577) == UNSUPPORTED
    # alignment of the workspace, then hidden <= 0 (the plan), then the workspace size
    st, out = _outputs(lib, odd, big)
    assert st == UNSUPPORTED and _untouched(out) and _run(lib, hires, odd, big) == UNSUPPORTED
    for hidden in (0, -64):
        st, out = _outputs(lib, p, big, hidden=hidden)
        assert st == INVALID and _untouched(out) and _run(lib, hires, p, big, hidden=hidden) == INVALID
    for B, n, C, hidden in ((1, 256, 128, 512), (2, 65, 64, 512), (9, 256, 192, 512), (2, 577, 128, 512), (3, 256, 768, 256)):
        need = lib.vpr_salad_f32_workspace_bytes(B, n, C, M, L, T, hidden)
        assert need > 0
        st, out = _outputs(lib, p, need - 1, B=B, n=n, C=C, hidden=hidden)
        assert st == WORKSPACE and _untouched(out)
        assert _run(lib, hires, p, need - 1, B=B, n=n, C=C, hidden=hidden) == WORKSPACE
        assert _outputs(lib, p, need, B=B, n=n, C=C, hidden=hidden)[0] == 0
    # the order, on double faults: argument before domain before alignment before size
    assert _outputs(lib, odd, 0, B=0, n=64)[0] == _run(lib, hires, odd, 0, B=0, n=64) == INVALID
    assert _outputs(lib, odd, 0, n=64)[0] == _run(lib, hires, odd, 0, n=64) == UNSUPPORTED
    assert _outputs(lib, odd, 0)[0] == _run(lib, hires, odd, 0) == UNSUPPORTED
    assert _outputs(lib, p, 0, hidden=0)[0] == _run(lib, hires, p, 0, hidden=0) == INVALID
    assert _outputs(lib, p, 0)[0] == _run(lib, hires, p, 0) == WORKSPACE
    # the optional outputs may be left out, each alone and all together; the others are still answered
    for left_out in [(k,) for k in OPTIONAL] + [OPTIONAL]:
        st, out = _outputs(lib, p, big, want=tuple(k for k in NAMES if k not in left_out))
        assert st == 0 and all((out[k] == SENTINEL) == (k in left_out) for k in NAMES)


@pytest.mark.parametrize("B,n,C,hidden", [(1, 256, 64, 512), (9, 256, 192, 512), (3, 256, 768, 512), (2, 65, 128, 512), (2, 577, 128, 512),
                                          (1, 1369, 1024, 512), (3, 256, 128, 256), (2, 529, 320, 1024)])
def test_buffers_lie_inside_the_workspace_and_apart(lib, B, n, C, hidden):
    """Every buffer the call names, at the size the header states, lies inside vpr_salad_f32_workspace_bytes, 16-byte
    aligned (the plan aligns to 256), and no two of them overlap; the last one ends within the workspace."""
    base = 1 << 24
    need = lib.vpr_salad_f32_workspace_bytes(B, n, C, M, L, T, hidden)
    st, out = _outputs(lib, ctypes.c_void_p(base), need, B=B, n=n, C=C, hidden=hidden)
    assert st == 0
    r = B * n
    size = dict(H=r * 2 * hidden * 4, Ht=B * hidden * 4, S=r * M * 4, F=r * L * 4, g=B * T * 4, A1=r * 6 * C * 2, cls3=B * 6 * C * 2,
                W1=2 * hidden * 6 * C * 2, H2=r * 12 * hidden * 2, W1t=hidden * 6 * C * 2, W2s=M * 6 * hidden * 2, W2c=L * 6 * hidden * 2,
                W2t=T * 6 * hidden * 2, Ht2=B * 6 * hidden * 2)
    regions = sorted((out[k], size[k]) for k in NAMES)
    for lo, sz in regions:
        assert lo % 256 == 0 and base <= lo and lo + sz <= base + need
    assert all(a + sa <= b for (a, sa), (b, _) in zip(regions, regions[1:]))
    assert regions[-1][0] + regions[-1][1] <= base + need and need - sum(size.values()) < 256 * len(NAMES)   # nothing but alignment padding
