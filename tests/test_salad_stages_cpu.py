"""CPU: the SALAD stage-output extension of the C ABI (include/vpr_amd_salad_stages.h) — header, binding table and exported
symbol agree, the older tables are what they were, every refusal comes back with the status the stage calls give before a
device is touched, and the pointers it returns lie inside the workspace, apart from each other, on both routes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
N, M, L, T, HID = 256, 64, 128, 256, 512


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def _outputs(lib, ws, ws_bytes, B=2, n=N, C=128, m=M, l=L, t=T, hidden=HID, want=("S", "F", "g", "H", "slabs", "rows")):
    S, F, g, H = (ctypes.c_void_p(0) for _ in range(4))
    slabs, rows = ctypes.c_int(-7), ctypes.c_longlong(-7)
    ref = lambda name, v: ctypes.byref(v) if name in want else None
    st = lib.vpr_salad_stage_outputs(ws, ws_bytes, B, n, C, m, l, t, hidden, ref("S", S), ref("F", F), ref("g", g), ref("H", H),
                                     ref("slabs", slabs), ref("rows", rows))
    return st, (S.value or 0, F.value or 0, g.value or 0, H.value or 0, slabs.value, rows.value)


def test_header_table_and_symbol_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_salad_stages.h")).read()
    assert re.search(r"additive\s+extension\s+of\s+ABI 6", header, flags=re.I) and "present iff" in header
    assert "b2_s" in header and "cancel" in header.lower()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.SALAD_STAGES_PROTOTYPES) == {"vpr_salad_stage_outputs"}
    restype, argtypes = _lib.SALAD_STAGES_PROTOTYPES["vpr_salad_stage_outputs"]
    fn = lib.vpr_salad_stage_outputs                         # exported by the built library, bound by _lib.lib()
    assert fn.restype == restype and fn.argtypes == argtypes and len(argtypes) == 15
    params = re.search(r"vpr_salad_stage_outputs\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(params.split(",")) == len(argtypes)
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_older_tables_are_unchanged_and_disjoint():
    from vpr_amd import _lib
    assert set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert set(_lib.EXPAND_PROTOTYPES) == {"vpr_query_expand", "vpr_query_expand_finish"}
    assert set(_lib.PROJECT_PROTOTYPES) == {"vpr_project_workspace_bytes", "vpr_project_route", "vpr_project_rows"}
    assert set(_lib.RERANK_PROTOTYPES) == {"vpr_rerank_workspace_bytes", "vpr_rerank_rows"}
    assert len(_lib.PROTOTYPES) == 61
    new = set(_lib.SALAD_STAGES_PROTOTYPES)
    for older in (_lib.PROTOTYPES, _lib.EXTENSION_PROTOTYPES, _lib.EXPAND_PROTOTYPES, _lib.PROJECT_PROTOTYPES, _lib.RERANK_PROTOTYPES):
        assert not new & set(older)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vpr_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", main)) - {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES)                  # vpr_amd.h still lists exactly the first table
    assert "vpr_salad_stage_outputs" not in main and re.search(r"#define VPR_AMD_ABI_VERSION 6\b", main)
    for other in ("vpr_amd_retrieval.h", "vpr_amd_expand.h", "vpr_amd_project.h", "vpr_amd_rerank.h"):
        assert "vpr_salad_stage_outputs" not in open(os.path.join(ROOT, "include", other)).read()


def test_refusals_are_those_of_the_stage_calls_and_need_no_device(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))               # never dereferenced: the call is pointer arithmetic
    big = 1 << 40
    untouched = (0, 0, 0, 0, -7, -7)
    for kw in (dict(ws=None), dict(B=0), dict(B=-3), dict(n=0), dict(C=0), dict(C=-64), dict(hidden=0), dict(hidden=-64),
               dict(want=("F", "g", "H", "slabs", "rows")), dict(want=("S", "g", "slabs", "rows")), dict(want=("S", "F", "slabs", "rows")),
               dict(want=("S", "F", "g", "rows")), dict(want=("S", "F", "g", "slabs"))):
        kw = dict(kw)
        st, out = _outputs(lib, kw.pop("ws", p), big, **kw)
        assert st == INVALID and all(o in (0, -7) for o in out), kw
    for kw in (dict(n=255), dict(n=257), dict(m=32), dict(m=128), dict(l=64), dict(t=128), dict(C=96), dict(C=1000), dict(hidden=500)):
        st, out = _outputs(lib, p, big, **kw)
        assert st == UNSUPPORTED and out == untouched, kw
    # the same refusal, with the same status, from the stage that would read these outputs
    assert lib.vpr_salad_stage_aggregate(2, 255, 128, 1.0, M, L, T, HID, 3, p, None, p, big, None) == UNSUPPORTED
    assert lib.vpr_salad_stage_aggregate(0, N, 128, 1.0, M, L, T, HID, 3, p, None, p, big, None) == INVALID
    for B, C, hidden in ((1, 128, 512), (2, 64, 512), (33, 1024, 512), (3, 768, 256)):
        need = lib.vpr_salad_workspace_bytes(B, N, C, M, L, T, hidden)
        assert need > 0
        assert _outputs(lib, p, need - 1, B=B, C=C, hidden=hidden) == (WORKSPACE, untouched)
        assert lib.vpr_salad_stage_aggregate(B, N, C, 1.0, M, L, T, hidden, 3, p, None, p, need - 1, None) == WORKSPACE
        assert _outputs(lib, p, need, B=B, C=C, hidden=hidden)[0] == 0
    assert _outputs(lib, p, big, want=("S", "F", "g", "slabs", "rows"))[0] == 0          # H is optional


@pytest.mark.parametrize("B,C,hidden,slabs", [(1, 128, 512, 2), (9, 192, 512, 2), (2, 1024, 512, 2), (2, 64, 512, 1),
                                              (3, 768, 256, 1), (3, 128, 1024, 1)])
def test_regions_lie_inside_the_workspace_and_apart(lib, tune, B, C, hidden, slabs):
    """The layout itself stays the library's business; what a caller may rely on: every region the call names lies inside
    vpr_salad_workspace_bytes, 16-byte aligned, behind the 4 KB counter area, and no two of them overlap.  The route is
    the one the A/B switch selects at the time of the call."""
    base = 1 << 20
    need = lib.vpr_salad_workspace_bytes(B, N, C, M, L, T, hidden)
    for variant, want_slabs in ((None, slabs), (1, 1)):
        tune("VPR_SALAD_VARIANT", variant)
        st, (S, F, g, H, ns, rows) = _outputs(lib, ctypes.c_void_p(base), need, B=B, C=C, hidden=hidden)
        assert st == 0 and ns == want_slabs and rows == B * N
        regions = [(S, ns * rows * M * 4), (F, ns * rows * L * 4), (g, B * T * 4)] + ([(H, rows * 2 * hidden * 2)] if ns == 1 else [])
        for lo, size in regions:
            assert lo % 16 == 0 and base + 4096 <= lo and lo + size <= base + need
        regions.sort()
        assert all(a + sa <= b for (a, sa), (b, _) in zip(regions, regions[1:]))
    tune("VPR_SALAD_VARIANT", None)
