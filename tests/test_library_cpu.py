"""CPU: the C-ABI library builds, loads, exports every symbol include/vpr_amd.h declares, and
rejects bad arguments before touching a device (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()          # hipcc cross-compiles gfx950 without a GPU
    from vpr_amd import _lib
    return _lib.lib()


def test_header_and_binding_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", header))
    declared -= {"vpr_status", "vpr_salad_weights", "vpr_salad_weights_f32"}
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by libvpr_amd.so"
    assert lib.vpr_abi_version() == _lib.ABI_VERSION


def test_status_strings(lib):
    assert lib.vpr_status_string(0) == b"ok"
    for code in (-1, -2, -3, -4, 17):
        assert len(lib.vpr_status_string(code)) > 0


def test_workspace_queries(lib):
    assert lib.vpr_knn_workspace_bytes(64, 100000, 8448, 10) >= 64 * 100000 * 4
    assert lib.vpr_knn_workspace_bytes(64, 1000, 8447, 10) == 0        # D % 64 != 0
    assert lib.vpr_knn_workspace_bytes(64, 1000, 8448, 65) == 0        # k > 64
    assert lib.vpr_knn_workspace_bytes(0, 1000, 8448, 10) == 0
    assert lib.vpr_salad_workspace_bytes(64, 256, 1024, 64, 128, 256, 512) >= 64 * 256 * 1024 * 2
    assert lib.vpr_pose_head_workspace_bytes(64, 8448, 512, 4) > 0
    assert lib.vpr_pose_head_workspace_bytes(64, 768, 0, 2) > 0


def test_invalid_arguments_are_rejected_without_a_device(lib):
    from vpr_amd import _lib
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.vpr_knn_topk(null, null, 1, 1, 64, 1, 0, null, null, null, 0, null) in (-1, -3)
    assert lib.vpr_knn_topk(p, p, 1, 10, 65, 1, 0, p, p, p, 4096, null) == -2           # D % 64
    assert lib.vpr_knn_topk(p, p, 1, 10, 64, 1, 0, p, p, p, 16, null) == -3             # workspace too small
    assert lib.vpr_topk_merge(null, null, 2, 1, 1, null, null, null) == -1
    assert lib.vpr_topk_merge(p, p, 5000, 1, 1, p, p, null) == -2
    assert lib.vpr_pose_head(null, null, null, null, null, null, 1, 64, 32, 2, -1, null, 0, null) == -1
    assert lib.vpr_pose_head(p, p, p, p, p, p, 1, 65, 32, 2, -1, p, 4096, null) == -2    # D % 16
    assert lib.vpr_pose_head(p, p, p, p, p, p, 1, 64, 32, 9, -1, p, 4096, null) == -2    # n_out > 8
    assert lib.vpr_ln_meanpool_head(p, 0, 1, 4, 100, p, p, 1e-5, p, null, null, 0, -1, null, null) == -2   # H unsupported
    # a non-negative sincos_offset needs sincos_offset + 2 <= n_out, at all five head entry points
    for n_out, off in ((2, 1), (2, 2), (1, 0), (8, 7)):
        assert lib.vpr_pose_head(p, p, p, p, p, p, 1, 64, 32, n_out, off, p, 4096, null) == -1
        assert lib.vpr_pose_head(p, null, null, p, p, p, 1, 64, 0, n_out, off, p, 4096, null) == -1          # linear head
        assert lib.vpr_pose_head_split(p, p, p, p, p, p, p, 1, 64, 32, n_out, off, p, 4096, null) == -1
        assert lib.vpr_pose_head_fused(p, p, p, p, p, p, p, 1, 64, 32, n_out, off, p, 4096, null) == -1
        assert lib.vpr_ln_meanpool_head(p, 0, 1, 4, 512, p, p, 1e-5, p, p, p, n_out, off, p, null) == -1
    assert lib.vpr_ln_meanpool_head(p, 0, 1, 4, 100, p, p, 1e-5, p, null, null, 0, 3, null, null) == -2      # no head: the offset is not looked at
    assert lib.vpr_topk_merge(p, p, 1, 1, 129, p, p, null) == -2                                             # k > 128
    assert lib.vpr_topk_merge(p, p, 4097, 1, 1, p, p, null) == -2                                            # shards * k > 4096
    assert lib.vpr_quantize_fp8_rows(p, 1, 6, p, p, null) == -2                                              # D % 4
    assert lib.vpr_gemm_nt_bf16(p, 64, 0, 0, p, 64, null, 0, p, 8, 0, 8, 8, 60, null) == -2   # K % 64
    a16 = ctypes.c_void_p((p.value + 15) // 16 * 16)
    b4 = ctypes.c_void_p(a16.value + 4)
    assert lib.vpr_gemm256_nt_bf16(a16, 128, 0, 0, a16, 128, b4, 0, a16, 8, 0, 8, 8, 128, null) == -2   # bias off 16 B
    assert lib.vpr_gemm_nt_group_bf16(None, 1, None) == -1
    bad = _lib.GemmProblemC(a16.value, 64, 0, 0, a16.value, 64, None, 0, a16.value, 8, 0, 8, 8, 60)
    assert lib.vpr_gemm_nt_group_bf16(ctypes.byref(bad), 1, null) == -2                          # K % 64
    assert lib.vpr_gemm_nt_group_bf16(ctypes.byref(bad), 4, null) == -1                          # more than 3 problems
    assert lib.vpr_salad_sinkhorn_aggregate(p, p, p, 1, 100, 64, 128, 256, 1.0, 3, p, null, null) == -2
    assert lib.vpr_f32_to_bf16(null, null, 4, null) == -1
    # head-only fine-tuning step: arguments are judged before anything is launched
    hp = (1e-5, 0.9, 0.999, 1e-8, 1e-2, 0, 0.0)           # lr, betas, eps, weight decay, VPR_LOSS_MSE, (delta unused)
    ws = lib.vpr_head_train_workspace_bytes(16, 64, 32, 2)
    assert ws > 0 and lib.vpr_head_train_workspace_bytes(65, 64, 32, 2) == 0 and lib.vpr_head_train_workspace_bytes(16, 60, 32, 2) == 0
    assert lib.vpr_head_train_workspace_bytes(16, 64, 48, 2) == 0 and lib.vpr_head_train_workspace_bytes(16, 64, 32, 9) == 0
    assert lib.vpr_head_train_state_floats(8448, 512, 2) == 512 * 8448 + 512 + 2 * 512 + 2
    assert lib.vpr_head_train_step(null, 64, null, null, 2, 16, 64, 32, 2, null, null, null, null, null, null, 1, *hp, null, null, 0, null) == -1
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 0, *hp, null, p, 4096, null) == -1        # step < 1
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 1, 1e-5, 1.0, 0.999, 1e-8, 0.0, 0, 0.0, null, p, 4096, null) == -1   # beta1 = 1
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 1, 1e-5, 0.9, 0.999, 1e-8, 0.0, 1, 0.0, null, p, 4096, null) == -1    # Huber needs delta > 0
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 1, 1e-5, 0.9, 0.999, 1e-8, 0.0, 2, 1.0, null, p, 4096, null) == -1    # unknown loss kind
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 65, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 4096, null) == -2        # B > 64
    assert lib.vpr_head_train_step(p, 62, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 4096, null) == -1        # x_stride < D
    assert lib.vpr_head_train_step(p, 64, null, p, 2, 16, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 16, null) == -3          # workspace too small
    assert lib.vpr_head_train_epoch(p, 64, null, 40, 16, p, 2, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 4096, null) == -1    # no order
    assert lib.vpr_head_train_epoch(p, 64, p, 100, 65, p, 2, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 1 << 20, null) == -2   # batch > 64
    assert lib.vpr_head_train_epoch(p, 64, p, 40, 16, p, 2, 64, 32, 2, p, p, p, p, p, p, 1, *hp, null, p, 16, null) == -3
    assert lib.vpr_f32_to_bf16(p, p, 0, null) == 0


def test_ops_refuse_cpu_tensors():
    import torch
    from vpr_amd import ops
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.knn_topk(torch.zeros(1, 64, dtype=torch.bfloat16), torch.zeros(4, 64, dtype=torch.bfloat16), 1)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.pose_head(torch.zeros(1, 64), None, None, torch.zeros(2, 64), torch.zeros(2))


def test_pair_offset_without_a_pair_raises_in_wrappers_fakes_and_oracle():
    """sincos_offset + 2 <= n_out: ops.check_sincos_offset (what the wrappers call before anything else is judged), the
    torch.ops.vpr fakes and the oracle all raise RuntimeError."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import ops, torch_ops  # noqa: F401
    from oracle import heads as oheads
    for n_out, off in ((2, 1), (2, 2), (1, 0), (8, 7)):
        with pytest.raises(RuntimeError, match="sincos_offset"):
            ops.check_sincos_offset("pose_head", off, n_out)
        with pytest.raises(RuntimeError, match="sincos_offset"):
            oheads.mlp_head(torch.zeros(1, 4), None, None, torch.zeros(n_out, 4), torch.zeros(n_out), off)
        with FakeTensorMode():
            x, W2, b2 = torch.empty(3, 64), torch.empty(n_out, 64), torch.empty(n_out)
            with pytest.raises(RuntimeError, match="sincos_offset"):
                torch.ops.vpr.pose_head(x, None, None, W2, b2, off)
            with pytest.raises(RuntimeError, match="sincos_offset"):
                torch.ops.vpr.ln_meanpool_head(torch.empty(3, 4, 512), torch.empty(512), torch.empty(512), 1e-5,
                                               torch.empty(n_out, 512), b2, off)
    for n_out, off in ((2, 0), (8, 6), (1, -1), (3, -5)):
        ops.check_sincos_offset("pose_head", off, n_out)
    with FakeTensorMode():
        assert torch.ops.vpr.pose_head(torch.empty(3, 64), None, None, torch.empty(2, 64), torch.empty(2), 0).shape == (3, 2)
        assert torch.ops.vpr.ln_meanpool_head(torch.empty(3, 4, 512), torch.empty(512), torch.empty(512), 1e-5, None, None, 5)[0].shape == (3, 512)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from vpr_amd import _lib
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setattr(_lib, "library_path", lambda: str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_lds_swizzle_is_conflict_free():
    """Host re-derivation of vpr_common.h::tile_off for every ds_read_b128 lane group of both
    MFMA operand maps (bank = (addr/4) % 64; a 16-lane group must hit 16 distinct 16-B slots)."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[x + 32 for x in g] for g in groups]
    off = lambda row, chunk: row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4)
    for kk in (0, 1):                                   # 16x16x32: row = lane&15, chunk = lane>>4 (+4)
        for g in groups:
            slots = {(off(l & 15, (l >> 4) + 4 * kk) // 16) % 16 for l in g}
            assert len(slots) == 16
    for s in range(4):                                  # 32x32x16: row = lane&31, chunk = lane>>5 (+2s)
        for g in groups:
            slots = {(off(l & 31, (l >> 5) + 2 * s) // 16) % 16 for l in g}
            assert len(slots) == 16
    # the staging side writes physical slot (row, p) with logical chunk p ^ swz(row): a bijection per row
    for row in range(16):
        assert sorted((p ^ ((row >> 1) & 7)) for p in range(8)) == list(range(8))


def test_tuning_switches_are_read_once_at_load(lib, monkeypatch):
    """include/vpr_amd.h, "State the library keeps": the VPR_* switches are read from the environment when the library
    is loaded; a later setenv() has no effect, vpr_tuning_set() is the only way to change one, unknown names are refused."""
    from vpr_amd import _lib
    before = _lib.tuning_get("VPR_KNN_VARIANT")
    monkeypatch.setenv("VPR_KNN_VARIANT", "6")
    monkeypatch.setenv("VPR_POSE_KS", "9")
    assert _lib.tuning_get("VPR_KNN_VARIANT") == before               # the environment is not consulted again
    assert lib.vpr_knn_scores_kernel_name(0, 64, 100000) == b"vpr::knn_scores_kernel<false, 208, 2, 4>" or before not in (None, 0)
    with _lib.tuning(VPR_KNN_VARIANT=1):
        assert _lib.tuning_get("VPR_KNN_VARIANT") == 1
        assert lib.vpr_knn_scores_kernel_name(0, 64, 100000) == b"vpr::knn_scores_kernel<false, 208, 2, 0>"
    assert _lib.tuning_get("VPR_KNN_VARIANT") == before
    v = ctypes.c_int(0)
    assert lib.vpr_tuning_get(b"VPR_NOT_A_SWITCH", ctypes.byref(v)) == -1
    assert lib.vpr_tuning_set(b"VPR_NOT_A_SWITCH", 1, 0) == -1
    assert lib.vpr_tuning_set(None, 1, 0) == -1


def test_score_kernel_name_is_the_kernel_the_launch_code_picks(lib):
    """vpr_knn_scores_kernel_name describes the call the way the score stage does.  Without a device the library counts
    256 CUs (an MI355X), so 100k / 120k / 140k rows sit below, between and above the tall-tile (N > 106 496) and
    multi-tile (N > 131 072) rules.  Every VPR_KNN_VARIANT of the release library, both operand types; then the GEMM
    routes, whose names come from gemm_nt.hip / gemm256.hip."""
    from vpr_amd import _lib
    nt, staged, staged_nt = 4, 36, 52
    by_shard = lambda flags: [(208, 2, flags), (256, 2, flags), (256, 2, flags)]
    expected = {
        None: [(208, 2, nt), (256, 2, nt), (256, 2, staged_nt)], 0: [(208, 2, nt), (256, 2, nt), (256, 2, staged_nt)],
        1: [(208, 2, 0)] * 3, 2: [(144, 3, nt)] * 3, 3: [(256, 2, nt)] * 3, 4: [(208, 2, nt)] * 3,
        5: by_shard(nt), 6: by_shard(staged), 7: by_shard(staged_nt),
    }
    switches = ("VPR_KNN_VARIANT", "VPR_KNN_GEMM_MIN_B", "VPR_KNN_GEMM_KSPLIT", "VPR_KNN_FP8_GEMM256", "VPR_GEMM_NT_STAGES")
    before = {s: _lib.tuning_get(s) for s in switches}
    try:
        for s in switches:
            _lib.tuning_set(s, None)
        for variant, triples in expected.items():
            _lib.tuning_set("VPR_KNN_VARIANT", variant)
            for N, (rows, wgpc, flags) in zip((100_000, 120_000, 140_000), triples):
                for fp8 in (0, 1):
                    want = f"vpr::knn_scores_kernel<{'true' if fp8 else 'false'}, {rows}, {wgpc}, {flags}>"
                    assert lib.vpr_knn_scores_kernel_name(fp8, 64, N).decode() == want, (variant, N, fp8)
        _lib.tuning_set("VPR_KNN_VARIANT", None)
        assert lib.vpr_knn_scores_kernel_name(0, 150, 3000) == b"vpr::gemm_nt_kernel<128, 2, 2, 2>"
        _lib.tuning_set("VPR_GEMM_NT_STAGES", 3)
        assert lib.vpr_knn_scores_kernel_name(0, 150, 3000) == b"vpr::gemm_nt_kernel<128, 2, 2, 3>"
        assert lib.vpr_knn_scores_kernel_name(1, 150, 3000) == b"vpr::gemm_nt_fp8_kernel"       # the switch is bf16 only
        _lib.tuning_set("VPR_GEMM_NT_STAGES", None)
        assert lib.vpr_knn_scores_kernel_name(0, 150, 40) == b"vpr::gemm_nt_kernel<64, 4, 1, 2>"
        assert lib.vpr_knn_scores_kernel_name(1, 150, 3000) == b"vpr::gemm_nt_fp8_kernel"
        assert lib.vpr_knn_scores_kernel_name(0, 512, 6378) == b"vpr::gemm256_kernel<false, 10>"
        assert lib.vpr_knn_scores_kernel_name(1, 512, 6378) == b"vpr::gemm256_kernel<true, 10>"
        assert lib.vpr_knn_scores_kernel_name(0, 0, 1000) == b""
    finally:
        for s, v in before.items():
            _lib.tuning_set(s, v)


def test_knn_invalid_calls_keep_their_statuses(lib):
    """One fault per call, every call refused before anything is launched: the status each kNN entry point answers.
    The stage / one-call / exhaustive forms call a non-positive size an invalid argument (-1); vpr_knn_scores,
    vpr_knn_select and vpr_knn_select_checked have always called it unsupported (-2).  Everything else agrees."""
    raw = (ctypes.c_char * (1 << 20))()
    base = (ctypes.addressof(raw) + 255) // 256 * 256
    P = ctypes.c_void_p(base)                       # 256-byte aligned, stands in for every pointer
    null, off2, WS = ctypes.c_void_p(0), ctypes.c_void_p(base + 2), 512 << 10
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3

    # call(name, **overrides): the base call B=1, N=10, k=1, D=64 (bf16) / 128 (fp8) with the given arguments replaced
    def call(name, fp8=False, **kw):
        a = dict(q=P, qs=P if fp8 else null, g=P, gs=P if fp8 else null, B=1, N=10, D=128 if fp8 else 64, k=1,
                 val=P, idx=P, ws=P, bytes=WS, bound=1.002, status=null, unc=null)
        a.update(kw)
        shape, out, ws = (a["B"], a["N"], a["D"], a["k"]), (0, a["val"], a["idx"]), (a["ws"], a["bytes"])
        cert = (a["bound"], a["status"], a["unc"])
        bf16, f8, any_ = (a["q"], a["g"]), (a["q"], a["qs"], a["g"], a["gs"]), (a["q"], a["qs"], a["g"], a["gs"], int(fp8))
        args = {
            "vpr_knn_topk": bf16 + shape + out + ws, "vpr_knn_topk_checked": bf16 + shape + out + ws + cert,
            "vpr_knn_topk_fp8": f8 + shape + out + ws, "vpr_knn_topk_fp8_checked": f8 + shape + out + ws + cert,
            "vpr_knn_topk_scores_stage": any_ + shape + ws, "vpr_knn_topk_select_stage": any_ + shape + out + ws + cert,
            "vpr_knn_topk_exhaustive": any_ + shape + out + ws,
            "vpr_knn_scores": bf16 + shape[:3] + ws, "vpr_knn_select": bf16 + shape + out + ws,
            "vpr_knn_select_checked": bf16 + shape + out + ws + cert,
        }[name]
        return getattr(lib, name)(*args, null)

    bf16_new = ["vpr_knn_topk", "vpr_knn_topk_checked", "vpr_knn_topk_scores_stage", "vpr_knn_topk_select_stage",
                "vpr_knn_topk_exhaustive"]
    fp8_new = ["vpr_knn_topk_fp8", "vpr_knn_topk_fp8_checked", "vpr_knn_topk_scores_stage", "vpr_knn_topk_select_stage",
               "vpr_knn_topk_exhaustive"]
    old = ["vpr_knn_scores", "vpr_knn_select", "vpr_knn_select_checked"]
    has_k = lambda n: n != "vpr_knn_scores"
    has_out = lambda n: n not in ("vpr_knn_scores", "vpr_knn_topk_scores_stage")
    seen = []

    def expect(name, status, **kw):
        got = call(name, **kw)
        seen.append((name, kw, got, status))

    for fp8, names in ((False, bf16_new + old), (True, fp8_new)):
        for n in names:
            bad_shape = UNSUPPORTED if n in old else INVALID
            for dim in ("B", "N", "D", "k"):
                for v in (0, -1):
                    if dim != "k" or has_k(n):
                        expect(n, bad_shape, fp8=fp8, **{dim: v})
            if has_k(n):
                expect(n, UNSUPPORTED, fp8=fp8, k=65)
            for D in ((64, 192) if fp8 else (65, 100)):
                expect(n, UNSUPPORTED, fp8=fp8, D=D)
            if fp8:
                expect(n, UNSUPPORTED, fp8=fp8, D=100)
                expect(n, INVALID, fp8=fp8, qs=null)
                expect(n, INVALID, fp8=fp8, gs=null)
            for ptr in ("q", "g", "ws") + (("val", "idx") if has_out(n) else ()):
                expect(n, INVALID, fp8=fp8, **{ptr: null})
            expect(n, WORKSPACE, fp8=fp8, bytes=16)
            expect(n, UNSUPPORTED, fp8=fp8, q=off2)
            expect(n, UNSUPPORTED, fp8=fp8, g=off2)
    for n in ("vpr_knn_select_checked", "vpr_knn_topk_select_stage"):
        for bound in (0.0, -1.0):
            expect(n, INVALID, bound=bound)
            expect(n, INVALID, bound=bound, B=0)             # the bound is judged before the shape
    wrong = [s for s in seen if s[2] != s[3]]
    assert not wrong, wrong
    assert len(seen) > 250


def test_tuning_switches_come_from_the_environment_of_the_loading_process():
    """A fresh process with VPR_KNN_VARIANT=1 in its environment loads a library that reports 1 (and picks that kernel)."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import vpr_amd; from vpr_amd import _lib; "
            "print(_lib.tuning_get('VPR_KNN_VARIANT'), _lib.tuning_get('VPR_POSE_KS'), "
            "_lib.lib().vpr_knn_scores_kernel_name(0, 64, 100000).decode())" % ROOT)
    env = dict(os.environ, VPR_KNN_VARIANT="1")
    env.pop("VPR_POSE_KS", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out[0] == "1" and out[1] == "None" and "208, 2, 0" in " ".join(out[2:])


def test_head_train_slice_count_matches_the_oracle_restatement(lib):
    """oracle/finetune.py restates head_train_slices (its error bounds need the slab count).  The first region of the
    training workspace is align256(ks * B * hidden * 4) bytes, so the library's ks shows in the total."""
    from oracle import finetune as oft
    shapes = [(B, D, hidden, 2) for D, hidden in oft.FORWARD_EDGES for B in oft.FORWARD_BATCHES] + list(oft.UPDATE_EDGES)
    shapes += [(6, 8448, 512, 2), (64, 8448, 1024, 4), (33, 256, 64, 8), (5, 64, 32, 2)]
    seen = set()
    for B, D, hidden, n_out in shapes:
        total = lib.vpr_head_train_workspace_bytes(B, D, hidden, n_out)
        assert total > 0, (B, D, hidden, n_out)
        ks = oft.head_train_slices(B, D, hidden)
        seen.add(ks)
        assert oft.head_train_first_region(total, B, hidden, n_out) == -(-ks * B * hidden * 4 // 256) * 256, (B, D, hidden, n_out, ks)
    assert {1, 64} <= seen and len(seen) >= 6, seen          # the clamp at one slice, the cap, and several in between
