"""CPU: every refusal of the three GEMM entry points of the C ABI (vpr_gemm_nt_bf16, vpr_gemm256_nt_bf16 and
vpr_gemm_nt_group_bf16 with 1 .. 3 members), as one table.  Dummy aligned non-null pointers, never dereferenced: each status
below is decided before a launch (without a device a launch would come back as VPR_ERR_LAUNCH, and the kernels would fault on
these pointers), so no row here describes a problem that an entry accepts.

Expected values are literals.  They follow include/vpr_amd.h: INVALID_ARG for a null A, W or C and for a non-positive M, N or
K, ahead of UNSUPPORTED for everything about shape, pitch and alignment.  The single faults are those of test_gemm_refusals in
tests/test_gemm_edges_gpu.py.  Where the header is silent the value is what the library answered before the launch side was
restructured, and the row says so."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
KINDS = ("128", "256", "group")


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 256)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)                   # 64-byte aligned
    ptr._keep = buf
    return ptr


def problem(p, A=0, lda=128, groups=(0, 0), W=0, ldw=128, bias=0, relu=0, C=0, ldc=64, out_bf16=0, M=64, N=64, K=128,
            null=()):
    """The 14 fields of one sound problem (64 x 64 x 128, f32 out, with a bias) except for the faults asked for.  A, W, bias
    and C are byte offsets on the dummy pointer; null names the pointers to pass as null."""
    ptr = lambda name, off: None if name in null else p.value + off
    return (ptr("A", A), lda, groups[0], groups[1], ptr("W", W), ldw, ptr("bias", bias), relu, ptr("C", C), ldc, out_bf16,
            M, N, K)


def call(lib, p, kind, count=1, member=0, **faults):
    """One call of the entry `kind`; the grouped entry gets `count` members, of which `member` carries the faults."""
    from vpr_amd import _lib
    if kind != "group":
        return (lib.vpr_gemm256_nt_bf16 if kind == "256" else lib.vpr_gemm_nt_bf16)(*problem(p, **faults), None)
    arr = (_lib.GemmProblemC * count)(*[_lib.GemmProblemC(*problem(p, **(faults if i == member else {}))) for i in range(count)])
    return lib.vpr_gemm_nt_group_bf16(arr, count, None)


def every(status, kinds=KINDS):
    return {k: status for k in kinds}


# (what, keyword faults, {kind: expected status}); a kind that accepts the problem (and would launch it) is not in the dict
SINGLE = [
    ("K % 64", dict(K=96), every(UNSUPPORTED)),
    ("lda < K", dict(lda=120), every(UNSUPPORTED)),
    ("ldw < K", dict(ldw=120), every(UNSUPPORTED)),
    ("ldc < N", dict(ldc=60), every(UNSUPPORTED)),
    ("lda % 8", dict(lda=132), every(UNSUPPORTED)),
    ("ldw % 8", dict(ldw=260), every(UNSUPPORTED)),
    ("A off 16 B", dict(A=2), every(UNSUPPORTED)),
    ("W off 16 B", dict(W=2), every(UNSUPPORTED)),
    ("a_group_stride % 8", dict(groups=(16, 16 * 128 + 4)), every(UNSUPPORTED)),
    ("M = 0", dict(M=0), every(INVALID)),
    ("N < 0", dict(N=-64), every(INVALID)),
    ("K = 0", dict(K=0), every(INVALID)),
    ("A null", dict(null=("A",)), every(INVALID)),
    ("W null", dict(null=("W",)), every(INVALID)),
    ("C null", dict(null=("C",)), every(INVALID)),
    # the 256-row tiles alone: two K-tiles at least, float4 / 8-byte stores and a float4 bias
    ("gemm256 K < 128", dict(lda=64, ldw=64, K=64), {"256": UNSUPPORTED}),
    ("gemm256 ldc % 4", dict(ldc=66), {"256": UNSUPPORTED}),
    ("gemm256 C off 16 B", dict(C=4), {"256": UNSUPPORTED}),
    ("gemm256 bias off 16 B", dict(bias=4), {"256": UNSUPPORTED}),
]

DOUBLE = [
    # a null pointer or a non-positive size is reported ahead of anything about shape or alignment
    ("A null + K % 64", dict(null=("A",), K=96), every(INVALID)),
    ("W null + K % 64", dict(null=("W",), K=96), every(INVALID)),
    ("C null + K % 64", dict(null=("C",), K=96), every(INVALID)),
    ("M = 0 + A off 16 B", dict(M=0, A=2), every(INVALID)),
    ("K = 0 + lda % 8", dict(K=0, lda=132), every(INVALID)),
    ("C null + ldc % 4 + K < 128", dict(null=("C",), ldc=66, lda=64, ldw=64, K=64), {"256": INVALID}),
    # several reasons for UNSUPPORTED at once are still UNSUPPORTED
    ("gemm256 K < 128 + ldc % 4 + bias off 16 B", dict(lda=64, ldw=64, K=64, ldc=66, bias=4), {"256": UNSUPPORTED}),
    ("K % 64 + A off 16 B", dict(K=96, A=2), every(UNSUPPORTED)),
]


def check(lib, p, rows, **where):
    wrong = []
    for what, faults, expected in rows:
        for kind, status in expected.items():
            got = call(lib, p, kind, **where, **faults)
            if got != status:
                wrong.append(f"{kind} {where or ''}: {what}: expected {status}, got {got}")
    assert not wrong, "\n".join(wrong)


def test_single_faults(lib, p):
    check(lib, p, SINGLE)


def test_double_faults_come_in_the_stated_order(lib, p):
    check(lib, p, DOUBLE)


@pytest.mark.parametrize("count", (1, 2, 3))
def test_group_refuses_a_fault_in_any_member(lib, p, count):
    """The grouped entry applies the rules of the 128-row entry to each member: a fault in any one of them refuses the whole
    launch, whichever position it has (the bad-second-member case of test_gemm_refusals among them)."""
    rows = [(what, faults, {"group": expected["group"]}) for what, faults, expected in SINGLE + DOUBLE if "group" in expected]
    for member in range(count):
        check(lib, p, rows, count=count, member=member)


def test_group_count_and_array(lib, p):
    from vpr_amd import _lib
    ok = _lib.GemmProblemC(*problem(p))
    arr = (_lib.GemmProblemC * 4)(ok, ok, ok, ok)
    assert lib.vpr_gemm_nt_group_bf16(None, 1, None) == INVALID
    assert lib.vpr_gemm_nt_group_bf16(arr, 0, None) == INVALID
    assert lib.vpr_gemm_nt_group_bf16(arr, 4, None) == INVALID
    assert lib.vpr_gemm_nt_group_bf16(arr, -1, None) == INVALID
    # count out of range + a bad member: the count is reported (the members are not looked at)
    bad = _lib.GemmProblemC(*problem(p, K=96))
    assert lib.vpr_gemm_nt_group_bf16((_lib.GemmProblemC * 4)(bad, bad, bad, bad), 4, None) == INVALID
    assert lib.vpr_gemm_nt_group_bf16(None, 0, None) == INVALID


def test_group_reports_the_first_bad_member(lib, p):
    """Two members with different faults: the header gives no order between members; the library walks them in order and
    answers for the first bad one (its answer before the restructuring)."""
    from vpr_amd import _lib
    shape = _lib.GemmProblemC(*problem(p, K=96))                    # UNSUPPORTED on its own
    null = _lib.GemmProblemC(*problem(p, null=("A",)))              # INVALID_ARG on its own
    ok = _lib.GemmProblemC(*problem(p))
    assert lib.vpr_gemm_nt_group_bf16((_lib.GemmProblemC * 2)(shape, null), 2, None) == UNSUPPORTED
    assert lib.vpr_gemm_nt_group_bf16((_lib.GemmProblemC * 2)(null, shape), 2, None) == INVALID
    assert lib.vpr_gemm_nt_group_bf16((_lib.GemmProblemC * 3)(ok, shape, null), 3, None) == UNSUPPORTED
    assert lib.vpr_gemm_nt_group_bf16((_lib.GemmProblemC * 3)(ok, null, shape), 3, None) == INVALID


def test_the_table_covers_every_entry():
    rows = SINGLE + DOUBLE
    assert all(set(expected) <= set(KINDS) for _, _, expected in rows)
    for kind in KINDS:
        statuses = {expected[kind] for _, _, expected in rows if kind in expected}
        assert statuses == {INVALID, UNSUPPORTED}
    assert sum(1 for _, _, expected in SINGLE if set(expected) == {"256"}) == 4
