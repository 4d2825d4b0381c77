"""CPU: every refusal of every SALAD entry point of the C ABI, as one table — twelve entries crossed with single faults and
with the double faults whose order matters.  Dummy non-null pointers, never dereferenced: each status below is decided before
a launch (without a device a launch would come back as VPR_ERR_LAUNCH, and the kernels would fault on these pointers).

Expected values are literals.  They follow the order the headers state (include/vpr_amd.h, vpr_amd_salad_stages.h,
vpr_amd_salad_anyres.h): INVALID_ARG for nulls and non-positive sizes, then UNSUPPORTED for the shape domain, then WORKSPACE;
the any-n entries give INVALID_ARG for sinkhorn_iters < 1 ahead of everything and UNSUPPORTED for a misaligned operand ahead
of WORKSPACE.  Where the headers are silent the value is what the library answered before the host side was restructured,
and the row says so."""
import ctypes

import pytest

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
M, L, T, HID = 64, 128, 256, 512
BIG = 1 << 42

BF16_RUNS = ("aggregate", "aggregate_split", "aggregate_train", "aggregate_n")       # whole aggregation, bf16 tokens
F32_RUNS = ("aggregate_f32", "aggregate_f32_n")
RUNS = BF16_RUNS + F32_RUNS
STAGES = ("stage_token", "stage_mlps", "stage_aggregate", "stage_outputs")
SINKHORNS = ("sinkhorn_aggregate", "sinkhorn_aggregate_n")
ENTRIES = RUNS + STAGES + SINKHORNS
ANY_N = ("aggregate_n", "aggregate_f32_n", "sinkhorn_aggregate_n")                   # 64 < n <= 576; the others n == 256
WITH_WEIGHTS = RUNS + ("stage_token", "stage_mlps")
WITH_WORKSPACE = RUNS + STAGES
WITH_C = RUNS + STAGES
WITH_ITERS = RUNS + ("stage_aggregate",) + SINKHORNS
WITH_OUT = WITH_ITERS
WITH_PATCH = RUNS + ("stage_mlps",)
WITH_CLS = ("aggregate_split", "aggregate_train", "aggregate_n") + F32_RUNS + ("stage_token",)
WITH_PATCH_STRIDE = ("aggregate_train", "aggregate_n", "stage_mlps") + F32_RUNS
WITH_CLS_STRIDE = ("aggregate_train", "aggregate_n", "stage_token") + F32_RUNS


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


def call(lib, p, entry, B=2, n=None, C=128, m=M, l=L, t=T, hidden=HID, iters=3, null=(), short=False, patch_off=0,
         patch_stride_off=0, cls_stride_off=0):
    """One call of `entry` with every argument sound except the faults asked for.  null: names among patch, cls, out, ws, w,
    w0 .. w9 (a member of the weights), scores, feats, tok, S, F, g, slabs, rows.  short: the workspace one byte short of
    the size call's answer for these very arguments.  Offsets: bytes on the patch pointer, elements on the strides."""
    from vpr_amd import _lib
    n = (529 if entry in ANY_N else 256) if n is None else n
    f32 = entry in F32_RUNS
    arg = lambda name, value=None: None if name in null else (p if value is None else value)
    members = [None if f"w{i}" in null else p.value for i in range(10)]
    w = _lib.SaladWeightsF32C(*members) if f32 else _lib.SaladWeightsC(*members, None, None)
    wref = None if "w" in null else ctypes.byref(w)
    ws_bytes = BIG
    if short:
        need = (lib.vpr_salad_f32_workspace_bytes if f32 else lib.vpr_salad_workspace_bytes)(B, n, C, m, l, t, hidden)
        ws_bytes = max(need - 1, 0)
    patch = arg("patch", ctypes.c_void_p(p.value + patch_off))
    dims = (m, l, t, hidden)
    tail = (arg("out"), None, arg("ws"), ws_bytes, None)
    if entry == "aggregate":
        return lib.vpr_salad_aggregate(patch, B, n + 1, C, wref, 1.0, *dims, iters, *tail)
    if entry == "aggregate_split":
        return lib.vpr_salad_aggregate_split(patch, arg("cls"), B, n, C, wref, 1.0, *dims, iters, *tail)
    strided = (patch, n * C + patch_stride_off, arg("cls"), C + cls_stride_off, B, n, C, wref)
    if entry == "aggregate_train":
        return lib.vpr_salad_aggregate_train(*strided, 1.0, *dims, iters, 0.3, 7, 0, 0, arg("out"), None, None, arg("ws"), ws_bytes, None)
    if entry in ("aggregate_n", "aggregate_f32", "aggregate_f32_n"):
        return getattr(lib, "vpr_salad_" + entry)(*strided, 1.0, *dims, iters, *tail)
    if entry == "stage_token":
        return lib.vpr_salad_stage_token(arg("cls"), C + cls_stride_off, B, n, C, wref, *dims, arg("ws"), ws_bytes, None)
    if entry == "stage_mlps":
        return lib.vpr_salad_stage_mlps(patch, n * C + patch_stride_off, B, n, C, wref, *dims, arg("ws"), ws_bytes, None)
    if entry == "stage_aggregate":
        return lib.vpr_salad_stage_aggregate(B, n, C, 1.0, *dims, iters, *tail)
    if entry == "stage_outputs":
        S, F, g, H = (ctypes.c_void_p(0) for _ in range(4))
        slabs, rows = ctypes.c_int(0), ctypes.c_longlong(0)
        ref = lambda name, v: None if name in null else ctypes.byref(v)
        return lib.vpr_salad_stage_outputs(arg("ws"), ws_bytes, B, n, C, *dims, ref("S", S), ref("F", F), ref("g", g), ctypes.byref(H),
                                           ref("slabs", slabs), ref("rows", rows))
    assert entry in SINKHORNS
    return getattr(lib, "vpr_salad_" + entry)(arg("scores"), arg("feats"), arg("tok"), B, n, m, l, t, 1.0, iters, arg("out"), None, None)


def every(entries, status, **other):
    """{entry: status} over `entries`, with the exceptions given by name."""
    return {**{e: status for e in entries}, **other}


OFF_N = dict(fixed=(255, 257, 529), any_n=(1, 64, 577, 1369))          # outside n == 256 / outside 64 < n <= 576

# (what, keyword faults, {entry: expected status}); an entry that does not expose the faulted argument is not in the dict
SINGLE = [
    ("null patch", dict(null=("patch",)), every(WITH_PATCH, INVALID)),
    ("null cls", dict(null=("cls",)), every(WITH_CLS, INVALID)),
    ("null out_f32", dict(null=("out",)), every(WITH_OUT, INVALID)),
    ("null workspace", dict(null=("ws",)), every(WITH_WORKSPACE, INVALID)),
    ("null weights", dict(null=("w",)), every(WITH_WEIGHTS, INVALID)),
    *[(f"null weight member {i}", dict(null=(f"w{i}",)), every(WITH_WEIGHTS, INVALID)) for i in range(10)],
    *[(f"null {name}", dict(null=(name,)), every(SINKHORNS, INVALID)) for name in ("scores", "feats", "tok")],
    *[(f"null {name}", dict(null=(name,)), {"stage_outputs": INVALID}) for name in ("S", "F", "g", "slabs", "rows")],
    ("B = 0", dict(B=0), every(ENTRIES, INVALID)),
    ("B < 0", dict(B=-2), every(ENTRIES, INVALID)),
    # n < 1: vpr_amd.h says nothing about it for vpr_salad_sinkhorn_aggregate, which reports it as a token count off 256
    # (the answer before the restructuring); every other entry calls it an invalid argument
    ("n = 0", dict(n=0), every(ENTRIES, INVALID, sinkhorn_aggregate=UNSUPPORTED)),
    ("n < 0", dict(n=-1), every(ENTRIES, INVALID, sinkhorn_aggregate=UNSUPPORTED)),
    ("C = 0", dict(C=0), every(WITH_C, INVALID)),
    *[(f"m, l or t off: {kw}", kw, every(ENTRIES, UNSUPPORTED)) for kw in (dict(m=32), dict(m=128), dict(l=64), dict(t=128))],
    ("C % 64", dict(C=96), every(WITH_C, UNSUPPORTED)),
    ("hidden % 64", dict(hidden=500), every(WITH_C, UNSUPPORTED)),
    ("workspace one byte short", dict(short=True), every(WITH_WORKSPACE, WORKSPACE)),
    ("workspace one byte short, other shape", dict(short=True, B=3, C=1024), every(WITH_WORKSPACE, WORKSPACE)),
    # a stage that reads no sinkhorn_iters cannot refuse it; the whole-aggregation entries of vpr_amd.h are in LAUNCHED_BEFORE
    ("iters < 1", dict(iters=0), every(ANY_N + ("stage_aggregate", "sinkhorn_aggregate"), INVALID)),
    ("iters < 0", dict(iters=-3), every(ANY_N + ("stage_aggregate", "sinkhorn_aggregate"), INVALID)),
    # misaligned operands (bf16: 16-byte pointers, strides % 8; f32: 16-byte pointers, strides % 4); aggregate_split is in
    # LAUNCHED_BEFORE.  vpr_salad_aggregate's one pointer is its cls pointer too.
    ("patch pointer + 2 bytes", dict(patch_off=2), every(("aggregate", "aggregate_train", "aggregate_n", "stage_mlps") + F32_RUNS, UNSUPPORTED)),
    ("patch stride + 4", dict(patch_stride_off=4), every(("aggregate_train", "aggregate_n", "stage_mlps"), UNSUPPORTED)),
    ("patch stride + 2", dict(patch_stride_off=2), every(WITH_PATCH_STRIDE, UNSUPPORTED)),
    ("cls stride + 4", dict(cls_stride_off=4), every(("aggregate_train", "aggregate_n", "stage_token"), UNSUPPORTED)),
    ("cls stride + 2", dict(cls_stride_off=2), every(WITH_CLS_STRIDE, UNSUPPORTED)),
    ("cls stride + 4 at n = 256", dict(n=256, cls_stride_off=4), {"aggregate_n": UNSUPPORTED}),
]

DOUBLE = [
    # shape outside the domain + short workspace: the shape is reported
    ("C % 64 + short workspace", dict(C=96, short=True), every(WITH_WORKSPACE, UNSUPPORTED)),
    ("m off + short workspace", dict(m=32, short=True), every(WITH_WORKSPACE, UNSUPPORTED)),
    # misaligned + short workspace.  The any-n header puts alignment in its domain, ahead of WORKSPACE, and the f32 forms
    # always did; the bf16 entries of vpr_amd.h size the workspace first and leave strides to the stages (their answer before
    # the restructuring; the header gives no order).  vpr_salad_aggregate_n at n == 256 is vpr_salad_aggregate_split's
    # chain and answered like it: kept.
    ("patch stride + 2 + short workspace", dict(patch_stride_off=2, short=True),
     {"aggregate_n": UNSUPPORTED, "aggregate_f32_n": UNSUPPORTED, "aggregate_f32": UNSUPPORTED,
      "aggregate_train": WORKSPACE, "stage_mlps": WORKSPACE}),
    ("cls stride + 2 + short workspace", dict(cls_stride_off=2, short=True),
     {"aggregate_n": UNSUPPORTED, "aggregate_f32_n": UNSUPPORTED, "aggregate_f32": UNSUPPORTED,
      "aggregate_train": WORKSPACE, "stage_token": WORKSPACE}),
    ("patch pointer + 2 bytes + short workspace", dict(patch_off=2, short=True),
     {"aggregate_n": UNSUPPORTED, "aggregate_f32_n": UNSUPPORTED, "aggregate_f32": UNSUPPORTED,
      "aggregate": WORKSPACE, "aggregate_split": WORKSPACE, "aggregate_train": WORKSPACE, "stage_mlps": WORKSPACE}),
    ("patch stride + 4 + short workspace at n = 256", dict(n=256, patch_stride_off=4, short=True), {"aggregate_n": WORKSPACE}),
    ("patch pointer + 2 bytes + short workspace at n = 256", dict(n=256, patch_off=2, short=True), {"aggregate_n": WORKSPACE}),
    # iters < 1 + short workspace: the any-n entries report iters ahead of everything, the older ones after WORKSPACE
    ("iters < 1 + short workspace", dict(iters=0, short=True),
     every(("aggregate", "aggregate_split", "aggregate_train", "aggregate_f32", "stage_aggregate"), WORKSPACE,
           aggregate_n=INVALID, aggregate_f32_n=INVALID)),
    # null weight member + shape outside the domain: the null is reported
    ("null weight member + C % 64", dict(null=("w4",), C=96), every(WITH_WEIGHTS, INVALID)),
    ("null weight member + m off", dict(null=("w9",), m=32), every(WITH_WEIGHTS, INVALID)),
]

# Refusals that the library used to reach only after stage T (or the whole f32 chain) had been enqueued, so that without a
# device it answered VPR_ERR_LAUNCH here: sinkhorn_iters < 1 on the whole-aggregation entries of vpr_amd.h (decided inside
# the stage-A launcher), a misaligned patch pointer of vpr_salad_aggregate_split and a misaligned patch operand of
# vpr_salad_aggregate_n at n == 256 (decided by stage M, after stage T).  With a device they were these statuses already
# (tests/test_salad_anyres_gpu.py shows what the refused calls wrote); now nothing is launched and no device is needed.
LAUNCHED_BEFORE = [
    ("iters < 1", dict(iters=0), every(("aggregate", "aggregate_split", "aggregate_train", "aggregate_f32"), INVALID)),
    ("patch pointer + 2 bytes", dict(patch_off=2), {"aggregate_split": UNSUPPORTED}),
    ("patch stride + 4 at n = 256", dict(n=256, patch_stride_off=4), {"aggregate_n": UNSUPPORTED}),
    ("patch pointer + 2 bytes at n = 256", dict(n=256, patch_off=2), {"aggregate_n": UNSUPPORTED}),
]


def check(lib, p, rows):
    wrong = []
    for what, faults, expected in rows:
        for entry, status in expected.items():
            got = call(lib, p, entry, **faults)
            if got != status:
                wrong.append(f"{entry}: {what}: expected {status}, got {got}")
    assert not wrong, "\n".join(wrong)


def test_single_faults(lib, p):
    check(lib, p, SINGLE)


def test_n_outside_the_domain(lib, p):
    """n == 256 for every entry of vpr_amd.h and for the stage calls, 64 < n <= 576 for the any-n entries — alone, with a
    short workspace (the shape is reported), and with sinkhorn_iters < 1: INVALID_ARG from the any-n entries (iters ahead of
    everything) and from vpr_salad_sinkhorn_aggregate (silent header; its answer before the restructuring), UNSUPPORTED
    from the older entries, which report iters last."""
    rows = []
    for entry in ENTRIES:
        for n in OFF_N["any_n" if entry in ANY_N else "fixed"]:
            rows.append((f"n = {n}", dict(n=n), {entry: UNSUPPORTED}))
            if entry in WITH_WORKSPACE:
                rows.append((f"n = {n} + short workspace", dict(n=n, short=True), {entry: UNSUPPORTED}))
            if entry in WITH_ITERS:
                iters_first = entry in ANY_N or entry == "sinkhorn_aggregate"
                rows.append((f"n = {n} + iters < 1", dict(n=n, iters=0), {entry: INVALID if iters_first else UNSUPPORTED}))
    check(lib, p, rows)


def test_double_faults_come_in_the_stated_order(lib, p):
    check(lib, p, DOUBLE)


def test_refusals_that_used_to_follow_a_launch(lib, p):
    check(lib, p, LAUNCHED_BEFORE)


def test_the_table_covers_every_entry_and_every_exposed_argument():
    rows = SINGLE + DOUBLE + LAUNCHED_BEFORE
    assert set().union(*(set(expected) for _, _, expected in rows)) == set(ENTRIES) and len(ENTRIES) == 12
    covered = lambda key: set().union(*(set(expected) for _, faults, expected in rows if key in faults))
    assert covered("patch_off") == set(WITH_PATCH) and covered("patch_stride_off") == set(WITH_PATCH_STRIDE)
    assert covered("cls_stride_off") == set(WITH_CLS_STRIDE) and covered("iters") >= set(WITH_ITERS)
    assert covered("short") == set(WITH_WORKSPACE)
