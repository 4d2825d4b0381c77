"""MFMA GEMMs (vpr_gemm_nt_bf16, vpr_gemm256_nt_bf16 and the grouped kernel behind vpr_gemm_nt_group_bf16) against f64
at the shapes, strides and layouts where tiled kernels go wrong: ragged M / N / K-tile counts, the N <= 64 single
column-tile form, padded leading dimensions (padding filled with NaN), row-group addressing with NaN gaps between the
groups, outputs into slices of a sentinel-filled buffer on both gemm256 store paths, the SALAD shapes, and refusals.

Two operand forms per case (oracle/gemm.py):
  exact   small-integer operands on which f32 accumulation is exact in any order: every kernel must return the f64
          value itself (f32 out) or its round-to-nearest-even bf16 — bit for bit;
  random  trained-layer-scale bf16 operands: |y - f64| within the per-element bound K u S + 2 u (|s| + 2|b|)
          (+ half a bf16 spacing for bf16 out).
The f64 references run on the CPU; shapes too large for that are checked on sampled rows.
"""
import ctypes
import functools

import pytest
import torch

from oracle import gemm as og

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
KINDS = ("nt", "256", "group")


def _nan_store(mat, ld):
    """[rows, ld] bf16 storage holding `mat` in its first K columns and NaN in the padding."""
    st = torch.full((mat.shape[0], ld), float("nan"), dtype=torch.bfloat16)
    st[:, :mat.shape[1]] = mat
    return st


def _sentinel_out(M, N, out_bf16, wide, dev):
    """An [M, N] slice (rows 2.., 16 bytes into the row) of a sentinel-filled buffer whose row stride is a multiple
    of 4 elements (gemm256's requirement) and, for bf16, either a multiple of 16 bytes (`wide`: whole-row 16-byte
    stores) or not (the scalar ragged-chunk path)."""
    dtype = torch.bfloat16 if out_bf16 else torch.float32
    col0 = 8 if out_bf16 else 4
    ldc = (col0 + N + 1 + 7) // 8 * 8
    if out_bf16 and not wide:
        ldc += 4
    buf = torch.full((M + 4, ldc), SENTINEL, dtype=dtype, device=dev)
    out = buf[2:2 + M, col0:col0 + N]
    assert out.data_ptr() % 16 == 0 and ((out.stride(0) * out.element_size()) % 16 == 0) == (wide or not out_bf16)
    return out, buf, (slice(2, 2 + M), slice(col0, col0 + N))


def _outside_untouched(buf, region, what):
    host = buf.to("cpu", copy=True)
    expect = torch.full_like(host, SENTINEL)
    host[region] = SENTINEL
    assert torch.equal(host, expect), f"{what}: wrote outside its [M, N] block"


def _launch(kind, dev_args, out, **kw):
    from vpr_amd import ops
    a, w, b, relu = dev_args
    if kind == "group":
        ops.gemm_nt_group_bf16([dict(a=a, w=w, bias=b, relu=relu, out=out, **kw)])
    else:
        ops.gemm_nt_bf16(a, w, b, relu, tile256=(kind == "256"), out=out, **kw)


def _compare(got, y, s, S, K, bias, out_bf16, exact, what):
    got = got.cpu().double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output (padding or a group gap was read)"
    if exact:
        want = og.exact_value(y, out_bf16)
        bad = (got != want)
        assert not bad.any(), (f"{what}: {int(bad.sum())} elements differ from the exactly rounded value, first at "
                               f"{tuple(bad.nonzero()[0].tolist())}: got {got[bad][0].item()!r}, want {want[bad][0].item()!r}")
    else:
        bound = og.gemm_bound(y, s, S, K, bias, out_bf16)
        ratio = ((got - y).abs() / bound).max().item()
        assert ratio <= 1.0, f"{what}: worst |err| / bound = {ratio:.3f}"


@functools.lru_cache(maxsize=8)
def _case(M, N, K, exact, with_bias, seed):
    a, w, b = (og.exact_operands if exact else og.random_operands)(M, N, K, seed, with_bias)
    return a, w, b


def _run_case(dev, kind, M, N, K, *, exact, with_bias, relu, out_bf16, pad_a, pad_w, wide, seed):
    a, w, b = _case(M, N, K, exact, with_bias, seed)
    a_st, w_st = _nan_store(a, K + pad_a), _nan_store(w, K + pad_w)
    dev_args = (a_st.to(dev)[:, :K], w_st.to(dev)[:, :K], None if b is None else b.to(dev), relu)
    out, buf, region = _sentinel_out(M, N, out_bf16, wide, dev)
    _launch(kind, dev_args, out)
    what = (f"{kind} M={M} N={N} K={K} {'exact' if exact else 'random'} bias={b is not None} relu={relu} "
            f"{'bf16' if out_bf16 else 'f32'} lda={K + pad_a} ldw={K + pad_w} ldc={out.stride(0)}")
    y, s, S = og.gemm_ref(a, w, b, relu)
    _compare(out, y, s, S, K, b, out_bf16, exact, what)
    _outside_untouched(buf, region, what)


# Every M, N and K of the sweep appears; K = 64 is one K-step (no gemm256), 128 gemm256's minimum, 192 an odd number
# of K-tiles; N <= 64 takes the single column-tile form of the 128-row kernel.
SHAPES = [
    (1, 516, 1088), (31, 3, 192), (127, 64, 128), (128, 65, 4096), (129, 129, 64), (255, 1, 128),
    (256, 256, 192), (257, 257, 1088), (1000, 63, 192), (1000, 255, 128), (127, 516, 4096), (257, 64, 4096),
    (1000, 516, 1088), (256, 3, 64), (31, 256, 4096),
]


@pytest.mark.parametrize("kind,M,N,K", [(k, *shape) for shape in SHAPES for k in KINDS if k != "256" or shape[2] >= 128])
def test_gemm_shapes(dev, kind, M, N, K):
    i = SHAPES.index((M, N, K))
    for exact in (True, False):
        # the variant rotates over the shapes; lda / ldw padded (NaN) on every other one; both bf16 store paths
        _run_case(dev, kind, M, N, K, exact=exact, with_bias=(i % 3 != 1), relu=(i % 2 == 0), out_bf16=((i + exact) % 2 == 0),
                  pad_a=8 * (i % 3), pad_w=8 * ((i + 1) % 3), wide=(i % 4 < 2), seed=i)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_gemm_variants(dev, kind, with_bias, relu, out_bf16):
    """Every bias / ReLU / output-type combination on a ragged shape, both store paths for bf16."""
    for (M, N, K) in ((300, 260, 256), (129, 65, 192)):
        for exact in (True, False):
            for wide in ((True, False) if out_bf16 else (True,)):
                _run_case(dev, kind, M, N, K, exact=exact, with_bias=with_bias, relu=relu, out_bf16=out_bf16,
                          pad_a=24, pad_w=8, wide=wide, seed=M + N + K + 2 * relu + with_bias)


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_bf16_rounds_ties_to_even(dev, kind):
    """y = W[n, c_r] + b[n] with a one-hot A, W = +-even integers in [258, 510] (exact in bf16: spacing 2 there) and
    b = +-1: every output is an odd integer in [257, 511] in magnitude, i.e. a bf16 tie, which round-to-nearest-even
    resolves to the multiple of 4; truncation (or ties away from zero) would not."""
    M, N, K = 257, 129, 128
    g = torch.Generator().manual_seed(5)
    a = torch.zeros(M, K)
    a[torch.arange(M), torch.arange(M) % K] = 1
    sign = torch.where(torch.rand(N, K, generator=g) < 0.5, -1.0, 1.0)
    w = 2 * torch.randint(129, 256, (N, K), generator=g).double() * sign
    b = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    a, w = a.to(torch.bfloat16), w.to(torch.bfloat16)
    y, s, S = og.gemm_ref(a, w, b)
    want = og.exact_value(y, True)
    assert bool((y.abs() % 2 == 1).all()) and bool((want.abs() % 4 == 0).all())
    assert bool((want.abs() > y.abs()).any()) and bool((want.abs() < y.abs()).any())   # ties resolved both ways
    out, buf, region = _sentinel_out(M, N, True, False, dev)
    _launch(kind, (a.to(dev), w.to(dev), b.to(dev), False), out)
    assert torch.equal(out.cpu().double(), want), f"{kind}: bf16 output not rounded to nearest even"
    _outside_untouched(buf, region, kind)


# ---------------------------------------------------------------------------------------------------------- row groups
def _grouped_store(a, lda, g_rows, g_stride):
    """Flat NaN storage with row r of `a` at (r // g_rows) * g_stride + (r % g_rows) * lda."""
    M, K = a.shape
    groups = (M + g_rows - 1) // g_rows
    flat = torch.full((groups * g_stride + lda,), float("nan"), dtype=torch.bfloat16)
    r = torch.arange(M)
    base = (r // g_rows) * g_stride + (r % g_rows) * lda
    flat[base[:, None] + torch.arange(K)[None, :]] = a
    return flat


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g_rows,M,N,K,lda,gap", [
    (256, 1000, 260, 256, 256, 64),       # SALAD's patch rows (image stride with a gap)
    (257, 1000, 65, 192, 200, 8),         # cls-first token count
    (100, 1000, 129, 128, 136, 24),
    (1, 129, 516, 128, 128, 16),          # a group per row: the stride acts as the row pitch
])
def test_gemm_row_groups(dev, kind, g_rows, M, N, K, lda, gap):
    """Row-group addressing A + (r / a_group_rows) * a_group_stride + (r % a_group_rows) * lda with NaN in the gaps
    between groups and in the lda padding (none of it may reach the output)."""
    g_stride = g_rows * lda + gap
    for exact in (True, False):
        a, w, b = _case(M, N, K, exact, True, g_rows)
        flat = _grouped_store(a, lda, g_rows, g_stride)
        fd = flat.to(dev)
        a_dev = fd[:min(g_rows, M) * lda].view(-1, lda)[:, :K]
        out_bf16 = not exact
        out, buf, region = _sentinel_out(M, N, out_bf16, True, dev)
        _launch(kind, (a_dev, w.to(dev), b.to(dev), True), out, a_group_rows=g_rows, a_group_stride=g_stride, m=M)
        y, s, S = og.gemm_ref(flat, w, b, True, g_rows, g_stride, lda, M)
        what = f"{kind} groups of {g_rows} stride {g_stride} M={M} N={N} K={K} {'exact' if exact else 'random'}"
        _compare(out, y, s, S, K, b, out_bf16, exact, what)
        _outside_untouched(buf, region, what)


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_row_groups_one_hot(dev, kind):
    """A one-hot A under row groups of 257: row r selects column c_r = (7 r) mod K, so C[r, :] must be W[:, c_r]
    exactly — a row read from the wrong place (group or in-group index) shows as a whole wrong row."""
    M, N, K, lda, g_rows = 771, 130, 256, 264, 257
    g_stride = g_rows * lda + 40
    c = (7 * torch.arange(M)) % K
    a = torch.zeros(M, K)
    a[torch.arange(M), c] = 1
    a = a.to(torch.bfloat16)
    w = torch.randint(-256, 257, (N, K), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    flat = _grouped_store(a, lda, g_rows, g_stride)
    fd = flat.to(dev)
    out, buf, region = _sentinel_out(M, N, False, True, dev)
    _launch(kind, (fd[:g_rows * lda].view(-1, lda)[:, :K], w.to(dev), None, False), out,
            a_group_rows=g_rows, a_group_stride=g_stride, m=M)
    got = out.cpu()
    want = w.float().T[c]
    wrong = (got != want).any(1).nonzero().flatten().tolist()
    assert not wrong, f"{kind}: rows {wrong[:8]} picked the wrong A row"
    _outside_untouched(buf, region, kind)


# ------------------------------------------------------------------------------------------------ grouped entry point
GROUP_MEMBERS = [
    # (M, N, K, bias, relu, out_bf16)
    (1000, 516, 192, True, True, True),
    (129, 64, 1088, False, False, False),
    (31, 3, 128, True, False, False),
]


def _group_problem(dev, M, N, K, bias, relu, out_bf16, exact, seed):
    a, w, b = _case(M, N, K, exact, bias, seed)
    a_dev, w_dev = _nan_store(a, K + 8).to(dev)[:, :K], w.to(dev)
    out, buf, region = _sentinel_out(M, N, out_bf16, seed % 2 == 0, dev)
    return dict(a=a_dev, w=w_dev, bias=None if b is None else b.to(dev), relu=relu, out=out), (a, w, b, buf, region)


@pytest.mark.parametrize("variant", [None, 0, 1])
@pytest.mark.parametrize("count", [1, 2, 3])
def test_gemm_group_members(dev, tune, variant, count):
    """1-3 different problems in one launch: each member equals f64 (exact form: bit for bit) and equals the same
    problem launched alone through the grouped entry point, bit for bit; nothing outside any output is written."""
    from vpr_amd import ops
    tune("VPR_GEMM_GROUP_VARIANT", variant)
    for exact in (True, False):
        members = [GROUP_MEMBERS[(i + count) % 3] for i in range(count)]
        probs, refs = zip(*[_group_problem(dev, *m, exact, seed=i) for i, m in enumerate(members)])
        ops.gemm_nt_group_bf16(probs)
        for i, ((M, N, K, bias, relu, out_bf16), p, (a, w, b, buf, region)) in enumerate(zip(members, probs, refs)):
            what = f"variant {variant} member {i}/{count} M={M} N={N} K={K} {'exact' if exact else 'random'}"
            y, s, S = og.gemm_ref(a, w, b, relu)
            _compare(p["out"], y, s, S, K, b, out_bf16, exact, what)
            _outside_untouched(buf, region, what)
            alone, _ = _group_problem(dev, M, N, K, bias, relu, out_bf16, exact, seed=i)
            ops.gemm_nt_group_bf16([alone])
            assert torch.equal(alone["out"], p["out"]), f"{what}: differs from the same problem launched alone"


# ------------------------------------------------------------------------------------------------------- SALAD shapes
def _sampled_rows(M, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor([0, M - 1]), torch.randperm(M, generator=g)[:n - 2]]).sort().values


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_salad_layer1(dev, kind):
    """SALAD layer 1 at B = 64: (16384 x 1024 x 1024) over patch rows in groups of 256 (image stride 257 rows: the
    cls-first hub layout), bias + ReLU, bf16 out; checked on 192 sampled rows."""
    B, n, C, N = 64, 256, 1024, 1024
    M = B * n
    for exact in (True, False):
        tok, w, b = _case(B * (n + 1), N, C, exact, True, 11)
        tok_dev = tok.to(dev)
        a_dev = tok_dev[1:1 + n]                            # patch rows: image b at row b * 257 + 1
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        _launch(kind, (a_dev, w.to(dev), b.to(dev), True), out, a_group_rows=n, a_group_stride=(n + 1) * C, m=M)
        rows = _sampled_rows(M, 192, 1)
        src = (rows // n) * (n + 1) + 1 + rows % n
        y, s, S = og.gemm_ref(tok[src], w, b, True)
        _compare(out.cpu()[rows], y, s, S, C, b, True, exact, f"{kind} SALAD layer 1 {'exact' if exact else 'random'}")


def test_gemm_salad_layer2_pair(dev, tune):
    """SALAD's second layers as one grouped launch: score (16384 x 64) and cluster (16384 x 128) halves of the hidden
    buffer H [16384, 2 * 512] (lda = 1024), K = 512, f32 out; both group variants."""
    from vpr_amd import ops
    M, hidden = 16384, 512
    for variant in (0, 1):
        tune("VPR_GEMM_GROUP_VARIANT", variant)
        for exact in (True, False):
            H, w2, b2 = _case(M, 192, 2 * hidden, exact, True, 12)
            Hd = H.to(dev)
            ws, wc = w2[:64, :hidden].contiguous(), w2[64:, :hidden].contiguous()
            bs, bc = b2[:64].contiguous(), b2[64:].contiguous()
            S_out, F_out = ops.gemm_nt_group_bf16([
                dict(a=Hd[:, :hidden], w=ws.to(dev), bias=bs.to(dev)),
                dict(a=Hd[:, hidden:], w=wc.to(dev), bias=bc.to(dev))])
            rows = _sampled_rows(M, 1024, 2)
            for got, a, w, b, what in ((S_out, H[rows, :hidden], ws, bs, "score"), (F_out, H[rows, hidden:], wc, bc, "cluster")):
                y, s, S = og.gemm_ref(a, w, b)
                _compare(got.cpu()[rows], y, s, S, hidden, b, False, exact, f"variant {variant} layer 2 {what}")


def test_gemm_salad_f32_path_shapes(dev):
    """The GEMMs of the f32-accurate SALAD path (three bf16 planes per operand): layer 1 K = 6 C = 6144 on gemm256,
    f32 out + bias + ReLU; second layers K2 = 6 hidden = 3072 as one grouped launch of three (two halves of one
    buffer, lda = 2 K2, and the token MLP's 4 rows)."""
    from vpr_amd import ops
    rows, C, hidden, B = 1024, 1024, 512, 4
    K1, K2 = 6 * C, 6 * hidden
    a, w, b = og.random_operands(rows, 2 * hidden, K1, 21)
    out = ops.gemm_nt_bf16(a.to(dev), w.to(dev), b.to(dev), True, torch.float32, tile256=True)
    sr = _sampled_rows(rows, 96, 3)
    y, s, S = og.gemm_ref(a[sr], w, b, True)
    _compare(out.cpu()[sr], y, s, S, K1, b, False, False, "f32 path layer 1")
    H2, w2, b2 = og.random_operands(rows, 64 + 128 + 256, 2 * K2, 22)
    ht, _, _ = og.random_operands(B, 1, K2, 23, with_bias=False)
    Hd = H2.to(dev)
    members = [(Hd[:, :K2], H2[:, :K2], w2[:64, :K2], b2[:64]), (Hd[:, K2:], H2[:, K2:], w2[64:192, K2:], b2[64:192]),
               (ht.to(dev), ht, w2[192:, :K2], b2[192:])]
    outs = ops.gemm_nt_group_bf16([dict(a=ad, w=wm.contiguous().to(dev), bias=bm.contiguous().to(dev))
                                   for ad, _, wm, bm in members])
    for i, (got, (_, ah, wm, bm)) in enumerate(zip(outs, members)):
        r = _sampled_rows(ah.shape[0], 96, 4) if ah.shape[0] > 96 else torch.arange(ah.shape[0])
        y, s, S = og.gemm_ref(ah[r], wm, bm)
        _compare(got.cpu()[r], y, s, S, K2, bm, False, False, f"f32 path layer 2 member {i}")


# ---------------------------------------------------------------------------------------------------------- refusals
def _raw(lib, kind, A, lda, W, ldw, bias, C, ldc, out_bf16, M, N, K, groups=(0, 0)):
    args = (ctypes.c_void_p(A), lda, groups[0], groups[1], ctypes.c_void_p(W), ldw, ctypes.c_void_p(bias), 0,
            ctypes.c_void_p(C), ldc, out_bf16, M, N, K)
    if kind == "group":
        from vpr_amd import _lib
        p = _lib.GemmProblemC(*[x.value if isinstance(x, ctypes.c_void_p) else x for x in args])
        return lib.vpr_gemm_nt_group_bf16(ctypes.byref(p), 1, None)
    fn = lib.vpr_gemm256_nt_bf16 if kind == "256" else lib.vpr_gemm_nt_bf16
    return fn(*args, None)


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_refusals(dev, kind):
    """Shape, stride and alignment checks answer before anything launches.  Every call is backed by 4 MB buffers (a
    launch that slipped through would still stay in bounds: M, N <= 64, K, lda, ldw, ldc <= 264), and the output
    buffer must still hold its sentinel afterwards."""
    from vpr_amd import _lib
    lib = _lib.lib()
    bufA = torch.zeros(1 << 21, dtype=torch.bfloat16, device=dev)
    bufW = torch.zeros(1 << 21, dtype=torch.bfloat16, device=dev)
    bufC = torch.full((1 << 20,), SENTINEL, device=dev)
    bias = torch.zeros(1024, device=dev)
    A, W, C, bp = bufA.data_ptr(), bufW.data_ptr(), bufC.data_ptr(), bias.data_ptr()
    UNS, INV = -2, -1
    cases = [
        ("K % 64", UNS, (A, 96, W, 96, bp, C, 64, 0, 64, 64, 96)),
        ("lda < K", UNS, (A, 120, W, 128, bp, C, 64, 0, 64, 64, 128)),
        ("ldw < K", UNS, (A, 128, W, 120, bp, C, 64, 0, 64, 64, 128)),
        ("ldc < N", UNS, (A, 128, W, 128, bp, C, 60, 0, 64, 64, 128)),
        ("lda % 8", UNS, (A, 132, W, 128, bp, C, 64, 0, 64, 64, 128)),
        ("ldw % 8", UNS, (A, 128, W, 260, bp, C, 64, 0, 64, 64, 128)),
        ("A off 16 B", UNS, (A + 2, 128, W, 128, bp, C, 64, 0, 64, 64, 128)),
        ("W off 16 B", UNS, (A, 128, W + 2, 128, bp, C, 64, 0, 64, 64, 128)),
        ("M = 0", INV, (A, 128, W, 128, bp, C, 64, 0, 0, 64, 128)),
        ("N < 0", INV, (A, 128, W, 128, bp, C, 64, 0, 64, -64, 128)),
        ("K = 0", INV, (A, 128, W, 128, bp, C, 64, 0, 64, 64, 0)),
        ("A null", INV, (0, 128, W, 128, bp, C, 64, 0, 64, 64, 128)),
        ("W null", INV, (A, 128, 0, 128, bp, C, 64, 0, 64, 64, 128)),
        ("C null", INV, (A, 128, W, 128, bp, 0, 64, 0, 64, 64, 128)),
    ]
    if kind == "256":
        cases += [
            ("gemm256 K < 128", UNS, (A, 64, W, 64, bp, C, 64, 0, 64, 64, 64)),
            ("gemm256 ldc % 4", UNS, (A, 128, W, 128, bp, C, 66, 0, 64, 64, 128)),
            ("gemm256 C off 16 B", UNS, (A, 128, W, 128, bp, C + 4, 64, 0, 64, 64, 128)),
            ("gemm256 bias off 16 B", UNS, (A, 128, W, 128, bp + 4, C, 64, 0, 64, 64, 128)),
        ]
    for what, want, args in cases:
        assert _raw(lib, kind, *args) == want, f"{kind}: {what} not refused"
    assert _raw(lib, kind, A, 128, W, 128, bp, C, 64, 0, 64, 64, 128, groups=(16, 16 * 128 + 4)) == UNS, \
        f"{kind}: a_group_stride % 8 not refused"
    if kind == "group":
        assert lib.vpr_gemm_nt_group_bf16(None, 1, None) == INV
        ok = _lib.GemmProblemC(A, 128, 0, 0, W, 128, bp, 0, C, 64, 0, 64, 64, 128)
        bad = _lib.GemmProblemC(A, 128, 0, 0, W, 128, bp, 0, C, 64, 0, 64, 64, 96)
        for count in (0, 4):
            arr = (_lib.GemmProblemC * 4)(ok, ok, ok, ok)
            assert lib.vpr_gemm_nt_group_bf16(arr, count, None) == INV, f"count {count} not refused"
        arr = (_lib.GemmProblemC * 2)(ok, bad)
        assert lib.vpr_gemm_nt_group_bf16(arr, 2, None) == UNS, "a bad second member must refuse the whole launch"
    torch.cuda.synchronize()
    assert bool((bufC == SENTINEL).all()), f"{kind}: a refused call wrote its output"


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_bias_at_4_byte_offset(dev, kind):
    """A bias that is 4-byte but not 16-byte aligned: gemm256 reads the bias as float4 and must refuse it; the 128-row
    kernels read it per element and must give the right result."""
    from vpr_amd import ops
    M, N, K = 300, 260, 256
    a, w, b = og.exact_operands(M, N, K, 9)
    bstore = torch.zeros(N + 4)
    bstore[1:1 + N] = b
    bd = bstore.to(dev)[1:1 + N]
    assert bd.data_ptr() % 16 == 4
    if kind == "256":
        with pytest.raises(RuntimeError, match="status -2"):
            ops.gemm_nt_bf16(a.to(dev), w.to(dev), bd, True, torch.float32, tile256=True)
        return
    out, buf, region = _sentinel_out(M, N, False, True, dev)
    _launch(kind, (a.to(dev), w.to(dev), bd, True), out)
    y, s, S = og.gemm_ref(a, w, b, True)
    _compare(out, y, s, S, K, b, False, True, f"{kind} bias at a 4-byte offset")
    _outside_untouched(buf, region, kind)
