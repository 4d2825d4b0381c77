"""Backbone LayerNorm kernels (layernorm_bf16, add_layernorm_bf16, bias_layernorm_bf16 and the fused
bias_layernorm_cls_linear_bf16) against the f64 layer_norm of the same bf16 values (plus the f32 pre-bias, added
exactly) on rows that break naive statistics, at every chunk count NCH = ceil(C / 512) and ragged C.

Bound per element (oracle/layernorm.py, shared with the backbone stage tests): |y - ref| <= 2^-8 |ref| + δ, one bf16
rounding of the exact value plus the f32 slack δ of the kernel's two-pass statistics.
"""
import pytest
import torch

from oracle.layernorm import ref_and_bound as _ref_and_bound

pytestmark = pytest.mark.gpu

EPS = 1e-6
C_SWEEP = (8, 64, 504, 520, 1024, 1032, 1536, 1544, 2048)   # NCH 1, 1, 1, 2, 2, 3, 3, 4, 4; ragged chunk counts
M_SWEEP = (1, 3, 5, 4097)
KINDS = ("unit", "constant", "offset300", "massive", "near_eps")


def _rows(kind, M, C, g, scale=1.0):
    """f32 rows of one kind (before the bf16 rounding of the caller)."""
    if kind == "unit":
        return torch.randn(M, C, generator=g) * scale
    if kind == "constant":                              # var = 0: the output is beta exactly
        return (torch.randn(M, 1, generator=g) * 20 * scale).expand(M, C).clone()
    if kind == "offset300":                             # |mean| / sigma = 300: catastrophic for E[x^2] - E[x]^2
        return 300 * scale + torch.randn(M, C, generator=g) * scale
    if kind == "massive":                               # two "massive activation" channels in a unit row
        x = torch.randn(M, C, generator=g) * scale
        x[:, 0] = 1000 * scale
        x[:, C // 2 + 1] = -1000 * scale
        return x
    if kind == "near_eps":                              # var ~ eps
        return torch.randn(M, C, generator=g) * 1e-3 * scale
    raise ValueError(kind)


def _params(C, pdtype, g):
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(pdtype)
    beta = (0.1 * torch.randn(C, generator=g)).to(pdtype)
    return gamma, beta


def _check(y, ref, bound, what):
    err = (y.cpu().double() - ref).abs()
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", C_SWEEP)
def test_layernorm_forms_at_edges(dev, C, kind):
    from vpr_amd import ops
    for M in M_SWEEP:
        for pdtype in (torch.bfloat16, torch.float32):
            g = torch.Generator().manual_seed(C * 31 + M)
            x = _rows(kind, M, C, g).to(torch.bfloat16)
            res = _rows(kind, M, C, g, scale=0.5).to(torch.bfloat16)
            pb = _rows("unit", 1, C, g, scale=1e-3 if kind == "near_eps" else 0.5)[0]
            gamma, beta = _params(C, pdtype, g)
            gd, bd = gamma.to(dev), beta.to(dev)
            what = f"C={C} M={M} {kind} {pdtype}"

            y = ops.layernorm_bf16(x.to(dev), gd, bd, EPS)
            ref, bound = _ref_and_bound(x, gamma, beta)
            _check(y, ref, bound, "plain " + what)

            s, y_add = ops.add_layernorm_bf16(x.to(dev), res.to(dev), gd, bd, EPS)
            s_ref = (x.float() + res.float()).to(torch.bfloat16)                      # one RNE rounding of the sum
            assert torch.equal(s.cpu(), s_ref), "add " + what
            ref_add, bound_add = _ref_and_bound(s_ref, gamma, beta)
            _check(y_add, ref_add, bound_add, "add " + what)

            y_b = ops.bias_layernorm_bf16(x.to(dev), pb.to(dev), gd, bd, EPS)
            ref_b, bound_b = _ref_and_bound(x.double() + pb.double(), gamma, beta)
            _check(y_b, ref_b, bound_b, "bias " + what)

            if kind == "constant":
                exact = beta.to(torch.bfloat16).expand(M, C)
                assert torch.equal(y.cpu(), exact), "plain " + what
                assert torch.equal(y_add.cpu(), exact), "add " + what


@pytest.mark.parametrize("C", C_SWEEP)
def test_layernorm_two_rows_per_wave_bit_identical(dev, tune, C):
    """VPR_LN_ROWS=2 (two rows per wave, used for C <= 1024) == the default, with odd M (a clamped last row)."""
    from vpr_amd import ops
    g = torch.Generator().manual_seed(C)
    for M in (1, 5, 4097):
        x = torch.cat([_rows(k, M, C, g) for k in KINDS]).to(torch.bfloat16).to(dev)   # 5 M rows: odd
        res = torch.randn(x.shape, generator=g).to(torch.bfloat16).to(dev)
        pb = torch.randn(C, generator=g).to(dev)
        gamma, beta = (t.to(dev) for t in _params(C, torch.bfloat16, g))
        runs = []
        for rows in (None, 2):
            tune("VPR_LN_ROWS", rows)
            runs.append((ops.layernorm_bf16(x, gamma, beta, EPS), *ops.add_layernorm_bf16(x, res, gamma, beta, EPS),
                         ops.bias_layernorm_bf16(x, pb, gamma, beta, EPS)))
        for a, b in zip(*runs):
            assert torch.equal(a, b), f"C={C} M={M}"


@pytest.mark.parametrize("C", (8, 520, 1544, 2048))
def test_layernorm_forms_share_one_row_pass(dev, C):
    """The three entries and both parameter types are one row pass behind different front ends: a zero pre-bias, a zero
    residual and f32 copies of bf16 gamma / beta each give the bits of the plain bf16-parameter call (the rows hold no
    negative zero, so adding +0.0 changes no value)."""
    from vpr_amd import ops
    g = torch.Generator().manual_seed(7000 + C)
    for M in (1, 5):
        x = torch.cat([_rows(k, M, C, g) for k in KINDS]).to(torch.bfloat16).to(dev)
        gamma, beta = (t.to(dev) for t in _params(C, torch.bfloat16, g))
        y = ops.layernorm_bf16(x, gamma, beta, EPS)
        what = f"C={C} M={M}"
        assert torch.equal(ops.bias_layernorm_bf16(x, torch.zeros(C, device=dev), gamma, beta, EPS), y), "bias " + what
        s, y_add = ops.add_layernorm_bf16(x, torch.zeros_like(x), gamma, beta, EPS)
        assert torch.equal(s, x), "add " + what
        assert torch.equal(y_add, y), "add " + what
        assert torch.equal(ops.layernorm_bf16(x, gamma.float(), beta.float(), EPS), y), "f32 parameters " + what


def test_layernorm_refusals(dev):
    """C % 8, C > 2048 and misaligned pointers are refused; M = 0 is a no-op."""
    from vpr_amd import ops
    g32 = torch.ones(2056, device=dev)
    for C in (12, 2056):
        x = torch.zeros(3, C, dtype=torch.bfloat16, device=dev)
        with pytest.raises(RuntimeError):
            ops.layernorm_bf16(x, g32[:C], g32[:C], EPS)
        with pytest.raises(RuntimeError):
            ops.add_layernorm_bf16(x, x, g32[:C], g32[:C], EPS)
        with pytest.raises(RuntimeError):
            ops.bias_layernorm_bf16(x, g32[:C], g32[:C], g32[:C], EPS)
    C = 64
    base = torch.zeros(3 * C + 8, dtype=torch.bfloat16, device=dev)
    x_mis = base[1:1 + 3 * C].view(3, C)                                  # 2 bytes off a 16-byte boundary
    x_ok = base[8:8 + 3 * C].view(3, C)
    p = torch.ones(C, device=dev)
    with pytest.raises(RuntimeError):
        ops.layernorm_bf16(x_mis, p, p, EPS)
    with pytest.raises(RuntimeError):
        ops.add_layernorm_bf16(x_ok, x_mis, p, p, EPS)
    with pytest.raises(RuntimeError):
        ops.bias_layernorm_bf16(x_mis, p, p, p, EPS)
    pb_mis = torch.zeros(C + 1, device=dev)[1:]                          # 4 bytes off
    with pytest.raises(RuntimeError):
        ops.bias_layernorm_bf16(x_ok, pb_mis, p, p, EPS)
    from vpr_amd import _lib
    y = torch.full((3, C), 7.0, dtype=torch.bfloat16, device=dev)                # M = 0 on real buffers: status 0, no write
    assert _lib.lib().vpr_layernorm_bf16(ops._ptr(x_ok), ops._ptr(p), ops._ptr(p), 0, EPS, ops._ptr(y), 0, C, ops._stream()) == 0
    assert _lib.lib().vpr_add_layernorm_bf16(ops._ptr(x_ok), ops._ptr(x_ok), ops._ptr(y), ops._ptr(p), ops._ptr(p), 0, EPS,
                                             ops._ptr(y), 0, C, ops._stream()) == 0
    assert _lib.lib().vpr_bias_layernorm_bf16(ops._ptr(x_ok), ops._ptr(p), ops._ptr(p), ops._ptr(p), 0, EPS, ops._ptr(y),
                                              0, C, ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    empty = torch.zeros(0, C, dtype=torch.bfloat16, device=dev)
    assert ops.layernorm_bf16(empty, p, p, EPS).shape == (0, C)
    s, y = ops.add_layernorm_bf16(empty, empty, p, p, EPS)
    assert s.shape == y.shape == (0, C)
    assert ops.bias_layernorm_bf16(empty, p, p, p, EPS).shape == (0, C)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,N,gelu", [(64, 48, False), (1024, 3072, True), (1536, 96, False), (2048, 64, True)])
def test_bias_layernorm_cls_linear_at_edges(dev, C, N, gelu, kind):
    """The fused launch on edge rows: == vpr_bias_layernorm_bf16 on all rows (bit-exact), and the cls rows' linear
    within the tolerance of test_heads_gpu.test_bias_layernorm_cls_linear (it merges 16-column partial statistics
    and subtracts mean · colsum, both of which the edge rows stress)."""
    from vpr_amd import ops
    g = torch.Generator().manual_seed(C + N)
    M, n_cls = 67, 5
    x = _rows(kind, M, C, g).to(torch.bfloat16).to(dev)
    pb = _rows("unit", 1, C, g, scale=1e-3 if kind == "near_eps" else 0.5)[0].to(dev)
    gamma, beta = (t.to(dev) for t in _params(C, torch.bfloat16, g))
    w = (torch.randn(N, C, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    lb = torch.randn(N, generator=g).to(torch.bfloat16).to(dev)
    row0 = M - n_cls
    # the statistics partials of the cls rows, from a skinny accumulate that adds exactly 0 (the rows stay edge rows)
    prev_in = torch.randn(n_cls, 64, generator=g).to(torch.bfloat16).to(dev)
    prev_w = torch.zeros(C, 64, dtype=torch.bfloat16, device=dev)
    x_before = x.clone()
    rs = torch.empty((C // 16, n_cls, 2), dtype=torch.float32, device=dev)
    ops.skinny_linear_bf16(prev_in, prev_w, None, x[row0:], 2, pb, rs)
    assert torch.equal(x, x_before)
    out = torch.full((n_cls, N), 7.0, dtype=torch.bfloat16, device=dev)
    consts = ops.ClsLinearConsts.build(w, lb, gamma, beta, pb)
    y = ops.bias_layernorm_cls_linear_bf16(x, pb, gamma, beta, EPS, row0, rs, consts, out, gelu=gelu)
    y_ref = ops.bias_layernorm_bf16(x, pb, gamma, beta, EPS)
    assert torch.equal(y, y_ref)
    v = x[row0:].double().cpu() + pb.double().cpu()
    ln = torch.nn.functional.layer_norm(v, (C,), gamma.double().cpu(), beta.double().cpu(), EPS)
    acc = ln @ w.double().cpu().T + lb.double().cpu()
    ref = torch.nn.functional.gelu(acc, approximate="tanh") if gelu else acc
    err = (out.cpu().double() - ref).abs().max().item()
    unfused = y_ref[row0:].double().cpu() @ w.double().cpu().T + lb.double().cpu()
    unfused = torch.nn.functional.gelu(unfused, approximate="tanh") if gelu else unfused
    err_unfused = (unfused.to(torch.bfloat16).double() - ref).abs().max().item()
    assert torch.isfinite(out).all()
    assert err < max(2.0 * err_unfused, 8e-3 * max(1.0, ref.abs().max().item())), (kind, err, err_unfused)
