"""kNN on real (MFMA) scores away from unit-norm rows, and the paths no other test reaches.

1. Soundness of the certificate on galleries that are NOT L2-normalised: wherever status is 0 or 1 the row is the exact
   top-k bit for bit; with exact_fallback=True every row is.  Each case names the queries that MAY be flagged (status 2);
   the plain model of the select stage (oracle/knn_select.py) on an f32 matmul of the same operands is held to the same
   allowance first, so a kernel cannot pass by flagging everything.
2. The general rescore / order path on e4m3 rows (rows wider than 24 KB: D > 24576).
3. The exhaustive kernel at its row limit (17408 bytes), at widths that do not fill a wave, on ragged N, and one step
   past the limit."""
import functools
import re

import pytest
import torch

from oracle import knn as oknn
from oracle import knn_select as oks

pytestmark = pytest.mark.gpu

B, N, K = 9, 20000, 10
ALL = frozenset(range(B))


def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)


def _spread(D, gen):
    return torch.randn(B, D, generator=gen), _unit(N, D, gen) * (10.0 ** (6 * torch.rand(N, generator=gen) - 3))[:, None]


def _big_row(D, gen):
    g = _unit(N, D, gen)
    g[1234] *= 1e4
    return _unit(B, D, gen), g


def _zero_rows(D, gen):
    g = _unit(N, D, gen)
    g[torch.rand(N, generator=gen) < 0.05] = 0
    return _unit(B, D, gen), g


def _zero_query(D, gen):
    q = _unit(B, D, gen)
    q[4] = 0
    return q, _unit(N, D, gen)


def _negative(D, gen, n=N):
    c = _unit(1, D, gen)
    g = torch.nn.functional.normalize(c + 0.3 * _unit(n, D, gen), dim=1) * (0.5 + 1.5 * torch.rand(n, generator=gen))[:, None]
    return -c + 0.05 * _unit(B, D, gen), g


def _negative_few(D, gen):
    return _negative(D, gen, n=5)


def _duplicates(D, gen):
    g = _unit(N, D, gen)
    q = _unit(B, D, gen)
    g[torch.randperm(N, generator=gen)[:40]] = g[77].clone()
    q[0] = g[77] + 0.01 * q[0]
    return q, g


def _scales(D, gen):
    q = _unit(B, D, gen) * (2.0 ** (40 * torch.rand(B, generator=gen) - 20))[:, None]
    return q, _unit(N, D, gen) * (2.0 ** (40 * torch.rand(N, generator=gen) - 20))[:, None]


# case -> (builder, queries that may come out status 2 (per D where it depends on D), why).  Everything else must be
# certified (0 or 1).
CASES = {
    "norms 1e-3..1e3": (_spread, frozenset(), "the top rows are the long ones, gaps of many eps"),
    "one row 1e4 x": (_big_row, {64: frozenset(), 512: ALL, 1024: ALL},
                      "the bound is 1e4 x every other row: eps = 0.04 |q| at D = 64 (a band of a few rows: widened), 0.34 |q| "
                      "and 0.67 |q| at D = 512 and 1024, above every score of a unit row (the band is the whole gallery)"),
    "zero gallery rows": (_zero_rows, frozenset(), "exact zeros sit far below the top-k"),
    "zero query": (_zero_query, frozenset({4}), "every score of query 4 ties at 0: each chunk list is cut inside the tie"),
    "all scores negative": (_negative, frozenset(), "the certificate has no sign assumption"),
    "negative, N < k": (_negative_few, frozenset(), "nothing is cut"),
    "40 duplicates of the best row": (_duplicates, frozenset({0}), "40 exact ties straddle the top-kp cut: widened, or flagged"),
    "scales 2^-20..2^20": (_scales, frozenset(), "as the spread norms, through the e4m3 scales"),
}
FORMS = [("bf16", 64), ("bf16", 1024), ("e4m3", 512)]


@functools.lru_cache(maxsize=None)
def _problem(case, form, D):
    """-> dict(args for ops.knn_topk[_fp8] on the CPU, oracle answer, norm bound, the model's statuses)."""
    gen = torch.Generator().manual_seed(len(case) * 1000 + D)
    q32, g32 = CASES[case][0](D, gen)
    if form == "e4m3":
        q, qs = oknn.quantize_fp8_rows(q32)
        g, gs = oknn.quantize_fp8_rows(g32)
        ref = oknn.knn_topk_fp8(q, qs, g, gs, K, 7)
        qd = q.view(torch.float8_e4m3fn).double() * qs.double()[:, None]
        gd = g.view(torch.float8_e4m3fn).double() * gs.double()[:, None]
        args = (q, qs, g, gs)
    else:
        q, g = q32.to(torch.bfloat16), g32.to(torch.bfloat16)
        ref = oknn.knn_topk(q, g, K, 7)
        qd, gd = q.double(), g.double()
        args = (q, g)
    bound = float(gd.norm(dim=1).max()) * 1.001
    row_bytes = D if form == "e4m3" else 2 * D
    model = oks.knn_select_model(qd.float() @ gd.float().T, qd, gd, K, bound, 7, row_bytes=row_bytes)
    return dict(args=args, ref=ref, bound=bound, model_status=model[2].tolist())


def _cases():
    return [(c, f, D) for c in CASES for f, D in FORMS if (c != "scales 2^-20..2^20" or f == "e4m3")]


@pytest.mark.parametrize("case,form,D", _cases())
def test_status_0_and_1_are_sound_on_unnormalised_operands(dev, case, form, D):
    """norm_bound = 1.001 x the largest (dequantised) gallery row norm.  Statuses observed on MI355X, the same for bf16
    D = 64, bf16 D = 1024 and e4m3 D = 512 unless noted, and in every case equal to the model's on f32-matmul scores:
      norms 1e-3..1e3, zero gallery rows, all scores negative (N = 20000 and N = 5 < k), scales 2^-20..2^20: all 0;
      one row 1e4 x: [1, 1, 1, 1, 0, 1, 1, 1, 1] at D = 64, all 2 at D = 1024 and at e4m3 D = 512;
      zero query: 2 for the zero query, 0 for the other eight;
      40 duplicates of the best row: 1 for the duplicated query (widened over the tie), 0 for the other eight."""
    from vpr_amd import ops
    p = _problem(case, form, D)
    may_flag = CASES[case][1]
    may_flag = may_flag[D] if isinstance(may_flag, dict) else may_flag
    assert {b for b, s in enumerate(p["model_status"]) if s == 2} <= may_flag, (p["model_status"], CASES[case][2])
    fn = ops.knn_topk_fp8 if form == "e4m3" else ops.knn_topk
    args = tuple(t.to(dev) for t in p["args"])
    v_ref, i_ref = p["ref"]
    nq = v_ref.shape[0]
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    v, i = fn(*args, K, 7, norm_bound=p["bound"], status=status)
    st = status.tolist()
    print(f"\n[kNN soundness] {case:30s} {form} D={D}: status {st} (model {p['model_status']})")
    assert all(s in (0, 1, 2) for s in st)
    assert {b for b, s in enumerate(st) if s == 2} <= may_flag, (st, CASES[case][2])
    ok = [b for b, s in enumerate(st) if s in (0, 1)]
    assert torch.equal(i.cpu()[ok], i_ref[ok]) and torch.equal(v.cpu()[ok].view(torch.int32), v_ref[ok].view(torch.int32))
    v, i = fn(*args, K, 7, norm_bound=p["bound"], status=status, exact_fallback=True)
    assert [3 if s == 2 else s for s in st] == status.tolist()
    assert torch.equal(i.cpu(), i_ref) and torch.equal(v.cpu().view(torch.int32), v_ref.view(torch.int32))


# ------------------------------------------------------------------------------- e4m3 rows wider than the fused kernel
def _fp8_rows(n, d, seed):
    gen = torch.Generator().manual_seed(seed)
    return oknn.quantize_fp8_rows(_unit(n, d, gen))


@pytest.mark.parametrize("D", [24704, 24576])
def test_fp8_rows_at_the_fused_kernels_width_limit(dev, D):
    """D = 24704 e4m3 bytes per row (193 K-steps) exceed the fused kernel's 24 KB: knn_rescore_kernel<true> and
    knn_order_kernel run — the bound alone decides between status 0 and 2 on a full list, and 12 rows < kp are
    status 0 whatever the bound.  D = 24576 is the last width the fused kernel takes: same oracle, same statuses (one
    level-0 list of kp rows: nothing to widen with, and the list is cut above the bar)."""
    from vpr_amd import ops
    assert oks.level_plan(300, 5, D)["fused"] == (D == 24576)
    for Bq, n, seed in ((3, 300, 11), (2, 12, 13)):
        q, qs = _fp8_rows(Bq, D, seed)
        g, gs = _fp8_rows(n, D, seed + 1)
        v_ref, i_ref = oknn.knn_topk_fp8(q, qs, g, gs, 5, 9)
        args = tuple(t.to(dev) for t in (q, qs, g, gs))
        for bound in (1e-9, 1e6):
            status = torch.full((Bq,), -1, dtype=torch.int32, device=dev)
            unc = torch.zeros(1, dtype=torch.int32, device=dev)
            v, i = ops.knn_topk_fp8(*args, 5, 9, norm_bound=bound, status=status, uncertified=unc)
            assert torch.equal(i.cpu(), i_ref) and torch.equal(v.cpu(), v_ref), (n, bound)
            flagged = bound > 1 and n > 16
            assert status.tolist() == [2 if flagged else 0] * Bq and int(unc) == (Bq if flagged else 0), (n, bound)


# ------------------------------------------------------------------------------------------------ exhaustive kernel
def _exhaustive_case(dev, form, Bq, n, D, k, base, seed):
    from vpr_amd import ops
    if form == "e4m3":
        q, qs = _fp8_rows(Bq, D, seed)
        g, gs = _fp8_rows(n, D, seed + 1)
        ref = oknn.knn_topk_fp8(q, qs, g, gs, k, base)
        got = ops.knn_topk_exhaustive(q.to(dev), g.to(dev), k, base, qs.to(dev), gs.to(dev))
    else:
        gen = torch.Generator().manual_seed(seed)
        q, g = _unit(Bq, D, gen).to(torch.bfloat16), _unit(n, D, gen).to(torch.bfloat16)
        ref = oknn.knn_topk(q, g, k, base)
        got = ops.knn_topk_exhaustive(q.to(dev), g.to(dev), k, base)
    assert torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[0].cpu(), ref[0]), (form, Bq, n, D, k)


@pytest.mark.parametrize("form,D", [("bf16", 8704), ("e4m3", 17408),      # rows of exactly 17408 bytes: 17 chunks in every lane
                                    ("bf16", 64), ("bf16", 128), ("e4m3", 128),     # 8 / 16 / 8 chunks for 64 lanes
                                    ("bf16", 1088)])                      # 136 chunks: the third chunk row is partial
def test_exhaustive_kernel_at_its_edges(dev, form, D):
    """knn_exact_scores_kernel against the oracle: N % 4 != 0 on the last workgroup, N < k, one query and several, an
    index base."""
    for j, (Bq, n, k, base) in enumerate([(1, 1, 8, 0), (5, 3, 8, 12345), (1, 5, 5, 0), (5, 1003, 10, 12345)]):
        _exhaustive_case(dev, form, Bq, n, D, k, base, 100 * j + D)


@pytest.mark.parametrize("form,D", [("bf16", 8768), ("e4m3", 17536)])
def test_exhaustive_one_step_past_the_row_limit_is_refused(dev, form, D):
    """Rows of 17536 bytes: VPR_ERR_UNSUPPORTED by name, outputs untouched.  knn_topk(..., exact_fallback=True) with a
    flagged query of such rows raises the same error after the checked search: the caller's status still reads 2 for
    the flagged query (never 3) and what the search certified for the others."""
    from vpr_amd import ops, _lib
    import ctypes
    lib = _lib.lib()
    unsupported = re.escape(lib.vpr_status_string(-2).decode()) + r" \(status -2\)"
    n, k = 300, 5
    gen = torch.Generator().manual_seed(D)
    q32, g32 = _unit(3, D, gen), _unit(n, D, gen)
    q32[1] = 0                                      # every score ties: the one chunk list is cut inside the tie -> status 2
    if form == "e4m3":
        (q, qs), (g, gs) = oknn.quantize_fp8_rows(q32), oknn.quantize_fp8_rows(g32)
        ref = oknn.knn_topk_fp8(q, qs, g, gs, k)
        q, qs, g, gs = (t.to(dev) for t in (q, qs, g, gs))
        search = lambda **kw: ops.knn_topk_fp8(q, qs, g, gs, k, **kw)
        scales = (ops._ptr(qs), ops._ptr(gs))
    else:
        q, g = q32.to(torch.bfloat16), g32.to(torch.bfloat16)
        ref = oknn.knn_topk(q, g, k)
        q, g = q.to(dev), g.to(dev)
        search = lambda **kw: ops.knn_topk(q, g, k, **kw)
        scales = (None, None)
    with pytest.raises(RuntimeError, match=unsupported):
        ops.knn_topk_exhaustive(q, g, k, 0, *((qs, gs) if form == "e4m3" else ()))
    ws = ops.knn_workspace(3, n, D, k, dev)
    vals = torch.full((3, k), 1234.5, device=dev)
    idx = torch.full((3, k), -99, dtype=torch.int32, device=dev)
    st = lib.vpr_knn_topk_exhaustive(ops._ptr(q), scales[0], ops._ptr(g), scales[1], int(form == "e4m3"), 3, n, D, k, 0,
                                     ops._ptr(vals), ops._ptr(idx), ops._ptr(ws), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert st == -2 and bool((vals == 1234.5).all()) and bool((idx == -99).all())
    status = torch.full((3,), -1, dtype=torch.int32, device=dev)
    v, i = search(status=status)
    first = status.tolist()
    assert first[1] == 2 and first[0] in (0, 1) and first[2] in (0, 1)
    assert torch.equal(i.cpu()[[0, 2]], ref[1][[0, 2]]) and torch.equal(v.cpu()[[0, 2]], ref[0][[0, 2]])
    status.fill_(-1)
    with pytest.raises(RuntimeError, match=unsupported):
        search(status=status, exact_fallback=True)
    assert status.tolist() == first
