"""Stage A of the SALAD aggregation (Sinkhorn, V = F^T P^T on the hi/lo planes, the three L2 normalisations) judged per element
— TEST ORACLE.  Three kernels implement the stage (salad.hip at n = 256, salad_anyres.hip at 65 .. 576, salad_hires.hip up to
1369 tokens); the descriptor averages the transport plan P over the tokens, so one mishandled token is diluted by 1 / n and no
max-abs gate on the descriptor sees it.  This file holds
  * true_stage_a        the stage in f64 (oracle.salad.matching_probs is the only Sinkhorn), every intermediate returned;
  * stage_a_f32_cpu     the kernels' arithmetic in plain torch f32 on the CPU, the yardstick of the rms criterion — exp
                        domain, K = exp(M - rowmax), alpha / beta with the kernels' marginals, P = K alpha beta (n + m),
                        hi = bf16(P), lo = bf16(P - hi), F split the same way, the products lo hi + hi lo + hi hi, three
                        F.normalize steps with eps 1e-12; its summation order is torch's, not any kernel's;
  * probe_inputs        feature probes that undo the dilution: B = ceil(n / 128) images with the SAME scores, image r carrying
                        the weighted one-hot features F[j][l] = x_j if j == 128 r + l else 0, so that the descriptor entry
                        256 + 64 l + m of image r is x_j P[m][j] / ||x . P[m, block r]|| / sqrt(65): ONE entry of the plan
                        (and a second family with the blocks moved by 64 tokens, see SHIFTS);
  * descriptor_bound    a per-element bound of |f32 stage - f64 stage| from the rounding model below; probe_bound is the same
                        bound read at the probes' judged entries (the model counts the non-zero products of a column, and a
                        probe column has one);
  * MUTATIONS           the exact difference one plausible mistake makes, applied inside stage_a_f32_cpu;
  * compare_descriptor / compare_probes   the two comparisons tests/test_salad_stage_a_gpu.py applies to a kernel's output;
                        tests/test_salad_stage_a_cpu.py applies the same functions to the restatement and to every mutation.

Rounding model (u = 2^-24; gamma_k = k u / (1 - k u), Higham 4.4; every sum is an f32 sum in SOME order; all relative and
to first order, the total times 1 + 2^-10 for the second-order terms — every relative error below is under 2^-11):
  K      d = M - rowmax is one f32 subtraction (u |d|); the device's fast exp is exp2(d * log2e) with log2e an f32 constant
         and the product rounded (2 u |d| in the exponent) and a 1-ulp exp2 (2 u):           eK_ij = (3 |d_ij| + 2) u
         (the maximum itself is exact; a library exp of 1 ulp on d is inside the same figure).
  alpha  s_i = sum_j K_ij beta_j has n positive terms, so its relative error is the weighted mean of the terms' errors — the
         weights are row i of the plan after the iteration before, normalised (the softmax of the scores before the first) —
         plus gamma_{n+1} for the sum; the marginal a_i is 1 / (n + m), times n - m for the dustbin (2 u), one division (u):
                                                       ea_i = sum_j W_ij (eK_ij + eb_j) + gamma_{n+1} + 3 u
  beta   the same down a column of 65 entries, weights = column j of the plan after this iteration (it sums to 1):
                                                       eb_j = sum_i P_ij (eK_ij + ea_i) + gamma_{66} + 2 u
  P      K alpha beta (n + m): three products.  The last alpha_i is ONE number on all of cluster i's row, whatever its error:
         it comes out of every kept product of that cluster and cancels in the cluster normalisation (the split's error is
         relative), so it is not counted; the errors of the alphas INSIDE the last beta differ from row to row and are:
                                                       eP_ij = eK_ij + eb_j + 3 u
  split  hi = bf16(v), lo = bf16(v - hi) (v - hi is exact in f32): |v - hi| <= 2^-8 B with B = 2^floor(log2 |v|) <= |v| the
         binade of v; either v - hi = +-2^-8 B, a power of two, and lo is exact, or |v - hi| < 2^-8 B lies in a binade <=
         2^-9 B and |v - hi - lo| <= 2^-17 B.  So v = hi + lo to 2^-17 B <= 2^-17 |v| — the header's "P = hi + lo to 2^-17",
         with the binade in place of |v| — as long as lo is a normal bf16 number or zero (|v| >= 2^-60 is far inside).  The
         kept products are (F_hi + F_lo)(P_hi + P_lo) - F_lo P_lo, |F_lo P_lo| <= 2^-16 |F P|:   2^-17 + 2^-17 + 2^-16 = 2^-15
  V      bf16 x bf16 is exact in f32; a column of F with z non-zero tokens adds 3 z non-zero products (adding an exact zero
         rounds nothing; z <= npad) of total magnitude <= (1 + 2^-7) sum |F| P:
                                A_lm = sum_j |F_jl| P_mj (eP_mj + 2^-15) + gamma_{3 z_l} (1 + 2^-7) sum_j |F_jl| P_mj
  norms  F.normalize three times, c = max(sqrt(sum of squares), 1e-12): N squares (u each) and N - 1 additions of
         non-negative terms give gamma_N on the sum and half of it on the root, plus u for the root, and the entries' own
         errors enter through d(c^2) = 2 sum |v| dv:
           cluster m over 128 dims   rho_m = sum_l |V_lm| A_lm / c_m^2 + 65 u,   dVn_lm = A_lm / c_m + |Vn_lm| (rho_m + u)
           token vector, 256 entries                                             dgn_k = |gn_k| (129 u + u)
           global, 8448 entries      rho_G = (sum |gn| dgn + sum |Vn| dVn) / G^2 + 4225 u
           output                    dout = [dgn | dVn] / G + |out| (rho_G + u)
         A block that is exactly zero stays exactly zero (0 / 1e-12 = 0), and its bound is 0.
Domain of the model: |d| <= 80 (no underflow of K) and every P entry >= 2^-60; both are asserted.

Mistakes that are provably invisible in the descriptor, and therefore NOT in MUTATIONS: any per-cluster factor on P — the last
iteration's alpha (a wrong a_reg in it, or a stale one), `scale`, a b_col that is wrong by the same factor in every column (the
next alpha undoes it, the last one is a factor on all of P) — cancels in the cluster normalisation, exactly for a power of two
and to rounding otherwise.
"""
import functools
import math

import torch

from .salad import matching_probs

U32 = 2.0 ** -24
M_, L_, T_ = 64, 128, 256
D_OUT = T_ + L_ * M_
EPS = 1e-12
G = 4.0                                   # rms(kernel - f64) <= G rms(stage_a_f32_cpu - f64): the project's margin for another summation order
SPLIT = 2.0 ** -15                        # the two splits and the dropped lo x lo product, relative to |F P|
SECOND_ORDER = 1 + 2.0 ** -10
P_FLOOR = 2.0 ** -60


def _gamma(k):
    k = torch.as_tensor(k, dtype=torch.float64)
    return k * U32 / (1 - k * U32)


def _norms(V, g):
    """V [B, l, m], g [B, t] (any float dtype) -> cluster norms, global norm, descriptor; F.normalize's eps rule throughout."""
    cn = V.pow(2).sum(1).sqrt()
    Vn = V / cn.clamp_min(EPS).unsqueeze(1)
    out = torch.cat([g / g.pow(2).sum(1, keepdim=True).sqrt().clamp_min(EPS), Vn.flatten(1)], dim=1)
    gn = out.pow(2).sum(1).sqrt()
    return cn, gn, out / gn.clamp_min(EPS).unsqueeze(1)


# ------------------------------------------------------------------------------------------------ f64
def _true_from_plan(P, feats, tok):
    V = torch.einsum("bnl,bmn->blm", feats.double(), P)
    cn, gn, desc = _norms(V, tok.double())
    return dict(P=P, V=V, cnorm=cn, gnorm=gn, desc=desc)


def true_stage_a(scores, feats, tok, dustbin: float, iters: int = 3):
    """scores [B, n, 64], feats [B, n, 128], tok [B, 256] (token-major, as the stage takes them) -> dict of f64 tensors:
    P [B, 64, n] (dustbin row dropped), V [B, 128, 64] before any normalisation, cnorm [B, 64], gnorm [B] (the norm of
    [g / ||g|| | V / cnorm]), desc [B, 8448]."""
    P = matching_probs(scores.double().transpose(1, 2).contiguous(), dustbin, iters)[:, :-1, :]
    return _true_from_plan(P.expand(feats.shape[0], -1, -1), feats, tok)


# ------------------------------------------------------------------------------------------------ plain f32, and the mutations
# (kind, argument).  A token argument is an index, or "last" for n - 1; a mutation applies to n if its token exists and, for
# the pad columns, if n is no multiple of 16 (applies()).
MUTATIONS = (("p_lo_token", "last"), ("p_lo_token", 256), ("p_lo_token", 512), ("p_lo_token", 1024),   # lo plane of P lost on one token
             ("p_lo_all", None),                    # ... on every token
             ("f_lo_all", None),                    # lo plane of F lost
             ("no_cross_term", "flo_phi"), ("no_cross_term", "fhi_plo"),
             ("token_not_aggregated", "last"),
             ("rowsum_skips_last_token", "first"), ("rowsum_skips_last_token", "final"),   # token n - 1 left out of one iteration's row sums
             ("pad_in_rowsums", None),              # columns n .. npad - 1 counted as score 0, beta 1
             ("dustbin_alpha_a_reg", None),         # the dustbin row's alpha from 1 / (n + m) instead of (n - m) / (n + m)
             ("one_iteration_fewer", None))


def _token(arg, n):
    return n - 1 if arg == "last" else arg


def applies(mutation, n: int, iters: int = 3) -> bool:
    kind, arg = mutation
    if kind in ("p_lo_token", "token_not_aggregated"):
        return _token(arg, n) < n
    if kind == "pad_in_rowsums":
        return n % 16 != 0
    if kind == "rowsum_skips_last_token" and arg == "final":
        return iters > 1                           # with one iteration "first" is the same mistake
    return True


def _split(v):
    hi = v.to(torch.bfloat16).float()
    return hi, (v - hi).to(torch.bfloat16).float()


def stage_a_f32_cpu(scores, feats, tok, dustbin: float, iters: int = 3, mutation=None):
    """The same stage in plain torch f32, arranged as the kernels arrange it (see the module docstring).  Returns the dict of
    true_stage_a, f32.  mutation: None or one of MUTATIONS — what a kernel with that mistake would leave."""
    kind, arg = mutation if mutation is not None else (None, None)
    f32 = torch.float32
    S = scores.to(f32).transpose(1, 2)
    B, m, n = S.shape
    npad = (n + 15) & ~15
    Mx = torch.cat([S, torch.full((B, 1, n), dustbin, dtype=f32)], dim=1)
    rmax = Mx.amax(dim=2, keepdim=True)
    K = torch.exp(Mx - rmax)
    inv_nm = torch.tensor(1.0, dtype=f32) / torch.tensor(float(n + m), dtype=f32)
    a = inv_nm.repeat(m + 1)
    if kind != "dustbin_alpha_a_reg":
        a[m] = torch.tensor(float(n - m), dtype=f32) * inv_nm
    b_col, scale = inv_nm, torch.tensor(float(n + m), dtype=f32)
    alpha, beta = torch.ones(B, m + 1, dtype=f32), torch.ones(B, n, dtype=f32)
    rounds = iters - 1 if kind == "one_iteration_fewer" else iters
    for it in range(rounds):
        Kb = K * beta.unsqueeze(1)
        skip = kind == "rowsum_skips_last_token" and it == (0 if arg == "first" else rounds - 1)
        rs = Kb[:, :, :n - 1].sum(2) if skip else Kb.sum(2)
        if kind == "pad_in_rowsums":
            rs = rs + (npad - n) * torch.exp(-rmax.squeeze(2))
        alpha = a / rs
        beta = b_col / (K * alpha.unsqueeze(2)).sum(1)
    P = K[:, :m] * alpha[:, :m].unsqueeze(2) * (beta * scale).unsqueeze(1)
    Ph, Pl = _split(P)
    Fm = feats.to(f32).transpose(1, 2)                         # [B, l, n]
    if Fm.shape[0] != B:
        Ph, Pl = Ph.expand(Fm.shape[0], -1, -1), Pl.expand(Fm.shape[0], -1, -1)
    Fh, Fl = _split(Fm)
    if kind == "p_lo_token":
        Pl = Pl.clone()
        Pl[:, :, _token(arg, n)] = 0
    if kind == "p_lo_all":
        Pl = torch.zeros_like(Pl)
    if kind == "f_lo_all":
        Fl = torch.zeros_like(Fl)
    if kind == "token_not_aggregated":
        Fh, Fl = Fh.clone(), Fl.clone()
        Fh[:, :, _token(arg, n)] = 0
        Fl[:, :, _token(arg, n)] = 0
    mm = lambda x, y: torch.einsum("bln,bmn->blm", x, y)
    V = mm(Fh, Ph)
    if not (kind == "no_cross_term" and arg == "fhi_plo"):
        V = mm(Fh, Pl) + V
    if not (kind == "no_cross_term" and arg == "flo_phi"):
        V = mm(Fl, Ph) + V
    cn, gn, desc = _norms(V, tok.to(f32))
    return dict(P=P, V=V, cnorm=cn, gnorm=gn, desc=desc)


# ------------------------------------------------------------------------------------------------ the bound
def plan_error(scores, dustbin: float, iters: int):
    """-> (P f64 [B, 64, n], eP [B, 64, n], ea [B, 64]): the true plan, the relative error the model allows on each of its
    entries up to the factor of its cluster, and the bound of that factor's error (the last alpha: |P^ / P - 1| <= eP + ea)."""
    S = scores.double().transpose(1, 2).contiguous()
    B, m, n = S.shape
    Mx = torch.cat([S, torch.full((B, 1, n), float(dustbin), dtype=torch.float64)], dim=1)
    d = Mx - Mx.amax(dim=2, keepdim=True)
    assert d.min().item() >= -80.0, "K would underflow in f32: outside the model"
    eK = (3 * d.abs() + 2) * U32
    ea, eb = torch.zeros(B, m + 1, dtype=torch.float64), torch.zeros(B, n, dtype=torch.float64)
    Pt = matching_probs(S, dustbin, 0)
    for t in range(1, iters + 1):
        W = Pt / Pt.sum(2, keepdim=True)
        ea = (W * (eK + eb.unsqueeze(1))).sum(2) + _gamma(n + 1) + 3 * U32
        Pt = matching_probs(S, dustbin, t)
        W = Pt / Pt.sum(1, keepdim=True)
        eb = (W * (eK + ea.unsqueeze(2))).sum(1) + _gamma(m + 2) + 2 * U32
    P = Pt[:, :m]
    assert P.min().item() >= P_FLOOR, "a plan entry below 2^-60: outside the model"
    return P, eK[:, :m] + eb.unsqueeze(1) + 3 * U32, ea[:, :m]


def descriptor_bound(scores, feats, tok, dustbin: float, iters: int = 3):
    """-> f64 [B, 8448]: |an f32 stage A - true_stage_a| may not exceed this on any element (module docstring).  scores may
    have batch 1 where every image carries the same ones."""
    P, eP, _ = plan_error(scores, dustbin, iters)
    Fa = feats.double().abs().transpose(1, 2)                  # [B, l, n]
    B = Fa.shape[0]
    nz = Fa[Fa > 0]
    assert nz.numel() == 0 or nz.min().item() >= P_FLOOR
    P, eP = P.expand(B, -1, -1), eP.expand(B, -1, -1)
    z = (Fa > 0).sum(2).double()                               # [B, l] non-zero tokens of a column
    mag = torch.einsum("bln,bmn->blm", Fa, P)
    A = torch.einsum("bln,bmn->blm", Fa, P * (eP + SPLIT)) + (_gamma(3 * z) * (1 + 2.0 ** -7)).unsqueeze(2) * mag
    t = _true_from_plan(P, feats, tok)
    V, cn, gnorm = t["V"], t["cnorm"], t["gnorm"]
    c = cn.clamp_min(EPS).unsqueeze(1)
    Vn = V / c
    rho = (V.abs() * A).sum(1, keepdim=True) / c.pow(2) + 65 * U32
    dVn = A / c + Vn.abs() * (rho + U32)
    g = tok.double()
    gn = g / g.pow(2).sum(1, keepdim=True).sqrt().clamp_min(EPS)
    dgn = gn.abs() * 130 * U32
    Gd = gnorm.clamp_min(EPS).unsqueeze(1)
    rho_g = ((gn.abs() * dgn).sum(1, keepdim=True) + (Vn.abs() * dVn).flatten(1).sum(1, keepdim=True)) / Gd.pow(2) + (D_OUT / 2 + 1) * U32
    dout = torch.cat([dgn, dVn.flatten(1)], dim=1) / Gd + t["desc"].abs() * (rho_g + U32)
    return dout * SECOND_ORDER


# ------------------------------------------------------------------------------------------------ probes
# A token that is ALONE in its block of 128 is judged on its sign only: its 64 entries are normalised to +-1 / sqrt(65) whatever
# P says, and with a few block-mates most of a relative error still cancels.  That is the last token at n = 128 k + 1 — 257,
# 513, 1025: the very tokens a column loop or a P block may drop — so every count is probed twice: blocks at 128 r (shift 0, the
# B = ceil(n / 128) images) and blocks at 128 r - 64 (shift 64, one image more at most).  Each token then has at least 63
# block-mates in one of the two families (asserted in tests/test_salad_stage_a_cpu.py).
SHIFTS = (0, 64)


def probe_inputs(n: int, seed: int, shift: int = 0):
    """-> scores [B, n, 64] (every image the same, randn * 2), feats [B, n, 128] (token j: x_j at [j][l] of image r, where
    128 r + l = j + shift), tok [B, 256] (random), x [n] f32 with both signs and |x| in [0.5, 2), not bf16 numbers.
    B = ceil((n + shift) / 128)."""
    g = torch.Generator().manual_seed(seed)
    B = (n + shift + 127) // 128
    scores = (torch.randn(1, n, M_, generator=g) * 2).expand(B, -1, -1).contiguous()
    x = (torch.rand(n, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    tok = torch.randn(B, T_, generator=g)
    feats = torch.zeros(B, n, L_)
    j = torch.arange(n)
    feats[(j + shift) // 128, j, (j + shift) % 128] = x
    return scores, feats, tok, x


def probe_entries(desc, n: int, shift: int = 0):
    """desc [B, 8448] -> [n, 64]: row j holds the descriptor entries 256 + 64 l + m of image r (128 r + l = j + shift), m = 0 .. 63."""
    return desc[:, T_:].reshape(-1, M_)[shift:shift + n]


def probe_expected(scores, feats, tok, dustbin: float, iters: int = 3, shift: int = 0):
    """-> (expected f64 [n, 64], true): the judged entries of the f64 descriptor — x_j P[m][j] / ||x . P[m, block r]|| / sqrt(65),
    which tests/test_salad_stage_a_cpu.py evaluates by brute force from P — and the dict of true_stage_a they were read from."""
    true = true_stage_a(scores[:1], feats, tok, dustbin, iters)      # every image carries the same scores: one Sinkhorn
    return probe_entries(true["desc"], scores.shape[1], shift), true


def probe_bound(scores, feats, tok, dustbin: float, iters: int = 3, shift: int = 0):
    """descriptor_bound of the probes (one non-zero token per feature column: three products, two additions) -> (the whole
    [B, 8448] bound, its judged entries [n, 64])."""
    bound = descriptor_bound(scores[:1], feats, tok, dustbin, iters)
    return bound, probe_entries(bound, scores.shape[1], shift)


# ------------------------------------------------------------------------------------------------ cases and comparisons
def _rms(a):
    return a.double().pow(2).mean().sqrt().item()


@functools.lru_cache(maxsize=8)            # a case at 1369 tokens holds 12 MB of inputs: the tests use each within a few steps
def probe_case(n: int, shift: int = 0, dustbin: float = 1.0, iters: int = 3):
    """Inputs, f64 answer, bound and the yardstick's errors of the probes at n tokens, computed once and shared (read-only).
    Both shifts carry the same scores and weights x (seed n)."""
    scores, feats, tok, x = probe_inputs(n, seed=n, shift=shift)
    expected, true = probe_expected(scores, feats, tok, dustbin, iters, shift)
    bound, _ = probe_bound(scores, feats, tok, dustbin, iters, shift)
    cpu = stage_a_f32_cpu(scores[:1], feats, tok, dustbin, iters)
    return dict(kind="probe", n=n, shift=shift, dustbin=dustbin, iters=iters, scores=scores, feats=feats, tok=tok, x=x, expected=expected,
                true=true, bound=bound, cpu=cpu, cpu_rms=_rms((probe_entries(cpu["desc"].double(), n, shift) - expected) / expected))


def gaussian_inputs(B: int, n: int, seed: int, scale: float = 2.0):
    """The _stage_inputs of tests/test_salad_anyres_gpu.py and tests/test_salad_hires_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, M_, generator=g) * scale, torch.randn(B, n, L_, generator=g), torch.randn(B, T_, generator=g)


def general_case(scores, feats, tok, dustbin: float, iters: int):
    """The f64 answer, the bound and the yardstick of stage A on arbitrary inputs, as a case of compare_descriptor."""
    true = true_stage_a(scores, feats, tok, dustbin, iters)
    cpu = stage_a_f32_cpu(scores, feats, tok, dustbin, iters)
    return dict(kind="gauss", n=scores.shape[1], dustbin=dustbin, iters=iters, scores=scores, feats=feats, tok=tok, true=true, cpu=cpu,
                bound=descriptor_bound(scores, feats, tok, dustbin, iters), cpu_rms=_rms(cpu["desc"].double() - true["desc"]))


@functools.lru_cache(maxsize=None)
def gaussian_case(n: int, dustbin: float, iters: int, B: int = 2):
    return general_case(*gaussian_inputs(B, n, seed=n), dustbin, iters)


def compare_descriptor(got, case):
    """got [B, 8448] against a case's f64 descriptor -> (worst |err| / bound over the elements, rms(err) / rms(yardstick's err)).
    An element whose bound is 0 (an exactly zero block) must be exactly 0."""
    err = (got.double() - case["true"]["desc"]).abs()
    bound = case["bound"]
    assert got.shape == bound.shape and torch.isfinite(err).all(), "descriptor not finite"
    zero = bound == 0
    worst = 0.0 if zero.all() else (err[~zero] / bound[~zero]).max().item()
    if (err[zero] != 0).any():
        worst = math.inf
    return worst, _rms(err) / case["cpu_rms"]


def compare_probes(got, case):
    """got [B, 8448] of a probe case -> (worst |err| / bound over the WHOLE descriptor — judged entries, token block, and the
    entries of no token in the first and last image, which must be exactly 0 —, rms of the judged entries' relative error /
    that of the yardstick, worst relative error of a judged entry and its (token, cluster))."""
    worst, _ = compare_descriptor(got, case)
    rel = (probe_entries(got.double(), case["n"], case["shift"]) - case["expected"]) / case["expected"]
    at = rel.abs().argmax().item()
    return worst, _rms(rel) / case["cpu_rms"], rel.abs().max().item(), (at // M_, at % M_)


def compare(got, case):
    """-> (worst |err| / bound, rms ratio) by the comparison of the case's kind."""
    return (compare_probes if case["kind"] == "probe" else compare_descriptor)(got, case)[:2]


def assert_within(worst: float, ratio: float, tag: str = ""):
    assert worst <= 1.0, f"{tag}: element bound exceeded, worst |err| / bound {worst:.3f}"
    assert ratio <= G, f"{tag}: rms ratio {ratio:.2f} > {G}"


# ------------------------------------------------------------------------------------------------ mutations against a case
def mutation_margins(got, case):
    """got [B, 8448]: a stage's output on `case` (probe_case or gaussian_case) that passes the comparisons.
    -> {mutation: max(worst |err| / bound, rms ratio / G)} of got + the exact difference the mistake makes in the restatement,
    for every mutation that applies to the case: > 1 means the comparison of that case rejects it."""
    out = {}
    scores = case["scores"][:1] if case["kind"] == "probe" else case["scores"]
    for mutation in MUTATIONS:
        if not applies(mutation, case["n"], case["iters"]):
            continue
        bad = stage_a_f32_cpu(scores, case["feats"], case["tok"], case["dustbin"], case["iters"], mutation)["desc"]
        worst, ratio = compare(got.double() + (bad.double() - case["cpu"]["desc"].double()), case)
        out[mutation] = max(worst, ratio / G)
    return out


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
# kernel -> token counts of the probes: every count at which a kernel changes path (columns tid + 256 q of the run-time-n
# kernel, its one or two staging rounds at 288 / 289, the 512-column P blocks of the high-resolution kernel, ragged 16-steps)
PROBE_N = {"fixed": (256,),
           "anyres": (65, 66, 80, 127, 128, 129, 255, 256, 257, 288, 289, 511, 512, 513, 529, 575, 576),
           "hires": (65, 256, 257, 511, 512, 513, 576, 577, 768, 769, 1023, 1024, 1025, 1280, 1281, 1368, 1369)}
GAUSS_N = {"fixed": (256,), "anyres": (65, 256, 529, 576), "hires": (65, 256, 529, 576, 577, 1369)}
GAUSS_ITERS, GAUSS_DUSTBIN = (1, 3, 7), 0.7
# (kernel, case): the cases on which the mutation tests corrupt an output, on the GPU and, with the restatement in the kernel's
# place, on the CPU.  Every mutation applies to, and is rejected on, at least one of them; a case is ("probe", n, shift) or
# ("gauss", n, iters).
MUTATION_RUNS = (("fixed", ("probe", 256, 0)), ("anyres", ("probe", 65, 0)), ("anyres", ("probe", 257, 64)), ("anyres", ("probe", 513, 64)),
                 ("hires", ("probe", 513, 64)), ("hires", ("probe", 1025, 64)), ("hires", ("probe", 1369, 0)),
                 ("anyres", ("gauss", 65, 1)), ("hires", ("gauss", 65, 3)), ("hires", ("gauss", 577, 1)))


def case_of(spec):
    kind, n, arg = spec
    return probe_case(n, arg) if kind == "probe" else gaussian_case(n, GAUSS_DUSTBIN, arg)
