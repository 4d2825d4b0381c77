"""Stage-level oracle of the f32-accurate SALAD path (vpr_salad_aggregate_f32 and its _n / _hires forms): the three bf16
planes of an f32 operand, the six-product "plane GEMM" both layers run, what the path leaves in its workspace (hidden values
H / Ht in f32, scores S, features F, token features g), the true f64 statement of the same MLPs, the outputs a subtly wrong
kernel would leave (MUTATIONS), and three families of inputs on which f32 accumulation is exact in ANY order, so that a
kernel must leave the plane model's bits.

Nothing here looks at a kernel: tests/test_oracle_selfchecks.py asserts every property the GPU tests rely on, on this file
alone.  Planes are bf16 BIT PATTERNS (int16 tensors); plane_values() turns them into numbers.

  x = h + m + q exactly,   h = bf16(x),  m = bf16(x - h),  q = bf16(x - h - m)       (round to nearest, ties to even)
  segment           0  1  2  3  4  5
  activation plane  q  h  m  m  h  h        ACT_ORDER
  weight plane      h  q  m  h  m  h        WGT_ORDER
so the kept products are (q,h) (h,q) (m,m) (m,h) (h,m) (h,h); dropped: (m,q) (q,m) (q,q).
"""
import functools

import torch

from . import salad_stages as ost

U32 = 2.0 ** -24                     # unit roundoff of f32
ACT_ORDER = (2, 0, 1, 1, 0, 0)       # index into (h, m, q)
WGT_ORDER = (0, 2, 1, 0, 1, 0)
DROPPED = ((1, 2), (2, 1), (2, 2))   # (activation plane, weight plane) of the products the path leaves out
GRID = 2.0 ** -18                    # every kept product of the exact families E1 / E2 is a multiple of it
EXACT_LIMIT = 2.0 ** 24 * GRID       # 64: below it every multiple of GRID is an f32 number
NNZ = 48                             # non-zeros per weight row in E1 / E2


# ------------------------------------------------------------------------------------------------ planes
def split3(x: torch.Tensor):
    """f32 tensor -> (h, m, q): int16 tensors holding bf16 bit patterns.  Each residual is formed exactly (in f64, and
    checked to be an f32 number, which is what lets a kernel form it in f32)."""
    assert x.dtype == torch.float32
    bits = lambda v: v.to(torch.bfloat16).view(torch.int16)
    h = x.to(torch.bfloat16)
    r1 = x.double() - h.double()
    assert torch.equal(r1.float().double(), r1)
    m = r1.float().to(torch.bfloat16)
    r2 = r1 - m.double()
    assert torch.equal(r2.float().double(), r2)
    return bits(x), m.view(torch.int16), bits(r2.float())


def plane_values(p: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    return p.view(torch.bfloat16).to(dtype)


def planes_in_order(x: torch.Tensor, order) -> torch.Tensor:
    """f32 [rows, K] -> int16 [rows, 6, K]: the six segments of a plane buffer in `order` (ACT_ORDER / WGT_ORDER)."""
    p = split3(x)
    return torch.stack([p[i] for i in order], dim=-2)


def segment_products(a: torch.Tensor, w: torch.Tensor, a_order=ACT_ORDER, w_order=WGT_ORDER) -> torch.Tensor:
    """a f32 [M, K], w f32 [N, K] -> f64 [6, M, N]: each segment's contribution to a w^T."""
    pa, pw = [plane_values(p) for p in split3(a)], [plane_values(p) for p in split3(w)]
    return torch.stack([pa[i] @ pw[j].T for i, j in zip(a_order, w_order)])


def plane_gemm(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The f64 sum of the six kept products: what the path's GEMM computes, without its accumulation error."""
    return segment_products(a, w).sum(0)


def dropped_bound(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """f64 [M, N]: sum over k of |m q| + |q m| + |q q|.  plane_gemm(a, w) - a w^T is minus the dropped products exactly (the
    planes sum back to the operands), so this bounds it."""
    pa, pw = [plane_values(p).abs() for p in split3(a)], [plane_values(p).abs() for p in split3(w)]
    return sum(pa[i] @ pw[j].T for i, j in DROPPED)


# ------------------------------------------------------------------------------------------------ the two layers
def _parts(tokens, w):
    C = tokens.shape[2]
    return tokens[:, 1:, :].reshape(-1, C).contiguous(), tokens[:, 0, :].contiguous(), w["w2_s"].shape[1]


def _layer2(H, Ht, w, hidden, a_order=ACT_ORDER, drop=(), b2_s=True):
    def gemm(a, wk):
        seg = segment_products(a, w[wk], a_order)
        return seg.sum(0) - sum(seg[s] for s in drop)
    S = gemm(H[:, :hidden].contiguous(), "w2_s") + (w["b2_s"].double() if b2_s else 0)
    return dict(S=S, F=gemm(H[:, hidden:].contiguous(), "w2_c") + w["b2_c"].double(), g=gemm(Ht, "w2_t") + w["b2_t"].double())


def f32_stage_outputs(tokens, w, mutation=None):
    """tokens f32 [B, 1+n, C] (cls first), w: dict of ten f32 tensors -> dict of the plane model of the workspace:
      H [B*n, 2*hidden], Ht [B, hidden]   f32: relu(plane GEMM + b1) rounded to f32 ONCE, which is what the workspace holds
      S [B*n, m], F [B*n, l], g [B, t]    f64: plane GEMM of those f32 hidden values + b2
    mutation: None, or one of MUTATIONS — the same as a wrong kernel would leave it."""
    x, cls, hidden = _parts(tokens, w)
    kind, arg = mutation if mutation is not None else (None, None)
    order1 = WGT_ORDER if kind == "act_order" and arg == 1 else ACT_ORDER
    seg, segt = segment_products(x, w["w1_sc"], order1), segment_products(cls, w["w1_t"], order1)
    drop = {1: (), 2: ()}
    if kind == "drop_segment":
        drop[arg[0]] = (arg[1],)
    if kind == "no_low_planes":
        drop = {1: (0, 1), 2: (0, 1)}
    z, zt = seg.sum(0) - sum(seg[s] for s in drop[1]), segt.sum(0) - sum(segt[s] for s in drop[1])
    H, Ht = torch.relu(z + w["b1_sc"].double()).float(), torch.relu(zt + w["b1_t"].double()).float()
    if kind == "hidden_bf16":
        H, Ht = H.to(torch.bfloat16).float(), Ht.to(torch.bfloat16).float()
    out = _layer2(H, Ht, w, hidden, a_order=WGT_ORDER if kind == "act_order" and arg == 2 else ACT_ORDER,
                  drop=drop[2], b2_s=kind != "drop_b2_s")
    out.update(H=H, Ht=Ht)
    if kind == "swap_token_rows":
        idx = torch.arange(H.shape[0])
        idx[-1], idx[-2] = idx[-2].clone(), idx[-1].clone()
        out.update({k: out[k][idx] for k in ("H", "S", "F")})
    return out


# What a wrong kernel would leave: one of the six K segments missing in layer 1 / layer 2, no low plane (segments 0 and 1)
# in either layer — a 16-bit-mantissa GEMM —, the weight plane order used on the activation side of layer 1 / layer 2, hidden
# values passed through bf16, the score head's second-layer bias left out, the last two token rows of the batch exchanged.
MUTATIONS = tuple([("drop_segment", (layer, s)) for layer in (1, 2) for s in range(6)] +
                  [("no_low_planes", None), ("act_order", 1), ("act_order", 2), ("hidden_bf16", None), ("drop_b2_s", None),
                   ("swap_token_rows", None)])
# those of them that no descriptor-level bound sees: a product of the size of f32's own rounding missing, and b2_s
FAINT_MUTATIONS = tuple(m for m in MUTATIONS if (m[0] == "drop_segment" and m[1][1] <= 2) or m[0] in ("no_low_planes", "drop_b2_s"))


def true_stage_outputs(tokens, w):
    """The same MLPs in f64 on the f32 operands, nothing rounded: H, Ht, S, F, g, all f64."""
    W = {k: v.double() for k, v in w.items()}
    x, cls, hidden = _parts(tokens.double(), w)
    H, Ht = torch.relu(x @ W["w1_sc"].T + W["b1_sc"]), torch.relu(cls @ W["w1_t"].T + W["b1_t"])
    return dict(H=H, Ht=Ht, S=H[:, :hidden] @ W["w2_s"].T + W["b2_s"], F=H[:, hidden:] @ W["w2_c"].T + W["b2_c"],
                g=Ht @ W["w2_t"].T + W["b2_t"])


def mlps_f32_cpu(tokens, w):
    """The same in plain torch f32 on the CPU: the yardstick of the RMS test — what an ordinary f32 implementation loses."""
    x, cls, hidden = _parts(tokens, w)
    H, Ht = torch.relu(x @ w["w1_sc"].T + w["b1_sc"]), torch.relu(cls @ w["w1_t"].T + w["b1_t"])
    return dict(H=H, Ht=Ht, S=H[:, :hidden] @ w["w2_s"].T + w["b2_s"], F=H[:, hidden:] @ w["w2_c"].T + w["b2_c"],
                g=Ht @ w["w2_t"].T + w["b2_t"])


def _gamma(n: int) -> float:
    return n * U32 / (1 - n * U32)


def _head_bound(x, w1, b1, w2, b2):
    """Per-element bounds of one two-layer head against the TRUE f64 result, for a kernel that sums the six kept products
    of every k and the bias in f32 in some order (n = 6K + 1 terms: |error| <= gamma_n sum|terms|, Higham 4.4).
      layer 1   e1 = gamma_{6K+1} (PL |x||w1| + |b1|) + dropped(x, w1), PL = 1.02 >= (1 + 2^-7 + 2^-16)^2: the six kept
                products of one k are together at most (|h| + |m| + |q|)_x (|h| + |m| + |q|)_w and |h| <= (1 + 2^-8) |x|,
                |m| <= 2^-8 |x|, |q| <= 2^-16 |x|; relu is 1-Lipschitz, so |H - H_true| <= e1.
      layer 2   the kernel's own hidden values are at most hi = H_true + e1:
                gamma_{6 hidden + 1} (PL hi |w2| + |b2|) + (2^-23 + 2^-32) hi |w2| [dropped: |m| <= 2^-8 |x|, |q| <= 2^-16 |x|]
                + e1 |w2|  (the layer-1 error carried through W2).
    -> (e1 [rows, hidden], e2 [rows, n_out]) f64."""
    d = torch.float64
    K, hidden = w1.shape[1], w2.shape[1]
    PL = 1.02
    e1 = _gamma(6 * K + 1) * (PL * (x.to(d).abs() @ w1.to(d).abs().T) + b1.to(d).abs()) + dropped_bound(x, w1)
    hi = torch.relu(x.to(d) @ w1.to(d).T + b1.to(d)) + e1
    hw = hi @ w2.to(d).abs().T
    e2 = _gamma(6 * hidden + 1) * (PL * hw + b2.to(d).abs()) + (2.0 ** -23 + 2.0 ** -32) * hw + e1 @ w2.to(d).abs().T
    return e1, e2


def stage_error_bounds(tokens, w):
    """-> dict H, Ht, S, F, g (f64): |kernel - true_stage_outputs| may not exceed these on any element.  Computed from the
    inputs alone; loose (every rounding at its worst at once)."""
    x, cls, hidden = _parts(tokens, w)
    e1s, S = _head_bound(x, w["w1_sc"][:hidden], w["b1_sc"][:hidden], w["w2_s"], w["b2_s"])
    e1c, F = _head_bound(x, w["w1_sc"][hidden:], w["b1_sc"][hidden:], w["w2_c"], w["b2_c"])
    Ht, g = _head_bound(cls, w["w1_t"], w["b1_t"], w["w2_t"], w["b2_t"])
    return dict(H=torch.cat([e1s, e1c], dim=1), Ht=Ht, S=S, F=F, g=g)


# ------------------------------------------------------------------------------------------------ inputs
def gaussian_inputs(C: int, B: int, seed: int, std: float = 0.02, n: int = 256, hidden: int = 512, m: int = 64, l: int = 128, t: int = 256):
    """Unit Gaussian f32 tokens [B, 1+n, C] and Gaussian f32 weights and biases of standard deviation `std`: values that are
    NOT bf16 numbers, what the reference's fp32 aggregator sees."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randn(B, 1 + n, C, generator=g)
    r = lambda *s: torch.randn(*s, generator=g) * std
    return tokens, dict(w1_sc=r(2 * hidden, C), b1_sc=r(2 * hidden), w2_s=r(m, hidden), b2_s=r(m), w2_c=r(l, hidden), b2_c=r(l),
                        w1_t=r(hidden, C), b1_t=r(hidden), w2_t=r(t, hidden), b2_t=r(t))


def e0_inputs(C: int, B: int, seed: int, n: int = 256):
    """E0, one plane: oracle.salad_stages.exact_inputs cast to f32.  Every value is a bf16 number, so m = q = 0, only the
    (h,h) segment is non-zero, and both layers are exact in f32 as they are on the bf16 path (its grids and limits)."""
    tokens, w = ost.exact_inputs(C, B, seed, n=n)
    return tokens.float(), {k: v.float() for k, v in w.items()}


def _three_plane(g, *shape):
    """+-{1, 1 + 2^-9, 1 + 2^-9 + 2^-18}: h = +-1, m = 0 or +-2^-9, q = 0 or +-2^-18."""
    kind = torch.randint(0, 3, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    v = sign * (1 + (kind >= 1) * 2.0 ** -9 + (kind >= 2) * 2.0 ** -18)
    assert torch.equal(v.float().double(), v)
    return v.float()


def _sparse_rows(g, rows: int, K: int, nnz: int = NNZ):
    """[rows, K] f32: at most `nnz` non-zeros per row, from the three-plane values."""
    keep = torch.zeros(rows, K, dtype=torch.bool)
    keep.scatter_(1, torch.rand(rows, K, generator=g).argsort(dim=1)[:, :min(nnz, K)], True)
    return _three_plane(g, rows, K) * keep


def e1_inputs(C: int, B: int, seed: int, n: int = 256, hidden: int = 512, m: int = 64, l: int = 128, t: int = 256):
    """E1, three planes, layer 1: dense three-plane tokens, first-layer rows of at most 48 three-plane non-zeros, b1 a
    multiple of 1/8 in [-2, 2].  Every kept product is a multiple of 2^-18 and sum|terms| + |b1| <= 48 (1 + 2^-8)^2 + 2 < 64,
    so H and Ht are exact in f32 in any order.  The second layers are those of E0 (bf16 numbers): S, F and g are finite
    but not exact, and this family does not judge them."""
    g = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    tokens = _three_plane(g, B, 1 + n, C)
    return tokens, dict(w1_sc=_sparse_rows(g, 2 * hidden, C), b1_sc=ints(-16, 16, 2 * hidden) / 8,
                        w1_t=_sparse_rows(g, hidden, C), b1_t=ints(-16, 16, hidden) / 8,
                        w2_s=ints(-2, 2, m, hidden) / 8, b2_s=ints(-64, 64, m) / 64, w2_c=ints(-2, 2, l, hidden) / 8,
                        b2_c=ints(-64, 64, l) / 64, w2_t=ints(-2, 2, t, hidden) / 8, b2_t=ints(-64, 64, t) / 64)


def e2_inputs(C: int, B: int, seed: int, n: int = 256, hidden: int = 512, m: int = 64, l: int = 128, t: int = 256):
    """E2, three planes, layer 2: W1 is a signed selection matrix (one +-1 per row) and b1 = 0, so H is exactly relu(+-x) on
    three-plane token values; second-layer rows of at most 48 three-plane non-zeros of `hidden`, b2 a multiple of 1/64 in
    [-1, 1]: sum|terms| + |b2| <= 48 (1 + 2^-8)^2 + 1 < 64 on the 2^-18 grid: S, F and g are exact in f32 in any order."""
    g = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()

    def selection(rows):
        w = torch.zeros(rows, C)
        w[torch.arange(rows), torch.randint(0, C, (rows,), generator=g)] = torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1
        return w

    tokens = _three_plane(g, B, 1 + n, C)
    return tokens, dict(w1_sc=selection(2 * hidden), b1_sc=torch.zeros(2 * hidden), w1_t=selection(hidden), b1_t=torch.zeros(hidden),
                        w2_s=_sparse_rows(g, m, hidden), b2_s=ints(-64, 64, m) / 64, w2_c=_sparse_rows(g, l, hidden),
                        b2_c=ints(-64, 64, l) / 64, w2_t=_sparse_rows(g, t, hidden), b2_t=ints(-64, 64, t) / 64)


FAMILIES = {"E0": (e0_inputs, ("H", "Ht", "S", "F", "g")), "E1": (e1_inputs, ("H", "Ht")), "E2": (e2_inputs, ("H", "Ht", "S", "F", "g"))}


@functools.lru_cache(maxsize=None)
def exact_case(family: str, C: int, B: int, n: int = 256):
    """(tokens, w, plane model) of one exact case, computed once per shape and shared (read-only)."""
    tokens, w = FAMILIES[family][0](C, B, seed=1000 * C + 10 * B + n + len(family) + int(family[1]), n=n)
    return tokens, w, f32_stage_outputs(tokens, w)


def rounding_cases(scales=(1.0, 2.0 ** -56, 2.0 ** 58, 2.0 ** -7, 2.0 ** 20)) -> torch.Tensor:
    """f32 values chosen for the two roundings of split3, each times every power of two in `scales` (the default keeps
    magnitudes in [2^-60, 2^60], where every plane is a normal bf16 number or zero): exact ties at the first rounding with an
    even and an odd kept mantissa, the same at the second rounding, residuals of both signs, powers of two, values whose m
    or q plane is zero, and +-0.  A multiple of 4 values."""
    base = [1.0, 1 + 2.0 ** -7, 3.0, 1.5,                                     # bf16 numbers: m = q = 0
            1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8,                         # ties at the first rounding: even below / odd below
            1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,           # just off the tie, either side
            1 + 2.0 ** -9, 1 + 2.0 ** -7 - 2.0 ** -9,                         # positive / negative first residual, q = 0
            1 + 2.0 ** -9 + 2.0 ** -17, 1 + 2.0 ** -9 + 2.0 ** -16 + 2.0 ** -17,    # ties at the second rounding, both parities
            1 - 2.0 ** -10 - 2.0 ** -18 - 2.0 ** -19,                         # below a power of two: finer grid, negative residuals
            1 + 2.0 ** -9 + 2.0 ** -18, 1 + 2.0 ** -23, 2 - 2.0 ** -23, 1 + 2.0 ** -18,   # all three planes; m tiny, q = 0; all ones; m = 2^-18
            1 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23, 0.1, 1 / 3, 2 / 3, 0.7]
    v = torch.tensor(base, dtype=torch.float64)
    assert torch.equal(v.float().double()[:18], v[:18])
    v = v.float()
    scaled = torch.cat([v * s for s in scales])
    zeros = torch.tensor([0.0, -0.0, 0.0, -0.0])
    out = torch.cat([scaled, -scaled, zeros])
    out = torch.cat([out, torch.ones((-out.numel()) % 4)])
    return out
