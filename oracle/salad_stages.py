"""Stage-level oracle of SALAD's three MLPs: what stages T and M leave in the workspace (the hidden activations H, the
partial-sum slabs of the cluster scores S and features F, the token features g), in f64; inputs for which f32 arithmetic
is exact in ANY summation order, so that a kernel must reproduce the f64 result bit for bit; and, for ordinary random
inputs, the per-element error a correct f32-accumulating kernel can show.

Nothing here looks at a kernel: tests/test_oracle_selfchecks.py asserts every property the GPU tests rely on
(exactness under a permuted K order and a slab split, the magnitude bound, the share of active units, the share of hidden
values the bf16 rounding changes and the ties among them) on this file alone.
"""
import torch

from .salad import bf16_round

SLAB = 256                  # hidden columns per partial-sum slab of the fused route (one 256 x 256 tile of layer 1)
U32 = 2.0 ** -24            # unit roundoff of f32

# Granularities of exact_inputs (all powers of two, every value a small integer multiple):
#   x  integers in [-3, 3]                w1  multiples of 1/64 in [-1/4, 1/4]      b1  multiples of 1/8  in [-2, 2]
#   w2 multiples of 1/8 in [-1/4, 1/4]    b2  multiples of 1/64 in [-1, 1]
# so z = x w1 + b1 is a multiple of Q1 = 1/64 with |z| <= 0.75 C + 2, h = bf16(relu(z)) is a multiple of 1/64 (rounding to 8
# significant bits keeps the grid), and every partial sum of layer 2 is a multiple of Q2 = 1/512.  A multiple of q below
# 2^24 q in magnitude is an f32 number, and so is every partial sum on the way: no addition rounds, whatever the order.
# bf16 keeps 8 significant bits: on the 1/64 grid every z >= 4 with an odd multiple is changed, [4, 8) by an exact tie.
Q1, Q2 = 1.0 / 64, 1.0 / 512
EXACT_LIMIT_1, EXACT_LIMIT_2 = 2.0 ** 24 * Q1, 2.0 ** 24 * Q2          # 2^18 and 2^15


def exact_inputs(C: int, B: int, seed: int, hidden: int = 512, m: int = 64, l: int = 128, t: int = 256, n: int = 256):
    """-> (tokens bf16 [B, 1+n, C], weights dict in the kernel format: bf16 matrices, f32 biases), on the grids above."""
    g = torch.Generator().manual_seed(seed)
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32)
    tokens = ints(-3, 3, B, 1 + n, C).to(torch.bfloat16)
    w1 = lambda *s: (ints(-16, 16, *s) / 64).to(torch.bfloat16)
    w2 = lambda *s: (ints(-2, 2, *s) / 8).to(torch.bfloat16)
    b1 = lambda *s: ints(-16, 16, *s) / 8
    b2 = lambda *s: ints(-64, 64, *s) / 64
    w = dict(w1_sc=w1(2 * hidden, C), b1_sc=b1(2 * hidden), w2_s=w2(m, hidden), b2_s=b2(m), w2_c=w2(l, hidden), b2_c=b2(l),
             w1_t=w1(hidden, C), b1_t=b1(hidden), w2_t=w2(t, hidden), b2_t=b2(t))
    return tokens, w


def gaussian_inputs(C: int, B: int, seed: int, std: float = 0.02, hidden: int = 512, m: int = 64, l: int = 128, t: int = 256):
    """Unit Gaussian bf16 tokens [B, 257, C] and the Gaussian weights of tests/test_salad_gpu.py (bf16 matrices, f32 biases,
    all of standard deviation `std`)."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randn(B, 257, C, generator=g).to(torch.bfloat16)
    r = lambda *s: torch.randn(*s, generator=g) * std
    w = dict(w1_sc=r(2 * hidden, C), b1_sc=r(2 * hidden), w2_s=r(m, hidden), b2_s=r(m), w2_c=r(l, hidden), b2_c=r(l),
             w1_t=r(hidden, C), b1_t=r(hidden), w2_t=r(t, hidden), b2_t=r(t))
    return tokens, {k: v.to(torch.bfloat16) if k.startswith("w") else v for k, v in w.items()}


def pre_activations(tokens, w, dtype=torch.float64):
    """-> (z_sc [B*n, 2*hidden], z_t [B, hidden]): layer 1 before the ReLU."""
    x = tokens[:, 1:, :].to(dtype).reshape(-1, tokens.shape[2])
    cls = tokens[:, 0, :].to(dtype)
    return x @ w["w1_sc"].to(dtype).T + w["b1_sc"].to(dtype), cls @ w["w1_t"].to(dtype).T + w["b1_t"].to(dtype)


def hidden_from(z, keep=None, scale: float = 1.0, quantize: bool = True):
    """relu(z), dropout (kept * scale, else 0) and then the ONE rounding to bf16 — the order of the fused epilogue."""
    h = torch.relu(z)
    if keep is not None:
        h = torch.where(keep.to(torch.bool), h * scale, torch.zeros_like(h))
    return bf16_round(h) if quantize else h


def salad_stage_outputs(tokens, w, keep=None, scale: float = 1.0, quantize: bool = True, dtype=torch.float64):
    """f64 statement of the workspace after stages T and M.  keep (uint8 / bool [B*n, 2*hidden], optional) and scale: the
    train form's dropout mask and 1 / (1 - p).  -> dict:
      H [B*n, 2*hidden], Ht [B, hidden]   hidden activations (bf16 values when quantize)
      S [slabs, B*n, m], F [slabs, B*n, l] partial sums over 256 hidden columns each, slab 0 with the bias
      g [B, t]
    The slabs of S / F summed give oracle.salad.salad_mlps' scores / feats."""
    W = {k: v.to(dtype) for k, v in w.items()}
    hidden = W["w2_s"].shape[1]
    z, zt = pre_activations(tokens, w, dtype)
    H, Ht = hidden_from(z, keep, scale, quantize), hidden_from(zt, None, 1.0, quantize)

    def slabs(h, w2, b2):
        parts = [h[:, k:k + SLAB] @ w2[:, k:k + SLAB].T for k in range(0, hidden, SLAB)]
        parts[0] = parts[0] + b2
        return torch.stack(parts)

    return dict(H=H, Ht=Ht, S=slabs(H[:, :hidden], W["w2_s"], W["b2_s"]), F=slabs(H[:, hidden:], W["w2_c"], W["b2_c"]),
                g=Ht @ W["w2_t"].T + W["b2_t"])


MUTATIONS = ("drop_b2_s", "swap_token_rows", "zero_w2_column", "skip_bf16_round")


def mutated_scores(tokens, w, kind: str, dtype=torch.float64):
    """Cluster scores [B*n, m] (slabs summed) as a subtly wrong kernel would leave them — the mistakes a descriptor-level
    tolerance cannot see: the second-layer bias left out, the last two token rows of the batch exchanged, one hidden
    unit's W2 column read as zero, the hidden values not rounded to bf16."""
    if kind == "drop_b2_s":
        return salad_stage_outputs(tokens, dict(w, b2_s=torch.zeros_like(w["b2_s"])), dtype=dtype)["S"].sum(0)
    if kind == "swap_token_rows":
        S = salad_stage_outputs(tokens, w, dtype=dtype)["S"].sum(0)
        idx = torch.arange(S.shape[0])
        idx[-1], idx[-2] = idx[-2].clone(), idx[-1].clone()
        return S[idx]
    if kind == "zero_w2_column":
        w2 = w["w2_s"].clone()
        w2[:, w2.shape[1] // 2 + 3] = 0
        return salad_stage_outputs(tokens, dict(w, w2_s=w2), dtype=dtype)["S"].sum(0)
    if kind == "skip_bf16_round":
        return salad_stage_outputs(tokens, w, quantize=False, dtype=dtype)["S"].sum(0)
    raise ValueError(kind)


def salad_mlps_f32(tokens, w):
    """The same two layers in plain torch f32 on the CPU (bf16 round of the hidden values): the yardstick of the RMS test —
    what an ordinary f32 implementation loses against f64.  -> scores [B*n, m], feats [B*n, l], tokfeat [B, t], all f32."""
    f = torch.float32
    W = {k: v.to(f) for k, v in w.items()}
    hidden = W["w2_s"].shape[1]
    z, zt = pre_activations(tokens, w, f)
    H, Ht = hidden_from(z), hidden_from(zt)
    return (H[:, :hidden] @ W["w2_s"].T + W["b2_s"], H[:, hidden:] @ W["w2_c"].T + W["b2_c"], Ht @ W["w2_t"].T + W["b2_t"])


def _head_bound(x, w1, b1, w2, b2):
    """Per-element bound of one two-layer head for a kernel that accumulates both layers in f32 in some order and rounds the
    hidden values to bf16 once.  Sources of difference from the f64 oracle, and nothing else:
      layer 1   |z_f32 - z| <= eps_z = (K + 1) u (sum |x||w1| + |b1|)   (K products and a bias, worst case of any order),
                so the hidden value is bf16(relu(z')) for some z' within eps_z of z: between h_lo and h_hi, the roundings
                of the two ends (f64 -> f32 -> bf16 and relu are monotone);
      layer 2   (hidden + 2) u (sum |h||w2| + |b2|): the products, the bias, the slab sum.
    -> sum_k |w2_ok| (h_hi - h_lo)_k + (hidden + 2) u (sum_k h_hi_k |w2_ok| + |b2_o|),  [rows, n_out] f64."""
    d = torch.float64
    x, w1, b1, w2, b2 = (v.to(d) for v in (x, w1, b1, w2, b2))
    K, hidden = w1.shape[1], w2.shape[1]
    z = x @ w1.T + b1
    eps_z = (K + 1) * U32 * (x.abs() @ w1.abs().T + b1.abs())
    h_lo, h_hi = bf16_round(torch.relu(z - eps_z)), bf16_round(torch.relu(z + eps_z))
    return (h_hi - h_lo) @ w2.abs().T + (hidden + 2) * U32 * (h_hi @ w2.abs().T + b2.abs())


def stage_error_bounds(tokens, w):
    """-> (bound_S [B*n, m], bound_F [B*n, l], bound_g [B, t]) f64: |kernel - salad_stage_outputs (slabs summed)| may not
    exceed these on any element.  Computed from the inputs alone; loose (every rounding at its worst at once)."""
    C = tokens.shape[2]
    hidden = w["w2_s"].shape[1]
    x, cls = tokens[:, 1:, :].reshape(-1, C), tokens[:, 0, :]
    return (_head_bound(x, w["w1_sc"][:hidden], w["b1_sc"][:hidden], w["w2_s"], w["b2_s"]),
            _head_bound(x, w["w1_sc"][hidden:], w["b1_sc"][hidden:], w["w2_c"], w["b2_c"]),
            _head_bound(cls, w["w1_t"], w["b1_t"], w["w2_t"], w["b2_t"]))
