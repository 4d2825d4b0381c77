"""f64 multi-head self-attention — TEST ORACLE of vpr_attention_qkv_bf16 / vpr_attention_qkv_split_bf16.

out[b, t, h*64 + d] = sum_k softmax_k(q[b,t,h] . k[b,k,h] * scale) v[b,k,h,d], non-causal, no mask, over the fused
projection output qkv [B, T, 3, H, 64] (flattened to [B, T, 3*H*64]).  Every operand is taken exactly (bf16 -> f64)
and the softmax is stabilised by the row max, so the result is the exact attention of the given values to f64
precision whatever constant a query's logits are shifted by.
"""
import torch

HEAD_DIM = 64


def attention_f64(qkv: torch.Tensor, heads: int, scale: float = 0.125) -> torch.Tensor:
    """qkv [B, T, 3*H*64] (any float dtype) -> [B, T, H*64] f64."""
    B, T, C3 = qkv.shape
    if C3 != 3 * heads * HEAD_DIM:
        raise ValueError("attention_f64: qkv must be [B, T, 3*H*64]")
    q, k, v = qkv.to(torch.float64).reshape(B, T, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)   # [B, H, T, 64] each
    s = q @ k.transpose(-1, -2) * scale
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    out = (p @ v) / p.sum(dim=-1, keepdim=True)
    return out.transpose(1, 2).reshape(B, T, heads * HEAD_DIM)


def split_row_index(B: int, T: int, body_tokens: int) -> torch.Tensor:
    """[B, T] int64: the row of token t of image b in the split layout — row b*body + t for t < body, else row
    B*body + b*(T - body) + (t - body) (the layout of ops.attention_qkv_split_bf16)."""
    if not 0 <= body_tokens <= T:
        raise ValueError("split_row_index: need 0 <= body_tokens <= T")
    b = torch.arange(B).unsqueeze(1)
    t = torch.arange(T).unsqueeze(0)
    tail = T - body_tokens
    return torch.where(t < body_tokens, b * body_tokens + t, B * body_tokens + b * tail + (t - body_tokens))


def to_split_rows(x: torch.Tensor, body_tokens: int) -> torch.Tensor:
    """Token-ordered [B, T, F] -> split-layout rows [B*T, F]."""
    B, T = x.shape[:2]
    rows = torch.empty((B * T,) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    rows[split_row_index(B, T, body_tokens).reshape(-1).to(x.device)] = x.reshape((B * T,) + tuple(x.shape[2:]))
    return rows


def from_split_rows(rows: torch.Tensor, B: int, T: int, body_tokens: int) -> torch.Tensor:
    """Split-layout rows [B*T, F] -> token-ordered [B, T, F]."""
    return rows[split_row_index(B, T, body_tokens).to(rows.device)]


# ---- per-element error bound of the HIP attention kernel (tests/test_attention_edges_gpu.py states the model) ----
U_BF16 = 2.0 ** -8                    # bf16 unit roundoff
SCALE = 0.125
GATE = 2e-2                           # the project's absolute gate on attention outputs (randn-scale V)


def half_ulp(x: torch.Tensor) -> torch.Tensor:
    """Half the bf16 spacing at |x| (the most one RNE rounding to bf16 can move x), at least at the smallest normal."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.clamp_min(2.0 ** -126)).exponent - 9)


def bound(qkv: torch.Tensor, H: int, scale: float = SCALE, terms: int = 288, gate: float = GATE):
    """(bound, exact output), both [B, T, H*64] f64, of attention on qkv [B, T, 3*H*64]: p_k rounded once to bf16
    (u / (1 - u) · Σ_k w_k |v_kd - o_d|), f32 logits ((e^2ε - 1) · the same sum), `terms` f32 additions in the row sum
    and P·V (the kernel pads every sequence to 288 keys), one bf16 rounding of the output; never above `gate`."""
    B, T, _ = qkv.shape
    q, k, v = qkv.double().reshape(B, T, 3, H, HEAD_DIM).permute(2, 0, 3, 1, 4)   # [B, H, T, 64]
    s = q @ k.transpose(-1, -2) * scale
    w = torch.softmax(s, dim=-1)                                                  # stable in f64
    o = w @ v
    mad = torch.empty_like(o)                                                     # Σ_k w_k |v_kd - o_d|
    for i in range(0, T, 32):
        mad[:, :, i:i + 32] = (w[:, :, i:i + 32, :, None] * (v[:, :, None] - o[:, :, i:i + 32, None]).abs()).sum(3)
    dot_abs = (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True)  # max_k Σ_d |q_d k_d|
    eps = 2 * 64 * 2.0 ** -24 * scale * dot_abs + 2.0 ** -22
    vmax = v.abs().amax(dim=2, keepdim=True)                                      # [B, H, 1, 64]
    pre = (U_BF16 / (1 - U_BF16) + torch.expm1(2 * eps)) * mad + 2 * terms * 2.0 ** -24 * vmax
    bnd = pre + half_ulp(o.abs() + pre)
    if gate is not None:
        bnd = bnd.clamp_max(gate)
    to_tok = lambda t: t.transpose(1, 2).reshape(B, T, H * HEAD_DIM)
    return to_tok(bnd), to_tok(o)
