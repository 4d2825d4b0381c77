"""f64 LayerNorm and the per-element error bound of the backbone's LayerNorm kernels (layernorm_bf16,
add_layernorm_bf16, bias_layernorm_bf16 and the LayerNorm rows of bias_layernorm_cls_linear_bf16).

Bound per element: |y - ref| <= 2^-8 |ref| + δ.  2^-8 |ref| is one bf16 rounding of the exact value; δ is the f32
slack of the kernel's two-pass statistics: each sum runs through at most 32 in-lane and 6 cross-lane additions
(< 40 roundings), so the mean is off by at most 40 u max|v| and the centred sum of squares by 40 u relative
(u = 2^-24); the normalisation and affine step add a few roundings of |γ ẑ| and |β|:
    δ = 2 · 40 u · (|γ_j| (max_i |v_ij| / σ_i + |ẑ_ij|) + |β_j|),   σ_i = sqrt(var_i + eps), ẑ = (v - mean) / σ.
"""
import torch

EPS = 1e-6


def ref_and_bound(v, gamma, beta, eps=EPS):
    """v: [M, C] f64 (the exact values the kernel normalises) -> (layer_norm(v), bound), both [M, C] f64."""
    v, gm, bt = v.double(), gamma.double(), beta.double()
    mean = v.mean(1, keepdim=True)
    sigma = ((v - mean).pow(2).mean(1, keepdim=True) + eps).sqrt()
    z = (v - mean) / sigma
    ref = z * gm + bt
    assert torch.allclose(ref, torch.nn.functional.layer_norm(v, (v.shape[1],), gm, bt, eps), rtol=1e-12, atol=1e-12)
    delta = 2 * 40 * 2.0 ** -24 * (gm.abs() * (v.abs().amax(1, keepdim=True) / sigma + z.abs()) + bt.abs())
    return ref, 2.0 ** -8 * ref.abs() + delta
