"""Backbone attention kernel (vpr_attention_qkv_bf16 / _split_bf16) against the f64 oracle (oracle/attention.py) at
the numeric edges: every real logit of a query far below (or above) 0, every T class of the 288-key padding, the
split row layout, the tuning variants and the refusals.

Error model of the kernel, per output element (b, t, h, d), with o the exact output and w_k the exact softmax
weights of query t:
  * each p_k is rounded once to bf16 before the row sum and P·V (relative error <= u = 2^-8); the weights the
    kernel effectively uses are p_k (1 + δ_k) / Σ p_j (1 + δ_j), which moves the output by at most
    u / (1 - u) · Σ_k w_k |v_kd - o_d|;
  * the logits come out of an f32 accumulation of 64 exact bf16 products (relative error of a logit difference
    <= 2 · 64 · 2^-24 · scale · max_k Σ_d |q_d k_d|, plus 2^-22 for exp2), which moves the output by
    (e^ε - 1) · Σ_k w_k |v_kd - o_d| in the same way;
  * the row sum and P·V accumulate up to 288 terms in f32: 2 · 288 · 2^-24 · max_k |v_kd|;
  * the output is rounded once to bf16: half the bf16 spacing at |o_d| + the error above (<= u · that value).
Nothing in the bound depends on the constant the logits of a query are shifted by, so the same bound holds at every
shift.  The assertion takes the smaller of this bound and the 2e-2 absolute gate of
test_heads_gpu.test_attention_matches_f64_reference (V here ~ randn, there 1.5 randn): never looser than that gate;
most elements are held to a few 1e-3.
"""
import math

import pytest
import torch

from oracle import attention as oattn

pytestmark = pytest.mark.gpu

SCALE, GATE = oattn.SCALE, oattn.GATE  # GATE: the absolute gate of the existing randn attention test
_bound = oattn.bound                  # the error model above, shared with the backbone stage tests
C_SWEEP = (-200.0, -96.0, -40.0, -24.0, -16.0, -12.0, -8.0, 0.0, 8.0, 40.0, 200.0)   # all exact in bf16
T_SWEEP = (1, 2, 15, 16, 17, 31, 33, 100, 255, 256, 257, 287, 288)


def _forced_qkv(B, T, H, c, seed, v_scale=1.0):
    """qkv [B, T, 3*H*64] bf16 whose head dimension 63 is 8 in every key and c[b, t, h] in query (b, t, h): that adds
    exactly c to every logit of that query (8 c / 8), on top of the ~N(0, 2.2) logits of the other 63 dims."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 3, H, 64, generator=g) * 1.5
    x[:, :, 2] = torch.randn(B, T, H, 64, generator=g) * v_scale
    x[:, :, 1, :, 63] = 8.0
    x[:, :, 0, :, 63] = torch.as_tensor(c, dtype=torch.float32).expand(B, T, H)
    return x.to(torch.bfloat16).reshape(B, T, 3 * H * 64)


def _mixed_offsets(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(C_SWEEP)[torch.randint(0, len(C_SWEEP), (B, T, H), generator=g)]


def _check(out, qkv, H, what):
    bound, ref = _bound(qkv, H)
    assert torch.allclose(ref, oattn.attention_f64(qkv, H), rtol=0, atol=1e-12)
    out = out.cpu().double()
    assert torch.isfinite(out).all(), f"{what}: non-finite outputs"
    err = (out - ref).abs()
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"{what}: max err {err.max().item():.3e}, worst err/bound {ratio:.3f}"
    return err.max().item(), bound.max().item()


@pytest.mark.parametrize("c", C_SWEEP)
@pytest.mark.parametrize("T", T_SWEEP)
def test_attention_forced_logit_offset(dev, T, c):
    """Every logit of every query shifted by c: the padded keys (T < 288) must neither set the stabiliser nor
    enter the row sum."""
    from vpr_amd import ops
    B, H = 2, 3
    qkv = _forced_qkv(B, T, H, c, seed=T)
    out = ops.attention_qkv_bf16(qkv.to(dev), H)
    err, bnd = _check(out, qkv, H, f"T={T} c={c}")
    print(f"T={T} c={c}: max err {err:.2e} (bound up to {bnd:.2e})")


@pytest.mark.parametrize("T", T_SWEEP)
def test_attention_mixed_offsets_in_one_call(dev, T):
    """Different c per query and per head in one launch (B*H = 8 workgroups, every query tile of a wave)."""
    from vpr_amd import ops
    B, H = 2, 4
    qkv = _forced_qkv(B, T, H, _mixed_offsets(B, T, H, seed=100 + T), seed=200 + T)
    _check(ops.attention_qkv_bf16(qkv.to(dev), H), qkv, H, f"T={T} mixed")


@pytest.mark.parametrize("B,T,H", [(3, 257, 2), (2, 17, 3), (1, 288, 1), (4, 100, 2), (2, 1, 1)])
def test_attention_split_layout_bit_identical(dev, B, T, H):
    """The split entry point with body_tokens in {0, 1, T-1, T} == the contiguous call on the same tokens."""
    from vpr_amd import ops
    qkv = _forced_qkv(B, T, H, _mixed_offsets(B, T, H, seed=T), seed=3 * T)
    ref = ops.attention_qkv_bf16(qkv.to(dev), H).cpu()
    for body in sorted({0, 1, T - 1, T}):
        rows = oattn.to_split_rows(qkv, body).contiguous().to(dev)
        out = ops.attention_qkv_split_bf16(rows, B, T, body, H).cpu()
        assert torch.equal(oattn.from_split_rows(out, B, T, body), ref), f"body_tokens={body}"


@pytest.mark.parametrize("variant", [1, 2, 3, 20, 25])
@pytest.mark.parametrize("B,T,H", [(20, 257, 16), (3, 17, 5), (2, 288, 3), (2, 100, 2)])
def test_attention_variants_bit_identical(dev, tune, variant, B, T, H):
    """Every VPR_ATTN_VARIANT does the same arithmetic per query tile (4 / 6 / 8 waves, pipelined or not, de-phased
    start): bit-identical to the default, on logits far below 0 too.  B*H = 320 workgroups reaches the de-phased
    second-slot range of variant 25."""
    from vpr_amd import ops
    qkv = _forced_qkv(B, T, H, _mixed_offsets(B, T, H, seed=B + T), seed=B * T).to(dev)
    tune("VPR_ATTN_VARIANT", None)
    ref = ops.attention_qkv_bf16(qkv, H)
    tune("VPR_ATTN_VARIANT", variant)
    out = ops.attention_qkv_bf16(qkv, H)
    assert torch.equal(out, ref)
    _check(out, qkv.cpu(), H, f"variant {variant}")


def test_attention_refusals(dev):
    """T > 288, head_dim != 64 and a non-positive scale are refused without touching the output."""
    from vpr_amd import ops, _lib
    qkv = torch.randn(1, 289, 3 * 64, device=dev).to(torch.bfloat16)
    with pytest.raises(RuntimeError):
        ops.attention_qkv_bf16(qkv, 1)
    rows = qkv[0].contiguous()
    with pytest.raises(RuntimeError):
        ops.attention_qkv_split_bf16(rows, 1, 289, 288, 1)
    lib = _lib.lib()
    out = torch.full((1, 289, 64), 7.0, dtype=torch.bfloat16, device=dev)
    args = lambda T, hd, scale: (ops._ptr(qkv), ops._ptr(out), 1, T, 1, hd, scale, ops._stream())
    assert lib.vpr_attention_qkv_bf16(*args(289, 64, SCALE)) == -2           # VPR_ERR_UNSUPPORTED
    assert lib.vpr_attention_qkv_bf16(*args(128, 32, SCALE)) == -2
    assert lib.vpr_attention_qkv_bf16(*args(128, 128, SCALE)) == -2
    for bad in (0.0, -0.125, math.inf, math.nan):
        assert lib.vpr_attention_qkv_bf16(*args(128, 64, bad)) == -1         # VPR_ERR_INVALID_ARG
    assert lib.vpr_attention_qkv_split_bf16(ops._ptr(qkv), ops._ptr(out), 1, 289, 289, 0, 1, 64, SCALE, ops._stream()) == -2
    assert lib.vpr_attention_qkv_split_bf16(ops._ptr(qkv), ops._ptr(out), 1, 128, 128, 0, 1, 32, SCALE, ops._stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
