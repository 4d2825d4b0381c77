"""GPU: every launch of a backbone forward judged per element against f64, in every mode (oracle/backbone.py: the stage
references, bounds and wiring checks; tests/backbone_trace.py: the capturing recorder).  The whole-forward comparisons
judge the final tokens by an RMS criterion that a wrong LayerNorm, a bias row off by half a block or a second rounding
passes; here each launch is held to the bound of that one launch, anchored on its own captured input, and the operands
between the launches are compared bit for bit.

Model: tests/backbone_trace.py make_model — vit_small cut to 3 blocks (vit_large to 2), every parameter away from its
init value, no two blocks alike.  The f64 references run on the CPU over at most ~1100 rows.

Measured allowances for what the LIBRARY computes on the patch rows (never for the project's kernels): see ALLOW."""
import pytest
import torch

import backbone_trace as bt
from oracle import backbone as ob

pytestmark = pytest.mark.gpu

# keyword switches of oracle.backbone.check_trace (its docstring): none needed — the library GEMM with beta = 1 rounds once,
# its tanh-GELU epilogue and the in-place erf-GELU stay within 16 u (|z| + 1), SDPA at T = 530 within the derived bound
ALLOW = {}

_MODELS = {}


def _model(dev, arch, img_size, L):
    key = (arch, img_size, L)
    if key not in _MODELS:
        m = bt.make_model(arch, img_size, L)
        _MODELS[key] = (m.to(dev), ob.Params(m))
    return _MODELS[key]


def _fused_rows_equal_plain_launch(dev, tr):
    """The all-rows output of every fused launch is bit-equal to ops.bias_layernorm_bf16 on the same captured input."""
    from vpr_amd import ops
    count = 0
    for s in tr.stages:
        if s.label == "bias_layernorm_cls_linear_bf16":
            y = ops.bias_layernorm_bf16(s.inp["x"].to(dev), s.inp["c"].to(dev), s.ref["gamma"], s.ref["beta"], s.scalars["eps"])
            assert torch.equal(y.cpu(), s.out["h"]), (s.block, s.stage)
            count += 1
    return count


def _run(dev, monkeypatch, arch, img_size, L, B, mode, gelu="tanh"):
    m, p = _model(dev, arch, img_size, L)
    x = bt.make_image(B, img_size).to(dev)
    tr = bt.trace(m, x, mode, monkeypatch, gelu)
    worst = ob.check_trace(tr, p, mode, gelu, **ALLOW)
    print(f"{arch} {img_size} px B={B} {mode} {gelu}: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(v for k, v in worst.items() if k != "attention.sdpa_vs_derived") <= 1.0
    if mode in ob.SPLIT_MODES:              # the cls rows of the raw-token buffer are still zero after the forward
        from vpr_amd import ops
        M = B * (1 + m.num_patches)
        assert not bool(ops.zero_rows_bf16(M, m.embed_dim, dev)[B * m.num_patches:].any())
    return tr


@pytest.mark.parametrize("mode", ob.MODES)
def test_stages_at_224_tanh(dev, monkeypatch, mode):
    """B = 2; the split row layout at 224 px, the cls-first layout at 196 px (W % 8 != 0), as in the schedule test."""
    tr = _run(dev, monkeypatch, "vit_small", 196 if mode in ob.CLS_FIRST_MODES else 224, 3, 2, mode)
    assert _fused_rows_equal_plain_launch(dev, tr) == (5 if mode == "fused" else 0)


@pytest.mark.parametrize("mode", ["split_side", "cf_resid", "fused"])
def test_stages_erf(dev, monkeypatch, mode):
    """gelu = "erf": the cls rows' skinny mode 4, the patch rows' biased GEMM + in-place erf-GELU; fuse_ln_cls has the tanh
    form only and must fall back to the unfused launches (the schedule the recorded calls are checked against)."""
    tr = _run(dev, monkeypatch, "vit_small", 196 if mode == "cf_resid" else 224, 3, 2, mode, gelu="erf")
    labels = {s.label for s in tr.stages}
    assert "gelu_" in labels and "bias_layernorm_cls_linear_bf16" not in labels and "_addmm_activation" not in labels
    assert ("skinny:4" in labels) == (mode != "cf_resid")


@pytest.mark.parametrize("mode", ["split_side", "fused"])
@pytest.mark.parametrize("B", [1, 3])
def test_stages_at_168(dev, monkeypatch, B, mode):
    """n = 144, T = 145: one cls row, an odd row count, a ragged last attention tile."""
    _run(dev, monkeypatch, "vit_small", 168, 3, B, mode)


def test_stages_at_322_sdpa(dev, monkeypatch):
    """T = 530: beyond the HIP attention kernel, the cls-first path with library attention."""
    tr = _run(dev, monkeypatch, "vit_small", 322, 3, 2, "cf_resid")
    assert [s.label for s in tr.stages if s.stage == "attention"] == ["sdpa"] * 3


@pytest.mark.parametrize("mode", ["split_side", "fused"])
def test_stages_vit_large(dev, monkeypatch, mode):
    """C = 1024: two LayerNorm chunks per lane, skinny with 8 waves (K = 1024) and 16 waves (K = 4096)."""
    _run(dev, monkeypatch, "vit_large", 168, 2, 2, mode)


@pytest.mark.parametrize("mode", ob.SPLIT_MODES)
def test_stages_repeat_bit_for_bit(dev, monkeypatch, mode):
    """The cached constants, the zero-row buffer and the workspaces are re-used: after a forward at another batch size the
    same forward leaves the same stage records, bit for bit."""
    m, _ = _model(dev, "vit_small", 168, 3)
    x = bt.make_image(2, 168).to(dev)
    first = bt.trace(m, x, mode, monkeypatch)
    m(bt.make_image(3, 168, seed=1).to(dev), split=True)
    again = bt.trace(m, x, mode, monkeypatch)
    assert [s.key() for s in first.stages] == [s.key() for s in again.stages]
    for a, b in zip(first.stages, again.stages):
        for kind in ("inp", "out"):
            da, db = getattr(a, kind), getattr(b, kind)
            assert da.keys() == db.keys()
            for name in da:
                assert ob._same(da[name], db[name]), (a.key(), kind, name)
    for a, b in zip(first.result, again.result):
        assert ob._same(a, b)
