"""CPU: train-mode SALAD (Dropout of the score / cluster MLPs active, dinov2salad_finetuning.py:34-37,115) — the mask
generator against the header's known answers, the operator's fake implementation, and the host-side refusals of
SaladAggregator.forward_train and finetune_head(TokenCache).  `salad_mask` is the numpy statement of the mask contract
in include/vpr_amd.h (vpr_salad_aggregate_train); tests/test_salad_dropout_gpu.py compares the kernel with it."""
import math
import os

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 with the Random123 constants on uint32 values held in uint64 arrays (broadcast) -> four words."""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in (c0, c1, c2, c3)]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                 # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def keep_threshold(p: float) -> int:
    return int(math.floor(p * 4294967296.0))


def salad_mask(B: int, n: int, hidden: int, p: float, seed: int, pass_index: int, image_base: int = 0) -> np.ndarray:
    """The keep mask of vpr_salad_aggregate_train: uint8 [B*n, 2*hidden] (row b*n + token, column u), 1 = kept.
    counter (u >> 2, image_base + b, token, pass), word u & 3, key (seed & 0xffffffff, seed >> 32), kept iff r >= t."""
    g = np.arange(2 * hidden // 4, dtype=np.uint64)[None, None, :]
    img = (image_base + np.arange(B, dtype=np.uint64))[:, None, None]
    tok = np.arange(n, dtype=np.uint64)[None, :, None]
    r = philox4x32_10(g, img, tok, pass_index, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack([np.broadcast_to(w, (B, n, 2 * hidden // 4)) for w in r], axis=-1)   # [B, n, u >> 2, u & 3]
    return (words >= np.uint64(keep_threshold(p))).reshape(B * n, 2 * hidden).astype(np.uint8)


def test_philox_reproduces_the_header_known_answers():
    hdr = open(os.path.join(ROOT, "include", "vpr_amd.h")).read()
    assert "6627e8d5 e169c58d bc57ac4c 9b00dbd8" in hdr and "d16cfe09 94fdcceb 5001e420 24126ea1" in hdr
    r = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in r] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    r = philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(x) for x in r] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_mask_statement_properties():
    """The numpy statement itself: rate, threshold rule at the ends, independence of the split into calls."""
    m = salad_mask(4, 256, 512, 0.3, seed=123, pass_index=2)
    assert m.shape == (1024, 1024) and m.dtype == np.uint8
    rate, N = m.mean(), m.size
    assert abs(rate - 0.7) < 6 * math.sqrt(0.21 / N)
    assert salad_mask(1, 8, 256, 0.0, 5, 0).all()                     # t = 0: every unit kept
    assert keep_threshold(0.5) == 1 << 31 and keep_threshold(0.3) == 1288490188
    both = salad_mask(3, 16, 256, 0.4, 9, 1, image_base=10)
    assert np.array_equal(both[:16], salad_mask(1, 16, 256, 0.4, 9, 1, image_base=10))
    assert np.array_equal(both[16:], salad_mask(2, 16, 256, 0.4, 9, 1, image_base=11))
    assert not np.array_equal(m, salad_mask(4, 256, 512, 0.3, seed=123, pass_index=3))


def test_library_exposes_the_train_entry_point_and_abi_6():
    from vpr_amd import _lib
    assert _lib.ABI_VERSION == 6
    assert "vpr_salad_aggregate_train" in _lib.PROTOTYPES
    hdr = open(os.path.join(ROOT, "include", "vpr_amd.h")).read()
    assert "#define VPR_AMD_ABI_VERSION 6" in hdr and "int vpr_salad_aggregate_train(" in hdr
    lib = _lib.lib()
    assert lib.vpr_abi_version() == 6
    assert lib.vpr_salad_aggregate_train.argtypes == _lib.PROTOTYPES["vpr_salad_aggregate_train"][1]


def test_library_refuses_bad_rates_without_a_gpu():
    """Argument checks come before any device work: a bad rate or image range is INVALID_ARG even with null buffers."""
    from vpr_amd import _lib
    L = _lib.lib()
    for p, base in ((-0.1, 0), (1.0, 0), (float("nan"), 0), (0.3, -1), (0.3, (1 << 32) - 1)):
        st = L.vpr_salad_aggregate_train(None, 0, None, 0, 2, 256, 1024, None, 1.0, 64, 128, 256, 512, 3, p, 1, 0, base,
                                         None, None, None, None, 0, None)
        assert st == -1, (p, base, st)


def _fake_weights(mk, C, h, f32):
    return [mk(2 * h, C), mk(2 * h, dtype=f32), mk(64, h), mk(64, dtype=f32), mk(128, h), mk(128, dtype=f32),
            mk(h, C), mk(h, dtype=f32), mk(256, h), mk(256, dtype=f32)]


def test_train_op_traces_under_fake_tensors():
    from vpr_amd import torch_ops
    assert "salad_aggregate_train" in torch_ops.OPS
    assert str(torch.ops.vpr.salad_aggregate_train.default._schema).startswith("vpr::salad_aggregate_train(")
    with FakeTensorMode():
        bf, f32 = torch.bfloat16, torch.float32
        mk = lambda *s, dtype=bf: torch.empty(*s, dtype=dtype, device="cuda")
        w = _fake_weights(mk, 1024, 512, f32)
        d, d16 = torch.ops.vpr.salad_aggregate_train(mk(4, 257, 1024), None, w, 1.0, 3, 0.3, -5, 7, 128)
        assert d.shape == d16.shape == (4, 8448) and d.dtype == f32 and d16.dtype == bf and d.device.type == "cuda"
        d, d16 = torch.ops.vpr.salad_aggregate_train(mk(3, 256, 1024), mk(3, 1024), w, 0.7, 3, 0.0, 1 << 40, 0, 0)
        assert d.shape == (3, 8448) and d16.dtype == bf


def test_forward_train_refuses_unequal_rates():
    """The fused kernel draws one rate for both MLPs: unequal p is refused before anything is packed or launched."""
    from vpr_amd.backbone import SplitTokens
    from vpr_amd.modules import SaladAggregator
    assert SaladAggregator(256).dropout_p() == pytest.approx(0.3)
    agg2 = SaladAggregator(256)
    agg2.cluster_features[1].p = 0.2
    with pytest.raises(ValueError, match="differ"):
        agg2.forward_train(torch.zeros(1, 257, 256, dtype=torch.bfloat16), seed=1, pass_index=0)
    with pytest.raises(ValueError, match="differ"):
        agg2.forward_train(SplitTokens(torch.zeros(1, 256, 256, dtype=torch.bfloat16), torch.zeros(1, 256, dtype=torch.bfloat16)),
                           seed=1, pass_index=0)


def test_forward_keeps_eval_arithmetic_and_points_to_forward_train():
    from vpr_amd.modules import SaladAggregator
    doc = SaladAggregator.forward.__doc__
    assert "forward_train" in doc and ".training" in doc


def test_finetune_head_refuses_a_cpu_token_cache():
    from vpr_amd.finetune import TokenCache, finetune_head
    from vpr_amd.modules import DINOv2RegressionModel, SaladAggregator
    agg = SaladAggregator(256)
    cache = TokenCache(torch.zeros(4, 256, 256, dtype=torch.bfloat16), torch.zeros(4, 256, dtype=torch.bfloat16), agg)
    model = DINOv2RegressionModel(agg)
    labels = np.random.default_rng(0).normal(size=(4, 2))
    for engine in ("hip", "torch"):
        with pytest.raises(RuntimeError, match="TokenCache .*GPU"):
            finetune_head(model, cache, labels, epochs=1, engine=engine, log=lambda s: None)


def test_token_cache_checks_its_layout():
    from vpr_amd.finetune import TokenCache
    with pytest.raises(ValueError, match=r"\[N, n, C\]"):
        TokenCache(torch.zeros(4, 256, 256, dtype=torch.bfloat16), torch.zeros(3, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16"):
        TokenCache(torch.zeros(4, 256, 256), torch.zeros(4, 256))
    c = TokenCache(torch.zeros(4, 256, 256, dtype=torch.bfloat16), torch.zeros(4, 256, dtype=torch.bfloat16))
    assert len(c) == 4 and not c.is_cuda


def test_default_salad_seed_is_distinct_from_the_head_seed():
    from vpr_amd.finetune import default_dropout_seed, default_salad_dropout_seed
    for s in (0, 1, 12345):
        a, b = default_salad_dropout_seed(s), default_dropout_seed(s)
        assert 0 <= a < 1 << 64 and a != b
        assert a == default_salad_dropout_seed(s)
    assert default_salad_dropout_seed(0) != default_salad_dropout_seed(1)
