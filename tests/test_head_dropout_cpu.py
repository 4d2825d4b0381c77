"""CPU: the dropout mask of the HIP head-training step (vpr_head_train_step_dropout / vpr_head_train_epoch_dropout,
include/vpr_amd.h) restated in numpy — Philox4x32-10 with the Random123 constants, checked against Random123's known-answer
vectors — plus what can be checked without a device: the library refuses a bad dropout rate before touching the GPU, the
operator is registered with its fake implementation, and the PyTorch engine still trains a Dropout head.

The reference trains Linear(H, 512) -> ReLU -> Dropout(0.3) -> Linear(512, 2) in model.train() mode:
dinov2salad/dinov2salad_finetuning_2.py:113-122, swin_transformer/swin_attempt_2.py:114-123."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [..., 4] (uint32 values), key (k0, k1) -> [..., 4] uint32: ten Philox rounds, key bumped between rounds."""
    c = np.asarray(counter, dtype=np.uint64)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _LO, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def dropout_threshold(p: float) -> int:
    return int(math.floor(float(p) * 4294967296.0))


def dropout_mask(seed: int, step: int, B: int, hidden: int, p: float, b0: int = 0) -> np.ndarray:
    """bool [B, hidden]: unit j of batch position b (b0 .. b0+B-1) kept at `step` — word j & 3 of Philox4x32-10 at counter
    (j >> 2, b, step, 0) under key (seed low 32 bits, seed high 32 bits), kept iff it is >= floor(p * 2^32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(hidden)
    b = np.arange(b0, b0 + B)
    ctr = np.zeros((B, hidden, 4), dtype=np.uint64)
    ctr[..., 0] = (j >> 2)[None, :]
    ctr[..., 1] = b[:, None]
    ctr[..., 2] = step
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    r = np.take_along_axis(words, np.broadcast_to((j & 3)[None, :, None], (B, hidden, 1)), axis=-1)[..., 0]
    return r >= np.uint32(dropout_threshold(p))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    got = philox4x32_10(np.zeros(4, dtype=np.uint64), (0, 0))
    assert [f"{w:08x}" for w in got] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    got = philox4x32_10(np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], dtype=np.uint64), (0xA4093822, 0x299F31D0))
    assert [f"{w:08x}" for w in got] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_keep_rate_and_threshold():
    p = 0.3
    keep = dropout_mask(0x0123456789ABCDEF, 7, 1000, 1000, p)          # 10^6 draws
    n = keep.size
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(keep.mean() - (1 - p)) <= 5 * sigma, keep.mean()
    assert dropout_threshold(0.0) == 0 and dropout_mask(5, 1, 4, 64, 0.0).all()
    assert dropout_threshold(0.5) == 1 << 31
    assert dropout_threshold(np.nextafter(1.0, 0.0)) == (1 << 32) - 1


def test_masks_differ_across_step_batch_position_and_seed():
    base = dropout_mask(11, 3, 16, 512, 0.3)
    assert not np.array_equal(base, dropout_mask(11, 4, 16, 512, 0.3))                 # step
    assert not np.array_equal(base, dropout_mask(12, 3, 16, 512, 0.3))                 # seed (low word)
    assert not np.array_equal(base, dropout_mask(11 + (1 << 32), 3, 16, 512, 0.3))     # seed (high word)
    assert not np.array_equal(base[1:], base[:-1])                                      # position in the batch
    # b is the position in the batch: a batch of 16 is the first 16 rows of a batch of 64, shape-independent
    assert np.array_equal(base, dropout_mask(11, 3, 64, 512, 0.3)[:16])
    assert np.array_equal(base[:, :32], dropout_mask(11, 3, 16, 32, 0.3))
    # a larger p drops a superset (the same words against a higher threshold)
    assert not (dropout_mask(11, 3, 16, 512, 0.5) & ~base).any()


@pytest.fixture(scope="module")
def lib():
    from vpr_amd import _lib
    return _lib.lib()


def test_library_refuses_bad_dropout_rates_before_any_launch(lib):
    """0 <= p < 1; p = 1, p < 0 and NaN are VPR_ERR_INVALID_ARG — checked before anything reaches the device."""
    buf = (ctypes.c_char * 4096)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    for p in (1.0, -0.1, float("nan"), float("inf")):
        st = lib.vpr_head_train_step_dropout(q, 64, None, q, 2, 4, 64, 32, 2, q, q, q, q, q, q, 1, 1e-3, 0.9, 0.999, 1e-8,
                                             1e-2, 0, 1.0, None, p, 5, None, q, 4096, None)
        assert st == -1, (p, st)
        st = lib.vpr_head_train_epoch_dropout(q, 64, q, 4, 4, q, 2, 64, 32, 2, q, q, q, q, q, q, 1, 1e-3, 0.9, 0.999, 1e-8,
                                              1e-2, 0, 1.0, None, p, 5, q, 4096, None)
        assert st == -1, (p, st)


def test_dropout_epoch_op_is_registered_with_a_fake_implementation():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "head_train_epoch_dropout" in torch_ops.OPS
    sch = str(torch.ops.vpr.head_train_epoch_dropout.default._schema)
    assert sch.count("!") == 6 and all(f"!) {n}" in sch for n in ("W1", "b1", "W2", "b2", "m", "v")), sch
    assert "float dropout_p" in sch and "Int dropout_seed" in sch
    f32 = torch.float32
    with FakeTensorMode():
        mk = lambda *s, dtype=f32: torch.empty(*s, dtype=dtype, device="cuda")
        n_state = 512 * 1024 + 512 + 2 * 512 + 2
        losses = torch.ops.vpr.head_train_epoch_dropout(mk(70, 1024), mk(70, 2), mk(70, dtype=torch.int32), 16, mk(512, 1024),
                                                        mk(512), mk(2, 512), mk(2), mk(n_state), mk(n_state), 1, 1e-5, 0.9, 0.999,
                                                        1e-8, 1e-2, "huber", 1.0, 0.3, -5)
        assert losses.shape == (5,) and losses.dtype == f32


def test_hip_engine_head_layouts():
    """The HIP step trains Linear-ReLU-Linear and Linear-ReLU-Dropout-Linear; other heads are refused with the way out."""
    from vpr_amd.finetune import _hip_head_layout
    lin, drop = _hip_head_layout(nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Dropout(0.3), nn.Linear(32, 2)))
    assert drop.p == 0.3 and [tuple(l.weight.shape) for l in lin] == [(32, 64), (2, 32)]
    assert _hip_head_layout(nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Linear(32, 2)))[1] is None
    for bad in (nn.Sequential(nn.Linear(64, 32), nn.Dropout(0.3), nn.ReLU(), nn.Linear(32, 2)),
                nn.Sequential(nn.Linear(64, 32), nn.ReLU(), nn.Dropout(0.3), nn.Dropout(0.3), nn.Linear(32, 2)),
                nn.Sequential(nn.Linear(64, 32), nn.GELU(), nn.Linear(32, 2))):
        with pytest.raises(RuntimeError, match='engine="torch"'):
            _hip_head_layout(bad)


def test_default_dropout_seed_is_a_fixed_function_of_the_seed():
    from vpr_amd.finetune import default_dropout_seed
    assert default_dropout_seed(3) == default_dropout_seed(3)
    assert default_dropout_seed(3) != default_dropout_seed(4)
    assert all(0 <= default_dropout_seed(s) < 1 << 64 for s in (0, 1, 2 ** 40))


class _Backbone(nn.Module):
    def __init__(self, hidden_size):
        super().__init__()
        from types import SimpleNamespace
        self.config = SimpleNamespace(hidden_size=hidden_size)


def test_finetune_head_torch_engine_trains_a_dropout_head(tmp_path):
    """engine="torch" on a SwinMLPRegressionModel head (Dropout(0.3) after the ReLU, swin_attempt_2.py:114-123) on the CPU:
    the loss goes down, dropout is active while training, and the checkpoint loads back."""
    from vpr_amd import finetune, modules
    torch.manual_seed(0)
    n, H = 96, 64
    desc = torch.nn.functional.normalize(torch.randn(n, H), dim=1)
    labels = (desc @ (torch.randn(H, 2) * 3)).numpy() * np.array([900.0, 1200.0]) + np.array([219658.0, 143506.0])
    model = modules.SwinMLPRegressionModel(_Backbone(H))
    assert isinstance(model.regressor[2], nn.Dropout) and model.regressor[2].p == 0.3
    out = finetune.finetune_head(model, desc, labels, epochs=6, batch_size=16, lr=3e-3, save_dir=str(tmp_path), seed=1,
                                 log=lambda s: None, engine="torch", loss="huber", weight_decay=0.05)
    got = [h["train_loss"] for h in out["history"]]
    assert got[-1] < got[0]
    model.regressor.train()
    with torch.no_grad():
        a, b = model.regressor(desc[:8]), model.regressor(desc[:8])
    assert not torch.equal(a, b)                                    # masks drawn per call in training mode
    re = modules.load_reference_checkpoint(modules.SwinMLPRegressionModel(_Backbone(H)), str(tmp_path / "checkpoint_5_.pth"))
    for p, q in zip(re.regressor.parameters(), model.regressor.parameters()):
        assert torch.equal(p, q)
