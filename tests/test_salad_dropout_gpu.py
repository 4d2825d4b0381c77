"""GPU: train-mode SALAD (vpr_salad_aggregate_train) — the hub model's Dropout layers of score / cluster_features active,
as under dinov2salad_finetuning.py:115's model.train().  The mask against the numpy statement of include/vpr_amd.h, the
descriptor against an f64 reference built from that mask, identity with the eval form at p = 0, independence of the
launch geometry, refusals, and finetune_head on a TokenCache against a hand-written loop."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from oracle import salad as osalad

pytestmark = pytest.mark.gpu
TOL = 1e-4                     # tests/test_salad_gpu.py's

_spec = importlib.util.spec_from_file_location("_salad_dropout_cpu", os.path.join(os.path.dirname(__file__),
                                                                                   "test_salad_dropout_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
salad_mask = _cpu.salad_mask


def _weights(C, seed, hidden=512, m=64, l=128, t=256, std=0.02):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * std
    w = dict(w1_sc=r(2 * hidden, C), b1_sc=r(2 * hidden), w2_s=r(m, hidden), b2_s=r(m),
             w2_c=r(l, hidden), b2_c=r(l), w1_t=r(hidden, C), b1_t=r(hidden),
             w2_t=r(t, hidden), b2_t=r(t))
    for k in list(w):
        if k.startswith("w"):
            w[k] = w[k].to(torch.bfloat16)
    return w


def _to_dev(w, dev, dustbin):
    from vpr_amd.ops import SaladWeights
    return SaladWeights(**{k: v.to(dev) for k, v in w.items()}, dustbin=dustbin)


def _tokens(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 257, C, generator=g).to(torch.bfloat16)


def _train(td, wd, p, seed, pass_index, image_base=0, mask=False, hub=False):
    from vpr_amd import ops
    B = td.shape[0]
    mo = torch.full((B * 256, wd.w1_sc.shape[0]), 7, dtype=torch.uint8, device=td.device) if mask else None
    pair = td if hub else (td[:, 1:].contiguous(), td[:, 0].contiguous())
    out, out16 = ops.salad_aggregate_train(pair, wd, p, seed, pass_index, image_base, 3, True, mask_out=mo)
    return out, out16, mo


def _reference(tokens, w, mask, p, dustbin):
    """f64: H = bf16(relu(x W1^T + b1) * mask * s) (s the f32 scale), second layers, token MLP, oracle Sinkhorn."""
    hidden = w["w1_sc"].shape[0] // 2
    W = {k: v.double() for k, v in w.items()}
    x = tokens[:, 1:, :].double()
    s = float(np.float32(1.0 / (1.0 - p)))
    H = torch.relu(x @ W["w1_sc"].T + W["b1_sc"])
    H = osalad.bf16_round(H * torch.from_numpy(mask).double().reshape(H.shape) * s)
    scores = H[..., :hidden] @ W["w2_s"].T + W["b2_s"]
    feats = H[..., hidden:] @ W["w2_c"].T + W["b2_c"]
    _, _, tok = osalad.salad_mlps(tokens, w)
    return osalad.sinkhorn_aggregate(scores, feats, tok, dustbin, 3)


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
@pytest.mark.parametrize("image_base", [0, 1000])
def test_mask_equals_numpy_philox(dev, B, p, image_base):
    w = _weights(256, seed=1)
    td, wd = _tokens(B, 256, seed=B).to(dev), _to_dev(w, dev, 1.0)
    seed, pass_index = 0x0123456789ABCDEF, 3
    _, _, mo = _train(td, wd, p, seed, pass_index, image_base, mask=True)
    ref = salad_mask(B, 256, 512, p, seed, pass_index, image_base)
    got = mo.cpu().numpy()
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} mask entries differ"
    if B == 64:
        N = got.size
        assert abs(got.mean() - (1 - p)) < 6 * math.sqrt(p * (1 - p) / N)
        assert not np.array_equal(got[:, :512], got[:, 512:])               # score and cluster units draw their own words


@pytest.mark.parametrize("C,B,p", [(768, 3, 0.3), (1024, 5, 0.3), (1024, 2, 0.5), (768, 1, 0.1)])
def test_descriptor_matches_f64_reference_of_its_mask(dev, C, B, p):
    w = _weights(C, seed=C + B)
    tokens = _tokens(B, C, seed=17 * C + B)
    dustbin = 0.7
    out, out16, mo = _train(tokens.to(dev), _to_dev(w, dev, dustbin), p, 99, 1, 5, mask=True)
    ref = _reference(tokens, w, mo.cpu().numpy(), p, dustbin)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"train-mode SALAD C={C} B={B} p={p}: max abs err {err:.3e}")
    assert err < TOL
    assert torch.equal(out16.cpu(), out.cpu().to(torch.bfloat16))
    # the dropout moved the descriptor away from the eval one by far more than the tolerance
    ev = osalad.salad_aggregate(tokens, w, dustbin, 3)
    assert (out.cpu().double() - ev).abs().max().item() > 10 * TOL


def test_p0_is_the_eval_form_bit_for_bit(dev):
    from vpr_amd import ops
    w = _weights(1024, seed=3)
    td, wd = _tokens(64, 1024, seed=3).to(dev), _to_dev(w, dev, 1.0)
    patch, cls = td[:, 1:].contiguous(), td[:, 0].contiguous()
    ev, ev16 = ops.salad_aggregate_split(patch, cls, wd, 3, True)
    tr, tr16, _ = _train(td, wd, 0.0, 5, 0)                      # p = 0, no mask: the eval kernel
    assert torch.equal(tr, ev) and torch.equal(tr16, ev16)
    trm, trm16, mo = _train(td, wd, 0.0, 5, 0, mask=True)        # p = 0 with a mask: the dropout kernel at t = 0, s = 1
    assert torch.equal(trm, ev) and torch.equal(trm16, ev16) and bool((mo == 1).all())
    hub, hub16, _ = _train(td, wd, 0.0, 5, 0, hub=True)
    assert torch.equal(hub, ev) and torch.equal(hub16, ev16)


def test_hub_and_split_layouts_agree(dev):
    w = _weights(1024, seed=4)
    td, wd = _tokens(8, 1024, seed=4).to(dev), _to_dev(w, dev, 1.0)
    a, a16, ma = _train(td, wd, 0.3, 11, 2, 40, mask=True)
    b, b16, mb = _train(td, wd, 0.3, 11, 2, 40, mask=True, hub=True)
    assert torch.equal(a, b) and torch.equal(a16, b16) and torch.equal(ma, mb)


def test_mask_is_independent_of_the_split_into_calls(dev):
    w = _weights(1024, seed=5)
    td, wd = _tokens(64, 1024, seed=5).to(dev), _to_dev(w, dev, 0.9)
    full, full16, mfull = _train(td, wd, 0.3, 77, 4, 0, mask=True)
    lo, lo16, mlo = _train(td[:32].contiguous(), wd, 0.3, 77, 4, 0, mask=True)
    hi, hi16, mhi = _train(td[32:].contiguous(), wd, 0.3, 77, 4, 32, mask=True)
    assert torch.equal(full, torch.cat([lo, hi])) and torch.equal(full16, torch.cat([lo16, hi16]))
    assert torch.equal(mfull, torch.cat([mlo, mhi]))
    again, again16, magain = _train(td, wd, 0.3, 77, 4, 0, mask=True)
    assert torch.equal(again, full) and torch.equal(again16, full16) and torch.equal(magain, mfull)
    other_pass, _, mp = _train(td, wd, 0.3, 77, 5, 0, mask=True)
    other_seed, _, ms = _train(td, wd, 0.3, 78, 4, 0, mask=True)
    assert not torch.equal(mp, mfull) and not torch.equal(ms, mfull)
    assert not torch.equal(other_pass, full) and not torch.equal(other_seed, full)


def _raw_call(td, wd, p, image_base, hidden, out, out16, mo, ws):
    from vpr_amd import _lib, ops
    L = _lib.lib()
    cw = wd.c_struct()
    B, C = td.shape[0], td.shape[2]
    return L.vpr_salad_aggregate_train(ctypes.c_void_p(td.data_ptr() + 2 * C), 257 * C, ctypes.c_void_p(td.data_ptr()), 257 * C,
                                       B, 256, C, ctypes.byref(cw), float(wd.dustbin), 64, 128, 256, hidden, 3, p, 1, 0,
                                       image_base, ops._ptr(out), ops._ptr(out16), ops._ptr(mo), ops._ptr(ws), ws.numel(),
                                       ops._stream())


def test_refusals_leave_the_outputs_untouched(dev, tune):
    from vpr_amd import _lib
    L = _lib.lib()
    B = 2
    cases = []
    for hidden in (512, 256):
        w = _weights(1024, seed=6, hidden=hidden)
        td, wd = _tokens(B, 1024, seed=6).to(dev), _to_dev(w, dev, 1.0)
        nbytes = L.vpr_salad_workspace_bytes(B, 256, 1024, 64, 128, 256, hidden)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        out = torch.full((B, 8448), 3.25, device=dev)
        out16 = torch.full((B, 8448), -2.5, dtype=torch.bfloat16, device=dev)
        mo = torch.full((B * 256, 2 * hidden), 9, dtype=torch.uint8, device=dev)
        cases.append((td, wd, hidden, out, out16, mo, ws))
    td, wd, hidden, out, out16, mo, ws = cases[0]
    for p, base in ((-0.1, 0), (1.0, 0), (float("nan"), 0), (0.3, -1), (0.3, (1 << 32) - 1)):
        assert _raw_call(td, wd, p, base, hidden, out, out16, mo, ws) == -1, (p, base)
    assert _raw_call(td, wd, 0.3, (1 << 32) - B, hidden, out, out16, mo, ws) == 0          # the last legal image range
    torch.cuda.synchronize()
    out.fill_(3.25), out16.fill_(-2.5), mo.fill_(9)
    tune("VPR_SALAD_VARIANT", 1)
    assert _raw_call(td, wd, 0.3, 0, hidden, out, out16, mo, ws) == -2
    tune("VPR_SALAD_VARIANT", None)
    td2, wd2, hidden2, out2, out16_2, mo2, ws2 = cases[1]
    assert _raw_call(td2, wd2, 0.3, 0, hidden2, out2, out16_2, mo2, ws2) == -2
    torch.cuda.synchronize()
    for o, o16, m in ((out, out16, mo), (out2, out16_2, mo2)):
        assert bool((o == 3.25).all()) and bool((o16 == -2.5).all()) and bool((m == 9).all())


def _finetune_setup(dev, p, N=96, C=768):
    from vpr_amd.finetune import TokenCache
    from vpr_amd.modules import DINOv2RegressionModel, SaladAggregator
    torch.manual_seed(0)
    agg = SaladAggregator(C).to(dev)
    agg.score[1].p = agg.cluster_features[1].p = p
    g = torch.Generator().manual_seed(21)
    tok = torch.randn(N, 257, C, generator=g).to(torch.bfloat16).to(dev)
    cache = TokenCache(tok[:, 1:].contiguous(), tok[:, 0].contiguous(), agg)
    labels = np.random.default_rng(1).normal(size=(N, 2)) * [0.01, 0.02] + [40.0, -75.0]
    model = DINOv2RegressionModel(agg)
    torch.manual_seed(1)
    model.regressor = torch.nn.Sequential(torch.nn.Linear(8448, 512), torch.nn.ReLU(), torch.nn.Linear(512, 2)).to(dev)
    return agg, cache, labels, model


def test_finetune_on_a_token_cache_equals_the_manual_loop(dev):
    from vpr_amd import ops
    from vpr_amd.finetune import default_salad_dropout_seed, finetune_head
    from vpr_amd.postproc import LatLonScaler
    p, epochs, bs, seed = 0.3, 2, 16, 0
    agg, cache, labels, model = _finetune_setup(dev, p)
    val_agg, val_cache, val_labels, _ = _finetune_setup(dev, p, N=20)
    head0 = [t.detach().clone() for t in (model.regressor[0].weight, model.regressor[0].bias,
                                          model.regressor[2].weight, model.regressor[2].bias)]
    res = finetune_head(model, cache, labels, epochs=epochs, batch_size=bs, lr=1e-4, seed=seed, val=(val_cache, val_labels),
                        log=lambda s: None)
    got = [t.detach() for t in (model.regressor[0].weight, model.regressor[0].bias, model.regressor[2].weight,
                                model.regressor[2].bias)]
    # by hand: one aggregation call over all 96 rows (another split into calls than finetune_head's chunks of 64)
    N = len(cache)
    W = [t.clone() for t in head0]
    mom, var = ops.head_train_state(W[0], W[2])
    scaler = LatLonScaler.fit(labels)
    Y = torch.from_numpy(scaler.transform(np.asarray(labels, dtype=np.float64)).astype(np.float32)).to(dev)
    X = torch.empty((N, 8448), dtype=torch.float32, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    step, losses = 0, []
    for e in range(epochs):
        ops.salad_aggregate_train((cache.patch, cache.cls), agg.pack(), p, default_salad_dropout_seed(seed), e, 0,
                                  want_bf16=False, out=X)
        perm = torch.randperm(N, generator=gen).to(dev).to(torch.int32)
        lo = ops.head_train_epoch(X, Y, perm, bs, *W, mom, var, step + 1, lr=1e-4)
        step += lo.numel()
        losses.append(float(lo.sum()) / lo.numel())
    for a, b in zip(got, W):
        assert torch.equal(a, b)
    assert [h["train_loss"] for h in res["history"]] == losses
    # validation: eval descriptors of the val cache, through the HIP pose head, de-normalised
    vd = val_cache.descriptors()
    pv = ops.pose_head(vd, *[t.float().contiguous() for t in W]).cpu().numpy()
    mae = float(np.mean(np.abs(scaler.inverse_transform(pv) - np.asarray(val_labels))))
    assert res["history"][-1]["val_mae"] == mae


def test_finetune_at_p0_equals_training_on_eval_descriptors(dev):
    from vpr_amd.finetune import finetune_head
    agg, cache, labels, model = _finetune_setup(dev, 0.0)
    _, _, _, model2 = _finetune_setup(dev, 0.0)
    finetune_head(model, cache, labels, epochs=2, batch_size=16, lr=1e-4, log=lambda s: None)
    finetune_head(model2, cache.descriptors(), labels, epochs=2, batch_size=16, lr=1e-4, log=lambda s: None)
    for a, b in zip(model.regressor.parameters(), model2.regressor.parameters()):
        assert torch.equal(a, b)


def test_forward_train_matches_the_op(dev):
    """SaladAggregator.forward_train: hub layout and SplitTokens, p read from the module."""
    from vpr_amd import ops
    from vpr_amd.backbone import SplitTokens
    agg, cache, _, _ = _finetune_setup(dev, 0.3, N=4)
    ref, _ = ops.salad_aggregate_train((cache.patch, cache.cls), agg.pack(), 0.3, (1 << 64) - 3, 9, 100)
    split = agg.forward_train(SplitTokens(cache.patch, cache.cls), seed=(1 << 64) - 3, pass_index=9, image_base=100)
    hub = agg.forward_train(torch.cat([cache.cls.unsqueeze(1), cache.patch], 1).contiguous(), seed=-3, pass_index=9,
                            image_base=100)
    assert torch.equal(split, ref) and torch.equal(hub, ref)
    assert not torch.equal(agg(SplitTokens(cache.patch, cache.cls)), ref)           # plain forward: eval arithmetic
