"""vpr_head_train_step_dropout / vpr_head_train_epoch_dropout (HIP): the head-training step with nn.Dropout(p) in training
mode after the ReLU — the head of dinov2salad/dinov2salad_finetuning_2.py:113-122 and swin_transformer/swin_attempt_2.py:
114-123 (Linear(H, 512) -> ReLU -> Dropout(0.3) -> Linear(512, 2), model.train()).

The device mask equals the numpy restatement of include/vpr_amd.h (tests/test_head_dropout_cpu.py) bit for bit, so the
parity tests hand torch autograd + torch.optim.AdamW (f64) the same masks as `h * (mask * s)`.  Tolerances are those of
tests/test_head_train_gpu.py: 0.05 * lr * steps per parameter, 2e-5 relative on the batch losses."""
import ctypes
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_head_dropout_cpu import _Backbone, dropout_mask
from vpr_amd import _lib, ops
from vpr_amd.finetune import default_dropout_seed, finetune_head
from vpr_amd.modules import SwinMLPRegressionModel, load_reference_checkpoint
from vpr_amd.postproc import LatLonScaler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _head(D, hidden, n_out, seed, p=0.3):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(D, hidden), nn.ReLU(), nn.Dropout(p), nn.Linear(hidden, n_out))


def _data(N, D, n_out, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    return X, torch.randn(N, n_out, generator=g)


def _gpu_params(head):
    return [p.detach().clone().to(DEV).contiguous() for p in (head[0].weight, head[0].bias, head[3].weight, head[3].bias)]


def _batches(N, bs, steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < steps:
        perm = rng.permutation(N)
        out += [perm[lo:lo + bs] for lo in range(0, N, bs)]
    return out[:steps]


def _run_hip_steps(head, X, Y, batches, lr, p, seed, want_masks=False, **hyper):
    W1, b1, W2, b2 = _gpu_params(head)
    m, v = ops.head_train_state(W1, W2)
    Xg, Yg = X.to(DEV), Y.to(DEV)
    losses = torch.zeros(len(batches), device=DEV)
    masks = []
    for i, idx in enumerate(batches):
        mk = torch.empty((len(idx), W1.shape[0]), dtype=torch.uint8, device=DEV) if want_masks else None
        ops.head_train_step(Xg, Yg, torch.as_tensor(idx, dtype=torch.int32, device=DEV), W1, b1, W2, b2, m, v, i + 1, lr=lr,
                            loss_out=losses[i:i + 1], dropout_p=p, dropout_seed=seed, mask_out=mk, **hyper)
        masks.append(mk)
    torch.cuda.synchronize()
    return [W1, b1, W2, b2], m, v, losses.cpu().numpy(), [None if t is None else t.cpu().numpy() for t in masks]


def _torch_f64(head, X, Y, batches, masks, p, lrs, loss="mse", huber_delta=1.0, weight_decay=1e-2):
    """Autograd + torch.optim.AdamW in f64 on the CPU; the dropout of step i is h * (masks[i] * s).  Also returns the smallest
    |z| met (how close a pre-activation came to the ReLU's kink)."""
    th = copy.deepcopy(head).double()
    opt = torch.optim.AdamW(th.parameters(), lr=lrs[0], weight_decay=weight_decay)
    loss_fn = nn.MSELoss() if loss == "mse" else nn.HuberLoss(delta=huber_delta)
    X64, Y64 = X.double(), Y.double()
    s = 1.0 / (1.0 - p)
    out, margin = [], float("inf")
    for idx, mk, lr in zip(batches, masks, lrs):
        for g in opt.param_groups:
            g["lr"] = lr
        i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
        z = th[0](X64[i])
        margin = min(margin, float(z.detach().abs().min()))
        h = torch.relu(z)
        l = loss_fn(th[3](h * (torch.from_numpy(mk.astype(np.float64)) * s)), Y64[i])
        opt.zero_grad()
        l.backward()
        opt.step()
        out.append(float(l.detach()))
    return th, np.array(out), margin


@pytest.mark.parametrize("B", [1, 16, 64])
@pytest.mark.parametrize("hidden", [32, 512])
def test_device_mask_equals_the_specification(B, hidden):
    D, n_out, N = 64, 2, 80
    X, Y = _data(N, D, n_out, 1)
    for p, seed in ((0.1, 0), (0.3, 0x0123456789ABCDEF), (0.5, (1 << 64) - 3)):
        head = _head(D, hidden, n_out, 2, p)
        batches = _batches(N, B, 3, 3)
        *_, masks = _run_hip_steps(head, X, Y, batches, 1e-3, p, seed, want_masks=True)
        for step, (idx, mk) in enumerate(zip(batches, masks), 1):
            ref = dropout_mask(seed, step, len(idx), hidden, p)        # B = 64 of 80 rows: the second batch is ragged
            assert mk.dtype == np.uint8 and np.array_equal(mk.astype(bool), ref), (p, seed, step, (mk.astype(bool) != ref).sum())
            assert set(np.unique(mk)) <= {0, 1}


PARITY = [
    # D, B, N, steps, loss, lr
    (768, 16, 70, 8, "mse", 1e-4),          # DINOv2-base CLS width (dinov2salad_finetuning_2.py); ragged 70 = 4 * 16 + 6
    (768, 64, 150, 6, "huber", 1e-4),       # ragged 150 = 2 * 64 + 22
    (1024, 16, 40, 9, "huber", 2e-4),       # Swin-B pooler width (swin_attempt_2.py); ragged 40 = 2 * 16 + 8
    (1024, 64, 128, 4, "mse", 1e-4),
    (8448, 16, 40, 6, "mse", 1e-5),         # SALAD descriptor width, the reference's lr (:95)
    (8448, 64, 100, 4, "huber", 1e-4),      # ragged 100 = 64 + 36
]


@pytest.mark.parametrize("D,B,N,steps,loss,lr", PARITY)
def test_dropout_step_matches_torch_with_the_same_masks(D, B, N, steps, loss, lr):
    hidden, n_out, p, seed = 512, 2, 0.3, 1234
    head = _head(D, hidden, n_out, 7, p)
    X, Y = _data(N, D, n_out, 5)
    if loss == "huber":
        Y = Y * 1.5
    hyper = dict(loss=loss, huber_delta=1.0, weight_decay=0.05)
    batches = _batches(N, B, steps, 6)
    params, _, _, losses, masks = _run_hip_steps(head, X, Y, batches, lr, p, seed, want_masks=True, **hyper)
    for step, (idx, mk) in enumerate(zip(batches, masks), 1):
        assert np.array_equal(mk.astype(bool), dropout_mask(seed, step, len(idx), hidden, p))
    assert any(len(i) < B for i in batches) or N % B == 0
    th, ref_losses, margin = _torch_f64(head, X, Y, batches, [dropout_mask(seed, s, len(i), hidden, p) for s, i in enumerate(batches, 1)],
                                p, [lr] * steps, **hyper)
    # A pre-activation within f32 rounding of 0 can take the other side of the ReLU in f32: that unit's whole W1 row then
    # gets a gradient on one side only, and AdamW moves it by ~lr per step from there on — outside any rounding bound.  The
    # head seed is chosen so that every |z| of these runs clears the kink by far more than the f32 error of z (~1e-9).
    assert margin > 5e-8, margin
    rel = np.abs(losses - ref_losses) / np.maximum(np.abs(ref_losses), 1e-12)
    worst = max(float(np.abs(a.cpu().double().numpy() - b.detach().numpy()).max())
                for a, b in zip(params, (th[0].weight, th[0].bias, th[3].weight, th[3].bias)))
    print(f"\n[head_train dropout D={D} B={B} {loss}] loss rel {rel.max():.1e}; params {worst / lr:.1e} lr (tol {0.05 * steps:.2f})")
    assert rel.max() <= 2e-5, (losses, ref_losses)
    assert worst <= 0.05 * lr * steps
    # dropout is in play: the same steps without it end elsewhere
    plain = _run_hip_steps(head, X, Y, batches, lr, 0.0, seed, **hyper)[0]
    assert not torch.equal(plain[0], params[0])


def _epoch_dropout_raw(X, Y, order, bs, W, m, v, first_step, lr, p, seed):
    """vpr_head_train_epoch_dropout through ctypes (ops routes p = 0 to the plain entry point)."""
    L = _lib.lib()
    D, hidden, n_out = X.shape[1], W[0].shape[0], W[2].shape[0]
    n = order.numel()
    ws = ops.workspace("head_train", L.vpr_head_train_workspace_bytes(min(bs, n), D, hidden, n_out), X.device)
    losses = torch.empty((n + bs - 1) // bs, dtype=torch.float32, device=X.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = L.vpr_head_train_epoch_dropout(ptr(X), X.stride(0), ptr(order), n, bs, ptr(Y), Y.stride(0), D, hidden, n_out,
                                        *(ptr(t) for t in W), ptr(m), ptr(v), first_step, lr, 0.9, 0.999, 1e-8, 1e-2, 0, 1.0,
                                        ptr(losses), p, seed, ptr(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st, "vpr_head_train_epoch_dropout")
    return losses


def test_p0_is_the_plain_step_and_the_epoch_is_its_steps():
    D, hidden, n_out, N, bs, lr = 8448, 512, 2, 70, 16, 1e-4
    head = _head(D, hidden, n_out, 7, 0.0)
    X, Y = _data(N, D, n_out, 8)
    order = np.random.default_rng(9).permutation(N)
    batches = [order[lo:lo + bs] for lo in range(0, N, bs)]
    Xg, Yg, og = X.to(DEV), Y.to(DEV), torch.as_tensor(order, dtype=torch.int32, device=DEV)
    # p = 0 through the dropout entry points == the plain entry points, bitwise
    plain = _run_hip_steps(head, X, Y, batches, lr, 0.0, 0)                       # vpr_head_train_step
    viamask = _run_hip_steps(head, X, Y, batches, lr, 0.0, 99, want_masks=True)   # vpr_head_train_step_dropout, p = 0
    assert all(mk.all() for mk in viamask[4])
    for a, b in zip(plain[0] + [plain[1], plain[2]], viamask[0] + [viamask[1], viamask[2]]):
        assert torch.equal(a, b)
    assert np.array_equal(plain[3], viamask[3])
    W = _gpu_params(head)
    m, v = ops.head_train_state(W[0], W[2])
    l0 = _epoch_dropout_raw(Xg, Yg, og, bs, W, m, v, 1, lr, 0.0, 5)
    torch.cuda.synchronize()
    for a, b in zip(plain[0] + [plain[1], plain[2]], W + [m, v]):
        assert torch.equal(a, b)
    assert np.array_equal(plain[3], l0.cpu().numpy())
    # p = 0.3: one epoch call == the same dropout steps one by one, bitwise (ragged last batch included)
    steps = _run_hip_steps(head, X, Y, batches, lr, 0.3, 5)
    W = _gpu_params(head)
    m, v = ops.head_train_state(W[0], W[2])
    l1 = ops.head_train_epoch(Xg, Yg, og, bs, *W, m, v, 1, lr=lr, dropout_p=0.3, dropout_seed=5)
    torch.cuda.synchronize()
    for a, b in zip(steps[0] + [steps[1], steps[2]], W + [m, v]):
        assert torch.equal(a, b)
    assert np.array_equal(steps[3], l1.cpu().numpy())


def test_epoch_is_reproducible_and_follows_the_seed():
    D, hidden, n_out, N, bs = 1024, 512, 2, 96, 16
    head = _head(D, hidden, n_out, 10)
    X, Y = _data(N, D, n_out, 11)
    Xg, Yg = X.to(DEV), Y.to(DEV)
    order = torch.as_tensor(np.random.default_rng(12).permutation(N), dtype=torch.int32, device=DEV)
    runs = []
    for seed in (77, 77, 78):
        W = _gpu_params(head)
        m, v = ops.head_train_state(W[0], W[2])
        step = 1
        for _ in range(2):
            l = ops.head_train_epoch(Xg, Yg, order, bs, *W, m, v, step, lr=1e-4, dropout_p=0.3, dropout_seed=seed)
            step += l.numel()
        torch.cuda.synchronize()
        runs.append((W, m, v, l.cpu()))
    (a, b, c) = runs
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert torch.equal(x, y)
    assert torch.equal(a[3], b[3])
    assert not torch.equal(a[0][0], c[0][0]) and not torch.equal(a[0][2], c[0][2])


def test_finetune_head_trains_a_swin_dropout_head_on_the_hip_engine(tmp_path):
    """SwinMLPRegressionModel's head (Dropout(0.3), swin_attempt_2.py:114-123) through finetune_head's default engine with
    HuberLoss, weight decay and a ReduceLROnPlateau-style schedule (dinov2salad_finetuning_2.py:152-155), against a torch loop
    fed the same batches and masks; the checkpoint loads back through load_reference_checkpoint."""
    H, N, epochs, bs, lr, seed = 1024, 40, 4, 16, 3e-4, 3
    X, _ = _data(N, H, 2, 13)
    rng = np.random.default_rng(14)
    labels = np.stack([219658.0 + 900 * rng.standard_normal(N), 143506.0 + 1100 * rng.standard_normal(N)], 1)

    def plateau(epoch, history):            # halve when the training loss stopped falling by 5 %
        cur = lr
        for i in range(1, len(history)):
            if history[i]["train_loss"] > 0.95 * min(h["train_loss"] for h in history[:i]):
                cur *= 0.5
        return cur

    torch.manual_seed(15)
    model = SwinMLPRegressionModel(_Backbone(H)).to(DEV)
    init = copy.deepcopy(model.regressor).cpu()
    out = finetune_head(model, X.to(DEV), labels, epochs=epochs, batch_size=bs, lr=lr, save_dir=str(tmp_path), seed=seed,
                        log=lambda s: None, loss="huber", huber_delta=0.5, weight_decay=0.05, lr_schedule=plateau)
    assert out["engine"] == "hip"
    # the torch side: same scaler, same permutations (finetune_head's generator), masks of the global steps
    scaler = LatLonScaler.fit(labels)
    y = torch.from_numpy(scaler.transform(labels).astype(np.float32))
    g = torch.Generator(device="cpu").manual_seed(seed)
    dseed = default_dropout_seed(seed)
    head, hist, step, lr_used = init, [], 0, []
    th = copy.deepcopy(head).double()
    opt = torch.optim.AdamW(th.parameters(), lr=lr, weight_decay=0.05)
    loss_fn = nn.HuberLoss(delta=0.5)
    s = 1.0 / 0.7
    for epoch in range(epochs):
        cur = plateau(epoch, hist)
        lr_used.append(cur)
        for grp in opt.param_groups:
            grp["lr"] = cur
        perm = torch.randperm(N, generator=g)
        tot = []
        for lo in range(0, N, bs):
            idx = perm[lo:lo + bs]
            step += 1
            mk = torch.from_numpy(dropout_mask(dseed, step, len(idx), 512, 0.3).astype(np.float64))
            l = loss_fn(th[3](torch.relu(th[0](X[idx].double())) * (mk * s)), y[idx].double())
            opt.zero_grad()
            l.backward()
            opt.step()
            tot.append(float(l.detach()))
        hist.append({"epoch": epoch, "train_loss": float(np.mean(tot))})
    assert out["optimizer"].param_groups[0]["lr"] == lr_used[-1]
    for a, b in zip(out["history"], hist):
        assert abs(a["train_loss"] - b["train_loss"]) <= 2e-5 * abs(b["train_loss"]), (out["history"], hist)
    worst = max(float((a.detach().cpu().double() - b.detach()).abs().max()) for a, b in zip(model.regressor.parameters(), th.parameters()))
    print(f"\n[finetune_head swin dropout] lrs {lr_used}; params {worst / lr:.1e} lr")
    assert worst <= 0.05 * lr * step
    assert out["history"][-1]["train_loss"] < out["history"][0]["train_loss"]
    ck = torch.load(tmp_path / f"checkpoint_{epochs - 1}_.pth", weights_only=True)
    assert all(float(st["step"]) == step for st in ck["optimizer_state_dict"]["state"].values())
    re = load_reference_checkpoint(SwinMLPRegressionModel(_Backbone(H)), str(tmp_path / f"checkpoint_{epochs - 1}_.pth"))
    for a, b in zip(re.regressor.parameters(), model.regressor.parameters()):
        assert torch.equal(a, b.detach().cpu())


def test_refusals():
    D, hidden, n_out = 64, 32, 2
    head = _head(D, hidden, n_out, 16)
    W = _gpu_params(head)
    m, v = ops.head_train_state(W[0], W[2])
    X, Y = (t.to(DEV) for t in _data(8, D, n_out, 17))
    before = [w.clone() for w in W]
    for p in (1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="dropout_p"):
            ops.head_train_step(X, Y, None, *W, m, v, 1, dropout_p=p)
        with pytest.raises(RuntimeError, match="dropout_p"):
            ops.head_train_epoch(X, Y, torch.arange(8, dtype=torch.int32, device=DEV), 4, *W, m, v, 1, dropout_p=p)
    with pytest.raises(RuntimeError, match="mask_out"):
        ops.head_train_step(X, Y, None, *W, m, v, 1, dropout_p=0.3, mask_out=torch.empty((8, hidden + 1), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(W, before))
    labels = np.random.default_rng(0).standard_normal((16, 2)) * 100 + 1000
    Xd = torch.nn.functional.normalize(torch.randn(16, D, device=DEV), dim=1)
    for reg in (nn.Sequential(nn.Linear(D, hidden), nn.ReLU(), nn.Dropout(0.3), nn.Dropout(0.3), nn.Linear(hidden, 2)),
                nn.Sequential(nn.Linear(D, hidden), nn.Dropout(0.3), nn.ReLU(), nn.Linear(hidden, 2))):
        model = SwinMLPRegressionModel(_Backbone(D))
        model.regressor = reg
        with pytest.raises(RuntimeError, match='engine="torch"'):
            finetune_head(model.to(DEV), Xd, labels, epochs=1, log=lambda s: None)
