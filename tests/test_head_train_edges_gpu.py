"""vpr_head_train_step per element: gradients, AdamW and addressing at the kernels' edges, against f64 with derived bounds
(oracle/finetune.py: head_grad_bounds, adamw_element_bound, exact_train_operands; their self-checks, mistakes included,
are in tests/test_oracle_selfchecks.py).

The gradient read-out.  The step is bitwise reproducible and its gradient does not depend on the optimizer's
hyper-parameters.  Called with betas = (0, 0), step = 1 and zeroed moments, the kernel's own update order gives
m = 0 + (g - 0) * 1 == g and v = 0 * 0 + 1 * g * g == fl(g * g): the f32 gradient of every parameter, bit for bit — W1's
included, which never exists in memory otherwise.  lr = 0 and weight_decay = 0 leave the parameters as they were (asserted).
For any other hyper-parameters a twin call on a copy of the same state yields g, and the real call's (p, m, v) -> (p', m', v')
is checked element by element against AdamW applied to (p, m, v, g).

Every assertion is per element, |gpu - f64| <= bound or bit equality; the worst err / bound per tensor is printed.  Before
every call the workspace is filled with 0xff bytes (NaN floats): it is scratch, nothing stale may be consumed — an empty
K-slice must be written as zeros by the forward kernel."""
import functools

import numpy as np
import pytest
import torch

from oracle import finetune as oft
from vpr_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("W1", "b1", "W2", "b2")
SENTINEL = 0x7FD23456            # a NaN bit pattern no kernel produces
GUARD = 64                       # sentinel floats on either side of an embedded tensor (a multiple of 4: 16-byte offsets)


@functools.lru_cache(maxsize=None)
def _case(B, D, hidden, n_out, seed, targets="far"):
    return oft.train_case_inputs(B, D, hidden, n_out, seed, targets)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poison_workspace(B, D, hidden, n_out):
    nbytes = _lib.lib().vpr_head_train_workspace_bytes(B, D, hidden, n_out)
    assert nbytes > 0
    ops.workspace("head_train", nbytes, torch.device(DEV)).fill_(255)


def _views(buf, W1, W2):
    return [t.cpu().numpy() for t in ops.head_train_state_views(buf, W1, W2)]


def _gradients(X, Y, idx, params, step=1, **kw):
    """The read-out call on copies of `params` (GPU tensors): dict of the f32 gradients (from m), v, and the loss."""
    W = [p.clone() for p in params]
    m, v = ops.head_train_state(W[0], W[2])
    B = X.shape[0] if idx is None else idx.numel()
    _poison_workspace(B, W[0].shape[1], W[0].shape[0], W[2].shape[0])
    loss = torch.full((1,), float("nan"), device=DEV)
    ops.head_train_step(X, Y, idx, *W, m, v, step, lr=0.0, betas=(0.0, 0.0), eps=1e-8, weight_decay=0.0, loss_out=loss, **kw)
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, W, params):
        assert torch.equal(a, b), f"lr = 0, weight_decay = 0 moved {name}"
    got = dict(zip(NAMES, _views(m, W[0], W[2])))
    got["v"] = dict(zip(NAMES, _views(v, W[0], W[2])))
    got["loss"] = float(loss)
    return got


def _check_v(got):
    """v == fl(m * m) in f32 (a square below the normal range may also have been flushed to zero)."""
    for k in NAMES:
        sq = got[k] * got[k]
        ok = (got["v"][k] == sq) | ((sq < np.float32(2.0 ** -126)) & (got["v"][k] == 0))
        assert ok.all(), f"v[{k}] != fl(m * m) at {int((~ok).sum())} elements"


def _ratio(err, b):
    """max err / bound; 0 / 0 counts as 0 (an element whose bound is 0 must be exact, which err <= bound asserts)."""
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))


def _check(tag, got, ref, bound):
    line, bad = [], []
    for k in ("loss",) + NAMES:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        b = np.asarray(bound[k], dtype=np.float64)
        assert np.isfinite(err).all(), f"{tag}: {k} has non-finite elements"
        ratio = _ratio(err, b)
        line.append(f"{k} {ratio:.2e}")
        if not (err <= b).all():
            bad.append(f"{k}: {int((err > b).sum())} of {err.size} elements outside the bound, worst err / bound {ratio:.3g}")
    print(f"\n[{tag}] err / bound: " + "  ".join(line))
    assert not bad, f"{tag}: " + "; ".join(bad)
    _check_v(got)


def _run_case(tag, case, idx=None, **kw):
    x, y, W1, b1, W2, b2 = case
    ref, bound = oft.head_grad_bounds(x, y, W1, b1, W2, b2, **{k: v for k, v in kw.items() if k in ("loss", "huber_delta")})
    got = _gradients(_gpu(x), _gpu(y), idx, [_gpu(t) for t in (W1, b1, W2, b2)], **kw)
    _check(tag, got, ref, bound)
    return got


# ------------------------------------------------------------------------------------------------------ forward edges
@pytest.mark.parametrize("targets", ["far", "near"])
@pytest.mark.parametrize("B", oft.FORWARD_BATCHES)
@pytest.mark.parametrize("D,hidden", oft.FORWARD_EDGES)
def test_forward_edges(dev, D, hidden, B, targets):
    """K-steps, slices (some empty), waves and load rounds of the forward kernels, narrow (B <= 16) and wide.  "near" targets
    sit 2^-8 of the largest output away from the f64 output: every gradient is then proportional to the forward's error."""
    _run_case(f"forward D={D} hidden={hidden} B={B} {targets} ks={oft.head_train_slices(B, D, hidden)}",
              _case(B, D, hidden, 2, 100 + B, targets))


# ------------------------------------------------------------------------------------------------------ update edges
@pytest.mark.parametrize("B,D,hidden,n_out", oft.UPDATE_EDGES)
def test_update_edges(dev, tune, B, D, hidden, n_out):
    """The 1024-column tile of the update kernel and its ragged last tile, the 8-row batch chunk and its tail, n_out 1 / 3 / 8,
    B * n_out above 256 (the P-strided output sum runs twice), hidden 32 and 96."""
    tune("VPR_HEAD_TRAIN_VARIANT", None)
    _run_case(f"update B={B} D={D} hidden={hidden} n_out={n_out}", _case(B, D, hidden, n_out, 200 + B))


@pytest.mark.parametrize("B,D,hidden,n_out", [oft.UPDATE_EDGES[3], oft.UPDATE_EDGES[5]])
def test_update_variants(dev, tune, B, D, hidden, n_out):
    case = _case(B, D, hidden, n_out, 200 + B)
    tune("VPR_HEAD_TRAIN_VARIANT", None)
    default = _run_case(f"update default B={B} D={D}", case)
    for variant in (1, 2, 3, 4):
        tune("VPR_HEAD_TRAIN_VARIANT", variant)
        got = _run_case(f"update variant {variant} B={B} D={D} hidden={hidden} n_out={n_out}", case)
        for k in NAMES:
            assert np.array_equal(got[k], default[k]) and np.array_equal(got["v"][k], default["v"][k]), (variant, k)
        assert got["loss"] == default["loss"]


# ------------------------------------------------------------------------------------------------------ addressing
def _embed(a):
    """(flat buffer full of sentinels, view of `a` inside it at a 16-byte aligned offset)."""
    n = a.size
    pad = -n % 4
    buf = torch.full((GUARD + n + pad + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    view = buf[GUARD:GUARD + n].view(*a.shape)
    view.copy_(_gpu(a))
    return buf, view


def _sentinels_intact(buf, n):
    raw = buf.view(torch.int32)
    return bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("B,form", [(9, "none"), (9, "perm"), (9, "twice"), (9, "last"), (33, "perm"), (33, "twice")])
def test_addressing_strides_index_and_sentinels(dev, B, form):
    """X with row stride D + 4, Y with row stride n_out + 3, NaN in the padding and in every row the batch does not name;
    parameters, moments and the loss inside sentinel-filled buffers that must come back untouched."""
    D, hidden, n_out, rows = 1040, 32, 3, B + 6
    x, y, W1, b1, W2, b2 = _case(B, D, hidden, n_out, 300 + B)
    rng = np.random.default_rng(B)
    if form == "none":
        index = np.arange(B)
    else:
        index = rng.permutation(rows)[:B]
        if form == "last" and rows - 1 not in index:
            index[B // 2] = rows - 1
    if form == "twice":
        index[B - 1] = index[0]
        x, y = x.copy(), y.copy()
        x[B - 1], y[B - 1] = x[0], y[0]
    ref, bound = oft.head_grad_bounds(x, y, W1, b1, W2, b2)          # the margin of a duplicated row is that of the row
    Xs = torch.full((rows, D + 4), float("nan"), device=DEV)
    Ys = torch.full((rows, n_out + 3), float("nan"), device=DEV)
    X, Y = Xs[:, :D], Ys[:, :n_out]
    ii = torch.as_tensor(index, dtype=torch.long, device=DEV)
    X[ii], Y[ii] = _gpu(x), _gpu(y)
    assert X.stride(0) == D + 4 and Y.stride(0) == n_out + 3 and not X.is_contiguous()
    bufs, params = zip(*(_embed(t) for t in (W1, b1, W2, b2)))
    nstate = W1.size + b1.size + W2.size + b2.size
    mbuf, m = _embed(np.zeros(nstate, dtype=np.float32))
    vbuf, v = _embed(np.zeros(nstate, dtype=np.float32))
    lbuf, loss = _embed(np.zeros(1, dtype=np.float32))
    _poison_workspace(B, D, hidden, n_out)
    idx = None if form == "none" else torch.as_tensor(index, dtype=torch.int32, device=DEV)
    if idx is None:                  # the batch is the first B rows of what is passed; the NaN rows lie behind them
        X, Y = X[:B], Y[:B]
    ops.head_train_step(X, Y, idx, *params, m, v, 1, lr=0.0, betas=(0.0, 0.0), weight_decay=0.0, loss_out=loss)
    torch.cuda.synchronize()
    got = dict(zip(NAMES, _views(m, params[0], params[2])))
    got["v"] = dict(zip(NAMES, _views(v, params[0], params[2])))
    got["loss"] = float(loss)
    _check(f"addressing B={B} idx={form}", got, ref, bound)
    for name, buf, t in zip(NAMES + ("m", "v", "loss"), bufs + (mbuf, vbuf, lbuf), (W1, b1, W2, b2, m, v, loss)):
        assert _sentinels_intact(buf, t.numel() if isinstance(t, torch.Tensor) else t.size), f"sentinels around {name} were overwritten"
    for p, t in zip(params, (W1, b1, W2, b2)):
        assert torch.equal(p, _gpu(t))
    assert torch.isnan(Xs[:, D:]).all() and torch.isnan(Ys[:, n_out:]).all()


def test_row_stride_not_a_multiple_of_four_is_refused(dev):
    B, D, hidden, n_out = 9, 1040, 32, 3
    x, y, W1, b1, W2, b2 = _case(B, D, hidden, n_out, 300 + B)
    Xs = torch.zeros((B, D + 2), device=DEV)
    Xs[:, :D] = _gpu(x)
    W = [_gpu(t) for t in (W1, b1, W2, b2)]
    m, v = ops.head_train_state(W[0], W[2])
    with pytest.raises(RuntimeError):
        ops.head_train_step(Xs[:, :D], _gpu(y), None, *W, m, v, 1)
    with pytest.raises(RuntimeError):
        ops.head_train_epoch(Xs[:, :D], _gpu(y), torch.arange(B, dtype=torch.int32, device=DEV), 4, *W, m, v, 1)
    torch.cuda.synchronize()
    assert all(torch.equal(a, _gpu(t)) for a, t in zip(W, (W1, b1, W2, b2))) and not m.any() and not v.any()


# ------------------------------------------------------------------------------------------------------ exact operands
def _exact_reference(case, **kw):
    x, y, W1, b1, W2, b2 = case
    return oft.loss_and_grads(oft.HeadState(W1, b1, W2, b2), x, y, **kw)


@pytest.mark.parametrize("variant", [None, 4])
@pytest.mark.parametrize("B,D,hidden", [(16, 1040, 64), (64, 1040, 64), (16, 4160, 32), (64, 4160, 32)])
def test_exact_operands_bit_for_bit(dev, tune, B, D, hidden, variant):
    """Operands on dyadic grids: every partial sum of the forward, of dz and of the gradients is exact in f32 in any order, so
    m must equal the f64 gradient bit for bit and v == fl(m * m).  Units that are dead for every row keep m == v == 0; where
    z + b1 == 0 exactly, h = 0 and the mask is false (torch's h > 0): a mask from h >= 0 changes thousands of elements."""
    tune("VPR_HEAD_TRAIN_VARIANT", variant)
    n_out = 2
    case = oft.exact_train_operands(B, D, hidden, n_out, 5)
    X, Y, params = _gpu(case[0]), _gpu(case[1]), [_gpu(t) for t in case[2:]]
    value, grads = _exact_reference(case)
    got = _gradients(X, Y, None, params)
    for k, g in zip(NAMES, grads):
        ne = int((got[k].astype(np.float64) != g).sum())
        assert ne == 0, f"{k}: {ne} elements differ from the f64 gradient"
    assert got["loss"] == value
    _check_v(got)
    for k in NAMES:
        assert np.array_equal(got["v"][k], got[k] * got[k])
    dead = np.arange(hidden) % 4 == 1
    for k in ("W1", "b1"):
        assert not got[k][dead].any() and not got["v"][k][dead].any()
    assert not got["W2"][:, dead].any() and not got["v"]["W2"][:, dead].any()
    # Huber with a huge delta: diff = d / 2, exactly half the MSE gradient; with a tiny one: +-delta / N through W2
    half = _gradients(X, Y, None, params, loss="huber", huber_delta=2.0 ** 20)
    for k in NAMES:
        assert np.array_equal(half[k], got[k] * np.float32(0.5)), k
    delta = 2.0 ** -6                        # below the 1/8 grid of the residuals: every non-zero residual is outside
    _, tiny_ref = _exact_reference(case, loss="huber", huber_delta=delta)
    tiny = _gradients(X, Y, None, params, loss="huber", huber_delta=delta)
    for k, g in zip(NAMES, tiny_ref):
        assert np.array_equal(tiny[k].astype(np.float64), g), k
    z = case[0].astype(np.float64) @ case[2].astype(np.float64).T + case[3]
    d = np.maximum(z, 0) @ case[4].astype(np.float64).T + case[5] - case[1]
    assert np.array_equal(tiny["b2"].astype(np.float64), np.sign(d).sum(0) * delta / (B * n_out))
    print(f"\n[exact B={B} D={D} hidden={hidden} variant={variant}] gradients, loss and both Huber forms bit for bit")


# ------------------------------------------------------------------------------------------------------ Huber, dropout
@pytest.mark.parametrize("B", [16, 33])
def test_huber_mixed_residuals(dev, B):
    D, hidden, n_out = 1040, 96, 3
    case = _case(B, D, hidden, n_out, 400 + B)
    ref, _ = oft.head_grad_bounds(*case)
    d = ref["diff"]
    delta = float(np.float32(np.median(np.abs(d))))
    for sign in (-1, 1):
        assert ((sign * d > delta).sum() > 0) and (((sign * d > 0) & (np.abs(d) < delta)).sum() > 0)
    _run_case(f"huber delta={delta:.3f} B={B}", case, loss="huber", huber_delta=delta)


@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("p", [0.3, 0.9])
def test_dropout_gradients(dev, p, B):
    """The kernel's own mask_out goes to the oracle; s = 1 / (1 - p) as f32.  dz carries s once more than hd does."""
    D, hidden, n_out = 1040, 96, 3
    x, y, W1, b1, W2, b2 = _case(B, D, hidden, n_out, 500 + B)
    mask = torch.full((B, hidden), 7, dtype=torch.uint8, device=DEV)
    got = _gradients(_gpu(x), _gpu(y), None, [_gpu(t) for t in (W1, b1, W2, b2)], step=3, dropout_p=p, dropout_seed=0xC0FFEE,
                     mask_out=mask)
    mk = mask.cpu().numpy()
    assert set(np.unique(mk)) <= {0, 1} and abs(mk.mean() - (1 - p)) < 0.1
    ref, bound = oft.head_grad_bounds(x, y, W1, b1, W2, b2, mask=mk, dropout_p=p)
    _check(f"dropout p={p} B={B} kept {mk.mean():.2f}", got, ref, bound)


# ------------------------------------------------------------------------------------------------------ AdamW
@functools.lru_cache(maxsize=None)
def _adam_start():
    """(X, Y, params, m, v, g) on the GPU: the state after three ordinary steps and the f32 gradient at that state."""
    B, D, hidden, n_out = 17, 1040, 32, 3
    x, y, W1, b1, W2, b2 = _case(B, D, hidden, n_out, 600)
    X, Y, W = _gpu(x), _gpu(y), [_gpu(t) for t in (W1, b1, W2, b2)]
    m, v = ops.head_train_state(W[0], W[2])
    for step in (1, 2, 3):
        ops.head_train_step(X, Y, None, *W, m, v, step, lr=1e-3)
    got = _gradients(X, Y, None, W)
    g = np.concatenate([got[k].ravel() for k in NAMES])
    assert np.count_nonzero(g) > 0.3 * g.size and m.any() and v.any()
    return X, Y, W, m, v, g


def _flat(W):
    return np.concatenate([t.cpu().numpy().ravel() for t in W])


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)])
def test_adamw_per_element(dev, betas):
    """eps x weight_decay x lr x step for one pair of betas: every element of all four tensors (and of both moments) inside
    adamw_element_bound; lr = 0 leaves the parameters bit for bit while m and v still move."""
    X, Y, W0, m0, v0, g = _adam_start()
    p0, mm0, vv0 = _flat(W0), m0.cpu().numpy(), v0.cpu().numpy()
    worst = [0.0, 0.0, 0.0]
    for eps in (1e-8, 1e-3):
        for wd in (0.0, 0.01, 0.5):
            for lr in (0.0, 1e-5, 1e-1):
                for step in (1, 2, 10, 1000, 100000):
                    W, m, v = [t.clone() for t in W0], m0.clone(), v0.clone()
                    ops.head_train_step(X, Y, None, *W, m, v, step, lr=lr, betas=betas, eps=eps, weight_decay=wd)
                    c = oft.adamw_consts(step, lr, betas, eps, wd)
                    ref, bound = oft.adamw_element(p0, mm0, vv0, g, c), oft.adamw_element_bound(p0, mm0, vv0, g, c)
                    got = (_flat(W), m.cpu().numpy(), v.cpu().numpy())
                    for i, name in enumerate("pmv"):
                        err = np.abs(got[i].astype(np.float64) - ref[i])
                        worst[i] = max(worst[i], _ratio(err, bound[i]))
                        assert (err <= bound[i]).all(), (f"{name}: {int((err > bound[i]).sum())} elements outside the bound at eps={eps} "
                                                         f"wd={wd} lr={lr} step={step}, worst err / bound {_ratio(err, bound[i]):.3g}")
                    if lr == 0.0:
                        assert np.array_equal(got[0], p0) and not np.array_equal(got[1], mm0) and not np.array_equal(got[2], vv0)
    print(f"\n[adamw betas={betas}] 90 settings, worst err / bound: p {worst[0]:.2e}  m {worst[1]:.2e}  v {worst[2]:.2e}")


# ------------------------------------------------------------------------------------------------------ epoch
def test_epoch_of_a_wide_and_a_narrow_batch_equals_the_two_steps(dev):
    """n = 70, batch_size = 64: a wide batch, then a narrow one of 6 rows in the same workspace; row-padded X and Y."""
    n, bs, D, hidden, n_out = 70, 64, 1040, 32, 2
    x, y, W1, b1, W2, b2 = _case(64, D, hidden, n_out, 700)
    rng = np.random.default_rng(7)
    rows = rng.permutation(64)[:6]
    x, y = np.concatenate([x, x[rows] * np.float32(0.5)]), np.concatenate([y, y[rows] + np.float32(0.25)])
    Xs, Ys = torch.full((n, D + 4), float("nan"), device=DEV), torch.full((n, n_out + 3), float("nan"), device=DEV)
    Xs[:, :D], Ys[:, :n_out] = _gpu(x), _gpu(y)
    X, Y = Xs[:, :D], Ys[:, :n_out]
    order = torch.as_tensor(rng.permutation(n), dtype=torch.int32, device=DEV)
    runs = []
    for whole in (True, False):
        W = [_gpu(t) for t in (W1, b1, W2, b2)]
        m, v = ops.head_train_state(W[0], W[2])
        _poison_workspace(bs, D, hidden, n_out)
        if whole:
            losses = ops.head_train_epoch(X, Y, order, bs, *W, m, v, 1, lr=1e-3)
        else:
            losses = torch.zeros(2, device=DEV)
            ops.head_train_step(X, Y, order[:bs], *W, m, v, 1, lr=1e-3, loss_out=losses[0:1])
            ops.head_train_step(X, Y, order[bs:], *W, m, v, 2, lr=1e-3, loss_out=losses[1:2])
        torch.cuda.synchronize()
        runs.append(W + [m, v, losses])
    for name, a, b in zip(NAMES + ("m", "v", "losses"), *runs):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    assert not torch.equal(runs[0][0], _gpu(W1)) and runs[0][6].numel() == 2
