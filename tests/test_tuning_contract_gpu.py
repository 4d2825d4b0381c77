"""The A/B tuning switches against their contract (include/vpr_amd.h, "per PROCESS" paragraph): every legal value of a
switch (a) keeps the kernel it steers within the f64 bound of that kernel's own test and (b) gives the default's bits,
unless the header lists the switch as one whose values change result bits.  The GEMM switches must also give identical
bits on exact operands (oracle/gemm.py: f32 sums exact in any order), whatever they do to the summation order.

The last test closes the loop the other way: a switch the header lists as changing bits must have been seen doing so.
"""
import copy
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import finetune as oft
from oracle import gemm as og
from oracle import heads as oheads
from oracle import salad as osalad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SEEN = {}          # switch -> True if some value changed result bits against the default (switches exercised so far)


def _bit_exceptions():
    """The switches the header's "per PROCESS" paragraph names as changing result bits."""
    text = open(os.path.join(ROOT, "include", "vpr_amd.h")).read()
    para = text[text.index("(2) per PROCESS"):text.index("dtype conventions")]
    clause = para[para.index("bit-identical results, except"):para.index("Timing-only")]
    return set(re.findall(r"VPR_[A-Z0-9_]+", clause))


def _same_bits(switch, value, a, b, what):
    """(b): identical bits unless the header lists the switch; records what was seen for the closing test."""
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    _SEEN[switch] = _SEEN.get(switch, False) or not same
    if switch not in _bit_exceptions():
        assert same, f"{switch}={value} changed the bits of {what}, and the header promises it does not"


# ------------------------------------------------------------------------------------------------------------ GEMMs
GEMM_SHAPES = [(300, 260, 256), (1000, 516, 1088), (129, 132, 192)]     # N % 4 == 0: gemm256's ldc (= N) rule


def _gemm(dev, kind, a, w, b, relu, out_bf16):
    from vpr_amd import ops
    a, w, b = a.to(dev), w.to(dev), None if b is None else b.to(dev)
    dt = torch.bfloat16 if out_bf16 else torch.float32
    if kind == "group":
        return ops.gemm_nt_group_bf16([dict(a=a, w=w, bias=b, relu=relu, out_dtype=dt)])[0].cpu()
    return ops.gemm_nt_bf16(a, w, b, relu, dt, tile256=(kind == "256")).cpu()


def _gemm_contract(dev, tune, switch, values, kind):
    cases = []
    for i, (M, N, K) in enumerate(GEMM_SHAPES):
        for exact in (True, False):
            a, w, b = (og.exact_operands if exact else og.random_operands)(M, N, K, seed=i)
            relu, out_bf16 = i % 2 == 0, (i + exact) % 2 == 1
            y, s, S = og.gemm_ref(a, w, b, relu)
            cases.append(((M, N, K, exact, out_bf16), (a, w, b, relu, out_bf16), (y, s, S)))
    tune(switch, None)
    default = [_gemm(dev, kind, *args) for _, args, _ in cases]
    for v in values:
        tune(switch, v)
        got = [_gemm(dev, kind, *args) for _, args, _ in cases]
        for (desc, (a, w, b, relu, out_bf16), (y, s, S)), g, d in zip(cases, got, default):
            M, N, K, exact, _ = desc
            what = f"{kind} {switch}={v} M={M} N={N} K={K} {'exact' if exact else 'random'}"
            gd = g.double()
            if exact:
                assert torch.equal(gd, og.exact_value(y, out_bf16)), f"{what}: exact operands, wrong bits"
            else:
                ratio = ((gd - y).abs() / og.gemm_bound(y, s, S, K, b, out_bf16)).max().item()
                assert ratio <= 1.0, f"{what}: worst |err| / bound {ratio:.3f}"
        _same_bits(switch, v, got, default, f"{kind} GEMMs")


@pytest.mark.parametrize("switch,values,kind", [
    ("VPR_GEMM_NT_STAGES", (2, 3), "nt"),
    ("VPR_GEMM_GROUP_VARIANT", (0, 1), "group"),
    ("VPR_GEMM256_STAGGER", (0, 1, 2, 3, 4, 5), "256"),
    ("VPR_GEMM256_DEPTH", (2, 6, 10), "256"),          # release library: read only by the timing-only build
])
def test_gemm_switches(dev, tune, switch, values, kind):
    _gemm_contract(dev, tune, switch, values, kind)


# ------------------------------------------------------------------------------------------------------------ SALAD
SALAD_TOL = 1e-4            # tests/test_salad_gpu.py
F32_PATH_BOUND = 5e-7       # tests/test_precision_gpu.py


def _salad_weights(C, seed, std=0.02, f32=False, hidden=512, m=64, l=128, t=256):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * std
    w = dict(w1_sc=r(2 * hidden, C), b1_sc=r(2 * hidden), w2_s=r(m, hidden), b2_s=r(m),
             w2_c=r(l, hidden), b2_c=r(l), w1_t=r(hidden, C), b1_t=r(hidden), w2_t=r(t, hidden), b2_t=r(t))
    if not f32:
        for k in list(w):
            if k.startswith("w"):
                w[k] = w[k].to(torch.bfloat16)
    return w


def _salad_contract(dev, tune, switch, values, B, C, setup=(), f32=False):
    from vpr_amd import ops
    g = torch.Generator().manual_seed(B * 3 + C)
    tokens = torch.randn(B, 257, C, generator=g)
    if not f32:
        tokens = tokens.to(torch.bfloat16)
    w = _salad_weights(C, seed=C + B, f32=f32)
    ref = osalad.salad_aggregate(tokens, w, dustbin=1.0, iters=3, quantize=not f32)
    td = tokens.to(dev)
    if f32:
        wd = ops.SaladWeightsF32(**{k: v.to(dev) for k, v in w.items()}, dustbin=1.0)
        run = lambda: ops.salad_aggregate_f32(td, wd, 3)[0].cpu()
        tol = F32_PATH_BOUND
    else:
        wd = ops.SaladWeights(**{k: v.to(dev) for k, v in w.items()}, dustbin=1.0)
        run = lambda: ops.salad_aggregate(td, wd, 3)[0].cpu()
        tol = SALAD_TOL
    for name, v in setup:
        tune(name, v)
    tune(switch, None)
    default = run()
    for v in values:
        tune(switch, v)
        out = run()
        err = (out.double() - ref).abs().max().item()
        assert err < tol, f"SALAD B={B} C={C} {switch}={v} {dict(setup)}: max err {err:.2e}"
        _same_bits(switch, v, [out], [default], f"SALAD B={B} C={C} {dict(setup)}")


def test_group_variant_on_salad_unfused_route(dev, tune):
    """VPR_SALAD_VARIANT=1: SALAD's second layers as one grouped launch."""
    _salad_contract(dev, tune, "VPR_GEMM_GROUP_VARIANT", (0, 1), B=4, C=768, setup=(("VPR_SALAD_VARIANT", 1),))


def test_group_variant_on_salad_f32_path(dev, tune):
    """The f32-accurate SALAD path: K = 6 C / 6 hidden GEMMs, second layers and token MLP grouped."""
    _salad_contract(dev, tune, "VPR_GEMM_GROUP_VARIANT", (0, 1), B=2, C=384, f32=True)


def test_stagger_on_fused_salad_stage(dev, tune):
    """The fused layer-1 + layer-2 kernel (hidden 512) walks its K-tiles in the staggered order too."""
    _salad_contract(dev, tune, "VPR_GEMM256_STAGGER", (0, 1, 2, 3, 4, 5), B=8, C=1024)


def test_salad_variant_4(dev, tune):
    """VPR_SALAD_VARIANT=4: the aggregation's B % 8 == 0 form, at B = 64."""
    _salad_contract(dev, tune, "VPR_SALAD_VARIANT", (4,), B=64, C=384)


def test_stagger_on_gathered_fp8_knn_scores(dev, tune):
    """The e4m3 score tile of a 512-query gathered batch (gemm256_kernel<true>): scores within the bound of
    tests/test_knn_gpu.py's GEMM-route test against the streaming kernel, final answers identical."""
    from vpr_amd import ops, _lib
    from oracle import knn as oknn
    B, N, D, k = 512, 3001, 8448, 10
    assert _lib.lib().vpr_knn_scores_kernel_name(1, B, N).decode() == "vpr::gemm256_kernel<true, 10>"
    gq = torch.Generator().manual_seed(41)
    q, qs = oknn.quantize_fp8_rows(torch.nn.functional.normalize(torch.randn(B, D, generator=gq), dim=1))
    g, gs = oknn.quantize_fp8_rows(torch.nn.functional.normalize(torch.randn(N, D, generator=gq), dim=1))
    q, qs, g, gs = q.to(dev), qs.to(dev), g.to(dev), gs.to(dev)

    def run():
        ws = ops.knn_workspace(B, N, D, k, dev)
        ws.zero_()
        v, i = ops.knn_topk_fp8(q, qs, g, gs, k, 0, ws)
        return ops.knn_scores_view(ws, B, N, D, k).clone().cpu(), v.cpu(), i.cpu()

    tune("VPR_KNN_GEMM_MIN_B", 100000)
    s_stream, v_ref, i_ref = run()
    tune("VPR_KNN_GEMM_MIN_B", None)
    tune("VPR_GEMM256_STAGGER", None)
    default = run()
    scale = max(s_stream.abs().max().item(), 1.0)
    for stagger in range(6):
        tune("VPR_GEMM256_STAGGER", stagger)
        s, v, i = run()
        assert (s - s_stream).abs().max().item() < 2e-6 * scale, f"stagger {stagger}: scores off"
        assert torch.equal(v, v_ref) and torch.equal(i, i_ref), f"stagger {stagger}: top-k differs"
        _same_bits("VPR_GEMM256_STAGGER", stagger, [s], [default[0]], "gathered e4m3 kNN scores")


# ------------------------------------------------------------------------------------------------------------ pose head
POSE_TOL = 1e-4             # tests/test_heads_gpu.py


def _linear_init(out_f, in_f, g):
    bound = 1.0 / in_f ** 0.5
    return ((torch.rand(out_f, in_f, generator=g) * 2 - 1) * bound, (torch.rand(out_f, generator=g) * 2 - 1) * bound)


POSE_SHAPES = [(64, 8448, 512, 4, 2), (64, 8448, 1024, 4, 2), (7, 768, 384, 2, 0)]


def _pose_case(B, D, hidden, n_out, off):
    g = torch.Generator().manual_seed(B + D + hidden)
    x = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1) if D == 8448 else torch.randn(B, D, generator=g)
    W1, b1 = _linear_init(hidden, D, g)
    W2, b2 = _linear_init(n_out, hidden, g)
    return (x, W1, b1, W2, b2), oheads.mlp_head(x, W1, b1, W2, b2, off)


def _pose_contract(dev, tune, switch, values, shape, fused):
    from vpr_amd import ops
    B, D, hidden, n_out, off = shape
    args, ref = _pose_case(*shape)
    dargs = [t.to(dev) for t in args]
    run = lambda: ops.pose_head(*dargs, off, split=True, fused=fused).cpu()
    tune(switch, None)
    default = run()
    for v in values:
        tune(switch, v)
        out = run()
        err = (out.double() - ref).abs().max().item()
        what = f"pose head {shape} {'fused' if fused else 'split'} {switch}={v}"
        assert err < POSE_TOL and err < 2e-5 * max(1.0, ref.abs().max().item()), f"{what}: max err {err:.2e}"
        _same_bits(switch, v, [out], [default], what)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("shape", POSE_SHAPES)
def test_pose_ks(dev, tune, shape, fused):
    D = shape[1]
    _pose_contract(dev, tune, "VPR_POSE_KS", [v for v in (1, 2, 7, 33, 64) if v <= D // 32], shape, fused)


@pytest.mark.parametrize("shape", POSE_SHAPES)
def test_pose_variant_8(dev, tune, shape):
    """Eight waves per workgroup in the two-launch split head."""
    _pose_contract(dev, tune, "VPR_POSE_VARIANT", (8,), shape, fused=False)


# ------------------------------------------------------------------------------------------------------ head training
DEV = "cuda:0"


def _head_setup(D, hidden, n_out, N, seed):
    torch.manual_seed(seed)
    head = nn.Sequential(nn.Linear(D, hidden), nn.ReLU(), nn.Linear(hidden, n_out))
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
    return head, X, torch.randn(N, n_out, generator=g)


def _head_batches(N, bs, steps, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < steps:
        perm = rng.permutation(N)
        out += [perm[lo:lo + bs] for lo in range(0, N, bs)]
    return out[:steps]


def _head_hip(head, X, Y, batches, lr, p, seed):
    from vpr_amd import ops
    W1, b1, W2, b2 = [t.detach().clone().to(DEV).contiguous() for t in (head[0].weight, head[0].bias, head[2].weight, head[2].bias)]
    m, v = ops.head_train_state(W1, W2)
    Xg, Yg = X.to(DEV), Y.to(DEV)
    masks = []
    for i, idx in enumerate(batches):
        mk = torch.empty((len(idx), W1.shape[0]), dtype=torch.uint8, device=DEV) if p > 0 else None
        ops.head_train_step(Xg, Yg, torch.as_tensor(idx, dtype=torch.int32, device=DEV), W1, b1, W2, b2, m, v, i + 1, lr=lr,
                            dropout_p=p, dropout_seed=seed, mask_out=mk)
        masks.append(None if mk is None else mk.cpu().numpy())
    torch.cuda.synchronize()
    return [t.cpu() for t in (W1, b1, W2, b2, m, v)], masks


def _head_reference(head, X, Y, batches, lr, p, masks):
    """oracle/finetune.py for p = 0; with dropout, autograd + torch.optim.AdamW in f64 on the device's masks (the
    reference of tests/test_head_train_dropout_gpu.py)."""
    if p == 0:
        st = oft.HeadState(*(t.detach().numpy() for t in (head[0].weight, head[0].bias, head[2].weight, head[2].bias)))
        Xn, Yn = X.numpy().astype(np.float64), Y.numpy().astype(np.float64)
        for idx in batches:
            oft.train_step(st, Xn[idx], Yn[idx], lr=lr)
        return [np.asarray(t) for t in st.p]
    th = copy.deepcopy(head).double()
    opt = torch.optim.AdamW(th.parameters(), lr=lr, weight_decay=1e-2)
    s = 1.0 / (1.0 - p)
    for idx, mk in zip(batches, masks):
        i = torch.as_tensor(np.asarray(idx), dtype=torch.long)
        h = torch.relu(th[0](X.double()[i]))
        loss = nn.functional.mse_loss(th[2](h * (torch.from_numpy(mk.astype(np.float64)) * s)), Y.double()[i])
        opt.zero_grad()
        loss.backward()
        opt.step()
    return [t.detach().numpy() for t in (th[0].weight, th[0].bias, th[2].weight, th[2].bias)]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("D,hidden,n_out,N,bs,steps,lr", [(8448, 512, 2, 80, 16, 6, 1e-5), (256, 64, 4, 40, 33, 6, 1e-3)])
def test_head_train_variants(dev, tune, D, hidden, n_out, N, bs, steps, lr, p):
    head, X, Y = _head_setup(D, hidden, n_out, N, 0)
    batches = _head_batches(N, bs, steps, 2)
    tol = 0.05 * lr * steps                                   # PARAM_TOL of tests/test_head_train_gpu.py
    tune("VPR_HEAD_TRAIN_VARIANT", None)
    default, masks0 = _head_hip(head, X, Y, batches, lr, p, 7)
    for v in (1, 2, 3, 4):
        tune("VPR_HEAD_TRAIN_VARIANT", v)
        got, masks = _head_hip(head, X, Y, batches, lr, p, 7)
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(masks, masks0))
        ref = _head_reference(head, X, Y, batches, lr, p, masks)
        worst = max(float(np.abs(t.numpy().astype(np.float64) - r).max()) for t, r in zip(got[:4], ref))
        assert worst <= tol, f"VPR_HEAD_TRAIN_VARIANT={v} p={p} D={D}: params off by {worst:.2e} (tol {tol:.1e})"
        _same_bits("VPR_HEAD_TRAIN_VARIANT", v, got, default, f"head_train_step D={D} p={p}")


# ------------------------------------------------------------------------------------------------------------ header
def test_header_lists_exactly_the_switches_seen_changing_bits():
    """Of the switches exercised above, the header names exactly those whose values changed result bits."""
    listed = _bit_exceptions()
    wrong = [f"{s}: {'changed bits but is not listed' if changed else 'listed, but no value changed bits'}"
             for s, changed in _SEEN.items() if changed != (s in listed)]
    assert not wrong, wrong
