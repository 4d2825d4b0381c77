"""CPU: closed-form known answers that pin the SALAD and kNN oracles (SURVEY.md §8c — both are
'parity unpinned' by the reference, so these identities are what holds them in place), and the f64 attention
oracle against PyTorch's own attention."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import attention as oattn
from oracle import knn as oknn
from oracle import salad as osalad


def test_sinkhorn_column_marginals_exact():
    """(1) the v-update is the last half-step, so every column of P (dustbin included) sums to 1."""
    g = torch.Generator().manual_seed(0)
    S = torch.randn(3, 64, 256, generator=g, dtype=torch.float64) * 3
    P = osalad.matching_probs(S, dustbin=0.7, num_iters=3)
    assert P.shape == (3, 65, 256)
    assert (P.sum(1) - 1).abs().max().item() < 1e-12
    # row sums only approximately 1 / (n-m) after 3 iterations
    assert (P[:, :64].sum(2) - 1).abs().max().item() < 0.5
    assert (P[:, 64].sum(1) - 192).abs().max().item() < 40


def test_uniform_scores_closed_form():
    """(2) all scores == dustbin: P = 1/n for clusters, (n-m)/n for the dustbin, after 1 iteration."""
    S = torch.full((1, 64, 256), 1.5, dtype=torch.float64)
    for iters in (1, 3):
        P = osalad.matching_probs(S, dustbin=1.5, num_iters=iters)
        assert (P[:, :64] - 1 / 256).abs().max().item() < 1e-14
        assert (P[:, 64] - 192 / 256).abs().max().item() < 1e-14


def test_descriptor_norm_shares_and_invariances():
    g = torch.Generator().manual_seed(1)
    scores = torch.randn(2, 256, 64, generator=g)
    feats = torch.randn(2, 256, 128, generator=g)
    tok = torch.randn(2, 256, generator=g)
    out = osalad.sinkhorn_aggregate(scores, feats, tok, 1.0, 3)
    assert out.shape == (2, 8448)
    assert (out.pow(2).sum(1) - 1).abs().max().item() < 1e-12                      # (3)
    assert (out[:, :256].pow(2).sum(1) - 1 / 65).abs().max().item() < 1e-12
    assert (out[:, 256:].reshape(2, 128, 64).pow(2).sum(1) - 1 / 65).abs().max().item() < 1e-12
    perm = torch.randperm(256, generator=g)                                         # (4)
    assert (osalad.sinkhorn_aggregate(scores[:, perm], feats[:, perm], tok, 1.0, 3) - out).abs().max().item() < 1e-12
    assert (osalad.sinkhorn_aggregate(scores.double() + 2.5, feats, tok, 3.5, 3) - out).abs().max().item() < 1e-12   # (5)
    out32 = osalad.sinkhorn_aggregate(scores, feats, tok, 1.0, 3, dtype=torch.float32)                       # (6)
    assert (out32.double() - out).abs().max().item() < 2e-6
    # flatten order is l-major: index 256 + l*64 + m
    V = out[0, 256:].reshape(128, 64)
    assert torch.allclose(V[:, 5].norm(), torch.tensor(1 / math.sqrt(65.0), dtype=torch.float64))


def test_salad_mlps_quantisation_points():
    g = torch.Generator().manual_seed(2)
    tokens = torch.randn(1, 257, 128, generator=g).to(torch.bfloat16)
    r = lambda *s: torch.randn(*s, generator=g) * 0.05
    w = dict(w1_sc=r(1024, 128).bfloat16(), b1_sc=r(1024), w2_s=r(64, 512).bfloat16(), b2_s=r(64),
             w2_c=r(128, 512).bfloat16(), b2_c=r(128), w1_t=r(512, 128).bfloat16(), b1_t=r(512),
             w2_t=r(256, 512).bfloat16(), b2_t=r(256))
    a = osalad.salad_aggregate(tokens, w, 1.0, 3, quantize=True)
    b = osalad.salad_aggregate(tokens, w, 1.0, 3, quantize=False)
    assert a.shape == (1, 8448) and 0 < (a - b).abs().max().item() < 1e-3


def test_knn_oracle_against_python_loop():
    g = torch.Generator().manual_seed(3)
    q = torch.randn(3, 64, generator=g).to(torch.bfloat16)
    gal = torch.randn(40, 64, generator=g).to(torch.bfloat16)
    gal[17] = gal[4]                                      # a tie
    v, i = oknn.knn_topk(q, gal, 6, index_base=100)
    for b in range(3):
        scores = []
        for n in range(40):
            s = sum(float(q[b, d]) * float(gal[n, d]) for d in range(64))   # python floats = fp64
            scores.append((-float(torch.tensor(s, dtype=torch.float64).to(torch.float32)), n))
        scores.sort()
        assert [100 + n for _, n in scores[:6]] == i[b].tolist()
        assert [-s for s, _ in scores[:6]] == v[b].tolist()


def test_knn_merge_equals_unsharded_and_pads():
    g = torch.Generator().manual_seed(4)
    q = torch.randn(5, 32, generator=g).to(torch.bfloat16)
    gal = torch.randn(90, 32, generator=g).to(torch.bfloat16)
    v_all, i_all = oknn.knn_topk(q, gal, 7)
    parts = [oknn.knn_topk(q, gal[lo:hi], 7, lo) for lo, hi in ((0, 30), (30, 33), (33, 90))]   # middle shard has < k rows
    vm, im = oknn.topk_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(im, i_all) and torch.equal(vm, v_all)
    v, i = oknn.knn_topk(q, gal[:3], 5)
    assert (i[:, 3:] == -1).all() and torch.isinf(v[:, 3:]).all()
    assert oknn.recall_at_1(i_all[:, 0], i_all[:, 0]) == 1.0


def test_resize_tables_and_oracle_match_pil():
    """The preprocessing restatement is pinned by PIL itself (the resizer the reference's
    torchvision / HF transforms end in): identical bytes for both filters, down- and up-scaling."""
    import numpy as np
    from PIL import Image
    from oracle import preprocess as opre
    from vpr_amd.preprocess import resample_coeffs
    rng = np.random.default_rng(0)
    for (H, W) in [(480, 640), (224, 224), (200, 300), (777, 1033)]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for filt, pf in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
            kx, xb, _ = resample_coeffs(W, 224, filt)
            ky, yb, _ = resample_coeffs(H, 224, filt)
            ref = np.asarray(Image.fromarray(img).resize((224, 224), pf))
            assert np.array_equal(opre.resize_u8(img, 224, kx, xb, ky, yb), ref), (H, W, filt)
    # the shapes and inputs of tests/test_preprocess_gpu.py (non-square outputs, up- and downscaling, binary images whose
    # bicubic overshoot is clamped at both ends): the oracle with separate output height and width, on the same images
    import preprocess_cases as pc
    for (H, W), (OH, OW), clips in pc.SHAPES:
        for filt in pc.FILTERS:
            kx, xb, _ = resample_coeffs(W, OW, filt)
            ky, yb, _ = resample_coeffs(H, OH, filt)
            for kind in pc.KINDS:
                ref = pc.pil_reference(H, W, OH, OW, kind, filt)
                assert ref.shape == (pc.B, OH, OW, 3)
                if clips and kind == "binary":
                    pc.assert_reference_clips(ref, (H, W, OH, OW, filt))
                for b in range(pc.B):
                    got = opre.resize_u8(pc.images(H, W, kind)[b], (OH, OW), kx, xb, ky, yb)
                    assert np.array_equal(got, ref[b]), (H, W, OH, OW, filt, kind, b)
    t = opre.to_tensor_normalize(np.array([[[0, 128, 255]]], dtype=np.uint8), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    assert t.shape == (3, 1, 1) and t[0, 0, 0] == -1.0 and t[2, 0, 0] == 1.0


# ------------------------------------------------------------------ frozen self-oracle fixtures
def _self_oracle():
    import importlib.util
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_self_oracle.py")
    spec = importlib.util.spec_from_file_location("make_self_oracle", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_oracle_reproduces_its_frozen_outputs():
    """The oracle is the contract of the two stages the reference cannot pin; these fixtures freeze it (self-oracle,
    not reference data): an edit that changes SALAD descriptors by > 1e-12 or any kNN index / value fails here."""
    mso = _self_oracle()
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fx = np.load(os.path.join(G, "salad_cpu.npz"))
    tokens, w = mso.salad_inputs(int(fx["seed"]))
    assert float(tokens.float().sum()) == float(fx["tokens_sum"])              # same inputs regenerated
    desc = osalad.salad_aggregate(tokens, w, dustbin=float(fx["dustbin"]), iters=3).numpy()
    assert np.abs(desc - fx["descriptor"]).max() < 1e-12
    fk = np.load(os.path.join(G, "knn_cpu.npz"))
    q, gal = mso.knn_inputs(int(fk["seed"]))
    assert float(q.sum()) == float(fk["q_sum"])
    v, i = oknn.knn_topk(q.to(torch.bfloat16), gal.to(torch.bfloat16), 7, 11)
    assert np.array_equal(i.numpy(), fk["idx"]) and np.array_equal(v.numpy(), fk["vals"])
    q8, qs = oknn.quantize_fp8_rows(q)
    g8, gs = oknn.quantize_fp8_rows(gal)
    v8, i8 = oknn.knn_topk_fp8(q8, qs, g8, gs, 7, 11)
    assert np.array_equal(i8.numpy(), fk["idx_fp8"]) and np.array_equal(v8.numpy(), fk["vals_fp8"])


@pytest.mark.gpu
def test_hip_path_matches_the_frozen_self_oracle(dev):
    from vpr_amd import ops
    from vpr_amd.ops import SaladWeights
    mso = _self_oracle()
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    fx = np.load(os.path.join(G, "salad_cpu.npz"))
    tokens, w = mso.salad_inputs(int(fx["seed"]))
    out, _ = ops.salad_aggregate(tokens.to(dev), SaladWeights(**{k: v.to(dev) for k, v in w.items()}, dustbin=float(fx["dustbin"])), 3)
    assert np.abs(out.cpu().double().numpy() - fx["descriptor"]).max() < 1e-4
    fk = np.load(os.path.join(G, "knn_cpu.npz"))
    q, gal = mso.knn_inputs(int(fk["seed"]))
    v, i = ops.knn_topk(q.to(torch.bfloat16).to(dev), gal.to(torch.bfloat16).to(dev), 7, 11)
    assert np.array_equal(i.cpu().numpy(), fk["idx"]) and np.array_equal(v.cpu().numpy(), fk["vals"])
    q8, qs = oknn.quantize_fp8_rows(q)
    g8, gs = oknn.quantize_fp8_rows(gal)
    v8, i8 = ops.knn_topk_fp8(q8.to(dev), qs.to(dev), g8.to(dev), gs.to(dev), 7, 11)
    assert np.array_equal(i8.cpu().numpy(), fk["idx_fp8"]) and np.array_equal(v8.cpu().numpy(), fk["vals_fp8"])


def test_sinkhorn_solver_equals_hf_superglue_log_sinkhorn():
    """An INDEPENDENT implementation of the log-domain Sinkhorn iteration is importable: Hugging Face's SuperGlue port
    (transformers.models.superglue.modeling_superglue.log_sinkhorn_iterations) — the routine SALAD's solver descends
    from (SuperGlue's log_optimal_transport, arXiv:1911.11763 §3.3; SALAD arXiv:2311.15937 §3.2 reuses it with a
    dustbin ROW only).  With SALAD's marginals it must give the oracle's log-assignment: this pins the solver half of
    oracle/salad.py against a third party; the SALAD-specific wiring around it (marginals, dustbin row, normalisation
    order, MLP layout) stays pinned by the closed-form identities above only."""
    sg = pytest.importorskip("transformers.models.superglue.modeling_superglue")
    g = torch.Generator().manual_seed(12)
    B, m, n = 3, 64, 256
    S = torch.randn(B, m + 1, n, generator=g, dtype=torch.float64) * 2.5
    norm = -math.log(n + m)
    log_a = torch.full((B, m + 1), norm, dtype=torch.float64)
    log_a[:, -1] += math.log(n - m)
    log_b = torch.full((B, n), norm, dtype=torch.float64)
    for iters in (1, 3, 10):
        ours = osalad.log_otp_solver(log_a, log_b, S, iters)
        theirs = sg.log_sinkhorn_iterations(S, log_a, log_b, iters)
        assert (ours - theirs).abs().max().item() < 1e-12
    # and through the oracle's public entry (dustbin row appended, exp, dustbin dropped later)
    P = osalad.matching_probs(S[:, :m], dustbin=0.3, num_iters=3)
    S_aug = torch.cat([S[:, :m], torch.full((B, 1, n), 0.3, dtype=torch.float64)], 1)
    P_hf = torch.exp(sg.log_sinkhorn_iterations(S_aug, log_a, log_b, 3) - norm)
    assert (P - P_hf).abs().max().item() < 1e-12


def test_knn_oracle_agrees_with_numpy_brute_force():
    """The kNN contract written a second time with numpy only (f64 products of the bf16 values, f32 rounding, stable
    argsort = value desc / index asc) — guards the torch-based oracle against a sort / gather mistake; includes ties."""
    g = torch.Generator().manual_seed(5)
    q = torch.nn.functional.normalize(torch.randn(6, 96, generator=g), dim=1).to(torch.bfloat16)
    gal = torch.nn.functional.normalize(torch.randn(500, 96, generator=g), dim=1).to(torch.bfloat16)
    gal[40] = gal[7]; gal[300] = gal[7]
    q[0] = gal[7]
    v, i = oknn.knn_topk(q, gal, 9, index_base=100)
    s = (q.double().numpy() @ gal.double().numpy().T).astype(np.float32)
    order = np.argsort(-s, axis=1, kind="stable")[:, :9]
    assert np.array_equal(i.numpy(), order.astype(np.int32) + 100)
    assert np.array_equal(v.numpy(), np.take_along_axis(s, order, axis=1))
    assert i[0, :3].tolist() == [107, 140, 400]


@pytest.mark.parametrize("B,T,H", [(2, 257, 3), (1, 1, 1), (3, 17, 2)])
def test_attention_oracle_equals_sdpa_f64(B, T, H):
    g = torch.Generator().manual_seed(T)
    qkv = (torch.randn(B, T, 3 * H * 64, generator=g, dtype=torch.float64) * 1.5).to(torch.bfloat16)
    q, k, v = qkv.double().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=0.125).transpose(1, 2).reshape(B, T, H * 64)
    assert (oattn.attention_f64(qkv, H) - sdpa).abs().max().item() < 1e-12
    ref = torch.softmax(q @ k.transpose(-1, -2) * 0.3, dim=-1) @ v
    assert (oattn.attention_f64(qkv, H, scale=0.3) - ref.transpose(1, 2).reshape(B, T, H * 64)).abs().max().item() < 1e-12


def test_attention_oracle_is_invariant_to_a_per_query_logit_offset():
    """A key dimension set to 8 in every key and to c in query i adds c to every logit of query i (scale 1/8):
    softmax must not move — also at offsets where an unstabilised exp over- or underflows in f64."""
    B, T, H = 2, 33, 2
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, T, 3, H, 64, generator=g, dtype=torch.float64)
    qkv[:, :, 1, :, 63] = 8.0
    qkv[:, :, 0, :, 63] = 0.0
    base = oattn.attention_f64(qkv.reshape(B, T, -1), H)
    offs = torch.tensor([-1000.0, -200.0, -40.0, 0.0, 40.0, 800.0], dtype=torch.float64)
    qkv[:, :, 0, :, 63] = offs[torch.randint(0, len(offs), (B, T, H), generator=g)]
    shifted = oattn.attention_f64(qkv.reshape(B, T, -1), H)
    assert torch.isfinite(shifted).all()
    assert (shifted - base).abs().max().item() < 1e-12


@pytest.mark.parametrize("B,T,body", [(3, 257, 256), (2, 17, 0), (2, 17, 17), (4, 5, 1), (1, 9, 4)])
def test_attention_split_rows_round_trip(B, T, body):
    x = torch.arange(B * T * 2, dtype=torch.float64).reshape(B, T, 2)
    rows = oattn.to_split_rows(x, body)
    assert torch.equal(oattn.from_split_rows(rows, B, T, body), x)
    idx = oattn.split_row_index(B, T, body)
    assert sorted(idx.reshape(-1).tolist()) == list(range(B * T))            # a permutation of the rows
    for b in range(B):
        for t in range(T):                                                     # the layout of ops.attention_qkv_split_bf16
            row = b * body + t if t < body else B * body + b * (T - body) + (t - body)
            assert torch.equal(rows[row], x[b, t])


# ------------------------------------------------------------------------------------------------ GEMM bound (oracle/gemm.py)
from oracle import gemm as ogemm  # noqa: E402


@pytest.mark.parametrize("M,N,K", [(67, 130, 64), (33, 257, 1088), (16, 40, 4096)])
@pytest.mark.parametrize("relu", [False, True])
def test_gemm_bound_holds_for_f32_matmul(M, N, K, relu):
    """The per-element bound covers an f32 GEMM of the same bf16 operands (torch's CPU matmul: another summation
    order), for f32 output and after RNE to bf16."""
    a, w, b = ogemm.random_operands(M, N, K, seed=M + N + K)
    y, s, S = ogemm.gemm_ref(a, w, b, relu)
    y32 = a.float() @ w.float().T + b
    if relu:
        y32 = y32.clamp_min(0)
    assert ((y32.double() - y).abs() <= ogemm.gemm_bound(y, s, S, K, b)).all()
    y16 = y32.to(torch.bfloat16).double()
    assert ((y16 - y).abs() <= ogemm.gemm_bound(y, s, S, K, b, out_bf16=True)).all()


def _truncate_bf16(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).double()


@pytest.mark.parametrize("M,N,K", [(64, 96, 256), (40, 130, 1088)])
def test_gemm_bound_is_not_vacuous(M, N, K):
    """The bound rejects a result with one 64-deep K-tile dropped, a bias shifted by one column, and bf16 conversion by
    truncation; the exact-operand form pins the same faults bit for bit."""
    a, w, b = ogemm.random_operands(M, N, K, seed=K)
    y, s, S = ogemm.gemm_ref(a, w, b)
    bound = ogemm.gemm_bound(y, s, S, K, b)
    for j in (0, K // 64 - 1):
        kt = slice(64 * j, 64 * j + 64)
        dropped = y - a[:, kt].double() @ w[:, kt].double().T
        assert ((dropped - y).abs() > bound).any(), f"K-tile {j} dropped passes"
    shifted = s + torch.roll(b, 1).double()[None, :]
    assert ((shifted - y).abs() > bound).any(), "bias shifted by one column passes"
    y32 = (a.float() @ w.float().T + b)
    trunc = _truncate_bf16(y32)
    assert ((trunc - y).abs() > ogemm.gemm_bound(y, s, S, K, b, out_bf16=True)).any(), "truncation to bf16 passes"
    # exact operands: f32 sums are exact in any order, the right answer is one value per element
    a, w, b = ogemm.exact_operands(M, N, K, seed=K)
    y, s, S = ogemm.gemm_ref(a, w, b)
    y32 = a.float() @ w.float().T + b
    assert torch.equal(y32.double(), y)
    assert torch.equal(torch.flip(a, [1]).float() @ torch.flip(w, [1]).float().T + b, y32)       # order-independent
    want16 = ogemm.exact_value(y, True)
    assert torch.equal(y32.to(torch.bfloat16).double(), want16)
    assert not torch.equal(_truncate_bf16(y32), want16), "truncation indistinguishable on exact operands"
    kt = slice(0, 64)
    assert not torch.equal(ogemm.exact_value(y - a[:, kt].double() @ w[:, kt].double().T, False), y)


def test_gemm_ref_resolves_row_groups():
    """rows_of / gemm_ref address row r at (r // g) * stride + (r % g) * lda, as the kernels do."""
    M, K, lda, g, stride = 10, 64, 72, 3, 3 * 72 + 16
    a = torch.randn(M, K).to(torch.bfloat16)
    flat = torch.full((4 * stride + lda,), float("nan"), dtype=torch.bfloat16)
    for r in range(M):
        o = (r // g) * stride + (r % g) * lda
        flat[o:o + K] = a[r]
    assert torch.equal(ogemm.rows_of(flat, M, K, lda, g, stride), a)
    w = torch.randn(5, K).to(torch.bfloat16)
    y, _, _ = ogemm.gemm_ref(flat, w, None, False, g, stride, lda, M)
    assert torch.equal(y, a.double() @ w.double().T)


@pytest.mark.parametrize("B,N,D", [(150, 130, 128), (65, 3, 256), (512, 257, 512)])
def test_exact_e4m3_operands_are_exact_in_any_order(B, N, D):
    """The preconditions of the bit-for-bit e4m3 score test: the bytes decode to the integers they were cast from, the sum
    of |products| of every score is below 2^24, both scale vectors are powers of two that vary per row, and the expected
    value is an f32 number that f32 arithmetic reproduces in another summation order."""
    q, qs, g, gs, want = ogemm.exact_e4m3_operands(B, N, D, seed=B + N + D)
    qv, gv = q.view(torch.float8_e4m3fn).float(), g.view(torch.float8_e4m3fn).float()
    for v in (qv, gv):
        assert torch.equal(v, v.round()) and v.abs().max() == 8 and v.min() == -8
        assert torch.equal(v.to(torch.float8_e4m3fn).float(), v)                      # the cast round-trips
    assert (qv.double().abs() @ gv.double().abs().T).max() < 2 ** 24
    for s in (qs, gs):
        mant, _ = torch.frexp(s)
        assert s.dtype == torch.float32 and torch.equal(mant, torch.full_like(s, 0.5)) and s.unique().numel() >= min(3, s.numel())
    assert torch.equal(want, (qv.double() @ gv.double().T) * qs.double()[:, None] * gs.double()[None, :])
    assert torch.equal(want.float().double(), want)
    got = (torch.flip(qv, [1]) @ torch.flip(gv, [1]).T) * qs[:, None] * gs[None, :]    # f32, another order
    assert torch.equal(got.double(), want)
    one_off = want.clone()
    one_off[B - 1, N - 1] += qs[B - 1].double() * gs[N - 1].double()                    # one unit of one product
    assert not torch.equal(one_off.float().double(), want)


# ------------------------------------------------------------------------- head bounds (oracle/heads.py)
def _head_ratio(out, x, W1, b1, W2, b2, split, slices):
    from oracle import heads as oheads
    ref = oheads.mlp_head(x, W1, b1, W2, b2)
    bound = oheads.mlp_head_bound(x, W1, b1, W2, b2, split, slices=slices)
    return ((out.double() - ref).abs() / bound).max().item()


def test_mlp_head_bound_holds_for_f32_and_split_arithmetic_and_rejects_mistakes():
    """On the inputs of the GPU edge tests (split-form K edges): plain torch f32 sits inside mlp_head_bound(split=False), the
    CPU emulation of the (hi, lo) plane arithmetic inside mlp_head_bound(split=True), and each mistake falls outside.
    A dropped lo plane (W1's, or x's as a broken split8 would) is an error of 2^-9 per product with random signs against a
    budget of 2^-16 Σ|x||w|: the margin shrinks like 1 / sqrt(D) but holds on all five cases (it is lost near D = 1000)."""
    from oracle import heads as oheads
    for B, D, hidden, n_out, off, ks in oheads.SPLIT_K_EDGE_CASES:
        x, W1, b1, W2, b2 = oheads.head_case_inputs(B, D, hidden, n_out, 1000 + D, off)
        slices = oheads.split_case_slices(D, ks)
        f32 = torch.relu(x @ W1.T + b1) @ W2.T + b2
        assert _head_ratio(f32, x, W1, b1, W2, b2, False, slices) <= 1.0, D
        for split in (False, True):
            clean = oheads.mlp_head_emulated(x, W1, b1, W2, b2, split, slices)
            assert _head_ratio(clean, x, W1, b1, W2, b2, split, slices) <= 1.0, (D, split)
            mistakes = ["bias_after_relu", "drop_step", "slice_twice"]
            if split:
                mistakes += ["lo_zero", "x_lo_zero"]
            for m in mistakes:
                bad = oheads.mlp_head_emulated(x, W1, b1, W2, b2, split, slices, m)
                assert _head_ratio(bad, x, W1, b1, W2, b2, split, slices) > 1.0, (D, split, m)
        # a normalised pair: the bound stays finite (r far from 0) and the f32 evaluation inside it
        if off >= 0:
            ref = oheads.mlp_head(x, W1, b1, W2, b2, off)
            bound = oheads.mlp_head_bound(x, W1, b1, W2, b2, False, off, slices)
            assert torch.isfinite(bound).all() and float(oheads.mlp_head(x, W1, b1, W2, b2)[:, off:off + 2].norm(dim=1).min()) > 0.05
            got = oheads._normalize_pair(f32.clone(), off)
            assert ((got.double() - ref).abs() <= bound).all()


def test_normalize_pair_refuses_an_offset_without_a_pair():
    from oracle import heads as oheads
    out = torch.ones(2, 3, dtype=torch.float64)
    for off in (2, 3, 7):
        with pytest.raises(RuntimeError):
            oheads._normalize_pair(out, off)
    assert torch.equal(oheads._normalize_pair(out, -1), out)
    assert (oheads._normalize_pair(out, 1)[:, 1:].norm(dim=1) - 1).abs().max().item() < 1e-15


@pytest.mark.parametrize("B,D,hidden,n_out", [(3, 32, 16, 4), (5, 1056, 208, 8), (2, 224, 48, 1), (4, 257, 0, 8)])
def test_exact_head_operands_are_exact_in_any_order(B, D, hidden, n_out):
    """f32 evaluation under a shuffled summation order (K-steps permuted, several slab counts, split planes or not) equals
    the f64 result bit for bit; the three kinds of hidden unit are all there; every lo plane is zero."""
    from oracle import heads as oheads
    x, W1, b1, W2, b2 = oheads.exact_head_operands(B, D, hidden, n_out, 7)
    ref = oheads.mlp_head(x, W1, b1, W2, b2)
    assert torch.equal(ref.float().double(), ref)
    g = torch.Generator().manual_seed(0)
    if hidden == 0:
        for _ in range(3):
            p = torch.randperm(D, generator=g)
            acc = torch.zeros(B, n_out)
            for d in p.tolist():
                acc = acc + x[:, d:d + 1] * W2[:, d][None, :]
            assert torch.equal((acc + b2).double(), ref)
        return
    z = x.double() @ W1.double().T + b1.double()
    assert (z > 0).any() and (z < 0).any() and (z == 0).any()
    assert (z[:, 0::4] > 0).all() and (z[:, 1::4] < 0).all() and (z[0, 2::4] == 0).all() and (z[:, 3::4] == 0).all()
    assert not oheads._split_planes(x)[1].any() and not oheads._split_planes(W1)[1].any()
    nsteps = -(-D // 32)
    for slices in (1, 2, 5):
        for split in (False, True):
            perm = torch.randperm(nsteps, generator=g).tolist()
            got = oheads.mlp_head_emulated(x, W1, b1, W2, b2, split, slices, perm=perm)
            assert torch.equal(got.double(), ref), (slices, split)
    h = torch.relu(z).float()                                   # second layer, one product at a time in a shuffled order
    acc = torch.zeros(B, n_out)
    for j in torch.randperm(hidden, generator=g).tolist():
        acc = acc + h[:, j:j + 1] * W2[:, j][None, :]
    assert torch.equal((acc + b2).double(), ref)


def test_ln_meanpool_bound_holds_for_two_pass_f32_and_rejects_one_pass_variance():
    from oracle import heads as oheads
    g = torch.Generator().manual_seed(5)
    eps = 1e-5
    for T, H in ((17, 512), (65, 1024), (33, 1536)):
        gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
        Wh, bh = torch.randn(4, H, generator=g) / H ** 0.5, torch.tensor([0.1, -0.2, 1.5, -2.0])
        for kind in ("unit", "offset1000"):
            x = oheads.ln_case_rows(kind, 2, T, H, g)
            pooled_ref, out_ref = oheads.ln_meanpool_head(x, gamma, beta, eps, Wh, bh, 2)
            pb, ob = oheads.ln_meanpool_bound(x, gamma, beta, eps, Wh, bh, 2)
            if kind == "unit":          # the bound is not slack: torch f32 comes within a factor 50 of it, and it is ~10x below 2e-5
                tight = (((torch.nn.functional.layer_norm(x, (H,), gamma, beta, eps).mean(1).double() - pooled_ref).abs() / pb).max().item())
                assert tight >= 0.02 and pb.median().item() < 4e-6, (T, H, tight, pb.median().item())
            y = torch.nn.functional.layer_norm(x, (H,), gamma, beta, eps)              # torch f32: two-pass statistics
            pooled = y.mean(1)
            out = oheads._normalize_pair(pooled @ Wh.T + bh, 2)
            assert ((pooled.double() - pooled_ref).abs() <= pb).all(), (T, H, kind)
            assert ((out.double() - out_ref).abs() <= ob).all(), (T, H, kind)
            if kind == "offset1000":                                                   # E[x^2] - mean^2 in f32: var is noise
                mean = x.mean(-1, keepdim=True)
                var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp_min(0)
                bad = (((x - mean) * torch.rsqrt(var + eps)) * gamma + beta).mean(1)
                assert ((bad.double() - pooled_ref).abs() > pb).any(), (T, H)


def test_merge_and_quantise_oracles_known_answers():
    """oracle/knn.py on hand-worked cases: the merge orders (value desc, index asc) with padding last as (-inf, -1) and +0.0
    above -0.0; the quantiser rounds e4m3 ties to even in the normal and the subnormal range."""
    inf = float("inf")
    vals = torch.tensor([[[0.5, inf, -0.0]], [[0.5, 0.0, -inf]]])
    idxs = torch.tensor([[[9, -3, 1]], [[4, 7, 2]]], dtype=torch.int32)
    v, i = oknn.topk_merge(vals, idxs)
    assert i.tolist() == [[4, 9, 7]] and v.tolist() == [[0.5, 0.5, 0.0]]
    v, i = oknn.topk_merge(vals[:, :, 1:], idxs[:, :, 1:])
    assert i.tolist() == [[7, 1]] and torch.signbit(v).tolist() == [[False, True]]
    v, i = oknn.topk_merge(vals[:1, :, :], idxs[:1, :, :])
    assert i.tolist() == [[9, 1, -1]] and v[0, 2].item() == -inf
    x = torch.tensor([[448.0, 17.0, 19.0, 232.0, 248.0, 432.0, 2.0 ** -10, 3 * 2.0 ** -10, -0.0, -(2.0 ** -10), 15 * 2.0 ** -10, 0.0]])
    q, s = oknn.quantize_fp8_rows(x)
    assert s.tolist() == [1.0]
    assert q.view(torch.float8_e4m3fn).float().tolist() == [[448.0, 16.0, 20.0, 224.0, 256.0, 448.0, 0.0, 2.0 ** -8, -0.0, -0.0, 2.0 ** -6, 0.0]]
    assert q[0, 8].item() == 0x80 and q[0, 9].item() == 0x80 and q[0, 11].item() == 0


# ------------------------------------------------------------------------------- head-training bounds (oracle/finetune.py)
from oracle import finetune as oft

_GRADS = ("W1", "b1", "W2", "b2")


def _ratios(got, ref, bound):
    """max |got - ref| / bound per tensor (0 / 0 counts as 0: an element whose bound is 0 must be exact)."""
    out = {}
    for k in ("loss",) + _GRADS:
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        b = np.asarray(bound[k], dtype=np.float64)
        out[k] = float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))))
    return out


def _torch_f32_grads(x, y, W1, b1, W2, b2):
    t = [torch.from_numpy(np.array(a)).requires_grad_(i >= 2) for i, a in enumerate((x, y, W1, b1, W2, b2))]
    loss = torch.nn.functional.mse_loss(torch.relu(t[0] @ t[2].T + t[3]) @ t[4].T + t[5], t[1])
    loss.backward()
    return dict(loss=float(loss.detach()), **{k: a.grad.numpy() for k, a in zip(_GRADS, t[2:])})


@pytest.mark.parametrize("targets", ["far", "near"])
@pytest.mark.parametrize("D,hidden", oft.FORWARD_EDGES)
def test_head_grad_bounds_hold_torch_f32(D, hidden, targets):
    for B in oft.FORWARD_BATCHES:
        ops_ = oft.train_case_inputs(B, D, hidden, 2, 100 + B, targets)
        ref, bound = oft.head_grad_bounds(*ops_)
        r = _ratios(_torch_f32_grads(*ops_), ref, bound)
        print(f"\n[torch f32 / bound D={D} hidden={hidden} B={B} {targets}] " + " ".join(f"{k} {v:.2e}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, r


def test_head_grad_bounds_hold_update_edges_and_emulation():
    for B, D, hidden, n_out in oft.UPDATE_EDGES:
        ops_ = oft.train_case_inputs(B, D, hidden, n_out, 200 + B)
        ref, bound = oft.head_grad_bounds(*ops_)
        for name, got in (("torch", _torch_f32_grads(*ops_)), ("slabs", oft.head_grads_f32(*ops_))):
            r = _ratios(got, ref, bound)
            print(f"\n[{name} f32 / bound B={B} D={D} hidden={hidden} n_out={n_out}] " + " ".join(f"{k} {v:.2e}" for k, v in r.items()))
            assert max(r.values()) <= 1.0, r


def _dropout_case(B, D, hidden, n_out, p, seed):
    ops_ = oft.train_case_inputs(B, D, hidden, n_out, seed)
    mask = np.random.default_rng(seed + 1).random((B, hidden)) >= p
    return ops_, mask


@pytest.mark.parametrize("mutate,case,tensor", [
    ("row_tail", ("far", 9, 1040, 32, 3), "W1"),
    ("drop_slice", ("near", 16, 4160, 32, 2), "W1"),
    ("slab_twice", ("near", 16, 4160, 32, 2), "W1"),
    ("gscale_pad", ("far", 17, 1040, 32, 3), "b2"),
])
def test_head_grad_bounds_reject_mistakes(mutate, case, tensor):
    targets, B, D, hidden, n_out = case
    ops_ = oft.train_case_inputs(B, D, hidden, n_out, 7, targets)
    ref, bound = oft.head_grad_bounds(*ops_)
    good, bad = _ratios(oft.head_grads_f32(*ops_), ref, bound), _ratios(oft.head_grads_f32(*ops_, mutate=mutate), ref, bound)
    print(f"\n[{mutate} at {case}] err / bound {tensor}: right {good[tensor]:.2e}, mistaken {bad[tensor]:.2e}")
    assert max(good.values()) <= 1.0 and bad[tensor] > 1.0


def test_head_grad_bounds_dropout_and_missing_scale():
    for p in (0.3, 0.9):
        ops_, mask = _dropout_case(17, 1040, 96, 3, p, 11)
        ref, bound = oft.head_grad_bounds(*ops_, mask=mask, dropout_p=p)
        good = _ratios(oft.head_grads_f32(*ops_, mask=mask, dropout_p=p), ref, bound)
        bad = _ratios(oft.head_grads_f32(*ops_, mask=mask, dropout_p=p, mutate="no_drop_s"), ref, bound)
        print(f"\n[dropout p={p}] err / bound: right {max(good.values()):.2e}; s left out of dz: W1 {bad['W1']:.2e} b1 {bad['b1']:.2e}")
        assert max(good.values()) <= 1.0 and bad["W1"] > 1.0 and bad["b1"] > 1.0
        assert bad["W2"] <= 1.0 and bad["b2"] <= 1.0            # the mistake is confined to dz


@pytest.mark.parametrize("B,D,hidden,n_out", [(16, 1040, 64, 4), (64, 4160, 32, 1)])
def test_exact_train_operands_are_exact_and_catch_the_mask(B, D, hidden, n_out):
    ops_ = oft.exact_train_operands(B, D, hidden, n_out, 5)
    value, grads = oft.loss_and_grads(oft.HeadState(*ops_[2:]), ops_[0], ops_[1])
    got = oft.head_grads_f32(*ops_)
    assert got["loss"] == value
    for k, g in zip(_GRADS, grads):
        assert np.array_equal(got[k].astype(np.float64), g), k
    kind = np.arange(hidden) % 4
    assert not grads[0][kind == 1].any() and not grads[1][kind == 1].any()
    bad = oft.head_grads_f32(*ops_, mutate="mask_ge")
    nbad = int((bad["W1"].astype(np.float64) != grads[0]).sum())
    print(f"\n[exact operands B={B} D={D} hidden={hidden}] h >= 0 as the mask changes {nbad} elements of gW1")
    assert nbad > 0 and bad["W1"][kind == 1].any()


def _adam_state(n, seed):
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)      # 1e-6 .. 1: eps = 1e-3 is first order
    m = (g * rng.uniform(0.2, 2.0, n) * rng.choice([-1.0, 1.0, 1.0], n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.1, 4.0, n)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32) * np.float32(0.05)
    return p, m, v, g


def _adam_ratio(got, p, m, v, g, c):
    ref, bound = oft.adamw_element(p, m, v, g, c), oft.adamw_element_bound(p, m, v, g, c)
    return [float(np.max(np.abs(a.astype(np.float64) - r) / b)) for a, r, b in zip(got, ref, bound)]


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)])
def test_adamw_bound_holds_numpy_f32_in_both_contraction_forms(betas):
    p, m, v, g = _adam_state(20000, 3)
    worst = 0.0
    for step in (1, 2, 10, 1000, 100000):
        for eps in (1e-8, 1e-3):
            for wd, lr in ((0.0, 1e-5), (0.01, 1e-1), (0.5, 1e-1), (0.5, 0.0)):
                c = oft.adamw_consts(step, lr, betas, eps, wd)
                for fused in (False, True):
                    r = _adam_ratio(oft.adamw_f32(p, m, v, g, c, fused=fused), p, m, v, g, c)
                    worst = max(worst, max(r))
                    assert max(r) <= 1.0, (step, eps, wd, lr, fused, r)
    print(f"\n[numpy f32 AdamW / bound betas={betas}] worst {worst:.2e}")


@pytest.mark.parametrize("mistake", ["eps_inside", "decay_after", "bc_prev", "swap_betas"])
def test_adamw_bound_rejects_mistakes(mistake):
    p, m, v, g = _adam_state(20000, 4)
    hyper = dict(step=2, lr=1e-1, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.5)
    c = oft.adamw_consts(**hyper)
    wrong = dict(hyper)
    if mistake == "bc_prev":
        wrong["step"] = 1
    if mistake == "swap_betas":
        wrong["betas"] = (0.999, 0.9)
    got = oft.adamw_f32(p, m, v, g, oft.adamw_consts(**wrong), mutate=mistake if mistake in ("eps_inside", "decay_after") else None)
    good, bad = _adam_ratio(oft.adamw_f32(p, m, v, g, c), p, m, v, g, c), _adam_ratio(got, p, m, v, g, c)
    print(f"\n[AdamW {mistake}] err / bound (p, m, v): right {good}, mistaken {bad}")
    assert max(good) <= 1.0 and bad[0] > 1.0


# ------------------------------------------------------------------------- SALAD stage oracle (oracle/salad_stages.py)
def _bf16_exact(x):
    return torch.equal(x.float().to(torch.bfloat16).float(), x.float())


@pytest.mark.parametrize("C", [64, 128, 192, 1536])
def test_exact_salad_inputs_are_exact_in_any_f32_order(C):
    """What tests/test_salad_stages_gpu.py relies on when it asks a kernel for the f64 bits: on the inputs of exact_inputs,
    f32 arithmetic is exact under a permuted K order and a two-slab split of layer 2 (every partial sum is a multiple of
    the grid below 2^24 grid steps), about half the hidden units are active, and the one rounding that IS there — hidden
    values to bf16 — changes at least 1 % of them, exact ties (to even, both ways) among them."""
    from oracle import salad_stages as ost
    B = 2
    tokens, w = ost.exact_inputs(C, B, seed=C)
    for k, v in w.items():                                    # the grids, and that bf16 / f32 hold them
        q = {"w1": 64, "b1": 8, "w2": 8, "b2": 64}[k[:2]]
        assert torch.equal((v.double() * q).round(), v.double() * q) and v.double().abs().max() <= {"w1": .25, "b1": 2, "w2": .25, "b2": 1}[k[:2]]
        assert v.dtype == (torch.bfloat16 if k.startswith("w") else torch.float32)
    assert tokens.dtype == torch.bfloat16 and torch.equal(tokens.double().round(), tokens.double()) and tokens.double().abs().max() == 3
    o = ost.salad_stage_outputs(tokens, w)
    z, zt = ost.pre_activations(tokens, w)
    W = {k: v.double() for k, v in w.items()}
    x, cls = tokens[:, 1:].double().reshape(-1, C), tokens[:, 0].double()
    hidden = 512
    # magnitudes: sum of absolute terms below 2^24 grid steps in both layers, at dropout scale 2 as well
    mag1 = max((x.abs() @ W["w1_sc"].abs().T + W["b1_sc"].abs()).max(), (cls.abs() @ W["w1_t"].abs().T + W["b1_t"].abs()).max()).item()
    mag2 = max((o["H"][:, :hidden] @ W["w2_s"].abs().T + W["b2_s"].abs()).max(), (o["H"][:, hidden:] @ W["w2_c"].abs().T + W["b2_c"].abs()).max(),
               (o["Ht"] @ W["w2_t"].abs().T + W["b2_t"].abs()).max()).item()
    print(f"\n[exact SALAD inputs C={C}] sum|x||w1|+|b1| <= {mag1:.1f} (limit {ost.EXACT_LIMIT_1:.0f}), "
          f"sum|h||w2|+|b2| <= {mag2:.1f} (limit {ost.EXACT_LIMIT_2:.0f})")
    assert mag1 < ost.EXACT_LIMIT_1 == 2.0 ** 18 and 2 * mag2 < ost.EXACT_LIMIT_2 == 2.0 ** 15
    for v, q in ((z, ost.Q1), (zt, ost.Q1), (o["H"], ost.Q1), (o["S"], ost.Q2), (o["F"], ost.Q2), (o["g"], ost.Q2)):
        assert torch.equal((v / q).round(), v / q)
    # layer 1 in f32 under a random permutation of K, and in two halves added afterwards
    g = torch.Generator().manual_seed(C)
    perm = torch.randperm(C, generator=g)
    xf, w1f = x.float(), w["w1_sc"].float()
    z32 = xf[:, perm] @ w1f[:, perm].T + w["b1_sc"]
    half = (xf[:, perm[:C // 2]] @ w1f[:, perm[:C // 2]].T + w["b1_sc"]) + xf[:, perm[C // 2:]] @ w1f[:, perm[C // 2:]].T
    assert torch.equal(z32.double(), z) and torch.equal(half.double(), z)
    # layer 2 in f32: the two slabs, each over permuted hidden columns, slab 0 with the bias, added in f32
    Hf = o["H"].float()
    assert torch.equal(Hf.double(), o["H"]) and _bf16_exact(Hf)
    for key, cols, w2, b2 in (("S", slice(0, hidden), w["w2_s"], w["b2_s"]), ("F", slice(hidden, 2 * hidden), w["w2_c"], w["b2_c"])):
        h, w2f = Hf[:, cols], w2.float()
        p0, p1 = torch.randperm(256, generator=g), 256 + torch.randperm(256, generator=g)
        s0, s1 = h[:, p0] @ w2f[:, p0].T + b2, h[:, p1] @ w2f[:, p1].T
        assert torch.equal(s0.double(), o[key][0]) and torch.equal(s1.double(), o[key][1])
        assert torch.equal((s0 + s1).double(), o[key].sum(0))
    s_ref, f_ref, g_ref = osalad.salad_mlps(tokens, w)            # the stage oracle is the MLP oracle, split
    assert torch.equal(s_ref.reshape(-1, 64), o["S"].sum(0)) and torch.equal(f_ref.reshape(-1, 128), o["F"].sum(0)) and torch.equal(g_ref, o["g"])
    s32, f32_, g32 = ost.salad_mlps_f32(tokens, w)
    assert torch.equal(s32.double(), o["S"].sum(0)) and torch.equal(f32_.double(), o["F"].sum(0)) and torch.equal(g32.double(), o["g"])
    # the one rounding: share of active units, of hidden values the rounding changes, ties both ways resolved to even
    for name, zz in (("score/cluster", z), ("token", zt)):
        h = torch.relu(zz)
        hq = osalad.bf16_round(h)
        active, changed = (zz > 0).double().mean().item(), (h != hq).double().mean().item()
        other = 2 * h - hq                                       # a tie: the value on the other side is a bf16 number too
        tie = (h != hq) & (osalad.bf16_round(other) == other)
        up, down = (tie & (hq > h)).sum().item(), (tie & (hq < h)).sum().item()
        print(f"  {name}: active {active:.3f}, changed by bf16 {changed:.4f}, ties up / down {up} / {down}")
        assert active >= 0.30 and changed >= 0.01 and up > 0 and down > 0
        even = (hq[tie].float().view(torch.int32) >> 16) & 1
        assert int(even.sum()) == 0
    # dropout at p = 0.5 doubles the kept values exactly (a power of two commutes with the rounding)
    keep = torch.rand(z.shape, generator=g) < 0.5
    assert torch.equal(ost.hidden_from(z, keep, 2.0), 2 * ost.hidden_from(z) * keep)
    # and the mistakes the GPU test must catch do change the exact scores
    for kind in ost.MUTATIONS:
        assert not torch.equal(ost.mutated_scores(tokens, w, kind), o["S"].sum(0)), kind
        assert torch.equal(ost.mutated_scores(tokens, w, kind).float().double(), ost.mutated_scores(tokens, w, kind)), kind


@pytest.mark.parametrize("C,std", [(128, 0.02), (128, 0.08), (768, 0.02)])
def test_salad_stage_error_bound_holds_plain_f32_and_rejects_mistakes(C, std):
    """stage_error_bounds: no element of a plain f32 implementation (torch on the CPU, another summation order than any
    kernel's) exceeds it, f32 with the K axis reversed neither; a dropped bias, exchanged rows and a zeroed W2 column do.
    Hidden values left unrounded exceed it at C = 128 only (the bound lets a hidden value move where z sits within eps_z of
    a rounding boundary, and eps_z grows with C): what catches them at every width is the RMS comparison of the GPU test,
    rms(err) <= 4 rms(plain f32 err), restated here on the oracle."""
    from oracle import salad_stages as ost
    B = 1
    tokens, w = ost.gaussian_inputs(C, B, seed=7, std=std)
    o = ost.salad_stage_outputs(tokens, w)
    ref = dict(S=o["S"].sum(0), F=o["F"].sum(0), g=o["g"])
    bS, bF, bg = ost.stage_error_bounds(tokens, w)
    assert bS.shape == ref["S"].shape and bF.shape == ref["F"].shape and bg.shape == ref["g"].shape
    flip = lambda v: v.flip(-1)
    for got in (ost.salad_mlps_f32(tokens, w),
                ost.salad_mlps_f32(flip(tokens), {k: flip(v) if k.startswith("w1") else v for k, v in w.items()})):
        ratios = [((a.double() - r).abs() / b).max().item() for a, r, b in zip(got, ref.values(), (bS, bF, bg))]
        print(f"\n[SALAD stage bound C={C} std={std}] max bound S {bS.max():.2e} F {bF.max():.2e} g {bg.max():.2e}; "
              f"f32 err / bound {[f'{r:.3f}' for r in ratios]}; S std {ref['S'].std():.3f}")
        assert max(ratios) <= 1.0
    assert bS.max().item() < 0.1 * ref["S"].std().item()          # loose, yet far below the signal
    for kind in ost.MUTATIONS:
        worst = ((ost.mutated_scores(tokens, w, kind) - ref["S"]).abs() / bS).max().item()
        print(f"  {kind}: err / bound {worst:.2f}")
        if kind != "skip_bf16_round":
            assert worst > 1.0, kind
        else:
            e_mut, e_f32 = (ost.mutated_scores(tokens, w, kind) - ref["S"]).pow(2).mean().sqrt().item(), (got[0].double() - ref["S"]).pow(2).mean().sqrt().item()
            print(f"  {kind}: rms err {e_mut:.2e} against plain f32 {e_f32:.2e}")
            assert (worst > 1.0) == (C == 128) and e_mut > 4 * 4 * e_f32


# ---------------------------------------------------------------- f32 SALAD stage oracle (oracle/salad_f32_stages.py)
def _shuffled_f32_gemm(a, w, bias, g):
    """The path's GEMM as a kernel may run it: the 6 K columns of the plane buffers in a random order, f32 throughout."""
    from oracle import salad_f32_stages as o32
    pa = o32.plane_values(o32.planes_in_order(a, o32.ACT_ORDER), torch.float32).reshape(a.shape[0], -1)
    pw = o32.plane_values(o32.planes_in_order(w, o32.WGT_ORDER), torch.float32).reshape(w.shape[0], -1)
    perm = torch.randperm(pa.shape[1], generator=g)
    return pa[:, perm] @ pw[:, perm].T + bias


def test_split3_planes_sum_back_and_pin_the_roundings():
    """split3 on the rounding cases: the planes sum back to x exactly, each is the nearest bf16 of its residual with ties
    to even (both parities occur at both roundings), residuals of both signs occur, -0 keeps its sign in h only, and no plane
    is a bf16 subnormal or infinite."""
    from oracle import salad_f32_stages as o32
    x = o32.rounding_cases()
    assert x.numel() % 4 == 0 and x.dtype == torch.float32
    mag = x[x != 0].abs()
    assert mag.min() >= 2.0 ** -60 and mag.max() <= 2.0 ** 60
    h, m, q = o32.split3(x)
    hv, mv, qv = (o32.plane_values(p) for p in (h, m, q))
    assert torch.equal(hv + mv + qv, x.double())
    for p in (hv, mv, qv):
        assert torch.isfinite(p).all() and (p[p != 0].abs() >= 2.0 ** -126).all()
    r1 = x.double() - hv
    tie1 = (r1.abs() * 2 == (osalad.bf16_round(hv * (1 + 2.0 ** -7)) - hv).abs()) & (r1 != 0)     # half a bf16 step of h's binade
    r2 = r1 - mv
    step2 = (osalad.bf16_round(mv * (1 + 2.0 ** -7)) - mv).abs()
    tie2 = (r2.abs() * 2 == step2) & (r2 != 0)
    for tie, plane in ((tie1, h), (tie2, m)):
        assert tie.sum() >= 8 and int((plane[tie] & 1).sum()) == 0              # resolved to the even mantissa, and ...
    assert (r1[tie1] > 0).any() and (r1[tie1] < 0).any() and (r2[tie2] > 0).any() and (r2[tie2] < 0).any()   # ... from both sides
    assert (mv < 0).any() and (mv > 0).any() and (qv < 0).any() and (qv > 0).any()
    assert ((mv == 0) & (x != 0)).any() and ((qv == 0) & (mv != 0)).any() and ((mv != 0) & (qv != 0)).any()
    zero = x == 0
    assert zero.sum() == 4 and sorted(h[zero].tolist()) == [-32768, -32768, 0, 0] and not m[zero].any() and not q[zero].any()
    # the six segments of each role are the planes in the documented order
    a, w = o32.planes_in_order(x.view(1, -1), o32.ACT_ORDER)[0], o32.planes_in_order(x.view(1, -1), o32.WGT_ORDER)[0]
    assert all(torch.equal(a[s], (q, h, m, m, h, h)[s]) and torch.equal(w[s], (h, q, m, h, m, h)[s]) for s in range(6))


@pytest.mark.parametrize("family,C", [("E0", 128), ("E0", 320), ("E1", 64), ("E1", 192), ("E2", 64), ("E2", 192)])
def test_exact_f32_salad_families_are_exact_in_any_order(family, C):
    """What tests/test_salad_f32_stages_gpu.py relies on when it asks the kernels for the plane model's bits.  E1 (layer 1)
    and E2 (layer 2): values on the three-plane grid, every kept product a multiple of 2^-18, sum|terms| + |b| < 64 = 2^24
    grid steps, so an f32 sum over the 6 K columns in ANY order is the f64 sum; all six segments contribute to most outputs.
    E0: one plane, the exact inputs of the bf16 path.  Every mutation moves the bits the family judges."""
    from oracle import salad_f32_stages as o32
    B, hidden = 2, 512
    tokens, w, o = o32.exact_case(family, C, B)
    judged = o32.FAMILIES[family][1]
    x, cls = tokens[:, 1:].reshape(-1, C), tokens[:, 0]
    g = torch.Generator().manual_seed(C)
    layers = {"H": (x, w["w1_sc"], w["b1_sc"]), "Ht": (cls, w["w1_t"], w["b1_t"]), "S": (o["H"][:, :hidden].contiguous(), w["w2_s"], w["b2_s"]),
              "F": (o["H"][:, hidden:].contiguous(), w["w2_c"], w["b2_c"]), "g": (o["Ht"], w["w2_t"], w["b2_t"])}
    for key in judged:
        a, wk, b = layers[key]
        seg = o32.segment_products(a, wk)
        want = seg.sum(0) + b.double()
        want = torch.relu(want) if key in ("H", "Ht") else want
        assert torch.equal(o[key].double(), want)
        for p in o32.split3(a) + o32.split3(wk):                       # planes sum back (split3 asserts exact residuals)
            assert torch.isfinite(o32.plane_values(p)).all()
        assert torch.equal(sum(o32.plane_values(p) for p in o32.split3(a)), a.double())
        got = _shuffled_f32_gemm(a, wk, b, g)
        got = torch.relu(got) if key in ("H", "Ht") else got
        assert torch.equal(got.double(), o[key].double()), key            # a permuted K order in f32 reproduces f64
        if family == "E0":                                                # one plane per operand: layer 1 has only (h,h) alive; the f32 hidden
            dead = (0, 1, 2, 3, 4) if key in ("H", "Ht") else (1, 2, 4)   # values do have m and q planes, the weights never
            assert not seg[list(dead)].any() and seg[5].any()
            continue
        if (family == "E2") == (key in ("H", "Ht")):
            continue                                                      # E2's first layer is a selection: exact, and not what it judges
        pa, pw = [o32.plane_values(p).abs() for p in o32.split3(a)], [o32.plane_values(p).abs() for p in o32.split3(wk)]
        mag = (sum(pa[i] @ pw[j].T for i, j in zip(o32.ACT_ORDER, o32.WGT_ORDER)) + b.double().abs()).max().item()
        alive = [(s != 0).double().mean().item() for s in seg]
        on_grid = all(torch.equal((s / o32.GRID).round(), s / o32.GRID) for s in seg) and torch.equal((b.double() / o32.GRID).round(), b.double() / o32.GRID)
        all_six = (seg != 0).all(0).double().mean().item()
        print(f"\n[{family} C={C}] {key}: sum|terms|+|b| <= {mag:.1f} (limit {o32.EXACT_LIMIT:.0f}); alive per segment {[f'{v:.2f}' for v in alive]}, all six {all_six:.2f}")
        assert on_grid and mag < o32.EXACT_LIMIT == 64 and min(alive) >= 0.8 and all_six >= 0.4
        assert (want != want.float().double()).sum() == 0
        # the plane model is the expected value, not the truth: it differs from true f64 by the dropped products only
        true = o32.true_stage_outputs(tokens, w)[key] if key in ("H", "Ht") else a.double() @ wk.double().T + b.double()
        gap, bound = (o[key].double() - true).abs(), o32.dropped_bound(a, wk)
        assert (gap <= bound + 1e-15).all() and gap.max() > 0
    assert (w["w1_sc"] != 0).sum(1).max() <= (o32.NNZ if family == "E1" else C) and (w["w2_s"] != 0).sum(1).max() <= (o32.NNZ if family == "E2" else hidden)
    for mutation in o32.MUTATIONS:
        kind, arg = mutation
        layer = arg[0] if kind == "drop_segment" else arg if kind == "act_order" else 2 if kind in ("hidden_bf16", "drop_b2_s") else 0
        if family == "E0" or (family == "E1" and layer == 2) or (family == "E2" and layer == 1):
            continue                                                      # E1 judges layer 1, E2 layer 2, E0 addressing
        mo = o32.f32_stage_outputs(tokens, w, mutation)
        assert any(not torch.equal(mo[k].double(), o[k].double()) for k in judged), mutation
    if family == "E0":                                                    # E0's mutations: the addressing ones
        for mutation in (("drop_b2_s", None), ("swap_token_rows", None), ("drop_segment", (1, 5)), ("drop_segment", (2, 5))):
            mo = o32.f32_stage_outputs(tokens, w, mutation)
            assert any(not torch.equal(mo[k].double(), o[k].double()) for k in judged), mutation


_rms64 = lambda a: a.double().pow(2).mean().sqrt().item()
F32_STAGE_G = 4.0              # tests/test_salad_f32_stages_gpu.py: rms(kernel - f64) <= G rms(torch f32 on the CPU - f64); the
                               # project's margin for another summation order, kept because an MI355X measures 0.32 ... 0.67


@pytest.mark.parametrize("C,std", [(128, 0.02), (768, 0.02), (768, 0.08)])
def test_f32_salad_stage_mutations_on_gaussian_inputs(C, std):
    """On the Gaussian cases of the GPU test: (1) the plane model itself — an exact six-product sum — is far closer to true
    f64 than plain f32, and plain f32 (two K orders) stays inside the per-element bound; (2) every mutation exceeds G times
    the plain-f32 RMS error on H, S, F or g, so G separates a right kernel from the mildest wrong one; (3) the faint ones
    (a low-order segment missing, no low planes at all, b2_s dropped) nevertheless leave the descriptor within
    F32_PATH_BOUND = 5e-7 of f64 — the bound tests/test_precision_gpu.py asserts cannot see them."""
    from oracle import salad_f32_stages as o32
    B = 3
    tokens, w = o32.gaussian_inputs(C, B, seed=31 * C + B, std=std)
    true, model, cpu = o32.true_stage_outputs(tokens, w), o32.f32_stage_outputs(tokens, w), o32.mlps_f32_cpu(tokens, w)
    bound = o32.stage_error_bounds(tokens, w)
    keys = ("H", "S", "F", "g")
    unit = {k: _rms64(cpu[k].double() - true[k]) for k in keys}
    flip = lambda v: v.flip(-1).contiguous()
    cpu_rev = o32.mlps_f32_cpu(flip(tokens), {k: flip(v) if k.startswith("w1") else v for k, v in w.items()})
    for k in keys + ("Ht",):
        assert ((model[k].double() - true[k]).abs() <= bound[k]).all() and ((cpu[k].double() - true[k]).abs() <= bound[k]).all()
        assert ((cpu_rev[k].double() - true[k]).abs() <= bound[k]).all()
    exact_ratio = {k: _rms64(model[k].double() - true[k]) / unit[k] for k in keys}
    print(f"\n[f32 SALAD stages C={C} std={std}] plain-f32 rms err {({k: f'{v:.2e}' for k, v in unit.items()})}; "
          f"plane model / plain f32 {({k: f'{v:.2f}' for k, v in exact_ratio.items()})}; "
          f"largest bound S {bound['S'].max():.2e} vs std {true['S'].std():.2f}")
    assert max(exact_ratio[k] for k in ("S", "F", "g")) < 0.5
    assert bound["S"].max().item() < 0.25 * true["S"].std().item()          # worst case of everything at once, yet below the signal
    ref_desc = osalad.sinkhorn_aggregate(true["S"].view(B, -1, 64), true["F"].view(B, -1, 128), true["g"], 0.7, 3)
    mildest = math.inf
    for mutation in o32.MUTATIONS:
        mo = o32.f32_stage_outputs(tokens, w, mutation)
        ratios = {k: _rms64(mo[k].double() - true[k]) / unit[k] for k in keys}
        over = max(((mo[k].double() - true[k]).abs() / bound[k]).max().item() for k in keys)
        line = f"  {mutation}: rms ratio {({k: f'{v:.2f}' for k, v in ratios.items()})}, max |err| / bound {over:.2f}"
        mildest = min(mildest, max(ratios[k] for k in ("H", "S", "F")))
        if mutation in o32.FAINT_MUTATIONS:
            desc = osalad.sinkhorn_aggregate(mo["S"].view(B, -1, 64), mo["F"].view(B, -1, 128), mo["g"], 0.7, 3)
            moved = (desc - ref_desc).abs().max().item()
            line += f", descriptor moved {moved:.2e}"
            assert moved < 5e-7, mutation
        print(line)
        assert max(ratios.values()) > F32_STAGE_G, mutation
    print(f"  mildest mutation: {mildest:.2f} x plain f32 (G = {F32_STAGE_G})")
    assert mildest > F32_STAGE_G
