"""GPU: the SALAD aggregation for 65 .. 1369 patch tokens (include/vpr_amd_salad_hires.h; 448 px = 1024 tokens, 518 px = 1369)
against oracle/salad.py (f64) and the closed-form known answers of SURVEY.md §8c, at the token counts where the
high-resolution kernel changes path: one past the minimum, fewer columns than threads, one column over a multiple of the
workgroup (257, 513, 769, 1025, 1281 ...), around its column-block size CB = 512 (511, 512, 513, 1024, 1025), not a multiple
of 16 (577, 593, 1369), an odd and an even number of columns per thread, and the maximum.  Tolerances are those of
tests/test_salad_gpu.py, tests/test_precision_gpu.py and tests/test_salad_anyres_gpu.py."""
import math

import numpy as np
import pytest
import torch

from oracle import salad as osalad

pytestmark = pytest.mark.gpu
TOL = 1e-4                        # one-call bf16 form vs the quantising oracle (tests/test_salad_gpu.py)
STAGE_TOL = 2e-6                  # stage A vs f64 (test_sinkhorn_stage_matches_oracle)
F32_PATH_BOUND = 5e-7             # tests/test_precision_gpu.py
CB = 512                          # HR_CB of csrc/salad_hires.hip: token columns per P block
STAGE_N = sorted({65, 66, 255, 256, 257, 529, 576, 577, 578, 592, 593, 768, 769, 1024, 1025, 1280, 1368, 1369,
                  CB - 1, CB, CB + 1, 2 * CB + 1})


def _stage_inputs(B, n, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, 64, generator=g) * scale, torch.randn(B, n, 128, generator=g), torch.randn(B, 256, generator=g)


def _run_stage(dev, scores, feats, tok, dustbin=1.0, iters=3, want_bf16=False):
    from vpr_amd import ops
    return ops.salad_sinkhorn_aggregate_hires(scores.to(dev), feats.to(dev), tok.to(dev), dustbin, iters, want_bf16=want_bf16)


def _weights(C, seed, hidden=512, m=64, l=128, t=256, std=0.02, bf16=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * std
    w = dict(w1_sc=r(2 * hidden, C), b1_sc=r(2 * hidden), w2_s=r(m, hidden), b2_s=r(m),
             w2_c=r(l, hidden), b2_c=r(l), w1_t=r(hidden, C), b1_t=r(hidden),
             w2_t=r(t, hidden), b2_t=r(t))
    if bf16:
        for k in list(w):
            if k.startswith("w"):
                w[k] = w[k].to(torch.bfloat16)
    return w


def _to_dev(w, dev, dustbin, f32=False):
    from vpr_amd import ops
    return (ops.SaladWeightsF32 if f32 else ops.SaladWeights)(**{k: v.to(dev) for k, v in w.items()}, dustbin=dustbin)


# ------------------------------------------------------------------------------------------------ stage A kernel
@pytest.mark.parametrize("n", STAGE_N)
def test_stage_matches_oracle(dev, n):
    scores, feats, tok = _stage_inputs(3, n, seed=n)
    ref = osalad.sinkhorn_aggregate(scores, feats, tok, 1.0, 3)
    out, out16 = _run_stage(dev, scores, feats, tok, want_bf16=True)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"n={n}: stage A max abs err {err:.3e}")
    assert torch.isfinite(out).all() and err < STAGE_TOL
    assert torch.equal(out16.cpu(), out.cpu().to(torch.bfloat16))


@pytest.mark.parametrize("iters", [1, 3, 7])
def test_iteration_count(dev, iters):
    scores, feats, tok = _stage_inputs(2, 1369, seed=iters, scale=1.0)
    ref = osalad.sinkhorn_aggregate(scores, feats, tok, 0.5, iters)
    out, _ = _run_stage(dev, scores, feats, tok, 0.5, iters)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"iters={iters}: {err:.3e}")
    assert err < STAGE_TOL


@pytest.mark.parametrize("n", [600, 1369])
def test_closed_forms(dev, n):
    """all scores == dustbin -> P = 1/n for every cluster, every cluster vector = normalize(mean_j F) /
    sqrt(65), all 64 columns identical; squared-norm shares 1/65 (token block) and 1/65 per cluster; token-permutation
    invariance; shift of scores and dustbin together."""
    scores, feats, tok = _stage_inputs(1, n, seed=1000 + n, scale=1.0)
    out = _run_stage(dev, torch.full((1, n, 64), 1.0), feats, tok)[0].cpu().double()[0]
    V = out[256:].reshape(128, 64)
    mean_dir = torch.nn.functional.normalize(feats[0].double().mean(0), dim=0) / math.sqrt(65.0)
    assert (V - mean_dir[:, None]).abs().max().item() < 1e-6
    assert (V - V[:, :1]).abs().max().item() < 1e-6
    t_ref = torch.nn.functional.normalize(tok[0].double(), dim=0) / math.sqrt(65.0)
    assert (out[:256] - t_ref).abs().max().item() < 1e-6
    run = lambda s, f, d: _run_stage(dev, s, f, tok, d)[0].cpu().double()[0]
    out = run(scores, feats, 1.0)
    assert abs(out.pow(2).sum().item() - 1.0) < 1e-6
    assert abs(out[:256].pow(2).sum().item() - 1.0 / 65.0) < 1e-6
    assert (out[256:].reshape(128, 64).pow(2).sum(0) - 1.0 / 65.0).abs().max().item() < 1e-6
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    assert (run(scores[:, perm], feats[:, perm], 1.0) - out).abs().max().item() < 1e-6
    assert (run(scores + 3.25, feats, 1.0 + 3.25) - out).abs().max().item() < 1e-6


@pytest.mark.parametrize("n", [577, 1369])
@pytest.mark.parametrize("case", ["wide", "dead_column", "hot_row", "all_equal_rows"])
def test_exp_domain_survives_extreme_scores(dev, case, n):
    """The four cases of tests/test_salad_gpu.py::test_sinkhorn_exp_domain_survives_extreme_scores at these token counts."""
    scores, feats, tok = _stage_inputs(3, n, seed=77, scale=1.0)
    if case == "wide":
        scores = scores * 50.0
    elif case == "dead_column":
        scores[:, 17, :] -= 300.0
    elif case == "hot_row":
        scores[:, :, 5] += 300.0
    else:
        scores[:, :, ::2] = 2.5
    ref = osalad.sinkhorn_aggregate(scores, feats, tok, 1.0, 3)
    assert torch.isfinite(ref).all()
    out, _ = _run_stage(dev, scores, feats, tok)
    assert torch.isfinite(out).all()
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"{case} n={n}: max abs err {err:.2e}")
    assert err < 5e-6


@pytest.mark.parametrize("n", [577, 1025, 1369])
def test_guard_rows(dev, n):
    """The three inputs as 16-byte-aligned views inside larger allocations whose other elements are NaN — more than one
    image's worth before and behind: a pad token that is loaded instead of predicated away, or a row index that runs past
    its image, would put a NaN into the output.  Every byte a correct kernel reads lies inside the view."""
    from vpr_amd import ops
    B = 2
    scores, feats, tok = _stage_inputs(B, n, seed=31 * n)
    plain, plain16 = _run_stage(dev, scores, feats, tok, want_bf16=True)

    def guarded(t, per_image):
        lead = (per_image + 3) // 4 * 4 + 4                       # >= one image, a multiple of 4 floats: the view stays 16-byte aligned
        buf = torch.full((lead + t.numel() + lead,), float("nan"), dtype=torch.float32, device=dev)
        view = buf[lead: lead + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 0 and view.is_contiguous()
        return buf, view

    bufs = [guarded(scores, n * 64), guarded(feats, n * 128), guarded(tok, 256)]
    out, out16 = ops.salad_sinkhorn_aggregate_hires(bufs[0][1], bufs[1][1], bufs[2][1], 1.0, 3, want_bf16=True)
    assert torch.isfinite(out).all()
    assert torch.equal(out, plain) and torch.equal(out16, plain16)


def test_images_are_independent_of_batch_and_position(dev):
    scores, feats, tok = _stage_inputs(5, 1369, seed=5)
    full, _ = _run_stage(dev, scores, feats, tok)
    again, _ = _run_stage(dev, scores, feats, tok)
    assert torch.equal(full, again)
    for b in range(5):
        alone, _ = _run_stage(dev, scores[b:b + 1], feats[b:b + 1], tok[b:b + 1])
        assert torch.equal(alone[0], full[b]), b
    order = [3, 0, 4]                                             # another batch size, other positions
    moved, _ = _run_stage(dev, scores[order], feats[order], tok[order])
    for pos, b in enumerate(order):
        assert torch.equal(moved[pos], full[b]), (pos, b)


@pytest.mark.parametrize("n", [256, 529, 576])
def test_against_the_other_stage_a_kernels(dev, n):
    """The direct A/B where two kernels are defined: each within the stage tolerance of the oracle (bits may differ)."""
    from vpr_amd import ops
    scores, feats, tok = _stage_inputs(4, n, seed=n + 1)
    ref = osalad.sinkhorn_aggregate(scores, feats, tok, 1.0, 3)
    new, _ = _run_stage(dev, scores, feats, tok)
    old, _ = ops.salad_sinkhorn_aggregate_n(scores.to(dev), feats.to(dev), tok.to(dev), 1.0, 3)
    e_new, e_old = (new.cpu().double() - ref).abs().max().item(), (old.cpu().double() - ref).abs().max().item()
    print(f"n={n}: high-resolution kernel {e_new:.3e}, run-time-n kernel {e_old:.3e}, mutual {(new - old).abs().max().item():.3e}")
    assert e_new < STAGE_TOL and e_old < STAGE_TOL


# ------------------------------------------------------------------------------------------------ one-call forms
@pytest.mark.parametrize("C,B,n", [(64, 2, 577), (128, 3, 1369), (384, 1, 1369), (768, 2, 577), (1024, 2, 1369)])
def test_one_call_form_matches_oracle(dev, C, B, n):
    """The (C, hidden) shapes of tests/test_salad_anyres_gpu.py: C = 64 takes the gemm_nt fallback of layer 1, the others the
    ragged 256-row tiles.  The hub layout [B, 1+n, C] and a contiguous (patch, cls) pair are the same numbers through
    other addresses."""
    from vpr_amd import ops
    g = torch.Generator().manual_seed(C + B + n)
    tokens = torch.randn(B, 1 + n, C, generator=g).to(torch.bfloat16)
    w = _weights(C, seed=C + n)
    ref = osalad.salad_aggregate(tokens, w, dustbin=1.0, iters=3, quantize=True)
    td, wd = tokens.to(dev), _to_dev(w, dev, 1.0)
    out, out16 = ops.salad_aggregate_hires(td, wd, 3, want_bf16=True)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"C={C} B={B} n={n}: max abs err {err:.3e}")
    assert err < TOL
    assert torch.equal(out16.cpu(), out.cpu().to(torch.bfloat16))
    pair, pair16 = ops.salad_aggregate_hires((td[:, 1:].contiguous(), td[:, 0].contiguous()), wd, 3, want_bf16=True)
    assert torch.equal(pair, out) and torch.equal(pair16, out16)


@pytest.mark.parametrize("C,B,n", [(128, 2, 1369), (768, 2, 577)])
def test_f32_form_matches_f64_on_f32_operands(dev, C, B, n):
    from vpr_amd import ops
    g = torch.Generator().manual_seed(2000 + C + n)
    tokens = torch.randn(B, 1 + n, C, generator=g)
    w = _weights(C, seed=C + 1, bf16=False)
    ref = osalad.salad_aggregate(tokens, w, 1.0, 3, quantize=False)
    td, w32 = tokens.to(dev), _to_dev(w, dev, 1.0, f32=True)
    out, out16 = ops.salad_aggregate_f32_hires(td, w32, 3, want_bf16=True)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"f32 form C={C} n={n}: {err:.3e}")
    assert err < F32_PATH_BOUND
    assert torch.equal(out16.cpu(), out.cpu().to(torch.bfloat16))
    pair, _ = ops.salad_aggregate_f32_hires((td[:, 1:].contiguous(), td[:, 0].contiguous()), w32, 3)
    assert torch.equal(pair, out)


def test_one_call_form_at_256_and_529_is_the_existing_chain(dev):
    from vpr_amd import ops
    g = torch.Generator().manual_seed(12)
    wd = _to_dev(_weights(768, seed=3), dev, 0.7)
    td = torch.randn(3, 257, 768, generator=g).to(torch.bfloat16).to(dev)
    patch, cls = td[:, 1:].contiguous(), td[:, 0].contiguous()
    want, want16 = ops.salad_aggregate_split(patch, cls, wd, 3, True, overlap=False)
    got, got16 = ops.salad_aggregate_hires((patch, cls), wd, 3, want_bf16=True)
    hub, _ = ops.salad_aggregate_hires(td, wd, 3)
    assert torch.equal(got, want) and torch.equal(got16, want16) and torch.equal(hub, want)
    td = torch.randn(2, 530, 768, generator=g).to(torch.bfloat16).to(dev)
    want, want16 = ops.salad_aggregate_n(td, wd, 3, want_bf16=True)
    got, got16 = ops.salad_aggregate_hires(td, wd, 3, want_bf16=True)
    assert torch.equal(got, want) and torch.equal(got16, want16)


def test_f32_form_at_256_and_529_is_the_existing_chain(dev):
    from vpr_amd import ops
    g = torch.Generator().manual_seed(13)
    w32 = _to_dev(_weights(128, seed=4, bf16=False), dev, 1.0, f32=True)
    tokens = torch.randn(2, 257, 128, generator=g).to(dev)
    want, want16 = ops.salad_aggregate_f32(tokens, w32, 3, want_bf16=True)
    got, got16 = ops.salad_aggregate_f32_hires(tokens, w32, 3, want_bf16=True)
    assert torch.equal(got, want) and torch.equal(got16, want16)
    tokens = torch.randn(2, 530, 128, generator=g).to(dev)
    want, want16 = ops.salad_aggregate_f32_n(tokens, w32, 3, want_bf16=True)
    got, got16 = ops.salad_aggregate_f32_hires(tokens, w32, 3, want_bf16=True)
    assert torch.equal(got, want) and torch.equal(got16, want16)


def test_refused_calls_raise_by_status_name(dev):
    from vpr_amd import ops
    scores, feats, tok = _stage_inputs(1, 1370, seed=1)
    with pytest.raises(RuntimeError, match="vpr_salad_sinkhorn_aggregate_hires failed"):
        _run_stage(dev, scores, feats, tok)
    tokens = torch.zeros(1, 1371, 128, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="vpr_salad_aggregate_hires failed"):
        ops.salad_aggregate_hires(tokens, _to_dev(_weights(128, seed=1), dev, 1.0), 3)


# ------------------------------------------------------------------------------------------------------- modules
def _extractor(dev, img_size, seed):
    from vpr_amd.modules import DinoV2Salad
    torch.manual_seed(seed)
    ext = DinoV2Salad("vit_small", img_size=img_size).to(dev).to(torch.bfloat16).eval()
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    ext.backbone.fold_layerscale()
    return ext


def _oracle_on_own_tokens(ext, x):
    w = ext.aggregator.pack()
    wcpu = {k: getattr(w, k).cpu() for k in ("w1_sc", "b1_sc", "w2_s", "b2_s", "w2_c", "b2_c", "w1_t", "b1_t", "w2_t", "b2_t")}
    return osalad.salad_aggregate(ext.tokens(x).cpu(), wcpu, w.dustbin, 3)


@pytest.mark.parametrize("img_size,n", [(448, 1024), (518, 1369)])
def test_extractor_at_448_and_518(dev, img_size, n):
    """The construction of tests/test_salad_anyres_gpu.py::test_extractor_at_other_image_sizes: the aggregator isolated from
    the backbone — features(x) against the oracle on the module's own tokens(x) — and GraphedForward returning the eager bits."""
    from vpr_amd.graphed import GraphedForward
    ext = _extractor(dev, img_size, seed=img_size)
    assert ext.backbone.num_patches == n
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(2, 3, img_size, img_size, device=dev, generator=g).to(torch.bfloat16)
    d, d16 = ext.features(x, want_bf16=True)
    assert ext.backbone.cls_tail_hook is None
    ref = _oracle_on_own_tokens(ext, x)
    err = (d.cpu().double() - ref).abs().max().item()
    print(f"img_size={img_size}: features vs oracle on own tokens {err:.3e}")
    assert d.shape == (2, 8448) and err < TOL
    assert (d.double().pow(2).sum(1) - 1.0).abs().max().item() < 1e-5                 # unit-norm descriptors
    assert torch.equal(d16.cpu(), d.cpu().to(torch.bfloat16))
    fwd = GraphedForward(lambda t: ext.features(t, want_bf16=True), module=ext)
    try:
        for _ in range(2):                                        # capture, then a replay on other images
            xb = torch.randn(2, 3, img_size, img_size, device=dev, generator=g).to(torch.bfloat16)
            e, e16 = ext.features(xb, want_bf16=True)
            r, r16 = fwd(xb)
            assert torch.equal(r, e) and torch.equal(r16, e16)
        assert fwd.fallback_reason is None and fwd.graphs() == 1
    finally:
        fwd.close()


def test_retrieval_evaluation_at_518(dev, tmp_path):
    """evaluate.build_gallery_from_images + calculate_retrieval_scores with image_size=518 on a 518 px extractor: every
    validation image is a lightly perturbed copy of one gallery image and finds it (the 322 px test's construction)."""
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, modules
    rng = np.random.default_rng(518)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g = 6
    gnames = [f"img_{i:04d}.png" for i in range(n_g)]
    imgs = [rng.integers(0, 256, (330, 340, 3), dtype=np.uint8) for _ in range(n_g)]
    for name, im in zip(gnames, imgs):
        Image.fromarray(im).save(gdir / name)
    lat, lon, ang = 219000 + 100.0 * np.arange(n_g), 143000 + 50.0 * np.arange(n_g), (17.0 * np.arange(n_g)) % 360
    pd.DataFrame({"filename": gnames, "timestamp": "t", "latitude": lat, "longitude": lon, "angle": ang,
                  "Region_ID": np.arange(n_g) // 2}).to_csv(tmp_path / "labels_train.csv", index=False)
    src = [4, 1, 5]
    vnames = [f"img_{i:04d}.png" for i in range(len(src))]
    for name, s in zip(vnames, src):
        noisy = np.clip(imgs[s].astype(np.int16) + rng.integers(-3, 4, imgs[s].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(vdir / name)
    pd.DataFrame({"filename": vnames, "timestamp": "t", "latitude": lat[src] + 3.0, "longitude": lon[src] - 4.0,
                  "angle": (ang[src] + 5.0) % 360, "Region_ID": np.array(src) // 2}).to_csv(tmp_path / "labels_val.csv", index=False)
    torch.manual_seed(1)
    ext = modules.DinoV2Salad("vit_base", img_size=518)
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    assert evaluate.build_gallery_from_images(ext, str(tmp_path / "labels_train.csv"), str(gdir), str(tmp_path / "gal"),
                                              batch_size=4, image_size=518) == n_g
    res = evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "labels_val.csv"), str(vdir), k=3,
                                              tau=10.0, batch_size=2, verbose=False, image_size=518)
    assert res["topk_indices"][:, 0].tolist() == src
    assert res["final_loss"] == pytest.approx(0.5 * (9.0 + 16.0)) and res["maae"] == pytest.approx(5.0)
    assert res["recall_at_1_tau"] == 1.0 and res["recall_at_1_region"] == 1.0
