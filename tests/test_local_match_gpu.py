"""GPU: vpr_local_rerank (include/vpr_amd_local.h) against its f64 restatement (tests/local_match_ref.py): bit for bit on integer
features (every similarity an exact integer, full of ties: the lowest-index rule and the padding masks), as epsilon-argmaxes on
Gaussian unit features, the recipe with the true image last, the edges of the contract, and bit-identity across batch, position,
padding, runs, optional outputs and graph replay."""
import numpy as np
import pytest
import torch

import local_match_ref as ref

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def run(dev, q, idx, g, base=0, k=None, min_sim=0.0, debug=True):
    from vpr_amd import ops
    out = ops.local_rerank(q.to(dev), idx.to(dev), g.to(dev), base, k, min_sim, debug=debug)
    torch.cuda.synchronize()
    res = dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy())
    if debug:
        res.update({f: getattr(out[3], f).cpu().numpy() for f in out[3]._fields})
    return res


def int_features(rng, *shape):
    return torch.from_numpy(rng.integers(-2, 3, shape).astype(np.float32)).to(torch.bfloat16)


def candidates(rng, B, kc, n_local, base):
    """Mostly rows of the shard (duplicates included), some padding and foreign rows."""
    idx = rng.integers(base, base + n_local, (B, kc))
    other = rng.choice(np.array([-1, base - 1, base + n_local, I32_MIN, I32_MAX, -7]), (B, kc))
    return torch.from_numpy(np.where(rng.random((B, kc)) < 0.2, other, idx).astype(np.int32))


def assert_equal_bits(got, want, fields):
    for f in fields:
        a, b = got[f], want[f]
        assert a.shape == b.shape and a.dtype == b.dtype, f
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (f, np.argwhere(a.view(np.int32) != b.view(np.int32))[:5])


ALL = ("row_nn", "col_nn", "pair_matches", "pair_score", "vals", "idx", "matches")

# (B, kc, k_out, n_q, n_g, l): every n in {1, 31, 32, 33, 64, 65, 196, 255, 256} on both sides with n_q != n_g included, every l,
# every B, every kc, k_out in {1, kc}; the large B x kc products ride on small images, the large images on small lists
SHAPES = [(1, 1, 1, 1, 1, 32), (3, 7, 1, 31, 33, 32), (3, 8, 8, 32, 32, 64), (3, 9, 9, 33, 31, 64), (1, 7, 7, 64, 65, 128),
          (1, 8, 1, 65, 64, 256), (3, 9, 9, 196, 196, 128), (1, 7, 7, 255, 256, 256), (1, 8, 8, 256, 255, 128), (1, 9, 1, 256, 256, 256),
          (37, 64, 64, 31, 32, 32), (37, 128, 128, 1, 33, 32), (3, 128, 1, 33, 1, 64), (1, 64, 64, 196, 255, 32), (3, 1, 1, 256, 196, 64),
          (1, 9, 9, 64, 256, 96), (1, 7, 7, 65, 33, 160), (3, 8, 1, 33, 255, 192), (1, 9, 9, 255, 65, 224)]


@pytest.mark.parametrize("B,kc,k,n_q,n_g,l", SHAPES)
def test_integer_features_bit_for_bit(dev, B, kc, k, n_q, n_g, l):
    """Entries in -2 .. 2: |S| <= 4 l <= 1024 and a score <= 256 * 1024 < 2^24 are exact in f32 whatever the order of the sums."""
    rng = np.random.default_rng(B * 1000 + kc * 7 + n_q + n_g + l)
    n_local, base = 11, 5
    q, g = int_features(rng, B, n_q, l), int_features(rng, n_local, n_g, l)
    idx = candidates(rng, B, kc, n_local, base)
    for min_sim in (0.0, 3.0):
        got = run(dev, q, idx, g, base, k, min_sim)
        want = ref.local_rerank(q, idx, g, base, k, min_sim)
        assert_equal_bits(got, want, ALL)
    assert (want["pair_matches"] > 0).any() or n_q * n_g == 1


@pytest.mark.parametrize("B,kc,n_q,n_g,l", [(2, 5, 256, 256, 128), (3, 4, 196, 255, 64), (2, 3, 33, 65, 256), (2, 8, 64, 31, 32)])
def test_gaussian_unit_features_are_epsilon_argmaxes(dev, B, kc, n_q, n_g, l):
    """e[i][j] = l 2^-24 sum_d |q g| bounds the f32 MFMA sum (the K u S term of oracle/gemm.py's gemm_bound).  Every device
    choice must be an epsilon-argmax, no row or column left out; given the device's own neighbours the match count is integer
    logic; the score is within sum_matched e + gamma_L_sum sum_matched |S| of the f64 sum."""
    rng = np.random.default_rng(n_q + n_g + l)
    n_local = 7
    q = torch.from_numpy(ref.unit(rng.standard_normal((B, n_q, l)))).to(torch.bfloat16)
    g = torch.from_numpy(ref.unit(rng.standard_normal((n_local, n_g, l)))).to(torch.bfloat16)
    g[3, : min(n_g, n_q)] = q[0, : min(n_g, n_q)]                          # one image shares the first query's patches
    idx = torch.from_numpy(rng.integers(0, n_local, (B, kc)).astype(np.int32))
    idx[0, 0] = 3
    q64, g64, cand = ref.f64(q), ref.f64(g), idx.numpy()
    worst = 0.0
    for min_sim in (0.0, 0.25):
        got = run(dev, q, idx, g, 0, None, min_sim)
        for b in range(B):
            for t in range(kc):
                S = q64[b] @ g64[cand[b, t]].T
                e = l * ref.U * (np.abs(q64[b]) @ np.abs(g64[cand[b, t]]).T)
                r, c = got["row_nn"][b, t], got["col_nn"][b, t]
                assert (r >= 0).all() and (r < n_g).all() and (c >= 0).all() and (c < n_q).all()
                i, j = np.arange(n_q), np.arange(n_g)
                assert (S[i, r] + e[i, r] >= (S - e).max(1)).all()
                assert (S[c, j] + e[c, j] >= (S - e).max(0)).all()
                mutual = r[c] == j
                assert (np.abs(S[c, j][mutual] - np.float32(min_sim)) > e.max()).all()     # min_sim decides no pair by rounding
                m = mutual & (S[c, j] >= np.float32(min_sim))
                assert got["pair_matches"][b, t] == m.sum()
                exact = S[c, j][m].sum()
                bound = e[c, j][m].sum() + ref.gamma(ref.SUM_ROUNDINGS) * np.abs(S[c, j][m]).sum()
                err = abs(float(got["pair_score"][b, t]) - exact)
                assert err <= bound, (b, t, err, bound)
                if bound > 0:
                    worst = max(worst, err / bound)
        if min_sim == 0.25:
            assert got["pair_matches"][0, 0] >= min(n_q, n_g) and got["idx"][0, 0] == 3
    print(f"local_rerank score error, largest fraction of its bound at ({n_q}, {n_g}, {l}): {worst:.4f}")


@pytest.mark.parametrize("n,l", [(64, 32), (33, 32), (256, 128)])
def test_recipe_true_image_comes_back_first(dev, n, l):
    q, gal = ref.recipe(3, n, l)
    N = gal.shape[0]
    idx = torch.arange(N, dtype=torch.int32)[None]                         # the true image at the last position of the list
    got = run(dev, q, idx, gal, 0, None, 0.0)
    assert got["idx"][0, 0] == N - 1 and got["matches"][0, 0] == n and 0.995 * n <= got["vals"][0, 0] <= 1.004 * n
    assert got["pair_score"][0, :N - 1].max() < got["vals"][0, 0] / 2
    if l == 128:
        hard = run(dev, q, idx, gal, 0, None, 0.6)
        assert (hard["pair_score"][0, :N - 1] == 0).all() and (hard["pair_matches"][0, :N - 1] == 0).all()
        assert hard["idx"][0, 0] == N - 1 and hard["matches"][0, 0] == n
        assert hard["idx"][0, 1:].tolist() == list(range(N - 1))           # all-zero scores: by ascending index


def test_edges(dev):
    rng = np.random.default_rng(17)
    n_q, n_g, l, base, n_local = 40, 37, 64, 100, 6
    q, g = int_features(rng, 4, n_q, l), int_features(rng, n_local, n_g, l)
    nan, inf = float("nan"), float("inf")
    g[1] = nan                                                             # never named by a live index: never read
    g[2, 3], g[2, 9, 5], g[2, 11, 0], g[2, 12, 1] = nan, nan, inf, -inf     # a live image with NaN and Inf rows
    g[4, 20:] = 0                                                          # zero feature rows
    q[1, 5], q[1, 6, 2] = inf, nan                                         # and a query with such rows
    q[3] = 0                                                               # an all-zero query: every S is 0, ties everywhere
    idx = torch.tensor([[102, -1, I32_MIN, I32_MAX, 99, 106, 102, 100, 104, 1, 2],
                        [105, 102, 102, 104, -1, -1, 103, 100, 106, 99, 0],
                        [-1, I32_MIN, I32_MAX, 99, 106, 1, 2, 3, 4, 5, -7],         # an all-padding query
                        [104, 100, 103, 105, 102, 104, -1, -1, -1, -1, -1]], dtype=torch.int32)
    assert not (idx == 101).any()
    for k in (1, 11):
        got = run(dev, q, idx, g, base, k, 0.0)
        want = ref.local_rerank(q, idx, g, base, k, 0.0)
        assert_equal_bits(got, want, ALL)
    assert np.isfinite(got["pair_score"][idx.numpy() == 102]).all()
    t = got["col_nn"][0, 0]
    assert t[3] == -1 and t[9] == -1 and t[11] == -1 and t[12] == -1 and not (got["row_nn"][0, 0][:, None] == [3, 9, 11, 12]).any()
    assert (got["row_nn"][1, 1][[5, 6]] == -1).all()
    assert (got["vals"][2] == -np.inf).all() and (got["idx"][2] == -1).all() and (got["matches"][2] == 0).all()
    assert got["idx"][0].tolist().count(102) == 2                          # duplicates: scored as often as they occur
    assert got["idx"][3].tolist() == [100, 102, 103, 104, 104, 105, -1, -1, -1, -1, -1] and (got["vals"][3, :6] == 0).all()
    # a shard that owns nothing of the list, and min_sim above every similarity
    none = run(dev, q, idx, g, 1000, 3, 0.0)
    assert (none["idx"] == -1).all() and (none["vals"] == -np.inf).all() and (none["pair_score"] == -np.inf).all()
    high = run(dev, q, idx, g, base, 11, 1e6)
    assert (high["pair_matches"] == 0).all() and (high["matches"] == 0).all()
    assert_equal_bits(high, ref.local_rerank(q, idx, g, base, 11, 1e6), ALL)


def test_bit_identical_across_batch_position_padding_runs_and_outputs(dev):
    from vpr_amd import ops
    rng = np.random.default_rng(23)
    B, kc, n_q, n_g, l, n_local, base = 9, 10, 70, 67, 96, 13, 40
    q = torch.from_numpy(ref.unit(rng.standard_normal((B, n_q, l)))).to(torch.bfloat16)
    g = torch.from_numpy(ref.unit(rng.standard_normal((n_local, n_g, l)))).to(torch.bfloat16)
    idx = candidates(rng, B, kc, n_local, base)
    full = run(dev, q, idx, g, base, 4, 0.05)
    again = run(dev, q, idx, g, base, 4, 0.05)
    assert_equal_bits(again, full, ALL)                                    # across runs
    plain = run(dev, q, idx, g, base, 4, 0.05, debug=False)                # without the optional outputs
    assert_equal_bits(plain, full, ("vals", "idx", "matches"))
    perm = torch.from_numpy(rng.permutation(B))
    moved = run(dev, q[perm], idx[perm], g, base, 4, 0.05)                 # across position in the batch
    assert_equal_bits({f: moved[f][np.argsort(perm.numpy())] for f in ALL}, full, ALL)
    for b in (0, 4, 8):                                                    # across B
        one = run(dev, q[b:b + 1], idx[b:b + 1], g, base, 4, 0.05)
        assert_equal_bits(one, {f: full[f][b:b + 1] for f in ALL}, ALL)
    pad = torch.cat([idx, torch.full((B, 7), -1, dtype=torch.int32)], 1)   # across trailing padding (another grid, too)
    padded = run(dev, q, pad, g, base, 4, 0.05)
    assert_equal_bits(padded, full, ("vals", "idx", "matches"))
    assert_equal_bits({f: padded[f][:, :kc] for f in ("pair_score", "pair_matches", "row_nn", "col_nn")}, full,
                      ("pair_score", "pair_matches", "row_nn", "col_nn"))
    # under graph replay, with new inputs copied into the captured tensors
    qd, id_, gd = q.to(dev), idx.to(dev), g.to(dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.local_rerank(qd, id_, gd, base, 4, 0.05)                       # warm-up: workspace, LDS opt-in
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.local_rerank(qd, id_, gd, base, 4, 0.05)
    for order in (perm, torch.arange(B)):
        qd.copy_(q[order])
        id_.copy_(idx[order])
        graph.replay()
        torch.cuda.synchronize()
        eager = run(dev, q[order], idx[order], g, base, 4, 0.05, debug=False)
        assert_equal_bits(dict(vals=out[0].cpu().numpy(), idx=out[1].cpu().numpy(), matches=out[2].cpu().numpy()), eager,
                          ("vals", "idx", "matches"))


def test_torch_op_and_sharded_merge(dev):
    """torch.ops.vpr.local_rerank is the wrapper; R hand-made shards scored apart and merged (vpr_topk_merge) give the single
    shard's answer."""
    from vpr_amd import ops, torch_ops  # noqa: F401  (registers torch.ops.vpr.*)
    rng = np.random.default_rng(31)
    B, kc, n, l, N = 5, 12, 50, 64, 23
    q, g = int_features(rng, B, n, l), int_features(rng, N, n, l)
    idx = torch.stack([torch.from_numpy(rng.permutation(N)[:kc].astype(np.int32)) for _ in range(B)])
    want = ref.local_rerank(q, idx, g, 0, 6, 2.0)
    v, i, m = torch.ops.vpr.local_rerank(q.to(dev), idx.to(dev), g.to(dev), 0, 6, 2.0)
    assert_equal_bits(dict(vals=v.cpu().numpy(), idx=i.cpu().numpy(), matches=m.cpu().numpy()), want, ("vals", "idx", "matches"))
    for R in (2, 3):
        vs, is_ = [], []
        for r in range(R):
            lo, hi = N * r // R, N * (r + 1) // R
            sv, si, _ = ops.local_rerank(q.to(dev), idx.to(dev), g[lo:hi].contiguous().to(dev), lo, 6, 2.0)
            vs.append(sv)
            is_.append(si)
        mv, mi = ops.topk_merge(torch.stack(vs), torch.stack(is_))
        assert np.array_equal(mi.cpu().numpy(), want["idx"]) and np.array_equal(mv.cpu().numpy(), want["vals"])


# -------------------------------------------------------------------------------------------------- integration
def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def rccl_one_rank(dev):
    import os
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dev
    dist.destroy_process_group()


def place_gallery(dev, seed, N=512, D=128, B=8, n=20, l=32, **kw):
    """ref.places as a bf16 ShardedGallery with local features; returns (gallery, queries, their local features, true rows)."""
    from vpr_amd.retrieval import ShardedGallery
    rows, local, q, ql, true = ref.places(seed, N, D, B, n, l)
    return ShardedGallery(rows.to(dev), N, local_feats=local.to(dev), **kw), q.to(dev), ql.to(dev), true


def test_search_local_reranked_finds_the_view_the_global_search_cannot(dev):
    sg, q, ql, true = place_gallery(dev, 2)
    k, kc = 4, 16
    v, i = sg.search_local_reranked(q, k, kc, ql, 0.3)
    _, ci = sg.search(q, kc)
    want = ref.local_rerank(ql.cpu(), ci.cpu(), sg.local_feats.cpu(), 0, k, 0.3)
    assert np.array_equal(i.cpu().numpy(), want["idx"]) and np.array_equal(i[:, 0].cpu().numpy(), true)
    assert np.abs(v.cpu().numpy() - want["vals"]).max() <= 20 * 32 * ref.U * 2 + 20 * ref.gamma(ref.SUM_ROUNDINGS) * 1.01
    assert not np.array_equal(ci[:, 0].cpu().numpy(), true)
    for a, b in zip(sg.search_local_queries(q, k, local_rerank=kc, q_local_feats=ql, min_sim=0.3), (v, i)):
        assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="local_rerank and rerank"):
        sg.search_local_queries(q, k, rerank=kc, local_rerank=kc, q_local_feats=ql)


def test_one_rank_collective_path_equals_local_path(rccl_one_rank):
    dev = rccl_one_rank
    local, q, ql, _ = place_gallery(dev, 4)
    coll, _, _, _ = place_gallery(dev, 4, force_collectives=True)
    assert coll.collective and not local.collective
    for a, b in zip(local.search_local_reranked(q, 5, 16, ql, 0.2), coll.search_local_reranked(q, 5, 16, ql, 0.2)):
        assert torch.equal(bits(a), bits(b))
    kw = dict(local_rerank=16, q_local_feats=ql, min_sim=0.2)
    for a, b in zip(local.search_local_queries(q, 5, **kw), coll.search_local_queries(q, 5, **kw)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("collective", [False, True])
def test_graphed_local_rerank_equals_eager(rccl_one_rank, collective):
    from vpr_amd.retrieval import GraphedRetrieval
    dev = rccl_one_rank
    B, k, kc = 8, 5, 16
    sg, q0, ql0, _ = place_gallery(dev, 6, force_collectives=collective)
    gr = GraphedRetrieval(sg, B, k, local_rerank=kc, min_sim=0.2)
    assert gr.q_feats.shape == ql0.shape and gr.q_feats.dtype == torch.bfloat16
    plain = GraphedRetrieval(sg, B, k)
    _, q1, ql1, _ = place_gallery(dev, 7)
    for seed, (q, ql) in enumerate(((q0, ql0), (q0.roll(3, 0).contiguous(), ql0.roll(3, 0).contiguous()), (q1, ql1))):
        v_g, i_g = gr(q, ql)
        v_g, i_g = v_g.clone(), i_g.clone()
        v_e, i_e = sg.search_local_reranked(q, k, kc, ql, 0.2)
        assert torch.equal(i_g, i_e) and torch.equal(bits(v_g), bits(v_e)), seed
        v_p, i_p = plain(q)
        v_1, i_1 = sg.search(q, k)
        assert torch.equal(i_p, i_1) and torch.equal(bits(v_p), bits(v_1)), seed
    gr.close(), plain.close()


# the largest element difference between DinoV2Salad.features(want_local=True) and the same MLP in f32 torch on the same bf16
# tokens and weights, measured on an MI355X at ViT-S, 224 px, and the gate at twice that: the margin covers
# the bf16 rounding of the hidden layer and of the output, which the f32 reference does not have
LOCAL_FEATURES_MEASURED = 0.001306
LOCAL_FEATURES_GATE = 2 * LOCAL_FEATURES_MEASURED


def test_features_want_local_at_vit_small(dev):
    from vpr_amd.modules import DinoV2Salad
    torch.manual_seed(0)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    ext.aggregator.pack()
    x = torch.randn(3, 3, 224, 224, device=dev).to(torch.bfloat16)
    d, d16 = ext.features(x, want_bf16=True)
    d, d16 = d.clone(), d16.clone()
    e, e16, local = ext.features(x, want_bf16=True, want_local=True)
    assert torch.equal(bits(d), bits(e)) and torch.equal(d16.view(torch.int16), e16.view(torch.int16))
    e1, local1 = ext.features(x, want_local=True)
    assert torch.equal(bits(e1), bits(d)) and torch.equal(local1.view(torch.int16), local.view(torch.int16))
    assert local.shape == (3, 256, 128) and local.dtype == torch.bfloat16
    tokens = ext.backbone(x, split=True).patch
    assert tokens.dtype == torch.bfloat16 and tokens.shape == (3, 256, 384)
    assert torch.equal(ext.aggregator.local_features(tokens).view(torch.int16), local.view(torch.int16))
    c = ext.aggregator.cluster_features
    w = lambda conv: conv.weight.detach().reshape(conv.weight.shape[0], -1).to(torch.bfloat16).float()
    with torch.no_grad():
        h = torch.relu(tokens.float().reshape(-1, 384) @ w(c[0]).T + c[0].bias.float())
        f = h @ w(c[3]).T + c[3].bias.float()
        want = (f / f.norm(dim=1, keepdim=True)).view(3, 256, 128)
    diff = float((local.float() - want).abs().max())
    print(f"features(want_local=True) vs the f32 MLP, largest element difference: {diff:.6f}")
    assert torch.allclose(local.float().norm(dim=2), torch.ones(3, 256, device=dev), atol=4e-3)
    assert diff <= LOCAL_FEATURES_GATE
    small = DinoV2Salad("vit_small", img_size=322)
    with pytest.raises(ValueError, match="at most 256"):
        small.features(torch.zeros(1, 3, 322, 322), want_local=True)     # refused before anything runs: a CPU tensor is fine


def test_retrieval_scores_with_local_rerank(dev, tmp_path, monkeypatch):
    """Generated images, a gallery kept with its local features: local_rerank=None gives the plain numbers; with it the result
    is retrieval_metrics, by hand, of search_local_reranked on the same descriptor and local-feature batches."""
    import os
    import pandas as pd
    from PIL import Image
    from vpr_amd import evaluate, gallery as G, modules
    from vpr_amd.retrieval import ShardedGallery
    rng = np.random.default_rng(21)
    gdir, vdir = tmp_path / "images_train", tmp_path / "images_val"
    gdir.mkdir(), vdir.mkdir()
    n_g = 20
    gnames = [f"img_{i:04d}.png" for i in range(n_g)]
    imgs = [rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(n_g)]
    for n, im in zip(gnames, imgs):
        Image.fromarray(im).save(gdir / n)
    lat, lon, ang = 219000 + 100.0 * np.arange(n_g), 143000 + 50.0 * np.arange(n_g), (17.0 * np.arange(n_g)) % 360
    pd.DataFrame({"filename": gnames, "timestamp": "t", "latitude": lat, "longitude": lon, "angle": ang,
                  "Region_ID": np.arange(n_g) // 5}).to_csv(tmp_path / "labels_train.csv", index=False)
    src = [3, 11, 0, 19, 7, 12]
    vnames = [f"img_{i:04d}.png" for i in range(len(src))]
    for n, s in zip(vnames, src):
        noisy = np.clip(imgs[s].astype(np.int16) + rng.integers(-3, 4, imgs[s].shape), 0, 255).astype(np.uint8)
        Image.fromarray(noisy).save(vdir / n)
    pd.DataFrame({"filename": vnames, "timestamp": "t", "latitude": lat[src] + 3.0, "longitude": lon[src] - 4.0,
                  "angle": (ang[src] + 5.0) % 360, "Region_ID": np.array(src) // 5}).to_csv(tmp_path / "labels_val.csv", index=False)
    torch.manual_seed(1)
    ext = modules.DinoV2Salad("vit_small")
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    train = (ext, str(tmp_path / "labels_train.csv"), str(gdir))
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "gal"), batch_size=8, keep_local=True, graph=False) == n_g
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "bare"), batch_size=8, graph=False) == n_g
    assert os.path.exists(tmp_path / "gal" / G.LOCAL_FILE) and not os.path.exists(tmp_path / "bare" / G.LOCAL_FILE)
    assert np.array_equal(np.load(tmp_path / "gal" / "descriptors.npy"), np.load(tmp_path / "bare" / "descriptors.npy"))
    assert evaluate.build_gallery_from_images(*train, str(tmp_path / "graphed"), batch_size=8, keep_local=True) == n_g   # graph replay
    for f in ("descriptors.npy", G.LOCAL_FILE):
        assert np.array_equal(np.load(tmp_path / "gal" / f), np.load(tmp_path / "graphed" / f)), f
    seen = []
    plain_search = ShardedGallery.search_local_queries

    def spy(self, q_local, k, expand=None, **kw):
        seen.append((q_local.clone(), k, expand, {n: (v.clone() if isinstance(v, torch.Tensor) else v) for n, v in kw.items()}))
        return plain_search(self, q_local, k, expand, **kw)

    monkeypatch.setattr(ShardedGallery, "search_local_queries", spy)
    run = lambda gal="gal", **kw: evaluate.calculate_retrieval_scores(ext, str(tmp_path / gal), str(tmp_path / "labels_val.csv"),
                                                                      str(vdir), k=5, tau=10.0, batch_size=4, verbose=False, graph=False, **kw)
    res = run()
    assert all(kw == {} for *_, kw in seen) and res["topk_indices"][:, 0].tolist() == src
    assert run("bare")["topk_scores"].tobytes() == res["topk_scores"].tobytes()  # the file changes nothing until it is asked for
    with pytest.raises(ValueError, match="keep_local"):
        run("bare", local_rerank=8)
    with pytest.raises(ValueError, match="neither with rerank nor with query_expansion"):
        run(local_rerank=8, rerank=8)
    del seen[:]
    got = run(local_rerank=8, min_sim=0.5)
    assert all(set(kw) == {"local_rerank", "q_local_feats", "min_sim"} and kw["local_rerank"] == 8 and kw["min_sim"] == 0.5 for *_, kw in seen)
    replayed = evaluate.calculate_retrieval_scores(ext, str(tmp_path / "gal"), str(tmp_path / "labels_val.csv"), str(vdir), k=5, tau=10.0,
                                                   batch_size=4, verbose=False, local_rerank=8, min_sim=0.5)        # graph=True
    assert replayed["topk_scores"].tobytes() == got["topk_scores"].tobytes() and replayed["topk_indices"].tobytes() == got["topk_indices"].tobytes()
    del seen[len(seen) // 2:]                                # the replayed run's batches: the same again
    shard = G.load_gallery_shard(str(tmp_path / "gal"), dev, load_local=True)
    assert shard.local.shape == (n_g, 256, 128) and shard.local.dtype == torch.bfloat16
    sg = ShardedGallery(shard.rows, shard.n_total, exact_fallback=True, local_feats=shard.local)
    batches = [sg.search_local_reranked(d16, k, 8, kw["q_local_feats"], 0.5) for d16, k, _, kw in seen]
    vals, idx = torch.cat([v for v, _ in batches]), torch.cat([i for _, i in batches])
    df = pd.read_csv(tmp_path / "labels_val.csv")
    top = idx.cpu().numpy()
    assert top[:, 0].tolist() == src and got["topk_indices"].tobytes() == top.tobytes()
    assert got["topk_scores"].tobytes() == vals.cpu().numpy().tobytes() and got["topk_scores"].tobytes() != res["topk_scores"].tobytes()
    assert (got["topk_scores"][:, 0] > 128).all()            # local scores: most of the 256 patches match at similarity ~1
    # the metrics by hand: top-1 label transfer, recalls from the lists
    labels = shard.labels
    pose = labels[top[:, 0]][:, :3]
    assert np.allclose(got["pose"], pose)
    tq = df[["latitude", "longitude"]].to_numpy(dtype=np.float64)
    near = lambda rows, b: np.hypot(*(labels[rows][:, :2] - tq[b]).T) <= 10.0
    assert got["recall_at_1_tau"] == np.mean([near(top[b, :1], b).any() for b in range(len(src))]) == 1.0
    assert got["recall_at_5_tau"] == np.mean([near(top[b], b).any() for b in range(len(src))])
    assert got["recall_at_1_region"] == np.mean([labels[top[b, 0], 3] == df["Region_ID"][b] for b in range(len(src))]) == 1.0
    err = np.abs((pose[:, 2] - df["angle"].to_numpy() + 180) % 360 - 180)
    assert abs(got["maae"] - err.mean()) < 1e-9 and abs(err.mean() - 5.0) < 1e-9
