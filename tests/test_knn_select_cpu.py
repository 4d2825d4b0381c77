"""CPU self-checks of oracle/knn_select.py, the plain model of the kNN select stage given a score matrix: it must
agree with oracle/knn.py where the two overlap, reproduce the certificate outcomes the GPU suite already pins on
_near_tie_problem, and plan the select levels as the library sizes its workspace."""
import numpy as np
import pytest
import torch

from oracle import knn as oknn
from oracle import knn_select as oks


def _rows(n, d, seed, spread=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    if spread:
        x = x * torch.logspace(-2, 2, n)[torch.randperm(n, generator=g)][:, None] / d ** 0.5
    return x.to(torch.bfloat16)


def _exact_S(q, g):
    return oknn.knn_scores_f64(q, g).to(torch.float32)


@pytest.mark.parametrize("B,N,D,k,row_bytes", [
    (3, 7, 64, 1, None), (3, 7, 64, 8, None), (2, 5000, 64, 10, None), (2, 20000, 128, 17, None),
    (2, 20000, 64, 64, None),                 # 3 level-0 lists of 128
    (1, 37 * 8192 + 11, 64, 64, None),        # > 4096 level-0 candidates: a later level, then the fused path
    (2, 600, 64, 5, 32768), (2, 12, 64, 5, 32768),      # the general path (rows wider than 24 KB)
])
def test_exact_scores_and_a_tiny_bound_give_the_brute_force_answer(B, N, D, k, row_bytes):
    q, g = _rows(B, D, N + k, spread=False), _rows(N, D, N + k + 1)
    v_ref, i_ref = oknn.knn_topk(q, g, k, 5)
    v, i, st, info = oks.knn_select_model(_exact_S(q, g), q, g, k, 1e-12, 5, row_bytes=row_bytes)
    assert st.tolist() == [0] * B
    assert torch.equal(i, i_ref) and torch.equal(v, v_ref)
    assert all(r["path"] == ("general" if row_bytes else "fused") for r in info)


def test_tied_rows_come_out_by_the_lower_index():
    g = torch.nn.functional.normalize(_rows(500, 64, 5, spread=False).float(), dim=1).to(torch.bfloat16)
    g[100] = g[7]
    g[300] = g[7]
    q = g[[7, 20]].clone()
    v_ref, i_ref = oknn.knn_topk(q, g, 4, 1000)
    v, i, st, _ = oks.knn_select_model(_exact_S(q, g), q, g, 4, 1e-12, 1000)
    assert i[0, :3].tolist() == [1007, 1100, 1300] and st.tolist() == [0, 0]
    assert torch.equal(i, i_ref) and torch.equal(v, v_ref)


def test_a_zero_query_ties_everything_and_saturates_every_chunk_list():
    """All scores equal: e_k == a_min, so nothing is certified; every level-0 list is cut inside the tie -> status 2.
    The answer is still the k lowest indices (the widening set holds every entry in hand)."""
    N, k = 20000, 10
    g = _rows(N, 64, 9)
    q = torch.zeros(1, 64, dtype=torch.bfloat16)
    v, i, st, info = oks.knn_select_model(_exact_S(q, g), q, g, k, 1.0)
    assert st.tolist() == [2] and i[0].tolist() == list(range(k)) and not info[0]["overflow"]
    assert len(info[0]["widening"]) == 3 * 24 - 24


def test_mixed_zeros_select_like_positive_zeros():
    g = _rows(1000, 64, 11)
    q = _rows(2, 64, 12, spread=False)
    S = torch.zeros(2, 1000)
    S[:, ::3] = -0.0
    S[:, 5::7] = -1.0
    a = oks.knn_select_model(S, q, g, 8, 1e-12)
    b = oks.knn_select_model(S + 0.0, q, g, 8, 1e-12)
    assert oks.compare(a[:3], b[:3]) is None and a[3][0]["candidates"] == b[3][0]["candidates"]
    assert a[3][0]["candidates"] == set(np.flatnonzero(S[0].numpy() == 0)[:16].tolist())


def _near_tie_problem(n_chunks, per_chunk):
    from test_knn_gpu import _near_tie_problem as make          # the suite's published construction
    return make(n_chunks, per_chunk)


@pytest.mark.parametrize("n_chunks,per_chunk,want", [(8, 8, [1, 0]), (3, 64, [2, 0])])
def test_model_reproduces_the_published_near_tie_outcomes(n_chunks, per_chunk, want):
    """The statuses tests/test_knn_gpu.py asserts on the device, from an f32 matmul on the CPU as the score matrix: 8
    band rows per chunk -> widened and certified; all 64 in one chunk -> its list is cut inside the band, flagged."""
    q, gal, rows = _near_tie_problem(n_chunks, per_chunk)
    k = 10
    S = q.float() @ gal.float().T
    bound = float(gal.float().norm(dim=1).max()) * 1.001
    v, i, st, info = oks.knn_select_model(S, q, gal, k, bound)
    assert st.tolist() == want
    assert info[0]["margin"] > 0 and not info[0]["overflow"]
    v_ref, i_ref = oknn.knn_topk(q, gal, k)
    assert torch.equal(i[1], i_ref[1]) and torch.equal(v[1], v_ref[1])
    if want[0] == 1:                                            # certified after widening: the exact answer
        assert torch.equal(i, i_ref) and torch.equal(v, v_ref)
        assert set(rows) <= info[0]["candidates"] | info[0]["widening"]


def test_level_plan_of_the_shapes_the_gpu_tests_rely_on():
    p = oks.level_plan(8192, 16, 128)
    assert (p["kp"], p["ch0"], p["run"], p["fused"], p["level0_lists"]) == (32, 8192, [8192], True, True)
    assert oks.level_plan(1025, 1, 128)["ch0"] == 2048 and oks.level_plan(1, 1, 128)["ch0"] == 1024
    assert [oks.knn_kp(k) for k in (1, 8, 16, 17, 32, 64)] == [16, 16, 32, 40, 64, 128]
    p = oks.level_plan(37 * 8192 + 11, 64, 128)                 # 38 lists of 128 > 4096
    assert (p["nchunk"], p["run"], p["fused"], p["level0_lists"]) == ([38, 2, 1], [8192, 4096], True, False)
    p = oks.level_plan(600, 5, 32768)                           # row > 24 KB
    assert (p["run"], p["fused"]) == ([1024], False)
    p = oks.level_plan(300000, 64, 32768)
    assert (p["run"], p["fused"]) == ([8192, 4096, 4096], False)


def test_level_plan_sizes_the_workspace_as_the_library_does():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    lib = _lib.lib()
    Ns = [1, 7, 63, 64, 65, 1023, 1024, 1025, 3328, 4097, 8191, 8192, 8193, 16385, 24581, 106497, 300000, 303115,
          1_000_000, 2_000_000, 40_000_000]
    for B, D in ((1, 64), (3, 64), (64, 8448), (300, 512)):
        for N in Ns:
            for k in (1, 8, 16, 17, 32, 64):
                assert lib.vpr_knn_workspace_bytes(B, N, D, k) == oks.workspace_bytes(B, N, D, k), (B, N, D, k)
    assert oks.workspace_bytes(1, 1000, 64, 65) == 0 and oks.workspace_bytes(1, 1000, 96, 5) == 0


def test_checker_rejects_what_it_should():
    q, g = _rows(2, 64, 3, spread=False), _rows(300, 64, 4)
    want = oks.knn_select_model(_exact_S(q, g), q, g, 5, 1e-12)
    v, i, st, info = want
    assert oks.compare((v, i, st), want[:3], info) is None
    i2 = i.clone(); i2[1, [0, 1]] = i[1, [1, 0]]
    v2 = v.clone(); v2[0, 3] = torch.nextafter(v[0, 3], torch.tensor(float("inf")))
    st2 = st.clone(); st2[1] = 1
    assert "indices" in oks.compare((v, i2, st), want[:3], info)
    assert "values" in oks.compare((v2, i, st), want[:3], info)
    assert "status" in oks.compare((v, i, st2), want[:3], info)
