"""GPU: every instantiation of the two match kernels (csrc/local_match.hip::local_match_dispatch: 12 (element, width) pairs x the
256-patch and the hires kernel x without and with the match list = 48 compiled kernels) against the f64 restatements, bit for
bit, on the inputs of tests/local_match_cases.py: per cell the shapes that cross every seam of its kernel, and per shape random
integers at two thresholds, all-negative similarities, non-finite patches beside every seam, on the routes with the list a
shifted / scrambled gallery at three tolerances, and a one-hot diagonal in both roles.  tests/test_local_match_matrix_cpu.py
shows that these inputs tell a kernel with a swizzle, K-step, tie, mask, seam, threshold or list mistake from a right one in
every cell.  A second test per (element, width) sets the routes against each other at 256 patches and below."""
import numpy as np
import pytest
import torch

import local_match_cases as lmc
import spatial_ref as sref

pytestmark = pytest.mark.gpu

CELL_IDS = [f"{route}-{kind}-{l}" for route, kind, l in lmc.CELLS]
MAIN = 3            # the first three fields of either route are the call's main outputs; the rest come with debug=True


@pytest.fixture(autouse=True, scope="module")
def one_torch_thread():
    """The restatements work on many small arrays; torch's thread pool and the BLAS one only get in each other's way there."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def run(dev, route, kind, q, idx, g, base, k, min_sim, gw_q=None, gw_g=None, tol=None, debug=True):
    """One call of the route's public entry -> dict of numpy arrays under the names of lmc.fields_of(route)."""
    from vpr_amd import ops
    entry = getattr(ops, lmc.ROUTES[route][2][kind])
    if lmc.has_list(route):
        out = entry(q.to(dev), idx.to(dev), g.to(dev), gw_q, gw_g, tol, base, k, min_sim, debug=debug)
    else:
        out = entry(q.to(dev), idx.to(dev), g.to(dev), base, k, min_sim, debug=debug)
    torch.cuda.synchronize()
    res = dict(zip(lmc.fields_of(route)[:MAIN], (t.cpu().numpy() for t in out[:MAIN])))
    if debug:
        res.update({f: getattr(out[3], f).cpu().numpy() for f in out[3]._fields})
    return res


def run_case(dev, route, kind, case, debug=True):
    return run(dev, route, kind, case.q, case.idx, case.g, case.base, case.k, case.min_sim, case.gw_q, case.gw_g, case.tol, debug)


def assert_equal_bits(got, want, fields, what=""):
    for f in fields:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.shape == b.shape and a.dtype == b.dtype and a.dtype.itemsize == 4, (what, f, a.shape, b.shape, a.dtype, b.dtype)
        a, b = a.view(np.int32), b.view(np.int32)
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:5].tolist(), a[a != b][:5], b[a != b][:5])


@pytest.mark.parametrize("route,kind,l", lmc.CELLS, ids=CELL_IDS)
def test_cell_bit_for_bit(dev, route, kind, l):
    """Every input of the cell, every output field of its route, with the optional outputs; input (a) once more without them:
    the optional pointers change what the kernel stores, the three main outputs must not change."""
    fields = lmc.fields_of(route)
    for case in lmc.cases(route, kind, l):
        assert case.q.shape[2] == case.g.shape[2] == l
        if lmc.has_list(route):
            assert lmc.kernel_for_counts(case.q.shape[1], case.g.shape[1]) == lmc.kernel_of(route)
        want = lmc.expected(case)
        assert_equal_bits(run_case(dev, route, kind, case), want, fields, case.name)
        if case.meta["input"] == "a":
            assert_equal_bits(run_case(dev, route, kind, case, debug=False), want, fields[:MAIN], case.name + " without the optional outputs")


@pytest.mark.parametrize("kind,l", [(kind, l) for kind in lmc.KINDS for l in lmc.WIDTHS[kind]])
def test_the_routes_agree_at_256_patches_and_below(dev, kind, l):
    """Input (a) at 256 patches and below.  The two entries without the list give the same bits in every field.  The call with
    the list shares row_nn, col_nn and pair_matches with them; where every match is an inlier (a bin plane of at most 9 x 9 at
    the largest tolerance) also the scores and the order.  With one more grid row of NaN patches on the candidate side the call
    with the list runs the hires kernel on the same similarities: the same bits again."""
    u = lmc.unit_sim(kind)
    nan_patch = float("nan") if kind == "bf16" else 0x7F
    for n_q, gw_q, n_g, gw_g, q, idx, g, all_inliers in lmc.agreement_inputs(kind, l):
        what = f"{n_q}x{n_g}"
        for min_sim, k in ((0.0, None), (3 * u, 2)):
            plain = run(dev, "rerank", kind, q, idx, g, lmc.BASE, k, min_sim)
            hires = run(dev, "hires", kind, q, idx, g, lmc.BASE, k, min_sim)
            assert_equal_bits(hires, plain, lmc.PLAIN_FIELDS, what)
            tol = sref.MAX_TOL if all_inliers else 1
            listed = run(dev, "spatial", kind, q, idx, g, lmc.BASE, k, min_sim, gw_q, gw_g, tol)
            assert_equal_bits(listed, plain, ("row_nn", "col_nn", "pair_matches"), what)
            if all_inliers:
                assert_equal_bits(listed, plain, ("vals", "idx", "pair_score"), what)
                assert_equal_bits(dict(matches=listed["inliers"], pair_matches=listed["pair_inliers"]), plain, ("matches", "pair_matches"), what)
            tall_g = torch.cat([g, torch.full((g.shape[0], gw_g * (-(-(lmc.MAX_N_256 + 1 - n_g) // gw_g)), l), nan_patch, dtype=g.dtype)], 1).contiguous()
            assert lmc.kernel_for_counts(n_q, tall_g.shape[1]) == "hires" and tall_g.shape[1] % gw_g == 0
            assert (gw_q + gw_g - 1) * (n_q // gw_q + tall_g.shape[1] // gw_g - 1) <= sref.MAX_BINS
            tall = run(dev, "spatial_hires", kind, q, idx, tall_g, lmc.BASE, k, min_sim, gw_q, gw_g, tol)
            assert_equal_bits(tall, listed, [f for f in lmc.SPATIAL_FIELDS if f != "col_nn"], what + " against the hires kernel")
            assert np.array_equal(tall["col_nn"][:, :, :n_g], listed["col_nn"]) and (tall["col_nn"][:, :, n_g:] == -1).all(), what
        assert (plain["pair_matches"] > 0).any(), what
