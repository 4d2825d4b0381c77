"""CPU: the matrix of tests/local_match_cases.py without a device.  The matrix is the dispatch's (the LM_CASE widths, the patch
limit, the chunk width and the group size are read from csrc/local_match.hip); every input meets the premises it was built for,
from the restatements alone; and the inputs can tell a wrong kernel from a right one: each mistake this kernel family can
plausibly make is applied to a copy of the numpy restatement (to the features, the similarity matrix, the argmax rule, the
threshold or the match list, never to device code) and must change a compared output in every cell it applies to."""
import os
import re

import numpy as np
import pytest
import torch

import local_match_cases as lmc
import local_match_fp8_ref as ref8
import local_match_ref as ref
import spatial_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL_IDS = [f"{route}-{kind}-{l}" for route, kind, l in lmc.CELLS]


@pytest.fixture(autouse=True, scope="module")
def one_torch_thread():
    """The restatements work on many small arrays; torch's thread pool and the BLAS one only get in each other's way there."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------ the matrix is the dispatch's
def source(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_matrix_is_the_dispatch_of_local_match_hip():
    import vpr_amd
    hip = source(vpr_amd.__path__[0], "csrc", "local_match.hip")
    body = hip[hip.index("int local_match_dispatch("):hip.index("#undef LM_CASE")]
    fp8, bf16 = body[body.index("if constexpr (FP8)"):].split("} else {")
    widths = lambda text: tuple(int(w) for w in re.findall(r"LM_CASE\((\d+)\)", text))
    assert widths(fp8) == lmc.WIDTHS["e4m3"] and widths(bf16) == lmc.WIDTHS["bf16"]
    # one LM_CASE = both kernels; the template's LIST flag doubles them: 4 instantiations per (element, width)
    assert "hires ? launch_local_match<Elem, LL, LIST, true>(LM_ARGS) : launch_local_match<Elem, LL, LIST, false>(LM_ARGS)" in body
    assert len(lmc.CELLS) == 4 * sum(len(w) for w in lmc.WIDTHS.values()) == 48 and len(set(lmc.CELLS)) == 48
    assert {(lmc.kernel_of(r), lmc.has_list(r)) for r in lmc.ROUTES} == {(k, flag) for k in ("256", "hires") for flag in (False, True)}
    # the patch limit of the 256-patch kernel and the switch of the call with the list
    assert re.search(r"constexpr int LM_MAX_N = VPR_LOCAL_MAX_N;", hip)
    assert int(re.search(r"#define VPR_LOCAL_MAX_N (\d+)", source("include", "vpr_amd_local.h")).group(1)) == lmc.MAX_N_256
    assert "const bool hires = n_q > LM_MAX_N || n_g > LM_MAX_N;" in hip
    assert [lmc.kernel_for_counts(*n) for n in ((256, 256), (257, 1), (1, 257), (256, 255))] == ["256", "hires", "hires", "256"]
    # the entries without the list: the kernel by the entry, not by the count
    assert "local_match_dispatch<Elem, false>(max_n > LM_MAX_N," in hip
    for entry, max_n in (("vpr_local_rerank", "LM_MAX_N"), ("vpr_patch_rerank_fp8", "LM_MAX_N"), ("vpr_hires_local_rerank", "LH_MAX_N"),
                         ("vpr_hires_patch_rerank_fp8", "LH_MAX_N")):
        assert re.search(rf'extern "C" int {entry}\([^{{]*\{{\s*return local_rerank_run<uint\d+_t>\({max_n},', hip), entry
    # what the shapes are sized by
    assert int(re.search(r"constexpr int LM_GROUP = (\d+);", hip).group(1)) == lmc.GROUP and lmc.KC % lmc.GROUP != 0
    assert int(re.search(r"constexpr int LH_BLOCK = (\d+);", hip).group(1)) == lmc.ROW_BLOCK
    assert "constexpr int lh_chunk_cols(int row_bytes) { return row_bytes <= 256 ? 256 : 128; }" in hip
    assert "constexpr int SH = CPR % 16 == 0 ? 0 : CPR % 8 == 0 ? 1 : 2, MASK = CPR % 16 == 0 ? 15 : CPR % 8 == 0 ? 7 : 3;" in hip
    assert "constexpr int NST = CW * CPR / LM_THREADS;" in hip and "constexpr int LM_WAVES = 8;" in hip
    facts = {(k, l): (lmc.chunks_per_row(k, l), lmc.swizzle_class(k, l), lmc.chunk_cols(k, l), lmc.staging_trips(k, l))
             for k in lmc.KINDS for l in lmc.WIDTHS[k]}
    assert facts["bf16", 96] == (12, (2, 3), 256, 6) and facts["bf16", 160] == (20, (2, 3), 128, 5)
    assert facts["bf16", 192] == (24, (1, 7), 128, 6) and facts["bf16", 224] == (28, (2, 3), 128, 7)
    assert facts["e4m3", 192] == (12, (2, 3), 256, 6) and facts["bf16", 256] == (32, (0, 15), 128, 8) and facts["e4m3", 64] == (4, (2, 3), 256, 2)
    assert {f[3] for f in facts.values()} == {2, 4, 5, 6, 7, 8}                # the staging trip counts that exist
    assert int(re.search(r"#define VPR_SPATIAL_MAX_TOL (\d+)", source("include", "vpr_amd_spatial.h")).group(1)) == sref.MAX_TOL


def test_the_shapes_cross_every_seam_of_their_kernel():
    for route, kind, l in lmc.CELLS:
        shapes = lmc.SHAPES[route]
        assert sum(n_q != n_g for n_q, _, n_g, _ in shapes) >= 2 and max(max(s[0], s[2]) for s in shapes) <= 400
        for n_q, gw_q, n_g, gw_g in shapes:
            if lmc.has_list(route):                                            # sv_check_grid
                sref.dims(n_q, gw_q, n_g, gw_g)
                assert (gw_q + gw_g - 1) * (n_q // gw_q + n_g // gw_g - 1) <= sref.MAX_BINS
                assert lmc.kernel_for_counts(n_q, n_g) == lmc.kernel_of(route)
        if lmc.kernel_of(route) == "256":
            assert all(max(s[0], s[2]) <= lmc.MAX_N_256 for s in shapes)
            assert any(s[0] % 32 and s[2] % 32 for s in shapes)                                      # a partial tile on both sides
            assert any({s[0], s[2]} == {lmc.MAX_N_256, lmc.MAX_N_256 - 1} for s in shapes)              # the limit beside one short of it
            assert any(s[0] == lmc.MAX_N_256 and s[2] <= 2 * 32 for s in shapes)                       # eight waves on few columns
        else:
            cw = lmc.chunk_cols(kind, l)
            n_gs = [s[2] for s in shapes]
            assert any(cw < n <= cw + 32 for n in n_gs) and any(n > 2 * cw for n in n_gs) or cw == 256   # over one and over two chunks
            assert any(cw < n for n in n_gs) and any(n > lmc.ROW_BLOCK for n in n_gs)               # a second chunk; a second block of the sum
            assert any(lmc.ROW_BLOCK < s[0] <= lmc.ROW_BLOCK + 32 for s in shapes)                  # just over one row block
            assert lmc.has_list(route) or any(max(s[0], s[2]) <= lmc.MAX_N_256 for s in shapes)    # these entries below 256, too
    idx = lmc.cases("rerank", "bf16", 32)[0].idx.numpy()
    assert idx[0, 4] == -1 and lmc.BASE <= idx[0, 5] < lmc.BASE + lmc.N_LOCAL                 # a group that opens dead and ends live


# ---------------------------------------------------------------------------------------------- premises of the inputs
def pair_of(case, b, r):
    return ref.pair(lmc.values(case.q)[b], lmc.values(case.g)[r], case.min_sim)


@pytest.mark.parametrize("route,kind,l", lmc.CELLS, ids=CELL_IDS)
def test_every_input_meets_its_premises(route, kind, l):
    u = lmc.unit_sim(kind)
    seen = set()
    for case in lmc.cases(route, kind, l):
        want, kind_of = lmc.expected(case), case.meta["input"]
        seen.add(kind_of)
        assert set(lmc.fields_of(route)) <= set(want), case.name
        pairs = [pair_of(case, b, r) for b, r in lmc.live_pairs(case)]
        for p in pairs:                                                        # every comparison is bit for bit: S exact in f32
            S = np.where(p["finite"], p["S"], 0.0)
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S), case.name
        if kind_of == "a":
            assert (want["pair_matches"] > 0).any(), case.name
            tied = lambda S, axis: ((S == S.max(axis, keepdims=True)).sum(axis) >= 2).any()
            assert any(tied(p["S"], 1) for p in pairs) and any(tied(p["S"], 0) for p in pairs), case.name
            if case.meta["units"] == 3:                                        # one matched pair sits exactly at min_sim
                p, (i0, j0) = pair_of(case, 0, 0), case.meta["planted"]
                assert p["S"][i0, j0] == float(np.float32(case.min_sim)) == 3 * u and p["matched"][j0] and p["col_nn"][j0] == i0, case.name
                assert case.idx[0, 0] == case.base and want["pair_matches"][0, 0] >= 1
        elif kind_of == "b":
            assert all((p["S"][p["finite"]] < 0).all() and p["finite"].all() and p["matches"] > 0 for p in pairs), case.name
            assert (want["pair_matches"] > 0).any() and all((p["S"] >= float(np.float32(case.min_sim))).all() for p in pairs)
        elif kind_of == "c":
            p = pair_of(case, 0, 0)
            rows, cols = case.meta["rows"], case.meta["cols"]
            assert len(rows) >= 4 and len(cols) >= 4 and case.idx[0, 0] == case.base
            assert (p["row_nn"][rows] == -1).all() and (p["col_nn"][cols] == -1).all(), case.name
            assert not np.isin(p["row_nn"], cols).any() and not np.isin(p["col_nn"], rows).any() and p["matches"] > 0, case.name
            assert (want["row_nn"][0, 0] == -1).any() and (want["col_nn"][0, 0] == -1).any()
        elif kind_of == "d":
            assert case.idx[0].tolist()[:2] == [case.base, case.base + 1] and case.idx[1, 0] == case.base + 3
            m, inl = want["pair_matches"], want["pair_inliers"]
            assert m[0, 0] > 0 and m[0, 1] > m[0, 0] and m[1, 0] > 0, case.name                       # the scrambled image: more matches
            if case.tol == 0:
                assert want["pair_shift"][0, 0].tolist() == list(case.meta["shifts"][0]) != [0, 0] and inl[0, 0] == m[0, 0], case.name
                assert want["pair_shift"][1, 0].tolist() == list(case.meta["shifts"][1]) and inl[1, 0] == m[1, 0], case.name
                assert inl[0, 1] < m[0, 1], case.name
                plain = (ref8.local_rerank_fp8 if kind == "e4m3" else ref.local_rerank)(case.q, case.idx, case.g, case.base, None, case.min_sim)
                place = lambda out, image: out["idx"][0].tolist().index(case.base + image)
                assert place(plain, 1) < place(plain, 0) and place(want, 0) < place(want, 1), case.name
            if case.tol == sref.MAX_TOL:
                assert inl[0, 1] == m[0, 1], case.name
        else:
            p = pair_of(case, 0, 1)
            n = min(p["S"].shape)
            assert n >= l and (np.diag(p["S"])[:l] != 0).all() and np.count_nonzero(p["S"]) == l, case.name
    assert seen == ({"a", "b", "c", "d", "e"} if lmc.has_list(route) else {"a", "b", "c", "e"})


# ------------------------------------------------------------------- the inputs tell a wrong kernel from a right one
def applies(mistake, route, kind, l):
    if mistake == "chunk^4":                                                   # the swizzle classes whose mask reaches bit 2
        return lmc.swizzle_class(kind, l)[1] & 4 != 0
    if mistake in ("skip_column_cw", "skip_row_256"):                          # seams of the hires kernel
        return lmc.kernel_of(route) == "hires"
    if mistake == "list_of_unmatched":
        return lmc.has_list(route)
    return True


MISTAKES = ("chunk^1", "chunk^4", "k_one_short", "row_ties_to_highest", "column_ties_to_highest", "padded_rows_unmasked",
            "padded_columns_unmasked", "skip_column_cw", "skip_row_256", "non_finite_wins", "min_sim_strict", "list_of_unmatched")


def nearest(S, finite, row_high, col_high):
    """local_match_ref.nearest, with the tie rule of either argmax as a switch."""
    masked = np.where(finite, S, -np.inf)
    first = lambda m, axis: m.argmax(axis)
    last = lambda m, axis: m.shape[axis] - 1 - np.flip(m, axis).argmax(axis)
    row_nn = np.where(finite.any(1), (last if row_high else first)(masked, 1), -1).astype(np.int32)
    col_nn = np.where(finite.any(0), (last if col_high else first)(masked, 0), -1).astype(np.int32)
    return row_nn, col_nn


def pair_outputs(case, b, r, kind, l, cw, mistake=None):
    """One (query, image) pair through a copy of the restatement with one mistake -> the outputs a test compares for it."""
    q, g = lmc.values(case.q)[b].copy(), lmc.values(case.g)[r].copy()
    n_q, n_g = q.shape[0], g.shape[0]
    if mistake in ("chunk^1", "chunk^4"):                                      # one class of candidate rows reads the last chunk from
        epc, c = lmc.elems_per_chunk(kind), lmc.chunks_per_row(kind, l) - 1    # the slot of its partner: feature positions permuted
        o = c ^ int(mistake[-1])                                               # on one operand only
        rows = np.arange(n_g) % 16 == 5
        g[rows, c * epc:(c + 1) * epc], g[rows, o * epc:(o + 1) * epc] = g[rows, o * epc:(o + 1) * epc].copy(), g[rows, c * epc:(c + 1) * epc].copy()
    if mistake == "k_one_short":
        g[:, l - lmc.k_step(kind):] = 0
    pad = lambda v: np.concatenate([v, np.zeros((-v.shape[0] % 32, l))])
    if mistake == "padded_rows_unmasked":
        q = pad(q)
    if mistake == "padded_columns_unmasked":
        g = pad(g)
    S, finite = ref.similarity(q, g)
    if mistake == "skip_column_cw" and n_g > cw:
        finite[:, cw] = False
    if mistake == "skip_row_256" and n_q > lmc.ROW_BLOCK:
        finite[lmc.ROW_BLOCK] = False
    if mistake == "non_finite_wins":
        S, finite = np.where(finite, S, np.inf), np.ones_like(finite)
    row_nn, col_nn = nearest(S, finite, mistake == "row_ties_to_highest", mistake == "column_ties_to_highest")
    j, c = np.arange(S.shape[1]), np.maximum(col_nn, 0)
    ms = float(np.float32(case.min_sim))
    with np.errstate(invalid="ignore"):
        matched = (col_nn >= 0) & (row_nn[c] == j) & ((S[c, j] > ms) if mistake == "min_sim_strict" else (S[c, j] >= ms))
        sim = np.where(matched, S[c, j], 0.0).astype(np.float32)
        partner = np.where(matched, col_nn, -1)
        if mistake == "list_of_unmatched":                                     # the list keeps c(j) and S of a column that is no match
            partner, sim = col_nn, np.where(col_nn >= 0, S[c, j], 0.0).astype(np.float32)
        out = dict(row_nn=row_nn[:n_q], col_nn=col_nn[:n_g])
        if case.tol is None:
            out.update(pair_matches=int(matched[:n_g].sum()), pair_score=np.float32(sim[:n_g].astype(np.float64).sum()))
        else:
            v = sref.verify(partner[:n_g], sim[:n_g], n_q, case.gw_q, case.gw_g, case.tol)
            out.update(pair_score=v["score"], pair_inliers=v["inliers"], pair_matches=v["matches"], pair_shift=np.array(v["shift"]))
    return out


def differs(a, b):
    return any(not np.array_equal(np.asarray(a[f]), np.asarray(b[f]), equal_nan=True) for f in a)


@pytest.fixture(scope="module")
def caught():
    """{(mistake, cell): the first input of the cell (smallest first) on which the mistake changes a compared output}."""
    table = {}
    for route, kind, l in lmc.CELLS:
        cw = lmc.chunk_cols(kind, l) if lmc.kernel_of(route) == "hires" else lmc.MAX_N_256
        todo = [m for m in MISTAKES if applies(m, route, kind, l)]
        right = {}
        for case in sorted(lmc.cases(route, kind, l), key=lambda c: c.q.shape[1] * c.g.shape[1]):
            for b, r in lmc.live_pairs(case):
                for m in list(todo):
                    if (case.name, b, r) not in right:
                        right[case.name, b, r] = pair_outputs(case, b, r, kind, l, cw)
                    if differs(right[case.name, b, r], pair_outputs(case, b, r, kind, l, cw, m)):
                        table[m, (route, kind, l)] = f"{case.name} pair ({b}, {r})"
                        todo.remove(m)
            if not todo:
                break
    return table


def test_the_copy_of_the_restatement_is_the_restatement():
    """Without a mistake, pair_outputs gives what the restatements give: the mistakes are told from the right thing."""
    for route, kind, l in (("rerank", "bf16", 96), ("hires", "e4m3", 192), ("spatial", "e4m3", 64), ("spatial_hires", "bf16", 160)):
        for case in lmc.cases(route, kind, l):
            want = lmc.expected(case)
            cand = case.idx.numpy().astype(np.int64) - case.base
            for b in range(cand.shape[0]):
                for t, r in enumerate(cand[b]):
                    if 0 <= r < case.g.shape[0]:
                        got = pair_outputs(case, b, int(r), kind, l, lmc.chunk_cols(kind, l))
                        for f in got:
                            assert np.array_equal(np.asarray(got[f]), want[f][b, t]), (case.name, f, b, t)


def test_print_the_mistake_by_cell_table(caught):
    print()
    for m in MISTAKES:
        cells = [c for c in lmc.CELLS if applies(m, *c)]
        hit = [c for c in cells if (m, c) in caught]
        by_input = {}
        for c in hit:
            by_input[caught[m, c].split("/")[0]] = by_input.get(caught[m, c].split("/")[0], 0) + 1
        print(f"{m:26s} caught in {len(hit):2d} of {len(cells):2d} applicable cells; first caught by input: "
              + ", ".join(f"({k}) x {v}" for k, v in sorted(by_input.items()))
              + ("" if len(hit) == len(cells) else f"; MISSED in {[c for c in cells if c not in hit]}"))
    assert all((m, c) in caught for m in MISTAKES for c in lmc.CELLS if applies(m, *c))


@pytest.mark.parametrize("route,kind,l", lmc.CELLS, ids=CELL_IDS)
def test_every_applicable_mistake_is_caught_in_the_cell(caught, route, kind, l):
    for m in MISTAKES:
        if applies(m, route, kind, l):
            assert (m, (route, kind, l)) in caught, m
    # and each by the input built for it, whatever caught it first
    cw = lmc.chunk_cols(kind, l) if lmc.kernel_of(route) == "hires" else lmc.MAX_N_256
    by_input = {name: [c for c in lmc.cases(route, kind, l) if c.meta["input"] == name] for name in "abcde"}
    changes = lambda case, b, r, m: differs(pair_outputs(case, b, r, kind, l, cw), pair_outputs(case, b, r, kind, l, cw, m))
    assert any(changes(c, 0, 0, "min_sim_strict") for c in by_input["a"] if c.meta["units"] == 3)
    assert any(changes(c, 0, 0, "non_finite_wins") for c in by_input["c"])
    assert all(changes(c, 0, 1, "chunk^1") for c in by_input["e"])
    small = [c for c in by_input["b"] if c.q.shape[1] % 32 and c.g.shape[1] % 32][0]      # a zero pad wins every argmax
    b, r = lmc.live_pairs(small)[0]
    assert changes(small, b, r, "padded_rows_unmasked") and changes(small, b, r, "padded_columns_unmasked")
