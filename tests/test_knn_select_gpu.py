"""The kNN tail (level-0 streaming select, register select levels, fused final kernel with widening, knn_rescore_kernel +
knn_order_kernel) on HAND-MADE score matrices: S is written into the workspace through ops.knn_scores_view, the tail
runs through ops.knn_select (vpr_knn_select_checked), and values, indices, status and the uncertified count are compared
bit for bit with oracle/knn_select.py, a plain model of what the stage promises given S.  Gallery rows have norms spread
over 1e-2 .. 1e2, so the exact scores have nothing to do with S.  Pad columns N .. ld-1 of the score matrix are poisoned."""
import functools

import numpy as np
import pytest
import torch

from oracle import knn_select as oks

pytestmark = pytest.mark.gpu

MARGIN = 1e-4            # the model's prediction binds when nothing sits closer to the bar than this (oracle/knn_select.py)
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _operands(N, D, positive=False):
    """(q [3, D], g [N, D]) bf16: random rows, gallery norms log-uniform in 1e-2 .. 1e2; positive: all entries > 0, so
    every exact score is positive."""
    gen = torch.Generator().manual_seed(1000 * D + N)
    g = torch.randn(N, D, generator=gen)
    q = torch.randn(3, D, generator=gen)
    if positive:
        g, q = g.abs() + 0.1, q.abs() + 0.1
    norms = 10.0 ** (4 * torch.rand(N, generator=gen) - 2)
    g = torch.nn.functional.normalize(g, dim=1) * norms[:, None]
    return q.to(torch.bfloat16), g.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _on_device(N, D, positive=False):
    q, g = _operands(N, D, positive)
    return q.cuda(), g.cuda()


def _run(dev, S, q, g, k, index_base=0, norm_bound=1.0, poison=INF, status=True, uncertified=0):
    """The harness: poison the whole padded score matrix, write S, run the tail.  -> (vals, idx, status, uncertified)."""
    from vpr_amd import ops
    B, N = S.shape
    D = q.shape[1]
    ws = ops.knn_workspace(B, N, D, k, dev)
    view = ops.knn_scores_view(ws, B, N, D, k)
    ld = view.stride(0)
    assert ld % 64 == 0 and ld >= N
    torch.as_strided(view, (B, ld), (ld, 1)).fill_(poison)          # pad columns included
    view.copy_(S)
    st = torch.full((B,), -7, dtype=torch.int32, device=dev) if status else None
    unc = torch.full((1,), uncertified, dtype=torch.int32, device=dev) if uncertified is not None else None
    v, i = ops.knn_select(q.to(dev), g.to(dev), k, ws, index_base, norm_bound=norm_bound, status=st, uncertified=unc)
    torch.cuda.synchronize()
    return v.cpu(), i.cpu(), None if st is None else st.cpu(), None if unc is None else int(unc)


def _assert_matches(got, want, info, q, g, index_base=0):
    """Bit compare with the model; rows the model cannot predict (overflow) are checked structurally."""
    assert min(r["margin"] for r in info) >= MARGIN, "badly built case: something sits on the bar"
    msg = oks.compare(got[:3], want, info)
    assert msg is None, msg
    for b, r in enumerate(info):
        if r["overflow"]:
            msg = oks.check_overflow_row(got[0][b].numpy(), got[1][b].numpy(), b, q, g, r, index_base)
            assert msg is None, f"row {b}: {msg}"


# ------------------------------------------------------------------------------------------------ selection layouts
BASE = -1.0e6            # far below every exact score (|e| <= |q| |g| < 2000): status 0 whatever the layout
WINNER = 5.0e5           # winners of the ownership layouts sit this far above the rest


def _perm(N, gen):
    return BASE - torch.randperm(N, generator=gen).float()        # distinct, exactly representable (< 2^24)


def _layouts(N, kp, seed):
    """name -> S row [N] f32.  Every layout keeps a_min <= BASE or -inf / -3e38, so the certificate holds at once."""
    gen = torch.Generator().manual_seed(seed)
    ar = torch.arange(N)
    out = {"perm": _perm(N, gen), "ascending": BASE - (N - 1 - ar).float(), "descending": BASE - ar.float(),
           "equal": torch.full((N,), BASE), "two values": BASE - (torch.rand(N, generator=gen) < 0.7).float()}

    def winners(mask):                                              # distinct winners on `mask`, distinct losers elsewhere
        s = _perm(N, gen)
        s[mask] += WINNER
        return s
    out["one thread"] = winners((ar % 1024) // 4 == 37)             # positions 4t + 1024 i + e of thread t = 37
    out["one wave"] = winners((ar % 1024) // 256 == 2)              # positions 256 w .. 256 w + 255 of every 1024, w = 2
    out["last 32"] = winners(ar >= N - 32)                          # the tail of the last, ragged chunk
    s = _perm(N, gen)
    s[torch.rand(N, generator=gen) < 0.5] = -INF                    # live -inf entries: candidates like any other
    out["-inf mixed"] = s
    s = _perm(N, gen)
    r = torch.rand(N, generator=gen)
    s[r < 0.3] = -3e38
    s[torch.randperm(N, generator=gen)[:kp // 2]] = 3e38            # fewer than kp of them: a_min stays low
    out["+-3e38"] = s
    return out


def _select_case(dev, N, k, index_base, poison, names=None, D=64):
    q, g = _operands(N, D)
    qd, gd = _on_device(N, D)
    lay = _layouts(N, oks.knn_kp(k), 7 * N + k)
    names = list(lay) if names is None else names
    for lo in range(0, len(names), 3):                              # three layouts per call, one per query; the last call has B = 1
        grp = names[lo:lo + 3]
        S = torch.stack([lay[n] for n in grp])
        B = len(grp)
        want = oks.knn_select_model(S, q[:B], g, k, 1.0, index_base)
        assert want[2].tolist() == [0] * B, grp
        got = _run(dev, S, qd[:B], gd, k, index_base, 1.0, poison)
        try:
            assert got[3] == 0, "uncertified counter moved"
            _assert_matches(got, want[:3], want[3], q[:B], g, index_base)
        except AssertionError as e:
            raise AssertionError(f"layouts {grp}, N={N} k={k}: {e}") from None


SWEEP_N = [1, 7, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 3 * 8192 + 5]


@pytest.mark.parametrize("poison,index_base", [(INF, 0), (3e38, 12345)])
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("k", [1, 8, 16, 17, 32, 64])
def test_selection_layouts(dev, k, N, poison, index_base):
    """kp = 16, 16, 32, 40, 64, 128 (the list capacity changes from 1024 to 4096 above kp = 32) x chunk edges x ten
    layouts: the output must be the exact order of the top-kp by S, status 0."""
    _select_case(dev, N, k, index_base, poison)


def _mixed_zero_rows(N, kp):
    """Two rows of +0.0 / -0.0 / -1.  Row 0 is the arrangement that breaks a select whose max pass and filter do not
    follow the key's order: the LAST kp threads hold -1 except a +0.0 in their last slot, every other thread holds -0.0.
    Row 1 mixes the three values at random."""
    ar = torch.arange(N)
    thread = (ar % 1024) // 4
    nthreads = int(thread.max()) + 1
    a = torch.full((N,), -0.0)
    own = thread >= nthreads - kp
    a[own] = -1.0
    slots = ar[own]
    for t in range(max(0, nthreads - kp), nthreads):
        mine = slots[thread[slots] == t]
        a[mine[-1]] = 0.0
    gen = torch.Generator().manual_seed(N + kp)
    r = torch.rand(N, generator=gen)
    b = torch.where(r < 0.4, torch.tensor(-0.0), torch.where(r < 0.8, torch.tensor(0.0), torch.tensor(-1.0)))
    return torch.stack([a, b])


@pytest.mark.parametrize("k,N", [(k, N) for k in (1, 8, 16) for N in (1, 7, 1023, 1024)] +
                         [(k, N) for k in (17, 32, 64) for N in (1, 7, 1023, 1024, 1025, 4095, 4096)])
def test_mixed_zeros_select_like_positive_zeros(dev, k, N):
    """-0.0 counts as +0.0: the expected candidate set is that of the all-+0.0 matrix (lowest indices first).  Shapes are
    bounded (N <= 1024 for k <= 16, N <= 4096 otherwise) so that a chunk never holds more scores than the level-0
    candidate list has room for: a select that mishandles the zeros fails here by a wrong answer, never by a fault."""
    kp = oks.knn_kp(k)
    assert N <= (1024 if kp <= 32 else 4096)
    q, g = _operands(N, 64, True)
    qd, gd = _on_device(N, 64, True)
    S = _mixed_zero_rows(N, kp)
    want = oks.knn_select_model(S, q[:2], g, k, 1e-6, 3)
    plus = oks.knn_select_model(S + 0.0, q[:2], g, k, 1e-6, 3)
    assert oks.compare(want[:3], plus[:3]) is None and want[2].tolist() == [0, 0]
    zeros = np.flatnonzero(S[0].numpy() == 0)
    assert want[3][0]["candidates"] >= set(zeros[:kp].tolist())
    got = _run(dev, S, qd[:2], gd, k, 3, 1e-6)
    _assert_matches(got, want[:3], want[3], q[:2], g, 3)


def test_more_than_4096_level0_candidates(dev):
    """38 level-0 lists of kp = 128: the knn_select_kernel level runs before the fused kernel."""
    N, k = 37 * 8192 + 11, 64
    assert oks.level_plan(N, k, 128)["run"] == [8192, 4096]
    _select_case(dev, N, k, 12345, 3e38, ["perm", "descending", "last 32"])


@pytest.mark.parametrize("N", [600, 12])
def test_general_path_selection(dev, N):
    """Rows of 32 KB: knn_rescore_kernel + knn_order_kernel on a list the select levels cut down to kp."""
    assert not oks.level_plan(N, 5, 2 * 16384)["fused"]
    _select_case(dev, N, 5, 12345, INF, ["perm", "equal", "-inf mixed"], D=16384)


# ------------------------------------------------------------------------------------------------------ certificate
NB = 1.0e4               # the norm bound of the certificate cases: eps = 1.1 D 2^-24 NB |q| (about 0.4 at D = 64)


def _design(qrow, g, k, above, certified, seed, fill=4):
    """One score row whose outcome is known.  above[c] rows of level-0 chunk c get S >= bar; kp of them (never the rows
    with the best exact score of their chunk, so that only widening reaches those) are the top-kp with a_min = bar + 2u (certified:
    every `above` row is a candidate and a_min = bar - u, one step short of the bar); `fill` more rows per chunk sit
    one to two steps BELOW the bar; everything else far below.  u = 1e-3 max(1, |bar|), ten times the model's margin.
    bar = e_k - eps follows from the candidate rows alone, so it is known before S is written."""
    N, D = g.shape
    kp = oks.knn_kp(k)
    gen = torch.Generator().manual_seed(seed)
    E = (g.double() @ qrow.double()).float()
    rows, n_chunks = [], (N + 8191) // 8192
    chunk_best = [c * 8192 + int(torch.argmax(E[c * 8192:(c + 1) * 8192])) for c in range(n_chunks)]
    best = set(chunk_best)
    assert len(above) == n_chunks and sum(above) >= kp and (not certified or sum(above) == kp)
    for c, n in enumerate(above):
        lo, hi = c * 8192, min(N, (c + 1) * 8192)
        pool = [r for r in (lo + torch.randperm(hi - lo, generator=gen)).tolist() if r not in best][:n + fill]
        rows.append(pool)
    hi_rows = [r for c, pool in enumerate(rows) for r in pool[:above[c]]]
    lo_rows = [r for c, pool in enumerate(rows) for r in pool[above[c]:]]
    cand = hi_rows[:kp] if certified else [hi_rows[j] for j in torch.randperm(len(hi_rows), generator=gen)[:kp].tolist()]
    extra = [r for r in hi_rows if r not in set(cand)]
    done = set()
    for j, r in enumerate(extra):                                   # one extra per chunk gives way to the chunk's best exact row
        if r // 8192 not in done:
            done.add(r // 8192)
            extra[j] = chunk_best[r // 8192]
    e_k = float(torch.sort(E[cand].double(), descending=True).values[k - 1])
    eps = 1.1 * D * 2.0 ** -24 * NB * float(qrow.double().norm())
    bar = e_k - eps
    u = 1e-3 * max(1.0, abs(bar))
    S = bar - 1e3 * u * (2 + torch.rand(N, generator=gen, dtype=torch.float64))
    top = bar + (-u if certified else 2 * u)
    for j, r in enumerate(cand):
        S[r] = top + 0.37 * u * j
    for r in extra:
        S[r] = bar + u * (0.3 + float(torch.rand((), generator=gen)))
    for r in lo_rows:
        S[r] = bar - u * (1 + float(torch.rand((), generator=gen)))
    return S.float(), set(cand), set(extra)


def _cert_rows(N, D, k, specs):
    """specs: (above, certified) per query -> (S, q, g, model outputs)."""
    q, g = _operands(N, D)
    B = len(specs)
    built = [_design(q[b], g.float(), k, above, cert, 31 * b + k) for b, (above, cert) in enumerate(specs)]
    S = torch.stack([s for s, _, _ in built])
    want = oks.knn_select_model(S, q[:B], g, k, NB)
    for b, (_, cand, extra) in enumerate(built):
        assert want[3][b]["candidates"] == cand
        if not want[3][b]["overflow"] and want[2][b] != 0 and want[3][b]["path"] == "fused":
            assert want[3][b]["widening"] == extra
    return S, q[:B], g, want


def _cert_check(dev, N, D, k, specs, statuses, **kw):
    S, q, g, want = _cert_rows(N, D, k, specs)
    assert want[2].tolist() == statuses
    qd, gd = _on_device(N, D)
    got = _run(dev, S, qd[:len(specs)], gd, k, norm_bound=NB, uncertified=5, **kw)
    _assert_matches(got, want[:3], want[3], q, g)
    assert got[3] == 5 + statuses.count(2)
    return S, q, g, want, got


N3 = 3 * 8192 - 100       # three level-0 chunks, the last one ragged


def test_certified_one_step_before_the_bar_and_widened_one_step_after(dev):
    """a_min = bar - u: status 0.  a_min = bar + 2u with nothing else in hand above the bar: status 1, nothing added."""
    _cert_check(dev, N3, 64, 10, [([8, 8, 8], True), ([8, 8, 8], False)], [0, 1])


def test_widening_by_one_row_and_by_all_the_room_there_is(dev):
    """Widening sets of exactly 1 row (k = 10, kp = 24) and of exactly 256 - kp = 128 rows (k = 64, kp = 128; no chunk
    holds more than kp - 1 = 127 rows above the bar, so no list is cut): status 1, and the answer holds rows that only
    the widening step reaches."""
    for k, above, extras in ((10, [9, 8, 8], 1), (64, [127, 127, 2], 128)):
        S, q, g, want, got = _cert_check(dev, N3, 64, k, [(above, False)], [1])
        wide = want[3][0]["widening"]
        assert len(wide) == extras
        assert set(got[1][0].tolist()) & wide, "no row of the answer comes from the widening step"


def test_flagged_by_a_cut_chunk_list(dev):
    """kp = 24 rows of ONE chunk above the bar: its list is cut inside the band (its kp-th entry is live and >= bar),
    although the widened set fits.  The other query has 23 there: status 1."""
    _cert_check(dev, N3, 64, 10, [([24, 8, 8], False), ([23, 9, 8], False)], [2, 1])


def test_flagged_by_lists_of_a_later_level(dev):
    """38 level-0 lists of 128: the fused kernel sees lists of the second level, whose per-chunk cuts it cannot know."""
    N, k = 37 * 8192 + 11, 64
    above = [4] * 38
    _cert_check(dev, N, 64, k, [(above, False), ([4] * 32 + [0] * 6, True)], [2, 0])


def test_flagged_by_overflow_keeps_a_sound_best_effort(dev):
    """3 x 127 rows above the bar, none of the lists cut: kp + extras = 381 > 256.  Which extras are rescored depends on
    atomics; the output must still be distinct live rows with their exact scores, in order, no worse than un-widened."""
    S, q, g, want, got = _cert_check(dev, N3, 64, 64, [([127, 127, 127], False)], [2])
    assert want[3][0]["overflow"]


def test_general_path_is_certified_or_flagged(dev):
    """Rows of 32 KB: no widening, status 0 or 2 by the same inequality; fewer rows than kp: 0 whatever S."""
    _cert_check(dev, 600, 16384, 5, [([16], True), ([20], False), ([16], False)], [0, 2, 2])
    q, g = _operands(12, 16384)
    qd, gd = _on_device(12, 16384)
    S = torch.full((3, 12), 1e30)
    want = oks.knn_select_model(S, q, g, 5, 1e6)
    assert want[2].tolist() == [0, 0, 0]
    _assert_matches(_run(dev, S, qd, gd, 5, norm_bound=1e6), want[:3], want[3], q, g)


def test_status_and_counter_are_optional_and_rows_are_independent(dev):
    """status=None / uncertified=None change nothing in the outputs; a query's result does not depend on the other rows
    of its batch (alone, at position 0 and at position 2 of B = 3)."""
    k = 10
    specs = [([24, 8, 8], False), ([8, 8, 8], True), ([9, 8, 8], False)]
    S, q, g, want = _cert_rows(N3, 64, k, specs)
    qd, gd = _on_device(N3, 64)
    full = _run(dev, S, qd, gd, k, norm_bound=NB, uncertified=5)
    _assert_matches(full, want[:3], want[3], q, g)
    bare = _run(dev, S, qd, gd, k, norm_bound=NB, status=False, uncertified=None)
    assert bare[2] is None and bare[3] is None
    assert torch.equal(bare[0], full[0]) and torch.equal(bare[1], full[1])
    # query 0's row and query 2's row change places with their operands; each alone as well
    perm = [2, 1, 0]
    swapped = _run(dev, S[perm], qd[perm], gd, k, norm_bound=NB)
    for b in range(3):
        alone = _run(dev, S[b:b + 1], qd[b:b + 1], gd, k, norm_bound=NB)
        for t in range(3):
            assert torch.equal(alone[t][0], full[t][b]) and torch.equal(swapped[t][perm.index(b)], full[t][b]), (b, t)


def test_mutations_of_the_outputs_are_caught(dev):
    """The comparison applied to the kernel's own outputs with one index pair swapped, one value moved by one ulp and
    one status changed: it rejects each of them."""
    S, q, g, want, got = _cert_check(dev, N3, 64, 10, [([9, 8, 8], False), ([8, 8, 8], True)], [1, 0])
    v, i, st, _ = got
    i2 = i.clone(); i2[0, [3, 4]] = i[0, [4, 3]]
    v2 = v.clone(); v2[1, 9] = torch.nextafter(v[1, 9], torch.tensor(-INF))
    st2 = st.clone(); st2[1] = 1
    for bad, what in (((v, i2, st), "indices"), ((v2, i, st), "values"), ((v, i, st2), "status")):
        with pytest.raises(AssertionError, match=what):
            _assert_matches(bad, want[:3], want[3], q, g)
