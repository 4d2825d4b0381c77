"""Plain model of the kNN select stage (vpr_knn_select_checked) GIVEN the score matrix S — TEST ORACLE.

Written from include/vpr_amd.h ("Checked forms") and the comments of csrc/knn.hip, not from the kernels' control flow:
what the tail promises is a pure function of S, the operands, k and the norm bound, so a test can write any S into the
workspace (ops.knn_scores_view), run the tail (ops.knn_select) and compare candidate set, answer and status exactly.

  kp          = ceil8(max(2k, k + 8)) candidates per list
  level 0     chunks of 8192 scores (one chunk of ceil1024(N) when N <= 8192); later levels chunks of 4096 list
              entries; every list = the top-kp of its chunk by the key (value desc, index asc; -0.0 counts as +0.0;
              a live -inf entry ranks ahead of padding)
  fused path  taken as soon as a query's lists hold <= 4096 entries and the operand row is <= 24 KB: top-kp of the
              lists in hand, exact rescoring (f64 sum, ONE rounding to f32), order by (exact desc, index asc),
              certificate, widening
  general     otherwise the levels run down to one list of kp; rescoring, order, certificate (status 0 / 2, no widening)
  certificate e_k = k-th best exact score, a_min = kp-th approximate score kept, eps = 1.1 D 2^-24 norm_bound |q|;
              certified iff the list is not full or e_k - eps > a_min
  widening    every entry of the lists in hand below the cut with S >= bar = e_k - eps; status 2 iff the lists are level
              0's and some chunk's kp-th entry is live and >= bar, or the lists come from a later level, or
              kp + extras > 256; else status 1

The kernels form eps in f32 from an f32 sum of squares, this model in f64: a prediction binds only when no compared
quantity sits on the bar — info["margin"], the smallest distance of an S value in hand from the bar and of e_k - eps
from a_min, relative to max(1, |bar|).  On overflow (kp + extras > 256) which extras the kernel keeps depends on atomics:
the model predicts status 2 only, and check_overflow_row() checks the best-effort output structurally.
"""
import numpy as np
import torch

STREAM_CHUNK = 8192      # scores per level-0 chunk
CHUNK = 4096             # list entries per chunk of the later levels; also the fused kernel's capacity
FUSED_ROW_BYTES = 24 * 1024
MAX_RESCORED = 256       # kp + extras the fused kernel can rescore


def knn_kp(k: int) -> int:
    return (max(2 * k, k + 8) + 7) // 8 * 8


def level_plan(N: int, k: int, row_bytes: int):
    """-> dict(kp, ch0, nchunk=[per level that the plan allows for], run=[chunk sizes of the levels that run], fused,
    level0_lists) or None when the shape needs more than four levels (unsupported)."""
    kp = knn_kp(k)
    ch0 = STREAM_CHUNK if N > STREAM_CHUNK else (N + 1023) // 1024 * 1024
    nchunk, L = [], N
    while True:
        if len(nchunk) >= 4:
            return None
        chunk = ch0 if not nchunk else CHUNK
        nchunk.append((L + chunk - 1) // chunk)
        L = nchunk[-1] * kp
        if nchunk[-1] == 1:
            break
    run, L, fused = [], N, False
    for lev in range(len(nchunk)):
        if lev > 0 and L <= CHUNK and row_bytes <= FUSED_ROW_BYTES:
            fused = True
            break
        run.append(ch0 if lev == 0 else CHUNK)
        L = nchunk[lev] * kp
    if not fused and L <= CHUNK and row_bytes <= FUSED_ROW_BYTES:
        fused = True                      # every planned level ran and left one list: the fused kernel takes it
    return dict(kp=kp, ch0=ch0, nchunk=nchunk, run=run, fused=fused, level0_lists=fused and len(run) == 1)


def _align(x: int, a: int = 256) -> int:
    return (x + a - 1) // a * a


def workspace_bytes(B: int, N: int, D: int, k: int) -> int:
    """What vpr_knn_workspace_bytes answers: score slabs (up to 16 K slices for small shards), two ping-pong candidate
    lists sized by level 0's output, one |q| per query; 0 for an unsupported shape."""
    if B <= 0 or N <= 0 or D <= 0 or k <= 0 or k > 64 or D % 64:
        return 0
    plan = level_plan(N, k, 2 * D)
    if plan is None:
        return 0
    ldS = (N + 63) // 64 * 64
    nrt = max((N + 207) // 208, min((N + 15) // 16, 32))
    ks = min(max(512 // nrt, 1), 16)
    if B > 64:
        tiles = ((B + 255) // 256) * ((N + 255) // 256)
        ks = min(1 if tiles >= 256 else 256 // tiles, 4)
    cand = B * plan["nchunk"][0] * plan["kp"]
    return _align(B * ldS * 4 * ks) + 2 * (_align(cand * 4) + _align(cand * 4)) + _align(B * 4)


def _top(vals: np.ndarray, idx: np.ndarray, kp: int):
    """Top-kp live entries by (value desc, index asc)."""
    o = np.lexsort((idx, -vals.astype(np.float64)))[:kp]
    return vals[o], idx[o]


def _lists(vals, idx, chunk, kp):
    """One select level: the top-kp list of every chunk -> (values, indices, list lengths)."""
    ov, oi, ln = [], [], []
    for lo in range(0, len(vals), chunk):
        v, i = _top(vals[lo:lo + chunk], idx[lo:lo + chunk], kp)
        ov.append(v), oi.append(i), ln.append(len(v))
    return np.concatenate(ov), np.concatenate(oi), ln


def _exact_order(e32: np.ndarray, idx: np.ndarray):
    """Order by (f32 exact score desc, index asc) -> permutation."""
    return np.lexsort((idx, -e32.astype(np.float64)))


def knn_select_model(S, q, g, k: int, norm_bound: float, index_base: int = 0, row_bytes=None):
    """S [B, N] f32 (torch or numpy), q [B, D] / g [N, D] bf16 torch -> (vals f32 [B, k], idx int32 [B, k],
    status int32 [B], info list of dicts).  info[b]: candidates (local rows rescored before widening), widening (rows
    the widening step adds; None on overflow), margin, overflow, unwidened (vals, idx of the answer without widening),
    exact (dict row -> f32 exact score of every row the model rescored)."""
    S = np.asarray(S.detach().cpu().numpy() if isinstance(S, torch.Tensor) else S, dtype=np.float32)
    S = S + np.float32(0.0)                                  # -0.0 counts as +0.0
    B, N = S.shape
    D = q.shape[1]
    plan = level_plan(N, k, 2 * D if row_bytes is None else row_bytes)
    if plan is None:
        raise ValueError("unsupported shape")
    kp = plan["kp"]
    qd, gc = q.detach().cpu().to(torch.float64).numpy(), g.detach().cpu()
    vals = np.full((B, k), -np.inf, dtype=np.float32)
    idxs = np.full((B, k), -1, dtype=np.int32)
    status = np.zeros(B, dtype=np.int32)
    info = []

    def exact(b, rows):
        rows = torch.from_numpy(np.asarray(rows, dtype=np.int64))
        return (gc[rows].to(torch.float64).numpy() @ qd[b]).astype(np.float32)      # f64 sum, one rounding

    def answer(e32, rows):
        o = _exact_order(e32, rows)[:k]
        v = np.full(k, -np.inf, dtype=np.float32)
        i = np.full(k, -1, dtype=np.int32)
        v[:len(o)], i[:len(o)] = e32[o], rows[o] + index_base
        return v, i

    for b in range(B):
        cv, ci = S[b].copy(), np.arange(N, dtype=np.int64)
        lens = [N]
        for chunk in plan["run"]:
            cv, ci, lens = _lists(cv, ci, chunk, kp)
        if not plan["fused"]:
            assert len(lens) == 1
        tv, ti = _top(cv, ci, kp)                            # the top-kp of the lists in hand, rank-ordered
        e = exact(b, ti)
        v0, i0 = answer(e, ti)
        full = len(ti) == kp
        e_k = float(np.sort(e.astype(np.float64))[::-1][k - 1]) if len(ti) >= k else -np.inf
        eps = 1.1 * D * 2.0 ** -24 * float(norm_bound) * float(np.sqrt((qd[b] ** 2).sum()))
        bar = e_k - eps
        scale = max(1.0, abs(bar)) if np.isfinite(bar) else 1.0
        a_min = float(tv[-1]) if full else -np.inf
        margin = abs(bar - a_min) / scale if full else np.inf
        rec = dict(candidates=set(ti.tolist()), widening=set(), margin=margin, overflow=False, unwidened=(v0, i0),
                   exact=dict(zip(ti.tolist(), e.tolist())), bar=bar, path="fused" if plan["fused"] else "general")
        if not full or bar > a_min:
            st, (v, i) = 0, (v0, i0)
        elif not plan["fused"]:
            st, (v, i) = 2, (v0, i0)
        else:
            below = ~np.isin(ci, ti)                         # entries of the lists in hand below the cut
            with np.errstate(invalid="ignore"):
                rec["margin"] = min(margin, float(np.min(np.abs(cv[below].astype(np.float64) - bar), initial=np.inf)) / scale)
            wi = ci[below & (cv >= bar)]
            cut = False
            if plan["level0_lists"]:
                ends = np.cumsum(lens)
                cut = any(n == kp and cv[end - 1] >= bar for n, end in zip(lens, ends))
            else:
                cut = True
            over = kp + len(wi) > MAX_RESCORED
            st = 2 if (cut or over) else 1
            if over:
                rec["overflow"], rec["widening"] = True, None
                v, i = v0, i0                                # not predicted: see check_overflow_row
            else:
                rows = np.concatenate([ti, wi])
                ee = np.concatenate([e, exact(b, wi)])
                rec["widening"] = set(wi.tolist())
                rec["exact"].update(zip(wi.tolist(), ee[len(ti):].tolist()))
                v, i = answer(ee, rows)
        vals[b], idxs[b], status[b] = v, i, st
        info.append(rec)
    return torch.from_numpy(vals), torch.from_numpy(idxs), torch.from_numpy(status), info


def check_overflow_row(v, i, b, q, g, info_b, index_base: int = 0):
    """Structural check of a best-effort row (status 2 by overflow): indices distinct and live, each value the exact
    score of its index, sorted by (value desc, index asc), and no worse than the un-widened answer position by
    position.  Returns None or a message."""
    v, i = np.asarray(v, dtype=np.float32), np.asarray(i, dtype=np.int64) - index_base
    N = g.shape[0]
    if len(set(i.tolist())) != len(i) or i.min() < 0 or i.max() >= N:
        return "indices are not distinct live rows"
    e = (g[torch.from_numpy(i)].to(torch.float64).numpy() @ q[b].to(torch.float64).numpy()).astype(np.float32)
    if not np.array_equal(e.view(np.int32), v.view(np.int32)):
        return "a value is not the exact score of its index"
    if not np.array_equal(_exact_order(v, i), np.arange(len(v))):
        return "not sorted by (value desc, index asc)"
    if np.any(v < info_b["unwidened"][0]):
        return "worse than the un-widened answer"
    return None


def compare(got, want, info=None):
    """The checker of the GPU tests: None when (vals, idx, status) match bit for bit, else what differs first."""
    gv, gi, gs = (t.detach().cpu() for t in got)
    wv, wi, ws = want
    if not torch.equal(gs.to(torch.int32), ws.to(torch.int32)):
        return f"status {gs.tolist()} != {ws.tolist()}"
    skip = [b for b in range(len(ws)) if info is not None and info[b]["overflow"]]
    keep = [b for b in range(len(ws)) if b not in skip]
    if not torch.equal(gi[keep].to(torch.int32), wi[keep]):
        return f"indices differ: {gi[keep].tolist()} != {wi[keep].tolist()}"
    if not torch.equal(gv[keep].view(torch.int32), wv[keep].view(torch.int32)):
        return "values differ (bit compare)"
    return None
