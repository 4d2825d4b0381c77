"""CPU: ShardedGallery.search_local_queries is the one path from a rank's queries to that rank's results.  Over the cross
product (expand, rerank) x (collective or not) x (projection or not) it returns the bits of the composition written out
here from project_queries, gather_queries, search, expand and search_reranked; on two gloo ranks every rank gets its own rows
of search_expanded over the gathered batch; ws / ws2 / score_events reach the engine.  Both sides of every comparison run
on the same injected CPU engine (the searches and the f64 re-rank of test_rerank_cpu.py, an expansion in plain torch), so the
expansion's arithmetic need not be the HIP kernels'."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_host_cpu import _free_port
from test_rerank_cpu import CpuEngine, near_duplicates

N, D, B, K, KC, N_USE, ALPHA = 83, 128, 6, 5, 8, 3, 3.0
EXPAND = (N_USE, ALPHA)


class ExpandEngine(CpuEngine):
    """CpuEngine plus the three expansion methods of HipEngine, in f32 torch."""

    def expand_partial(self, q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, add_query):
        x = rows.float() if scales is None else rows.view(torch.float8_e4m3fn).float() * scales[:, None]
        out = q_weight * q.float() if add_query else torch.zeros(q.shape, dtype=torch.float32)
        for b in range(q.shape[0]):
            for j in range(n_use):                           # ascending j
                r = int(idx[b, j]) - index_base
                if 0 <= r < x.shape[0] and float(vals[b, j]) > 0:
                    out[b] += vals[b, j] ** alpha * x[r]
        return out

    def expand_finish(self, partials, q):
        s = partials[0].clone()
        for p in partials[1:]:                               # in shard order
            s += p
        n = s.norm(dim=1, keepdim=True)
        out = (s / n).to(torch.bfloat16)
        bad = ~(torch.isfinite(n) & (n > 0)).squeeze(1)
        out[bad] = q[bad]
        return out

    def expand_whole(self, q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight):
        return self.expand_finish(self.expand_partial(q, vals, idx, rows, scales, index_base, n_use, alpha, q_weight, True)[None], q)


class FirstColumns:
    """A stand-in for projection.DescriptorProjection (whose apply is GPU-only): the first d columns, re-normalised."""
    d, d_in = D // 2, D

    def apply(self, x):
        return torch.nn.functional.normalize(x[:, :self.d].float(), dim=1).to(torch.bfloat16)


def make_gallery(fine, projection, rank=0, world=1, engine=None, **kw):
    from vpr_amd.retrieval import ShardedGallery, shard_bounds
    lo, hi = shard_bounds(fine.shape[0], rank, world)
    rows = fine[lo:hi].contiguous() if projection is None else projection.apply(fine[lo:hi])
    return ShardedGallery(rows, fine.shape[0], rank, world, engine=engine or ExpandEngine(), projection=projection,
                          fine_rows=fine[lo:hi].contiguous(), **kw)


def composed(sg, q, k, expand, rerank):
    """search_local_queries written out from the public pieces: project, gather, the fine queries (the caller's unprojected
    rows), search [-> expand -> search], the last search re-ranked if asked, this rank's rows."""
    q_all = sg.gather_queries(sg.project_queries(q))
    q_fine = q_all if sg.projection is None else sg.gather_queries(q)
    last = (lambda x: sg.search(x, k)) if rerank is None else (lambda x: sg.search_reranked(x, k, rerank, q_fine))
    if expand is None:
        v, i = last(q_all)
    else:
        v, i = sg.search(q_all, k)
        v, i = last(sg.expand(q_all, v, i, *expand))
    b = q.shape[0]
    return v[sg.rank * b:(sg.rank + 1) * b], i[sg.rank * b:(sg.rank + 1) * b]


def same_bits(a, b):
    return (a[0].shape == b[0].shape and torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))
            and a[1].dtype == b[1].dtype == torch.int32 and torch.equal(a[1], b[1]))


@pytest.fixture(scope="module")
def one_rank_gloo():
    assert not dist.is_initialized()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def data():
    return near_duplicates(23, N, D, B)                      # fine rows bf16 [N, D], queries bf16 [B, D]


@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("collective", [False, True])
@pytest.mark.parametrize("expand,rerank", [(None, None), (EXPAND, None), (None, KC), (EXPAND, KC)])
def test_local_queries_equal_the_composition(one_rank_gloo, data, expand, rerank, collective, projected):
    fine, q = data
    sg = make_gallery(fine, FirstColumns() if projected else None, force_collectives=collective)
    assert sg.collective == collective and sg.query_width == D
    got = sg.search_local_queries(q, K, expand, rerank)
    assert got[0].shape == got[1].shape == (B, K) and bool((got[1] >= 0).all())
    assert same_bits(got, composed(sg, q, K, expand, rerank))
    if rerank is None:                                       # an expanded query scores differently: the forms are told apart
        assert same_bits(got, sg.search(q, K)) == (expand is None)


def _two_rank_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fine, q_all = near_duplicates(29, N, D, world * B)
    sg = make_gallery(fine, None, rank, world)
    got = sg.search_local_queries(q_all[rank * B:(rank + 1) * B].contiguous(), K, EXPAND, KC)
    v, i = sg.search_expanded(q_all, K, N_USE, ALPHA, rerank=KC, q_fine=q_all)
    ret[rank] = bool(same_bits(got, (v[rank * B:(rank + 1) * B], i[rank * B:(rank + 1) * B])) and (got[1] >= 0).all())
    dist.destroy_process_group()


def test_two_ranks_get_their_own_rows_of_the_expanded_reranked_search():
    world = 2
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_two_rank_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_workspaces_and_score_events_reach_the_engine(data):
    from vpr_amd.retrieval import HipEngine

    class SpyEngine(HipEngine):                              # a HipEngine by type: ShardedGallery hands it every argument
        def __init__(self):
            self.cpu, self.seen = ExpandEngine(), []

        def local_topk(self, q, gallery, k, index_base, scales=None, norm_bound=None, uncertified=None, ws=None,
                       score_events=None, exact_fallback=False):
            self.seen.append((k, ws, score_events))
            return self.cpu.local_topk(q, gallery, k, index_base, *([] if scales is None else [scales]))

        merge = lambda self, *a: self.cpu.merge(*a)
        rerank = lambda self, *a, **kw: self.cpu.rerank(*a, **kw)
        expand_whole = lambda self, *a: self.cpu.expand_whole(*a)

    fine, q = data
    spy = SpyEngine()
    sg, ref = make_gallery(fine, None, engine=spy), make_gallery(fine, None)
    ws, ws2, events = object(), object(), []
    for expand, rerank, kw, seen in (
            (None, None, dict(ws=ws, score_events=events), [(K, ws, events)]),
            (None, KC, dict(ws=ws, score_events=events), [(KC, ws, events)]),
            (EXPAND, None, dict(ws=ws, ws2=ws2), [(K, ws, None), (K, ws2, None)]),
            (EXPAND, None, dict(ws=ws), [(K, ws, None), (K, ws, None)]),
            (EXPAND, KC, dict(ws=ws, ws2=ws2), [(K, ws, None), (KC, ws2, None)]),
            (EXPAND, KC, {}, [(K, None, None), (KC, None, None)])):
        spy.seen.clear()
        got = sg.search_local_queries(q, K, expand, rerank, **kw)
        assert len(spy.seen) == len(seen) and all(a[0] == b[0] and a[1] is b[1] and a[2] is b[2] for a, b in zip(spy.seen, seen))
        assert same_bits(got, ref.search_local_queries(q, K, expand, rerank))
    spy.seen.clear()
    for call in (lambda: sg.search_local_queries(q, K, EXPAND, score_events=events),
                 lambda: sg.search_local_queries(q, K, {"n_use": N_USE}, KC, ws=ws, score_events=events),
                 lambda: sg.search_gathered(q, K, EXPAND, score_events=events)):
        with pytest.raises(ValueError, match="score_events"):
            call()
    assert spy.seen == [] and events == []                   # refused before anything ran
