"""GPU: what _streams owns, on the device.  The two fork / join options of the backbone's cls side chain that only
bench.py --side-sync ever ran ("light", "signals") against the default and the in-stream path, bit for bit; a drop of a
main stream forgets every helper stream, fork / join object and workspace made for it; close() of the three graph wrappers
leaves nothing keyed by their private streams.  vit_small, 224 px, B = 2 (two cls rows: the smallest batch where the
cls-row kernels see more than one row), all 12 blocks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _keys(raw):
    from vpr_amd import ops
    return [k for c in ops._STREAM_KEYED for k in c._entries if k[1] == raw]


@pytest.fixture(scope="module")
def small(dev):
    """(extractor, images [2, 3, 224, 224] bf16, the backbone's tokens with the side chain off, and with it on by events)."""
    from vpr_amd.modules import DinoV2Salad
    torch.manual_seed(11)
    ext = DinoV2Salad("vit_small").to(dev).to(torch.bfloat16).eval()
    for p in ext.aggregator.parameters():
        if p.dim() > 0:
            torch.nn.init.normal_(p, std=0.05)
    ext.backbone.fold_layerscale()
    x = torch.randn(2, 3, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(4)).to(torch.bfloat16)
    m = ext.backbone
    m.cls_side_chain = False
    in_stream = m(x, split=True)
    m.cls_side_chain = True
    events = m(x, split=True)
    torch.cuda.synchronize()
    assert torch.equal(events.patch, in_stream.patch) and torch.equal(events.cls, in_stream.cls)
    return ext, x, in_stream, events


@pytest.mark.parametrize("mode", ["light", "signals"])
def test_side_sync_modes_are_bit_identical_to_events_and_to_the_in_stream_path(small, dev, mode):
    from vpr_amd import _streams, ops
    ext, x, in_stream, events = small
    m = ext.backbone
    s = torch.cuda.Stream(device=dev)           # a main stream of the test's own: its drop below runs the object's close()
    s.wait_stream(torch.cuda.current_stream(dev))
    m.side_sync = mode
    try:
        with torch.cuda.stream(s):
            outs = [m(x, split=True) for _ in range(3)]
    finally:
        m.side_sync = "events"
    torch.cuda.synchronize()
    for t in outs:
        assert torch.equal(t.patch, events.patch) and torch.equal(t.cls, events.cls)
        assert torch.equal(t.patch, in_stream.patch) and torch.equal(t.cls, in_stream.cls)
    sync = _streams._SYNCS._entries[(dev.index, s.cuda_stream, mode)][0]
    assert len(sync._handles) == (2 if mode == "signals" else _streams._RawEvents.RING)
    ops.drop_stream_caches(s.cuda_stream)
    assert _keys(s.cuda_stream) == [] and sync._handles == []


def test_unknown_side_sync_mode_is_refused(small):
    ext, x, _, _ = small
    ext.backbone.side_sync = "semaphores"
    try:
        with pytest.raises(RuntimeError, match="unknown mode"):
            ext.backbone(x, split=True)
    finally:
        ext.backbone.side_sync = "events"
    torch.cuda.synchronize()


def test_drop_stream_caches_forgets_everything_made_for_a_main_stream(small, dev):
    import torch.nn as nn
    from vpr_amd import _streams, ops
    from vpr_amd.modules import FusedGeoPoseHead
    from vpr_amd.pipeline import VPRGeoPosePipeline
    from vpr_amd.retrieval import ShardedGallery
    ext, x, _, events = small
    torch.manual_seed(0)
    pos = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    ang = nn.Sequential(nn.Linear(8448, 64), nn.ReLU(), nn.Linear(64, 2)).to(dev)
    gal = torch.nn.functional.normalize(torch.randn(3000, 8448, device=dev), dim=1).to(torch.bfloat16)
    images = torch.randn(4, 3, 224, 224, device=dev).to(torch.bfloat16)
    pipe = VPRGeoPosePipeline(ext, FusedGeoPoseHead(pos, ang, normalize=True), ShardedGallery(gal, 3000), 5, overlap_head=True)
    w = ext.aggregator._packed or ext.aggregator.pack()

    def on_a_new_stream(everything):
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            out = [ext.features(x, want_bf16=True)]                     # backbone side chain ("cls") + token MLP on it
            if everything:
                out.append(ops.salad_aggregate_split(events.patch, events.cls, w, overlap=True))      # "salad"
                out.append(pipe.step(images))                           # "head"
        torch.cuda.synchronize()
        return s, out

    s, first = on_a_new_stream(True)
    raw = s.cuda_stream
    assert {k[2] for k in _streams._SIDES._entries if k[1] == raw} == {"cls", "salad", "head"}
    assert any(k[1] == raw for k in ops._WORKSPACES._entries) and any(k[1] == raw for k in ops._ZERO_ROWS._entries)
    assert torch.equal(first[1][0], first[0][0]) and torch.equal(first[1][1], first[0][1])   # overlap == the hooked form
    ops.drop_stream_caches(raw)
    assert _keys(raw) == []
    s2, again = on_a_new_stream(False)
    assert s2.cuda_stream != raw
    assert torch.equal(again[0][0], first[0][0]) and torch.equal(again[0][1], first[0][1])
    ops.drop_stream_caches(s2.cuda_stream)


def test_graphed_forward_captures_under_signals_and_close_forgets_its_stream(small, dev):
    from vpr_amd.graphed import GraphedForward
    ext, x, _, _ = small
    ext.backbone.side_sync = "signals"          # under capture (and with the side chain off inside it) the mode is "events"
    try:
        eager, eager16 = ext.features(x, want_bf16=True)
        gf = GraphedForward(lambda t: ext.features(t, want_bf16=True), module=ext)
        d, d16 = gf(x)
        torch.cuda.synchronize()
    finally:
        ext.backbone.side_sync = "events"
    assert gf.fallback_reason is None and gf.graphs() == 1
    assert torch.equal(d, eager) and torch.equal(d16, eager16)
    raws = [cap.stream.cuda_stream for cap, _ in gf._graphs.values()]
    assert len(raws) == 1 and _keys(raws[0]) != []
    gf.close()
    assert _keys(raws[0]) == [] and gf.graphs() == 0
    gf.close()                                  # idempotent


def test_graphed_retrieval_and_local_topk_close_forget_their_streams(dev):
    from vpr_amd import gallery, ops
    from vpr_amd.retrieval import GraphedRetrieval, ShardedGallery
    g = torch.Generator(device=dev).manual_seed(9)
    N, D = 9000, 8448
    gal = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1).to(torch.bfloat16)
    q = torch.nn.functional.normalize(torch.randn(64, D, device=dev, generator=g), dim=1).to(torch.bfloat16)
    sg = ShardedGallery(gal, N)
    gr = GraphedRetrieval(sg, 8, 5, expand=(4, 2.0))       # the expanded form keeps a workspace of its own on the private stream
    v, i = gr(q[:8])
    v_e, i_e = sg.search_local_queries(q[:8], 5, (4, 2.0))
    assert torch.equal(i, i_e) and torch.equal(v, v_e)
    shard = gallery.GalleryShard(gal[N // 2:], None, np.zeros((N, 4)), N, N // 2, "bf16")
    lt = gallery.GraphedLocalTopK(shard, 64, 10)
    v, i = lt(q)
    v_e, i_e = ops.knn_topk(q, shard.rows, 10, shard.index_base)
    assert torch.equal(i, i_e) and torch.equal(v, v_e)
    torch.cuda.synchronize()
    assert _keys(gr._captured.stream.cuda_stream) != []
    for wrapper in (gr, lt):
        raw = wrapper._captured.stream.cuda_stream
        wrapper.close()
        assert _keys(raw) == [] and wrapper._captured.stream is None
        wrapper.close()
