"""The graph-safe cache (_cache.Cache) driven on CPU tensors with a substituted capture probe, the one corrected cache key
(DinoV2._cumulative_bias), and the ctypes prototype table against a literal snapshot."""
import gc
import weakref

import torch

from vpr_amd import _lib, _streams, ops
from vpr_amd._cache import Cache, tensor_key
from vpr_amd.backbone import DinoV2


class Probe:
    """Stands in for ops.capturing()."""
    def __init__(self):
        self.on = False

    def __call__(self):
        return self.on


def _buf(n=4):
    return torch.zeros(n)


def test_unpinned_entries_are_evicted_oldest_first_at_capacity():
    c = Cache(Probe(), capacity=3)
    built = []
    for i in range(5):
        c.get(i, lambda i=i: built.append(i) or _buf())
        assert len(c) == min(i + 1, 3)
    assert [k in c for k in range(5)] == [False, False, True, True, True]
    c.get(2, lambda: built.append("again") or _buf())        # a hit builds nothing and does not change the age order
    c.get(5, _buf)
    assert built == [0, 1, 2, 3, 4] and [k in c for k in range(6)] == [False, False, False, True, True, True]


def test_get_returns_the_cached_object_and_passes_args_to_build():
    c = Cache(Probe())
    a = c.get("k", torch.zeros, (3,))
    assert a.shape == (3,) and c.get("k", torch.ones, (5,)) is a
    for i in range(100):                                     # no capacity: nothing is evicted
        c.get(i, _buf)
    assert len(c) == 101 and c.get("k", _buf) is a


def test_entry_handed_out_under_capture_survives_capacity_pressure_and_is_still_hit():
    probe = Probe()
    c = Cache(probe, capacity=2)
    probe.on = True
    pinned = c.get("graph", _buf)
    probe.on = False
    alive = weakref.ref(pinned)
    for i in range(10):
        c.get(i, _buf)
    assert "graph" in c and c.get("graph", _buf) is pinned
    assert len(c) == 3 and 8 in c and 9 in c and 7 not in c  # the pinned entry does not count against the capacity
    del pinned
    gc.collect()
    assert alive() is not None


def test_entry_cached_before_capture_is_pinned_when_a_capture_hits_it():
    probe = Probe()
    c = Cache(probe, capacity=1)
    first = c.get("warm", _buf)                               # the warm-up call, outside capture
    probe.on = True
    assert c.get("warm", _buf) is first                       # the captured call
    probe.on = False
    c.get("other", _buf)
    c.get("third", _buf)
    assert c.get("warm", _buf) is first and "other" not in c


def test_pinned_entry_survives_a_version_bump_of_its_source():
    probe = Probe()
    c = Cache(probe, capacity=1)
    src = torch.ones(8)
    old_key = tensor_key(src)
    probe.on = True
    packed = c.get(old_key, src.clone, sources=(src,))
    probe.on = False
    alive = weakref.ref(packed)
    src.add_(1)                                               # in-place update: same address, next version
    new_key = tensor_key(src)
    assert new_key != old_key and new_key[0][0] == old_key[0][0]
    repacked = c.get(new_key, src.clone, sources=(src,))
    assert repacked is not packed and torch.equal(repacked, src)
    c.get(tensor_key(torch.ones(8)), _buf)                    # pressure: evicts the unpinned repacked entry only
    assert new_key not in c and old_key in c
    assert c.get(old_key, _buf) is packed and torch.equal(packed, torch.ones(8))
    del packed
    gc.collect()
    assert alive() is not None


def test_pinned_entry_survives_a_grow_request_and_the_old_buffer_stays_referenced():
    probe = Probe()
    c = Cache(probe)
    key = (0, 1234, "ws")
    probe.on = True
    small = c.get(key, _buf, (16,), need=16)
    probe.on = False
    assert c.get(key, _buf, (16,), need=8) is small           # a smaller request is served by the same buffer
    alive = weakref.ref(small)
    big = c.get(key, _buf, (64,), need=64)
    assert big is not small and big.numel() == 64 and c.get(key, _buf, (64,), need=16) is big
    del small
    gc.collect()
    assert alive() is not None                                # a captured graph still addresses it
    unpinned_old = weakref.ref(big)
    bigger = c.get(key, _buf, (128,), need=128)               # `big` was never handed out under capture: it is freed
    del big
    gc.collect()
    assert unpinned_old() is None and bigger.numel() == 128
    c.drop(lambda k: k[1] == 1234)                            # the stream is gone: the outgrown pinned buffer goes too
    gc.collect()
    assert alive() is None and key not in c


def test_drop_by_stream_removes_pinned_entries_of_that_stream_only():
    probe = Probe()
    c = Cache(probe, capacity=4)
    probe.on = True
    a = c.get((0, 111, "salad"), _buf)
    b = c.get((0, 222, "salad"), _buf)
    probe.on = False
    c.get((0, 111, "knn"), _buf)
    c.drop(lambda k: k[1] == 111)
    assert (0, 111, "salad") not in c and (0, 111, "knn") not in c and len(c) == 1
    assert c.get((0, 222, "salad"), _buf) is b
    assert c.get((0, 111, "salad"), _buf) is not a


def test_entry_keeps_its_source_tensor_alive_while_cached():
    c = Cache(Probe(), capacity=1)
    src = torch.arange(6.0)
    key = tensor_key(src)
    assert key == ((src.data_ptr(), 0, src.shape, src.device),)
    c.get(key, src.clone, sources=(src,))
    alive = weakref.ref(src)
    del src
    gc.collect()
    assert alive() is not None                                # so its address cannot be recycled under this key
    c.get("next", _buf)                                       # evicted: the entry lets go of the source
    gc.collect()
    assert alive() is None


def test_package_caches_read_the_probe_through_ops_capturing(monkeypatch):
    c = ops.cache(1)
    monkeypatch.setattr(ops, "capturing", lambda: True)
    pinned = c.get("a", _buf)
    monkeypatch.setattr(ops, "capturing", lambda: False)
    c.get("b", _buf)
    c.get("c", _buf)
    assert c.get("a", _buf) is pinned and "b" not in c


def test_drop_stream_caches_reaches_every_stream_keyed_cache(monkeypatch):
    monkeypatch.setattr(ops, "capturing", lambda: True)
    stream = 0x5EED
    for c, key in ((ops._WORKSPACES, (0, stream, "test")), (ops._ZERO_ROWS, (0, stream, 4, 8))):
        c.get(key, _buf)
        assert key in c
    # the one list holds every registry keyed by a stream: _streams' helper streams and fork / join objects included
    assert [id(c) for c in ops._STREAM_KEYED] == [id(c) for c in (ops._WORKSPACES, ops._ZERO_ROWS, _streams._SIDES, _streams._SYNCS)]
    for c in ops._STREAM_KEYED:
        c.get((0, stream, "any"), _buf)
        c.get((0, stream + 1, "any"), _buf)
    ops.drop_stream_caches(stream)
    assert (0, stream, "test") not in ops._WORKSPACES and (0, stream, 4, 8) not in ops._ZERO_ROWS
    for c in ops._STREAM_KEYED:
        assert (0, stream, "any") not in c and (0, stream + 1, "any") in c
    ops.drop_stream_caches(stream + 1)
    assert all(len([k for k in c._entries if k[1] in (stream, stream + 1)]) == 0 for c in ops._STREAM_KEYED)


def test_cumulative_bias_follows_an_in_place_change_of_fc2_bias():
    torch.manual_seed(0)
    m = DinoV2("vit_small", img_size=28)
    for b in m.blocks:
        torch.nn.init.normal_(b.proj.bias)
        torch.nn.init.normal_(b.fc2.bias)
    cpu = torch.device("cpu")
    before = m._cumulative_bias(cpu)
    assert m._cumulative_bias(cpu) is before                  # cached
    expect = torch.stack([t for b in m.blocks for t in (b.proj.bias, b.fc2.bias)]).detach().cumsum(0)
    assert torch.allclose(before, expect, atol=1e-5)
    with torch.no_grad():
        m.blocks[0].fc2.bias.add_(1)
    after = m._cumulative_bias(cpu)
    assert torch.allclose(after[0], before[0]) and torch.allclose(after[1:], before[1:] + 1, atol=1e-5)
    with torch.no_grad():
        m.blocks[0].proj.bias.add_(1)
    assert torch.allclose(m._cumulative_bias(cpu), before + torch.tensor([1.0] + [2.0] * (len(before) - 1))[:, None], atol=1e-5)


# ------------------------------------------------------------------------------- the hand-over between streams, on fakes
class FakeStreams:
    """Stands in for ops._PROBES: a settable current stream and a log of every device action a hand-over enqueues."""
    def __init__(self):
        self.cur, self.log, self.events = "A", [], 0

    def probes(self):
        from vpr_amd._cache import StreamProbes
        return StreamProbes(lambda: self.cur, self._record, lambda e: self.log.append(("wait", e, self.cur)),
                            lambda v: self.log.append(("keep", id(v), self.cur)))

    def _record(self):
        self.events += 1
        self.log.append(("record", self.events, self.cur))
        return self.events


def test_hit_from_the_builders_stream_enqueues_nothing():
    fs = FakeStreams()
    c = Cache(Probe(), capacity=2, probes=fs.probes())
    v = c.get("k", _buf)
    assert fs.log == [("record", 1, "A")]                     # one event, recorded on the building stream after the build
    for _ in range(3):
        assert c.get("k", _buf) is v
    assert fs.log == [("record", 1, "A")]


def test_first_hit_from_another_stream_waits_once_and_later_hits_enqueue_nothing():
    fs = FakeStreams()
    c = Cache(Probe(), probes=fs.probes())
    v = c.get("k", _buf)
    fs.cur = "B"
    assert c.get("k", _buf) is v
    assert fs.log[1:] == [("wait", 1, "B"), ("keep", id(v), "B")]
    for _ in range(3):
        c.get("k", _buf)
    fs.cur = "A"
    c.get("k", _buf)
    assert len(fs.log) == 3                                   # neither B again nor the builder
    fs.cur = "C"                                              # every further stream gets its own single wait, for the same event
    c.get("k", _buf)
    c.get("k", _buf)
    assert fs.log[3:] == [("wait", 1, "C"), ("keep", id(v), "C")]


def test_nothing_is_waited_for_under_capture_and_a_value_built_under_capture_has_no_event():
    fs, probe = FakeStreams(), Probe()
    c = Cache(probe, probes=fs.probes())
    v = c.get("warm", _buf)
    fs.cur, probe.on = "G", True                              # a capturing stream hits what another stream built
    assert c.get("warm", _buf) is v and len(fs.log) == 1      # (the device was synchronised before the capture began)
    g = c.get("in_graph", _buf)                               # built during capture: belongs to the graph, nothing recorded
    assert len(fs.log) == 1
    probe.on = False
    fs.cur = "B"
    assert c.get("in_graph", _buf) is g and len(fs.log) == 1  # nothing to wait for
    fs.cur = "G"                                              # the capture did not count as a hand-over to G: outside it, G waits
    c.get("warm", _buf)
    assert fs.log[1:] == [("wait", 1, "G"), ("keep", id(v), "G")]


def test_drop_and_eviction_forget_the_bookkeeping_with_the_entry():
    fs = FakeStreams()
    c = Cache(Probe(), capacity=1, probes=fs.probes())
    c.get((0, 7, "a"), _buf)
    fs.cur = "B"
    c.get((0, 7, "a"), _buf)
    assert [e[0] for e in fs.log] == ["record", "wait", "keep"]
    c.drop(lambda k: k[1] == 7)
    v = c.get((0, 7, "a"), _buf)                              # rebuilt, now by B: a new event, B is the builder
    assert fs.log[3:] == [("record", 2, "B")]
    c.get((0, 7, "a"), _buf)
    fs.cur = "A"                                              # and the old builder is a borrower like any other
    c.get((0, 7, "a"), _buf)
    assert fs.log[4:] == [("wait", 2, "A"), ("keep", id(v), "A")]
    c.get("other", _buf)                                      # capacity 1: evicts the entry
    assert (0, 7, "a") not in c
    fs.cur = "B"
    w = c.get((0, 7, "a"), _buf)
    assert fs.log[6:] == [("record", 3, "A"), ("record", 4, "B")] and w is not v
    fs.cur = "A"
    c.get((0, 7, "a"), _buf)
    assert fs.log[8:] == [("wait", 4, "A"), ("keep", id(w), "A")]


def test_a_grown_entry_is_a_new_build_with_a_new_event():
    fs = FakeStreams()
    c = Cache(Probe(), probes=fs.probes())
    c.get("ws", _buf, (16,), need=16)
    fs.cur = "B"
    c.get("ws", _buf, (16,), need=8)
    big = c.get("ws", _buf, (64,), need=64)                   # B rebuilds: B's event; A has to wait for it
    fs.cur = "A"
    c.get("ws", _buf, (64,), need=64)
    assert fs.log[3:] == [("record", 2, "B"), ("wait", 2, "A"), ("keep", id(big), "A")]


def test_pinned_entries_behave_as_before_with_stream_probes():
    fs, probe = FakeStreams(), Probe()
    c = Cache(probe, capacity=1, probes=fs.probes())
    first = c.get("warm", _buf)
    fs.cur, probe.on = "G", True
    assert c.get("warm", _buf) is first                       # pinned by the captured hit
    probe.on = False
    c.get("x", _buf)
    c.get("y", _buf)
    assert c.get("warm", _buf) is first and "x" not in c and len(c) == 2
    fs.cur = "B"
    assert c.get("warm", _buf) is first                       # still lent in order after it was pinned
    assert ("wait", 1, "B") in fs.log


def test_no_stream_means_no_event_and_no_wait():
    fs = FakeStreams()
    fs.cur = None                                             # the process has not touched a GPU
    c = Cache(Probe(), probes=fs.probes())
    c.get("k", _buf)
    fs.cur = "B"
    c.get("k", _buf)
    assert fs.log == []


def test_handover_survives_a_deepcopy_as_one_that_remembers_nothing():
    import copy
    from vpr_amd._cache import Handover
    fs = FakeStreams()
    h = Handover(fs.probes(), Probe())
    twin = copy.deepcopy({"order": h})["order"]
    assert h.event == 1 and twin.event is None and twin.stream is None
    fs.cur = "B"
    twin.lend(())
    assert len(fs.log) == 1
    h.lend(())
    assert fs.log[1:] == [("wait", 1, "B"), ("keep", id(()), "B")]


def test_package_caches_and_handovers_touch_no_gpu_in_a_process_without_one():
    if torch.cuda.is_initialized():
        return                                                # (a GPU session that ran GPU tests first: nothing to show here)
    c = ops.cache(1)
    v = c.get("a", _buf)
    assert c._entries["a"][4].stream is None and c.get("a", _buf) is v
    assert ops.handover().event is None and not torch.cuda.is_initialized()


# restype and argtypes of every entry point, taken from the commit before the table was built from shared prefixes
# (P(x) = POINTER(x); c_ulong is what c_size_t names here)
PROTOTYPES_SNAPSHOT = {
    "vpr_status_string": ("c_char_p", "c_int"),
    "vpr_abi_version": ("c_int", ""),
    "vpr_tuning_set": ("c_int", "c_char_p c_int c_int"),
    "vpr_tuning_get": ("c_int", "c_char_p P(c_int)"),
    "vpr_salad_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int c_int c_int c_int"),
    "vpr_salad_aggregate": ("c_int", "c_void_p c_int c_int c_int P(SaladWeightsC) c_float c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_salad_aggregate_split": ("c_int", "c_void_p c_void_p c_int c_int c_int P(SaladWeightsC) c_float c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_salad_stage_token": ("c_int", "c_void_p c_long c_int c_int c_int P(SaladWeightsC) c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_salad_stage_mlps": ("c_int", "c_void_p c_long c_int c_int c_int P(SaladWeightsC) c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_salad_stage_aggregate": ("c_int", "c_int c_int c_int c_float c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_salad_f32_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int c_int c_int c_int"),
    "vpr_salad_pack_w2_fragments": ("c_int", "c_void_p c_int c_int c_void_p c_void_p"),
    "vpr_salad_aggregate_f32": ("c_int", "c_void_p c_long c_void_p c_long c_int c_int c_int P(SaladWeightsF32C) c_float c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_salad_aggregate_train": ("c_int", "c_void_p c_long c_void_p c_long c_int c_int c_int P(SaladWeightsC) c_float c_int c_int c_int c_int c_int c_double c_ulong c_uint c_long c_void_p c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_salad_sinkhorn_aggregate": ("c_int", "c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_float c_int c_void_p c_void_p c_void_p"),
    "vpr_gemm_nt_bf16": ("c_int", "c_void_p c_int c_int c_long c_void_p c_int c_void_p c_int c_void_p c_int c_int c_int c_int c_int c_void_p"),
    "vpr_gemm256_nt_bf16": ("c_int", "c_void_p c_int c_int c_long c_void_p c_int c_void_p c_int c_void_p c_int c_int c_int c_int c_int c_void_p"),
    "vpr_gemm_nt_group_bf16": ("c_int", "P(GemmProblemC) c_int c_void_p"),
    "vpr_knn_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int"),
    "vpr_knn_topk": ("c_int", "c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_knn_topk_fp8": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_knn_topk_checked": ("c_int", "c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_float c_void_p c_void_p c_void_p"),
    "vpr_knn_select_checked": ("c_int", "c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_float c_void_p c_void_p c_void_p"),
    "vpr_knn_topk_fp8_checked": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_float c_void_p c_void_p c_void_p"),
    "vpr_knn_topk_exhaustive": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_quantize_fp8_rows": ("c_int", "c_void_p c_long c_int c_void_p c_void_p c_void_p"),
    "vpr_knn_scores": ("c_int", "c_void_p c_void_p c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_knn_select": ("c_int", "c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "vpr_knn_topk_scores_stage": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_knn_topk_select_stage": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_int c_void_p c_void_p c_void_p c_ulong c_float c_void_p c_void_p c_void_p"),
    "vpr_knn_scores_kernel_name": ("c_char_p", "c_int c_int c_int"),
    "vpr_knn_scores_ptr": ("c_void_p", "c_void_p c_int c_int c_int c_int P(c_int)"),
    "vpr_topk_merge": ("c_int", "c_void_p c_void_p c_int c_int c_int c_void_p c_void_p c_void_p"),
    "vpr_pose_head_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int"),
    "vpr_pose_head": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_ln_meanpool_head": ("c_int", "c_void_p c_int c_int c_int c_int c_void_p c_void_p c_float c_void_p c_void_p c_void_p c_int c_int c_void_p c_void_p"),
    "vpr_preprocess_workspace_bytes": ("c_ulong", "c_int c_int c_int"),
    "vpr_preprocess_resize_normalize": ("c_int", "c_void_p c_int c_int c_int c_int c_int c_void_p c_void_p c_int c_void_p c_void_p c_int P(c_float) P(c_float) c_void_p c_int c_void_p c_void_p c_ulong c_void_p"),
    "vpr_layernorm_bf16": ("c_int", "c_void_p c_void_p c_void_p c_int c_float c_void_p c_long c_int c_void_p"),
    "vpr_bias_layernorm_bf16": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_int c_float c_void_p c_long c_int c_void_p"),
    "vpr_attention_qkv_split_bf16": ("c_int", "c_void_p c_void_p c_int c_int c_int c_long c_int c_int c_float c_void_p"),
    "vpr_skinny_linear_bf16": ("c_int", "c_void_p c_int c_void_p c_int c_void_p c_int c_int c_void_p c_int c_int c_int c_int c_void_p"),
    "vpr_bias_layernorm_cls_linear_bf16": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_float c_void_p c_long c_int c_long c_int c_void_p c_void_p c_int c_void_p c_void_p c_void_p c_int c_void_p c_int c_int c_void_p"),
    "vpr_skinny_linear_stats_bf16": ("c_int", "c_void_p c_int c_void_p c_int c_void_p c_int c_int c_void_p c_int c_int c_int c_int c_void_p c_void_p c_void_p"),
    "vpr_pose_head_pack_w1": ("c_int", "c_void_p c_long c_void_p c_void_p c_void_p"),
    "vpr_pose_head_split_workspace_bytes": ("c_ulong", "c_int c_int c_int"),
    "vpr_pose_head_fused_workspace_bytes": ("c_ulong", "c_int c_int c_int"),
    "vpr_pose_head_fused_counter_bytes": ("c_ulong", "c_int c_int c_int"),
    "vpr_pose_head_pack_w1_frag": ("c_int", "c_void_p c_int c_int c_void_p c_void_p c_void_p"),
    "vpr_pose_head_fused": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_pose_head_split": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_int c_int c_int c_int c_void_p c_ulong c_void_p"),
    "vpr_head_train_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int"),
    "vpr_head_train_state_floats": ("c_long", "c_int c_int c_int"),
    "vpr_head_train_step": ("c_int", "c_void_p c_long c_void_p c_void_p c_long c_int c_int c_int c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_double c_double c_double c_double c_double c_int c_double c_void_p c_void_p c_ulong c_void_p"),
    "vpr_head_train_epoch": ("c_int", "c_void_p c_long c_void_p c_int c_int c_void_p c_long c_int c_int c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_double c_double c_double c_double c_double c_int c_double c_void_p c_void_p c_ulong c_void_p"),
    "vpr_head_train_step_dropout": ("c_int", "c_void_p c_long c_void_p c_void_p c_long c_int c_int c_int c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_double c_double c_double c_double c_double c_int c_double c_void_p c_double c_ulong c_void_p c_void_p c_ulong c_void_p"),
    "vpr_head_train_epoch_dropout": ("c_int", "c_void_p c_long c_void_p c_int c_int c_void_p c_long c_int c_int c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_double c_double c_double c_double c_double c_int c_double c_void_p c_double c_ulong c_void_p c_ulong c_void_p"),
    "vpr_patchify_bf16": ("c_int", "c_void_p c_int c_int c_int c_int c_int c_int c_int c_void_p c_void_p"),
    "vpr_add_layernorm_bf16": ("c_int", "c_void_p c_void_p c_void_p c_void_p c_void_p c_int c_float c_void_p c_long c_int c_void_p"),
    "vpr_attention_qkv_bf16": ("c_int", "c_void_p c_void_p c_int c_int c_int c_int c_float c_void_p"),
    "vpr_f32_to_bf16": ("c_int", "c_void_p c_void_p c_long c_void_p"),
}


def _name(t):
    if hasattr(t, "_type_") and not isinstance(t._type_, str):
        return f"P({t._type_.__name__})"
    return t.__name__


def test_prototypes_equal_the_snapshot():
    assert list(_lib.PROTOTYPES) == list(PROTOTYPES_SNAPSHOT)
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert (_name(restype), " ".join(_name(a) for a in argtypes)) == PROTOTYPES_SNAPSHOT[name], name
