"""CPU: the retrieval-pose extension of the C ABI (include/vpr_amd_retrieval.h) — header and binding table agree, bad
arguments are refused before a device is touched, the torch op has a fake implementation, the wrapper refuses what it
cannot take, recall_from_first_hit equals recall_at_k, and retrieval_metrics' default path gives today's numbers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import vpr_amd
    vpr_amd.build_library()
    from vpr_amd import _lib
    return _lib.lib()


def test_extension_header_and_table_agree(lib):
    from vpr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vpr_amd_retrieval.h")).read()
    assert re.search(r"additive\s+(\*\s+)?extension\s+(\*\s+)?of\s+(\*\s+)?ABI 6", header, flags=re.I) and "present iff" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vpr_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_lib.EXTENSION_PROTOTYPES) == {"vpr_retrieval_pose"}
    assert not set(_lib.EXTENSION_PROTOTYPES) & set(_lib.PROTOTYPES)
    for name, (restype, argtypes) in _lib.EXTENSION_PROTOTYPES.items():
        fn = getattr(lib, name)                              # exported by the built library, bound by _lib.lib()
        assert fn.restype == restype and fn.argtypes == argtypes
    for const, value in (("VPR_POSE_TOP1", _lib.POSE_TOP1), ("VPR_POSE_WEIGHTED", _lib.POSE_WEIGHTED)):
        assert re.search(rf"#define {const} {value}\b", code)
    # the parameter count of the declaration is the binding's
    params = re.search(r"vpr_retrieval_pose\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(params.split(",")) == len(_lib.EXTENSION_PROTOTYPES["vpr_retrieval_pose"][1]) == 16
    assert lib.vpr_abi_version() == _lib.ABI_VERSION == 6    # an additive extension: the version does not move


def test_invalid_arguments_are_rejected_without_a_device(lib):
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd = ctypes.c_void_p(p.value + 4)                       # 4-byte aligned only
    scaler = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    base = (ctypes.addressof(buf) + 2048 + 7) // 8 * 8         # four good doubles at an address that is 4 mod 8
    ctypes.memmove(base + 4, ctypes.addressof(scaler), 32)
    odd_scaler = ctypes.c_void_p(base + 4)
    nan, inf = float("nan"), float("inf")

    def call(vals=p, idx=p, B=1, k=5, labels=p, n=10, mode=0, temp=0.01, q=null, tau=0.0, sc=None, p64=p, p4=p, ht=p, hr=p):
        return lib.vpr_retrieval_pose(vals, idx, B, k, labels, n, mode, temp, q, tau, sc, p64, p4, ht, hr, null)

    INVALID, UNSUPPORTED = -1, -2
    for kw in (dict(vals=null), dict(idx=null), dict(labels=null), dict(B=-1), dict(n=0), dict(n=-5), dict(mode=2), dict(mode=-1),
               dict(mode=1, temp=0.0), dict(mode=1, temp=-0.01), dict(mode=1, temp=nan),
               dict(q=p, tau=-1.0), dict(q=p, tau=nan),
               dict(sc=(ctypes.c_double * 4)(0.0, 0.0, 0.0, 1.0)), dict(sc=(ctypes.c_double * 4)(0.0, 0.0, 1.0, -2.0)),
               dict(sc=(ctypes.c_double * 4)(0.0, 0.0, nan, 1.0))):
        assert call(**kw) == INVALID, kw
    for kw in (dict(k=0), dict(k=65), dict(k=-3), dict(labels=odd), dict(q=odd), dict(p64=odd),
               dict(sc=odd_scaler)):
        assert call(**kw) == UNSUPPORTED, kw
    # what the rules leave alone: top-1 ignores the temperature, tau is not looked at without q_targets, B = 0 launches nothing
    assert call(B=0) == 0
    assert call(B=0, mode=0, temp=nan, tau=-1.0, sc=scaler, p64=null, p4=null, ht=null, hr=null) == 0
    assert call(B=0, mode=1, temp=inf, q=p, tau=inf, k=64) == 0
    assert call(B=0, k=1, n=1 << 40) == 0


def test_fake_op_gives_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vpr_amd import torch_ops
    assert "retrieval_pose" in torch_ops.OPS
    schema = str(torch.ops.vpr.retrieval_pose.default._schema)
    assert schema.startswith("vpr::retrieval_pose(") and "Tensor? q_targets" in schema and "float[]? scaler" in schema
    with FakeTensorMode():
        mk = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
        v, i, lab = mk(37, 10, dtype=torch.float32), mk(37, 10, dtype=torch.int32), mk(1000, 4, dtype=torch.float64)
        for args in ((), ("weighted", 0.05, mk(37, 3, dtype=torch.float64), 25.0, [1.0, 2.0, 3.0, 4.0])):
            p64, p4, ht, hr = torch.ops.vpr.retrieval_pose(v, i, lab, *args)
            assert p64.shape == (37, 3) and p64.dtype == torch.float64 and p64.device.type == "cuda"
            assert p4.shape == (37, 4) and p4.dtype == torch.float32
            assert ht.shape == hr.shape == (37,) and ht.dtype == hr.dtype == torch.int32


def test_wrapper_refuses_cpu_tensors_and_wrong_dtypes(monkeypatch):
    from vpr_amd import ops
    v, i, lab = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.retrieval_pose(v, i, lab)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.vpr.retrieval_pose(v, i, lab)
    # the remaining checks, with the device test answered "yes": nothing below reaches the library
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail("the library must not be called"))
    for bad, match in (((v.double(), i, lab), "vals: expected dtype"), ((v, i.long(), lab), "idx: expected dtype"),
                       ((v, i, lab.float()), "labels_dev: expected dtype"), ((v, i[:, :2], lab), "contiguous"),
                       ((v, i[:1], lab), "shapes differ"), ((v[0], i[0], lab), "expected 2 dims"),
                       ((v, i, torch.zeros(5, 3, dtype=torch.float64)), r"\[N, 4\]")):
        with pytest.raises(RuntimeError, match=match):
            ops.retrieval_pose(*bad)
    with pytest.raises(RuntimeError, match="mode"):
        ops.retrieval_pose(v, i, lab, mode="vote")
    with pytest.raises(RuntimeError, match="q_targets: expected dtype"):
        ops.retrieval_pose(v, i, lab, q_targets=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match=r"\[B, 3\]"):
        ops.retrieval_pose(v, i, lab, q_targets=torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="scaler"):
        ops.retrieval_pose(v, i, lab, scaler=[0.0, 0.0, 1.0])


def test_recall_from_first_hit_equals_recall_at_k():
    from vpr_amd import postproc
    rng = np.random.default_rng(5)
    Q, N, k = 41, 60, 10
    for pad in (False, True):
        top = np.stack([rng.permutation(N)[:k] for _ in range(Q)]).astype(np.int32)
        if pad:
            for q in range(Q):
                top[q, rng.integers(0, k + 1):] = -1            # a padded tail, down to an empty list
        positives = [rng.choice(N, size=rng.integers(0, 6), replace=False) for _ in range(Q)]
        hit = np.full(Q, -1, dtype=np.int32)
        for q in range(Q):
            at = [j for j in range(k) if top[q, j] >= 0 and top[q, j] in set(positives[q].tolist())]
            hit[q] = at[0] if at else -1
        seen = set()
        for j in range(1, k + 1):
            r = postproc.recall_from_first_hit(hit, j)
            assert r == postproc.recall_at_k(top[:, :j], positives), (pad, j)
            seen.add(r)
        assert len(seen) > 3                                    # the recalls move with j: the case is not degenerate
    assert postproc.recall_from_first_hit(np.zeros(0, dtype=np.int32), 3) == postproc.recall_at_k(np.zeros((0, 3)), []) == 0.0


def test_retrieval_metrics_default_path_is_todays_code():
    """retrieval_metrics(on_device=False) against the metric block of calculate_retrieval_scores as it stood before the
    function was factored out, restated here line for line, on a seeded case (CPU tensors: the host path needs no GPU)."""
    from vpr_amd import evaluate, gallery as G, postproc
    rng = np.random.default_rng(11)
    Q, N, k, tau = 29, 200, 5, 30.0
    labels = np.stack([219658.0 + rng.normal(0, 60, N), 143506.0 + rng.normal(0, 60, N), rng.uniform(0, 360, N),
                       rng.integers(0, 6, N).astype(np.float64)], 1)
    idx = torch.from_numpy(np.stack([rng.permutation(N)[:k] for _ in range(Q)]).astype(np.int32))
    vals = torch.from_numpy(np.sort(rng.uniform(0.2, 0.9, (Q, k)).astype(np.float32), axis=1)[:, ::-1].copy())
    idx[3, 3:] = -1
    vals[3, 3:] = float("-inf")
    targets = labels[idx[:, 0].numpy(), :2] + rng.normal(0, 25, (Q, 2))
    regions, angles = rng.integers(0, 6, Q), rng.uniform(0, 360, Q)
    for mode in ("top1", "weighted"):
        got = evaluate.retrieval_metrics(vals, idx, labels, targets, regions, angles, tau, mode)
        pose = G.label_transfer(vals, idx, labels, mode=mode)
        top = idx.cpu().numpy()
        pos_d = G.positives_by_distance(targets, labels[:, :2], tau)
        pos_r = G.positives_by_region(regions, labels[:, 3])
        want = {"topk_scores": vals.cpu().numpy(), "topk_indices": top, "pose": pose,
                "final_loss": postproc.final_loss(pose[:, :2], targets),
                "maae": postproc.mean_absolute_angular_error(pose[:, 2], angles),
                "recall_at_1_tau": postproc.recall_at_k(top[:, :1], pos_d), f"recall_at_{k}_tau": postproc.recall_at_k(top, pos_d),
                "recall_at_1_region": postproc.recall_at_k(top[:, :1], pos_r)}
        assert list(got) == list(want)
        for key, w in want.items():
            if isinstance(w, np.ndarray):
                assert got[key].dtype == w.dtype and got[key].tobytes() == w.tobytes(), key
            else:
                assert got[key] == w, key
        assert 0.0 < got["recall_at_1_tau"] < 1.0 and got["recall_at_1_tau"] <= got[f"recall_at_{k}_tau"]


def test_gallery_shard_carries_the_device_label_table_when_asked(tmp_path):
    from vpr_amd import gallery as G
    rng = np.random.default_rng(3)
    n = 12
    labels = np.stack([rng.normal(2e5, 900, n), rng.normal(1.4e5, 1100, n), rng.uniform(0, 360, n), rng.integers(0, 4, n)], 1)
    G.save_gallery(str(tmp_path), torch.randn(n, 64).to(torch.bfloat16), labels)
    cpu = torch.device("cpu")
    plain = G.load_gallery_shard(str(tmp_path), cpu)
    assert plain.labels_dev is None and plain.dtype == "bf16"
    for rank in (0, 1):
        shard = G.load_gallery_shard(str(tmp_path), cpu, rank, 2, device_labels=True)
        assert shard.rows.shape[0] == n // 2                                    # the rows are sharded, the table is whole
        assert shard.labels_dev.dtype == torch.float64 and tuple(shard.labels_dev.shape) == (n, 4)
        assert shard.labels_dev.is_contiguous() and shard.labels_dev.numpy().tobytes() == labels.tobytes()
    t = G.device_labels(labels[:, ::-1][:, ::-1].astype(np.float32), cpu)      # any float array in, contiguous f64 out
    assert t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == (n, 4)
    with pytest.raises(ValueError, match="labels must be"):
        G.device_labels(labels[:, :3], cpu)
    assert G.GalleryShard(plain.rows, None, labels, n, 0, "bf16").labels_dev is None      # the new field is last and optional


def test_scaler_and_label_arguments_of_the_python_layers():
    from vpr_amd import postproc
    from vpr_amd.pipeline import StepOutput
    from vpr_amd.retrieval import pose_labels, pose_scaler
    assert pose_scaler(None) is None
    assert pose_scaler(postproc.LatLonScaler.campus()) == [*postproc.CAMPUS_MEAN, *postproc.CAMPUS_SCALE]
    assert pose_scaler((1, 2, 3, 4)) == [1.0, 2.0, 3.0, 4.0]
    labels = np.arange(8, dtype=np.float32).reshape(2, 4)
    t = pose_labels(labels, torch.device("cpu"))
    assert t.dtype == torch.float64 and t.tolist() == labels.tolist()
    same = torch.zeros(3, 4, dtype=torch.float64)
    assert pose_labels(same, torch.device("cpu")).data_ptr() == same.data_ptr()          # a device table is taken as it is
    out = StepOutput(*(torch.zeros(1) for _ in range(4)))
    assert out.retrieval_pose is None                                                   # four positional fields, as before
