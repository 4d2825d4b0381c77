"""GPU: bench.py honours its contract (one JSON line, required keys) on a reduced workload, for
one rank and for two ranks rehearsed on the same GPU over gloo (the N>1 code path: query
all-gather, shard search with global indices, top-k all-gather, on-device merge)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--arch", "vit_small", "--gallery", "3000", "--batch", "8", "--no-tune",
         "--fp8-rows", "20000"]
REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"}


def _json_line(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_single_rank_contract(dev):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full"] + SMALL,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _json_line(p.stdout)
    assert REQUIRED <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["value"] - 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "images" in c["sample"]
    c1 = c["config1_swin_tiny"]                               # BASELINE config 1: the reference's CPU-runnable case
    assert c1["cpu_images_per_s"] > 0 and c1["gpu_images_per_s"] > c1["cpu_images_per_s"]
    assert d["recall_at_1"] == 1.0 and "workload" in d["config"]
    # 3000-row shard: the K-split form of the score stage, timed between the two stages of the call; no PMC traffic for it
    assert r["kernel"] == "vpr::knn_scores_kernel<false, 208, 2, 4>" and r["traffic"] is None and r["kernel_ms"] > 0
    assert d["uncertified_queries"] == 0
    rows = d["kernels"]                                       # per-kernel roofline rows (configs 2, 4, 5)
    assert {"salad_aggregate", "pose_head", "ln_meanpool_head_T49", "ln_meanpool_head_T144", "knn_topk_bf16",
            "knn_topk_bf16_graph_replay", "knn_topk_fp8", "retrieval_fp8_graph_replay"} <= set(rows)
    for name, row in rows.items():
        assert row["ms"] > 0 and 0 < row["frac"] < 1.0 and abs(row["frac"] - row["achieved"] / row["peak"]) < 1e-12, name
    assert rows["salad_aggregate"]["bound"] == "mfma" and rows["knn_topk_fp8"]["uncertified_queries"] == 0


def test_bench_plain_run_times_the_steps_and_dumps_what_they_computed(dev, tmp_path):
    """Without --full the line holds the headline and the roofline read from the timed steps' events, nothing measured
    after them; --dump-outputs writes the last timed step's StepOutput.  The same arguments with --full (whose extra
    work all comes after the timed region) dump the same arrays: same seeded inputs, same timed path."""
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-kernel-rows"])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(tmp_path / mode)]
                           + extra + SMALL, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        if mode == "plain":
            d = _json_line(p.stdout)
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"} <= set(d)
    assert not {"recall_at_1", "uncertified_queries", "stages", "dist", "kernels", "cpu_baseline"} & set(d)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["roofline"]["kernel_ms"] > 0
    assert abs(d["value"] - 8 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    load = lambda mode, name: np.load(tmp_path / mode / f"{name}.npy")
    assert sorted(os.listdir(tmp_path / "plain")) == ["descriptors.npy", "pose.npy", "topk_indices.npy", "topk_scores.npy"]
    desc, scores, idx, pose = (load("plain", n) for n in ("descriptors", "topk_scores", "topk_indices", "pose"))
    assert desc.shape == (8, 8448) and desc.dtype == np.float32 and np.isfinite(desc).all()
    assert scores.shape == idx.shape == (8, 10) and idx.dtype == np.float64 and (np.diff(scores, axis=1) <= 0).all()
    assert ((idx >= 0) & (idx < 3000) & (idx == np.round(idx))).all()
    assert pose.shape == (8, 4) and np.allclose(pose[:, 2] ** 2 + pose[:, 3] ** 2, 1.0, atol=1e-5)   # unit (sin, cos)
    for name in ("descriptors", "topk_scores", "pose"):
        np.testing.assert_allclose(load("full", name), load("plain", name), rtol=1e-5, atol=1e-6, err_msg=name)
    np.testing.assert_array_equal(load("full", "topk_indices"), idx)


def test_bench_force_dist_runs_the_collectives_on_rccl(dev):
    """--force-dist: one rank, but a real RCCL process group and both all-gathers + the merge inside every step."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--force-dist", "--no-cpu-baseline",
                        "--no-kernel-rows"] + SMALL, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json_line(p.stdout)
    assert p.stdout.strip().startswith("{") and len(p.stdout.strip().splitlines()) == 1      # RCCL's banner kept off stdout
    # bare `python bench.py --gpus 1 --force-dist` (no launcher in the environment) took the self-spawn path: the
    # script started its rank under torch.distributed.run before touching the GPU and forwarded rank 0's line
    assert "spawning 1 rank(s)" in p.stderr
    assert d["dist"]["process_group"] == "nccl" and d["dist"]["collectives_in_step"] is True
    assert d["dist"]["ranks_seen"] == 1 and d["dist"]["collective_ms_per_step"] > 0       # RCCL group size, exchange steps alone
    assert "merge" in d["recall_path"]
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["recall_at_1"] == 1.0 and d["uncertified_queries"] == 0
    # two batches in flight on two streams, each step with its collectives on the one process group
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--force-dist", "--no-cpu-baseline",
                        "--no-kernel-rows", "--in-flight", "2"] + SMALL + ["--steps", "6"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env=dict(env, MASTER_PORT=str(port + 1)))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json_line(p.stdout)
    assert d["config"]["batches_in_flight"] == 2 and d["dist"]["collectives_in_step"] and d["recall_at_1"] == 1.0


def test_bench_config5_flags_graph_retrieval_with_collectives(dev):
    """BASELINE config 5 as the driver (or anyone with an 8-GPU node) would launch it, on the one rank available here:
    e4m3 gallery, the retrieval leg of every step replayed from ONE HIP graph that holds both RCCL all-gathers, the
    query quantisation, the shard search and the merge."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--force-dist", "--knn-dtype", "fp8",
                        "--graph-retrieval", "--no-cpu-baseline", "--no-kernel-rows"] + SMALL,
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json_line(p.stdout)
    assert d["config"]["graph_retrieval"] is True and d["dist"]["collectives_in_step"] and "fp8" in d["dtype"]
    assert "hipGraph replay" in d["roofline"]["kernel"] and "all-gathers" in d["roofline"]["kernel"] and d["roofline"]["kernel_ms"] > 0
    assert d["value"] > 0 and d["recall_at_1"] == 1.0 and d["uncertified_queries"] == 0


def test_bench_fp8_gallery(dev):
    """--knn-dtype fp8: e4m3 shard + per-row scales through the same pipeline; planted neighbours still found."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--knn-dtype", "fp8",
                        "--no-cpu-baseline"] + SMALL, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _json_line(p.stdout)
    assert REQUIRED <= set(d) and "fp8" in d["dtype"] and "fp8 kNN" in d["config"]["workload"]
    assert d["roofline"]["algorithmic_bytes"] == 3000 * 8448 + 8 * 8448 + 8 * 10 * 8
    assert d["value"] > 0 and d["recall_at_1"] == 1.0


def test_bench_two_batches_in_flight(dev):
    """--in-flight 2: consecutive steps on two streams (per-stream workspaces, per-stream side chain)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--in-flight", "2",
                        "--no-cpu-baseline"] + SMALL + ["--steps", "4"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = _json_line(p.stdout)
    assert d["config"]["batches_in_flight"] == 2 and d["steps"] == 4 and d["value"] > 0 and d["recall_at_1"] == 1.0


def test_bench_four_ranks_gloo_rehearsal(dev):
    """Four ranks on the one GPU (gloo), bare launch: four gallery shards (uneven: 3001 rows), 32 gathered queries per
    shard scan, Recall@1 through the 4-way merge with positives in every shard, counters summed over the group."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--full", "--backend", "gloo", "--no-cpu-baseline",
           "--no-kernel-rows", "--steps", "2", "--warmup", "1", "--arch", "vit_small", "--gallery", "3001", "--batch", "8", "--no-tune"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json_line(p.stdout)
    assert d["n_gpus"] == 4 and d["config"]["global_batch"] == 32 and d["config"]["parallelism"] == "dp4+gallery-shard4"
    assert d["recall_at_1"] == 1.0 and d["dist"]["ranks_seen"] == 4 and d["uncertified_queries"] == 0
    assert d["roofline"]["kernel_ms"] > 0


@pytest.mark.parametrize("launcher", ["torchrun", "self-spawn"])
def test_bench_two_ranks_gloo_rehearsal(dev, launcher):
    """Two ranks sharing the one GPU over gloo, launched the way the driver does (torch.distributed.run) and bare
    (`python bench.py --gpus 2`: the script spawns its ranks itself).  Recall@1 is computed THROUGH the sharded path: each
    rank plants its queries next to rows of its own shard, every query is searched on both shards, the per-shard top-k
    are all-gathered and merged — 1.0 means the merge picked the right shard's answer for the queries of both ranks."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--backend", "gloo", "--no-cpu-baseline"] + SMALL
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + tail
    else:
        cmd = [sys.executable] + tail
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json_line(p.stdout)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2+gallery-shard2"
    assert d["value"] > 0 and d["recall_at_1"] == 1.0 and d["cpu_baseline"] is None
    assert d["dist"]["ranks_seen"] == 2 and d["dist"]["collective_ms_per_step"] > 0 and "merge" in d["recall_path"]
    assert d["uncertified_queries"] == 0                        # summed over both shards
