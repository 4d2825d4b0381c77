"""Retrieval pose and first-hit ranks from a merged top-k: vpr_retrieval_pose (one launch, device) beside the host path it
replaces on the same inputs (gallery.label_transfer + positives_by_distance + positives_by_region, numpy, including the
device-to-host copy of the two top-k tensors).  Default shape B = 64, k = 10, N = 100 000.  Prints one JSON line:
  op_us           torch.ops.vpr.retrieval_pose per call, HIP events over back-to-back eager calls (launch-bound)
  graph_kernel_us the same launch inside a HIP graph of `--chain` consecutive calls, per call (kernel + graph node gap)
  host_ms         the host functions, wall clock, median of `--host-reps` runs
and checks that both paths agree (hits and recalls exactly, pose to 1e-9 relative)."""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpr_amd import gallery as G, postproc, torch_ops  # noqa: F401,E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--mode", default="weighted")
ap.add_argument("--tau", type=float, default=25.0)
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--chain", type=int, default=200)
ap.add_argument("--host-reps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
B, k, N = a.batch, a.k, a.rows

rng = np.random.default_rng(0)
labels = np.stack([postproc.CAMPUS_MEAN[0] + rng.normal(0, postproc.CAMPUS_SCALE[0], N),
                   postproc.CAMPUS_MEAN[1] + rng.normal(0, postproc.CAMPUS_SCALE[1], N),
                   rng.uniform(0, 360, N), rng.integers(0, 40, N).astype(np.float64)], 1)
idx_np = np.stack([rng.choice(N, k, replace=False) for _ in range(B)]).astype(np.int32)
vals_np = np.sort(rng.uniform(0.3, 0.9, (B, k)).astype(np.float32), axis=1)[:, ::-1].copy()
q_np = np.concatenate([labels[idx_np[:, 0], :2] + rng.normal(0, a.tau, (B, 2)), labels[idx_np[:, k // 2], 3:4]], 1)
vals, idx = torch.from_numpy(vals_np).to(dev), torch.from_numpy(idx_np).to(dev)
labels_dev, q = G.device_labels(labels, dev), torch.from_numpy(q_np).to(dev)
scaler = [*postproc.CAMPUS_MEAN, *postproc.CAMPUS_SCALE]


def op():
    return torch.ops.vpr.retrieval_pose(vals, idx, labels_dev, a.mode, 0.01, q, a.tau, scaler)


def events_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for _ in range(20):
    out = op()
torch.cuda.synchronize()
op_us = min(events_us(op, a.calls) for _ in range(3))

side = torch.cuda.Stream(device=dev)
side.wait_stream(torch.cuda.current_stream())
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, stream=side):
    for _ in range(a.chain):
        op()
for _ in range(3):
    graph.replay()
torch.cuda.synchronize()
graph_kernel_us = min(events_us(graph.replay, 20) for _ in range(3)) / a.chain


def host():
    pose = G.label_transfer(vals, idx, labels, a.mode, 0.01)
    top = idx.cpu().numpy()
    pos_d = G.positives_by_distance(q_np[:, :2], labels[:, :2], a.tau)
    pos_r = G.positives_by_region(q_np[:, 2], labels[:, 3])
    return pose, [postproc.recall_at_k(top[:, :j], p) for p in (pos_d, pos_r) for j in (1, k)]


host()
times = []
for _ in range(a.host_reps):
    t0 = time.perf_counter()
    pose_h, recalls_h = host()
    times.append((time.perf_counter() - t0) * 1e3)

pose_d, _, ht, hr = (t.cpu().numpy() for t in out)
recalls_d = [postproc.recall_from_first_hit(h, j) for h in (ht, hr) for j in (1, k)]
assert recalls_d == recalls_h, (recalls_d, recalls_h)
d = np.abs(pose_d - pose_h)
d[:, 2] = np.minimum(d[:, 2], 360.0 - d[:, 2])
assert (d <= 1e-9 * np.maximum(np.abs(pose_h), 1.0)).all(), d.max()
print(json.dumps({"shape": {"B": B, "k": k, "N": N, "mode": a.mode}, "op_us": round(op_us, 2),
                  "graph_kernel_us": round(graph_kernel_us, 3), "host_ms": round(statistics.median(times), 2),
                  "host_ms_min": round(min(times), 2), "recalls": recalls_d}))
