"""Local-feature re-ranking on one MI355X: vpr_local_rerank (match + order kernels) beside the PyTorch form a caller would have
written without it — gather of the candidates' features, bmm, two argmax, an index gather, a masked sum, topk — on the same
GPU (HIP events on torch's stream; needs a GPU).
Usage: python scripts/local_match_bench.py [--N 4096] [--B 64] [--kc 16 32 64] [--n 256] [--l 128] [--k 10] [--iters 100] [--out FILE]

Columns (times in us, medians; the two forms take turns inside one timed loop, after a warm-up of every shape):
  op_us        one ops.local_rerank call on a preallocated workspace, events around the call
  op_chain_us  the raw C call 10 times in one HIP graph, per call: the two kernels without the host between them
  torch_us     the PyTorch form, its gather INSIDE the timed region (it is part of what the caller has to do); bf16 bmm, so
               its similarities are rounded to bf16
  torch_f32_us the same with the operands widened to f32 before the bmm: f32 similarities, as the kernel has them
  GFLOP        2 * B * kc * n * n * l, the MFMA work of the score matrices
  mfma_frac    GFLOP / op_chain_us over the 2.5 PFLOP/s dense bf16 peak
  gather_MB    B * kc * n * l * 2, the scattered candidate features
  gather_frac  gather_MB / op_chain_us over the 8 TB/s HBM peak (the gallery, N * n * l * 2 bytes, is larger than the 256 MB
               Infinity Cache at the default N, and every candidate list is random)
  agree        fraction of (query, position) pairs of the k-lists at which the op and the bf16 PyTorch form name the same image:
               similarities rounded to bf16 are full of ties, so its neighbours among random distractors differ
  agree_f32    the same against the f32 PyTorch form (sums in another order may still swap a near-tie)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12


def events(fns, iters, warmup=10):
    """Median event time (us) of each function, the functions taking turns within one loop."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    for it in range(iters):
        for f, fn in enumerate(fns):
            a, b = evs[f][it]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    out = []
    for per_fn in evs:
        ts = sorted(a.elapsed_time(b) for a, b in per_fn)
        out.append(ts[len(ts) // 2] * 1e3)
    return out


def graph_chain(fns, iters):
    """Per-call time (us) of the calls `fns` captured back to back in one HIP graph (median over `iters` replays)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fns[0]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for fn in fns:
            fn()
    return events([graph.replay], iters)[0] / len(fns)


def torch_local_rerank(q_local, idx, g_local, k, min_sim, widen=False):
    """What a caller writes today: single shard, every index valid, no non-finite features, ties as argmax leaves them.
    widen: the operands widened to f32 before the bmm (f32 similarities, as the kernel has them) instead of a bf16 bmm."""
    g = g_local[idx.long()]                                           # [B, kc, n_g, l]: the materialised gather
    if widen:
        S = torch.matmul(q_local.float()[:, None], g.float().transpose(2, 3))
    else:
        S = torch.matmul(q_local[:, None], g.transpose(2, 3)).float() # [B, kc, n_q, n_g]
    r = S.argmax(3)                                                   # [B, kc, n_q]
    cv, c = S.max(2)                                                  # [B, kc, n_g]
    mutual = r.gather(2, c) == torch.arange(S.shape[3], device=S.device)
    m = mutual & (cv >= min_sim)
    score = torch.where(m, cv, torch.zeros_like(cv)).sum(2)
    v, o = score.topk(k, dim=1)
    return v, idx.gather(1, o), m.sum(2).gather(1, o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--kc", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--l", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--min-sim", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("local_match_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, device=dev, generator=g), dim=-1).to(torch.bfloat16)
    g_local = torch.cat([unit(min(512, a.N - lo), a.n, a.l) for lo in range(0, a.N, 512)])
    q_local = unit(a.B, a.n, a.l)
    lines = [f"# local_match_bench: library {os.path.basename(_lib.library_path())}, B {a.B}, N {a.N}, n {a.n}, l {a.l}, k {a.k}, "
             f"min_sim {a.min_sim}, iters {a.iters}; gallery {a.N * a.n * a.l * 2 / 1e6:.0f} MB",
             "%4s %10s %12s %10s %13s %9s %8s %10s %10s %12s %7s %10s" % ("kc", "op_us", "op_chain_us", "torch_us", "torch_f32_us", "torch/op",
                                                                            "GFLOP", "mfma_frac", "gather_MB", "gather_frac", "agree", "agree_f32")]
    for kc in a.kc:
        k = min(a.k, kc)
        idx = torch.randint(0, a.N, (a.B, kc), device=dev, generator=g, dtype=torch.int32)
        idx[:, 0] = torch.arange(a.B, device=dev, dtype=torch.int32)         # one candidate per query shares its patches
        g_local[:a.B] = q_local[:, torch.randperm(a.n, device=dev, generator=g)]
        ws = torch.empty(_lib.lib().vpr_local_workspace_bytes(a.B, kc), dtype=torch.uint8, device=dev)
        vals = torch.empty((a.B, k), dtype=torch.float32, device=dev)
        out = torch.empty((a.B, k), dtype=torch.int32, device=dev)
        mt = torch.empty((a.B, k), dtype=torch.int32, device=dev)
        null = ops._ptr(None)
        raw = lambda: ops._call("vpr_local_rerank", ops._ptr(q_local), a.n, ops._ptr(idx), a.B, kc, ops._ptr(g_local), a.n, a.l, a.N, 0,
                                a.min_sim, k, ops._ptr(vals), ops._ptr(out), ops._ptr(mt), null, null, null, null, ops._ptr(ws),
                                ws.numel(), ops._stream())
        hip = lambda: ops.local_rerank(q_local, idx, g_local, 0, k, a.min_sim, ws)
        ref = lambda: torch_local_rerank(q_local, idx, g_local, k, a.min_sim)
        ref32 = lambda: torch_local_rerank(q_local, idx, g_local, k, a.min_sim, True)
        agree = float((hip()[1] == ref()[1]).float().mean())
        agree32 = float((hip()[1] == ref32()[1]).float().mean())
        assert bool((hip()[1][:, 0] == idx[:, 0]).all())                      # the planted image comes back first
        op_us, torch_us, torch32_us = events([hip, ref, ref32], a.iters)
        chain = graph_chain([raw] * 10, a.iters)
        flop, gather = 2.0 * a.B * kc * a.n * a.n * a.l, a.B * kc * a.n * a.l * 2.0
        lines.append("%4d %10.1f %12.1f %10.1f %13.1f %9.2f %8.2f %10.4f %10.1f %12.4f %7.4f %10.4f" % (
            kc, op_us, chain, torch_us, torch32_us, torch_us / op_us, flop / 1e9, flop / (chain * 1e-6) / MFMA_PEAK, gather / 1e6,
            gather / (chain * 1e-6) / HBM_PEAK, agree, agree32))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
