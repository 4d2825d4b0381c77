"""Two-tier retrieval on one MI355X: the re-rank op (vpr_rerank_rows: score + order kernels), the PyTorch gather + bmm a caller
would have written without it, and e4m3 scan + re-rank against the bf16 scan of the same gallery (HIP events on torch's stream;
needs a GPU).
Usage: python scripts/rerank_bench.py [--N 100000] [--B 64] [--kc 64] [--k 10] [--iters 200] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/rerank_bench.py --trace
           (a run of its own: the op 200 times, each on its own random candidate rows, nothing timed)
       python scripts/rerank_bench.py --trace-summary OUT      (per-kernel medians of that trace; no GPU needed)

Numbers (bf16 fine rows; times in us):
  op_us            median over `iters` single ops.rerank_rows calls on fixed buffers, events around each call: two launches and
                   the host between them, an upper bound of the kernels
  op_chain_us      the op 20 times in one HIP graph on the SAME candidates, per op: rows from cache
  op_cold_us       a graph of 40 ops, each on its own random candidate rows (40 x row_bytes = 2.8 GB at the defaults, more than
                   the 256 MB Infinity Cache), per op: rows from HBM, as after a coarse search that has just streamed its gallery
  order_chain_us   the op with every candidate foreign (index_base past them all), per op in a graph of 20: the score
                   workgroups end at their first test, so this is the order kernel plus two launch boundaries
  row_bytes        B * kc * D * 2: the scattered row reads, the traffic the score kernel exists for
  row_GBps_cold    row_bytes / (op_cold_us - order_chain_us): the achieved scattered-read rate of the score kernel, beside the
                   4-5 TB/s DESIGN §9 quotes for knn_final_fused_kernel; hbm_fraction = that over the 8 TB/s peak
  torch_f32_us / torch_bf16_us   the comparison: rows[idx] -> bmm with the query (operands widened to f32 / left in bf16) -> topk,
                   gather of the indices; events, median; every index valid, single shard — the easy case for it
  coarse_us / coarse_kc_us / two_tier_us / bf16_us   ShardedGallery.search on the e4m3 gallery for k and for kc, .search_reranked
                   on it (kc candidates -> k), and .search for k on the bf16 gallery of the same rows; events, median
  top1_agree_*     fraction of the queries whose top-1 equals that of the bf16 scan: e4m3 scan alone, and after the re-rank
The HIP and PyTorch forms are timed alternately in one loop, and their index lists are compared before timing."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


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


def host_clock(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def torch_rerank(q, idx, rows, k, widen):
    """What a caller writes today: single shard, every index valid, no defined order of the sum."""
    g = rows[idx.long()]                                              # [B, kc, D]: the materialised gather
    s = torch.bmm(g.float(), q.float()[:, :, None]) if widen else torch.bmm(g, q[:, :, None]).float()
    v, o = s.squeeze(2).topk(k, dim=1)
    return v, idx.gather(1, o)


def trace_summary(directory):
    """Median duration per kernel name of a rocprofv3 --kernel-trace CSV (the op's two kernels alternate, so by name)."""
    f = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)[0]
    by = {}
    for r in csv.DictReader(open(f)):
        by.setdefault(r["Kernel_Name"][:90], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, d in sorted(by.items()):
        if "rerank" in name:
            d.sort()
            print("%-92s n=%4d median %8.1f us  p10 %8.1f  p90 %8.1f" % (name, len(d), d[len(d) // 2], d[len(d) // 10], d[len(d) * 9 // 10]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--D", type=int, default=8448)
    ap.add_argument("--kc", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true", help="only launch the op 200 times on cold rows (for a kernel trace)")
    ap.add_argument("--trace-summary", default="", help="print per-kernel medians of a kernel-trace directory and exit")
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    if not torch.cuda.is_available():
        sys.exit("rerank_bench: needs a GPU (there is nothing to measure without one)")
    if a.N < 12:
        sys.exit("rerank_bench: N must hold at least one group of 12 rows")
    from vpr_amd import _lib, ops
    from vpr_amd.retrieval import ShardedGallery
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    fine = torch.empty((a.N, a.D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, a.N, 20000):                  # groups of 12 near-duplicates: consecutive video frames
        n = min(20000, a.N - lo)
        c = torch.nn.functional.normalize(torch.randn((n + 11) // 12, a.D, device=dev, generator=g), dim=1).repeat_interleave(12, 0)[:n]
        fine[lo:lo + n] = torch.nn.functional.normalize(c + 0.45 * torch.randn(n, a.D, device=dev, generator=g) / a.D ** 0.5, dim=1).to(torch.bfloat16)
    # a query = the mean of one whole group, so its 12 rows score almost alike and the e4m3 order among them is unreliable
    blocks = a.N // 20000                            # 1666 whole groups in every full block of 20000 rows
    first = torch.randint(0, blocks * 1666 if blocks else max(a.N // 12, 1), (a.B,), device=dev, generator=g)
    first = first // 1666 * 20000 + first % 1666 * 12 if blocks else first * 12
    assert int(first.max()) + 12 <= a.N
    q = torch.nn.functional.normalize(fine[first[:, None] + torch.arange(12, device=dev)].float().mean(1), dim=1).to(torch.bfloat16)
    ws = torch.empty(_lib.lib().vpr_rerank_workspace_bytes(a.B, a.kc), dtype=torch.uint8, device=dev)
    vals = torch.empty((a.B, a.k), dtype=torch.float32, device=dev)
    out = torch.empty((a.B, a.k), dtype=torch.int32, device=dev)
    raw = lambda i, base=0: ops._call("vpr_rerank_rows", ops._ptr(q), 0, ops._ptr(i), a.B, a.D, a.kc, ops._ptr(fine), 0, a.N, base,
                                      a.k, ops._ptr(vals), ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream())
    cold_sets = [torch.randint(0, a.N, (a.B, a.kc), device=dev, generator=g, dtype=torch.int32) for _ in range(40)]
    if a.trace:
        for it in range(200):
            raw(cold_sets[it % 40])
        torch.cuda.synchronize()
        return
    res = {"library": os.path.basename(_lib.library_path()), "B": a.B, "N": a.N, "D": a.D, "kc": a.kc, "k": a.k, "iters": a.iters}
    g8 = torch.empty((a.N, a.D), dtype=torch.uint8, device=dev)
    gs = torch.empty((a.N,), dtype=torch.float32, device=dev)
    for lo in range(0, a.N, 20000):
        g8[lo:lo + 20000], gs[lo:lo + 20000] = ops.quantize_fp8_rows(fine[lo:lo + 20000].float())
    two = ShardedGallery(g8, a.N, scales=gs, fine_rows=fine)
    wide = ShardedGallery(fine, a.N)
    _, idx = two.search(q, a.kc)                                      # the candidates of a real coarse search: every index valid
    hip = lambda: ops.rerank_rows(q, idx, fine, 0, a.k, ws)
    t32, t16 = (lambda: torch_rerank(q, idx, fine, a.k, True)), (lambda: torch_rerank(q, idx, fine, a.k, False))
    same = float((hip()[1] == t32()[1]).float().mean())               # near-duplicates: f32 sums in another order may swap a pair
    op_us, t32_us, t16_us = events([hip, t32, t16], a.iters)
    op_chain = graph_chain([lambda: raw(idx)] * 20, a.iters)
    order_chain = graph_chain([lambda: raw(idx, a.N)] * 20, a.iters)
    op_cold = graph_chain([lambda i=i: raw(i) for i in cold_sets], max(a.iters // 4, 10))
    row_bytes = a.B * a.kc * a.D * 2
    score_cold = max(op_cold - order_chain, 1e-3)
    coarse_us, coarse_kc_us, two_us, bf16_us = events([lambda: two.search(q, a.k), lambda: two.search(q, a.kc),
                                                       lambda: two.search_reranked(q, a.k, a.kc), lambda: wide.search(q, a.k)],
                                                      max(a.iters // 4, 10))
    top = wide.search(q, 1)[1][:, 0]
    res.update({"op_us": round(op_us, 2), "op_eager_host_us": round(host_clock(hip, a.iters), 2), "op_chain_us": round(op_chain, 2),
                "op_cold_us": round(op_cold, 2), "order_chain_us": round(order_chain, 2), "row_bytes": row_bytes,
                "row_GBps_chain": round(row_bytes / max(op_chain - order_chain, 1e-3) / 1e3, 1),
                "row_GBps_cold": round(row_bytes / score_cold / 1e3, 1),
                "hbm_fraction": round(row_bytes / (score_cold * 1e-6) / HBM_PEAK, 3),
                "torch_f32_us": round(t32_us, 2), "torch_bf16_us": round(t16_us, 2), "torch_f32_over_op": round(t32_us / op_us, 2),
                "torch_bf16_over_op": round(t16_us / op_us, 2), "index_agreement_with_torch_f32": round(same, 4),
                "coarse_us": round(coarse_us, 2), "coarse_kc_us": round(coarse_kc_us, 2), "two_tier_us": round(two_us, 2), "bf16_us": round(bf16_us, 2),
                "two_tier_over_bf16": round(two_us / bf16_us, 3),
                "top1_agree_coarse": float((two.search(q, 1)[1][:, 0] == top).float().mean()),
                "top1_agree_two_tier": float((two.search_reranked(q, 1, a.kc)[1][:, 0] == top).float().mean()),
                "uncertified": two.uncertified_queries() + wide.uncertified_queries()})
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
