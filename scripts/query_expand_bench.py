"""Query expansion on one MI355X: the two kernels, the eager op, the whole two-pass search, and the PyTorch composition a
caller would have written without them (HIP events on torch's stream; needs a GPU).
Usage: python scripts/query_expand_bench.py [--N 100000] [--B 64] [--k 10] [--n-use 10] [--iters 200] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/query_expand_bench.py --trace
           (a run of its own: 200 launches of each kernel per format, nothing timed; scripts/trace_medians.py OUT reads it)
       VPR_AMD_LIBRARY=/path/to/another/libvpr_amd.so python scripts/query_expand_bench.py ...   (e.g. a -DVPR_EXPAND_NT=1 build)

Numbers, per gallery format (bf16, e4m3):
  partial_us / finish_us   median over `iters` single launches of vpr_query_expand (partial only) / vpr_query_expand_finish
                           (R = 1), events around each call: at this size mostly the launch, an upper bound of the kernel
  partial_chain_us / finish_chain_us   the same launch 20 times in one HIP graph, replayed `iters` times, per launch: the kernel
                           with its ~1 us boundary and nothing of the host
  partial_cold_us          a graph of 40 partial launches, each on its own random neighbour rows (40 x row_bytes = 432 MB in bf16,
                           more than the 256 MB Infinity Cache), per launch: rows from HBM, as after a search that has just
                           streamed the whole gallery; the chain above re-reads the same 640 rows, i.e. from cache
  row_bytes                B * n_use * D * bytes per element: the scattered row reads, the traffic the partial kernel exists for
  hbm_fraction             row_bytes / partial_cold time over the 8 TB/s HBM3E peak (the kernel is bound by bytes, not operations)
  eager_us                 host clock per ops.query_expand(finish=True) call over a synchronised loop: launch-bound at this size
  torch_us                 the comparison: (w[..., None] * rows[idx].float()).sum(1) + weighted query, normalised, to bf16 — with
                           the dequantisation rows.view(e4m3).float() * scales[idx] for the e4m3 gallery; events, median
  search_us / expanded_us  ShardedGallery.search and .search_expanded (search, expand, search), events, median
The HIP and PyTorch variants are timed alternately in one loop, and their expanded queries are compared before timing."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpr_amd import _lib, ops  # noqa: E402
from vpr_amd.retrieval import ShardedGallery  # noqa: E402

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
    """Per-launch time (us) of the calls `fns` captured back to back in one HIP graph (median over `iters` replays)."""
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


def torch_expand(q, vals, idx, rows, scales, n_use, alpha, q_weight):
    """What a caller writes today, single shard, every index valid."""
    i = idx[:, :n_use].long()
    w = torch.where(vals[:, :n_use] > 0, vals[:, :n_use].double().pow(alpha).float(), 0.0)
    g = rows[i].float() if scales is None else rows[i].view(torch.float8_e4m3fn).float() * scales[i][..., None]
    s = q_weight * q.float() + (w[..., None] * g).sum(1)
    return torch.nn.functional.normalize(s, dim=1).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--D", type=int, default=8448)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-use", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true", help="only launch each kernel 200 times (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("query_expand_bench: needs a GPU (there is nothing to measure without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {"library": os.path.basename(_lib.library_path()), "B": a.B, "N": a.N, "D": a.D, "k": a.k, "n_use": a.n_use,
           "alpha": a.alpha, "iters": a.iters}
    gal = torch.empty((a.N, a.D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, a.N, 20000):                  # clusters of 8 rows, so a query's neighbours score well above 0
        n = min(20000, a.N - lo)
        c = torch.randn((n + 7) // 8, a.D, device=dev, generator=g).repeat_interleave(8, 0)[:n]
        gal[lo:lo + n] = torch.nn.functional.normalize(c + 0.5 * torch.randn(n, a.D, device=dev, generator=g), dim=1).to(torch.bfloat16)
    pos = torch.randint(0, a.N, (a.B,), device=dev, generator=g)
    q = torch.nn.functional.normalize(gal[pos].float() + 0.004 * torch.randn(a.B, a.D, device=dev, generator=g), dim=1).to(torch.bfloat16)
    for fmt in ("bf16", "e4m3"):
        if fmt == "bf16":
            rows, scales, bytes_per = gal, None, 2
        else:
            rows = torch.empty((a.N, a.D), dtype=torch.uint8, device=dev)
            scales = torch.empty((a.N,), dtype=torch.float32, device=dev)
            for lo in range(0, a.N, 20000):
                rows[lo:lo + 20000], scales[lo:lo + 20000] = ops.quantize_fp8_rows(gal[lo:lo + 20000].float())
            bytes_per = 1
        sg = ShardedGallery(rows, a.N, scales=scales)
        vals, idx = sg.search(q, a.k)
        partial = torch.empty((a.B, a.D), dtype=torch.float32, device=dev)
        out32 = torch.empty((a.B, a.D), dtype=torch.float32, device=dev)
        out16 = torch.empty((a.B, a.D), dtype=torch.bfloat16, device=dev)
        # the two entry points on fixed buffers (what a graph may hold): partial only; finish of that partial
        raw_partial = lambda v=vals, i=idx: ops._call(
            "vpr_query_expand", ops._ptr(q), ops._ptr(v), ops._ptr(i), a.B, a.D, a.k, ops._ptr(rows), ops._ptr(scales), a.N, 0,
            a.n_use, a.alpha, 1.0, 1, ops._ptr(partial), None, None, ops._stream())
        raw_finish = lambda: ops._call("vpr_query_expand_finish", ops._ptr(partial), 1, ops._ptr(q), a.B, a.D, ops._ptr(out32),
                                       ops._ptr(out16), ops._stream())
        if a.trace:
            for fn in (raw_partial, raw_finish):
                for _ in range(200):
                    fn()
            torch.cuda.synchronize()
            continue
        hip = lambda: ops.query_expand(q, vals, idx, rows, scales, 0, a.n_use, a.alpha, 1.0, True, finish=True)[1]
        ref = lambda: torch_expand(q, vals, idx, rows, scales, a.n_use, a.alpha, 1.0)
        diff = (hip().float() - ref().float()).abs().max().item()          # bf16 outputs: one ulp at 2^-7 is 2^-15
        part_us, fin_us, hip_us, torch_us = events(
            [lambda: ops.query_expand(q, vals, idx, rows, scales, 0, a.n_use, a.alpha, 1.0, True, partial=partial),
             lambda: ops.query_expand_finish(partial[None], q), hip, ref], a.iters)
        part_chain, fin_chain = graph_chain([raw_partial] * 20, a.iters), graph_chain([raw_finish] * 20, a.iters)
        cold_sets = [(torch.rand(a.B, a.k, device=dev, generator=g) * 0.7 + 0.2,
                      torch.randint(0, a.N, (a.B, a.k), device=dev, generator=g, dtype=torch.int32)) for _ in range(40)]
        part_cold = graph_chain([lambda v=v, i=i: raw_partial(v, i) for v, i in cold_sets], max(a.iters // 4, 10))
        row_bytes = a.B * a.n_use * a.D * bytes_per
        search_us, expanded_us = events([lambda: sg.search(q, a.k), lambda: sg.search_expanded(q, a.k, a.n_use, a.alpha)],
                                        max(a.iters // 4, 10))
        res[fmt] = {"partial_us": round(part_us, 2), "finish_us": round(fin_us, 2), "partial_chain_us": round(part_chain, 2),
                    "finish_chain_us": round(fin_chain, 2), "row_bytes": row_bytes,
                    "partial_cold_us": round(part_cold, 2), "row_GBps": round(row_bytes / part_cold / 1e3, 1),
                    "hbm_fraction": round(row_bytes / (part_cold * 1e-6) / HBM_PEAK, 3),
                    "expand_events_us": round(hip_us, 2), "eager_us": round(host_clock(hip, a.iters), 2),
                    "torch_us": round(torch_us, 2), "torch_over_hip": round(torch_us / hip_us, 2),
                    "max_abs_diff_vs_torch": diff, "search_us": round(search_us, 2), "expanded_us": round(expanded_us, 2),
                    "expanded_over_search": round(expanded_us / search_us, 3), "uncertified": sg.uncertified_queries()}
        del sg
    if a.trace:
        return
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
