"""Descriptor projection on one MI355X: vpr_project_rows at the serving shape beside the PyTorch a caller would write, the
64-query search of a 100k-row gallery at full width against projection + search at d = 512, bulk projection throughput, the
sweep of `rows` the route boundary was chosen from, and (--fit) the wall time of fit_projection (HIP events on torch's
stream; needs a GPU).
Usage: python scripts/project_bench.py [--N 100000] [--B 64] [--iters 200] [--out FILE] [--fit]
       VPR_AMD_LIBRARY=/path/to/libvpr_amd_stream.so python scripts/project_bench.py --sweep-only
           (a build with -DVPR_PROJECT_STREAM_MAX_ROWS=4096: the split-K route measured beyond its boundary)

Numbers:
  project[d]   64 x 8448 -> d, d in {512, 2048}:
    warm_us      the call 20 times in one HIP graph, replayed `iters` times, per call (both kernels, ~1 us boundaries): P from cache
    cold_us      a graph of 40 calls, each on its own copy of P (40 x 2 d D bytes, more than the 256 MB Infinity Cache), per call:
                 the matrix from HBM, as on a serving step that has just streamed the gallery
    hbm_fraction 2 d D bytes / cold_us over the 8 TB/s HBM3E peak
    eager_us     events around ops.project_rows, median: launch-bound at this size
    torch_us / torch_cold_us   normalize(x.float() @ P.float().T + c).bfloat16(), events, median; cold: rotating over the 40 copies
  search[fmt]  fmt in {bf16, e4m3}, k = 10: full_us = ShardedGallery.search at D = 8448 (the figure of
               profiles/query_expand_bench.txt, re-measured here); projected_us = search of D-wide queries on the gallery
               projected to d = 512 (projection + search); search_only_us = the same on already projected queries
  bulk         65536 x 8448 -> 512 on the tiled route: us per call and rows / s
  sweep        rows -> us per call in a 20-call graph (P warm): `call` = vpr_project_rows as routed (route 0 up to
               VPR_PROJECT_STREAM_MAX_ROWS, route 1 beyond), `gemm256` = the tiled GEMM of route 1 alone at that row count (route 1
               without its finish kernel: a lower bound), `torch` = the PyTorch composition (events)
  fit_s        (--fit) wall time of fit_projection(n = 16384, D = 8448, d = 512) on the device, one run
The HIP and PyTorch variants are compared before timing."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpr_amd import _lib, ops  # noqa: E402
from vpr_amd.projection import DescriptorProjection, fit_projection  # noqa: E402
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
    us = events([graph.replay], iters)[0] / len(fns)
    del graph
    ops.drop_stream_caches(side.cuda_stream)
    return us


def torch_project(x, P, c):
    """What a caller writes today."""
    return torch.nn.functional.normalize(x.float() @ P.float().T + c, dim=1).bfloat16()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--D", type=int, default=8448)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--fit", action="store_true", help="only time fit_projection at n = 16384 (minutes)")
    ap.add_argument("--sweep-only", action="store_true", help="only the sweep of rows (e.g. on a timing-only build of the library)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("project_bench: needs a GPU (there is nothing to measure without one)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    D, B = a.D, a.B
    res = {"library": os.path.basename(_lib.library_path()), "B": B, "N": a.N, "D": D, "iters": a.iters,
           "stream_max_rows": _lib.PROJECT_STREAM_MAX_ROWS}

    def finish():
        text = json.dumps(res)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")

    if a.fit:
        n = 16384
        x = torch.nn.functional.normalize(torch.randn(n, D, device=dev, generator=g), dim=1).to(torch.bfloat16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = fit_projection(x, 512)
        torch.cuda.synchronize()
        res["fit_s"] = round(time.perf_counter() - t0, 2)
        res["fit_n"], res["fit_d"] = p.n_fit, p.d
        return finish()

    def operands(d, copies=1):
        P = (torch.randn(d, D, device=dev, generator=g) / D ** 0.5).to(torch.bfloat16)
        c = 0.02 * torch.randn(d, device=dev, generator=g)
        return [P] + [P.clone() for _ in range(copies - 1)], c

    def unit(rows, P):      # rows that lie mostly in the span of P, like descriptors in the span of their principal axes
        x = torch.randn(rows, P.shape[0], device=dev, generator=g) @ P.float() / P.shape[0] ** 0.5
        return torch.nn.functional.normalize(x + 0.5 * torch.randn(rows, D, device=dev, generator=g) / D ** 0.5, dim=1).to(torch.bfloat16)

    def fixed_call(x, P, c):
        """vpr_project_rows on fixed buffers (what a graph may hold)."""
        rows, d = x.shape[0], P.shape[0]
        o16 = torch.empty((rows, d), dtype=torch.bfloat16, device=dev)
        ws = torch.empty(max(_lib.lib().vpr_project_workspace_bytes(rows, D, d), 256), dtype=torch.uint8, device=dev)
        return lambda P=P: ops._call("vpr_project_rows", ops._ptr(x), D, rows, D, ops._ptr(P), ops._ptr(c), d, 1, None, ops._ptr(o16),
                                     ops._ptr(ws), ws.numel(), ops._stream())

    # 1. the serving shape
    res["project"] = {}
    for d in () if a.sweep_only else (512, 2048):
        copies = 40
        Ps, c = operands(d, copies)
        x = unit(B, Ps[0])
        hip = lambda: ops.project_rows(x, Ps[0], c)[1]
        ref = lambda: torch_project(x, Ps[0], c)
        diff = (hip().float() - ref().float()).abs().max().item()
        call = fixed_call(x, Ps[0], c)
        warm = graph_chain([call] * 20, a.iters)
        cold = graph_chain([lambda P=P: call(P) for P in Ps], max(a.iters // 4, 10))
        turn = [0]

        def ref_cold():
            turn[0] = (turn[0] + 1) % copies
            return torch_project(x, Ps[turn[0]], c)

        eager_us, torch_us, torch_cold_us = events([hip, ref, ref_cold], a.iters)
        mbytes = 2 * d * D
        res["project"][str(d)] = {"warm_us": round(warm, 2), "cold_us": round(cold, 2), "matrix_bytes": mbytes,
                                  "hbm_fraction": round(mbytes / (cold * 1e-6) / HBM_PEAK, 3), "eager_us": round(eager_us, 2),
                                  "torch_us": round(torch_us, 2), "torch_cold_us": round(torch_cold_us, 2),
                                  "torch_cold_over_cold": round(torch_cold_us / cold, 2), "max_abs_diff_vs_torch": diff}
        del Ps

    # 4. the sweep the route boundary comes from (d = 512)
    (P,), c = operands(512)
    sweep = {}
    for rows in (1, 16, 32, 64, 96, 128, 129, 192, 256, 384, 512, 768, 1024, 1536, 2048, 4096):
        x = unit(rows, P)
        z = torch.empty((rows, 512), dtype=torch.float32, device=dev)
        it = max(a.iters // 4, 10)
        entry = {"route": ops.project_route(rows, D, 512), "call": round(graph_chain([fixed_call(x, P, c)] * 20, it), 2),
                 "gemm256": round(graph_chain([lambda: ops.gemm_nt_bf16(x, P, tile256=True, out=z)] * 20, it), 2),
                 "torch": round(events([lambda: torch_project(x, P, c)], it)[0], 2)}
        sweep[str(rows)] = entry
    res["sweep"] = sweep
    if a.sweep_only:
        return finish()

    # 3. bulk projection
    x = unit(65536, P)
    bulk = graph_chain([fixed_call(x, P, c)] * 4, max(a.iters // 10, 5))
    res["bulk"] = {"rows": 65536, "us": round(bulk, 1), "rows_per_s": round(65536 / (bulk * 1e-6)),
                   "torch_us": round(events([lambda: torch_project(x, P, c)], 5, warmup=2)[0], 1)}
    del x

    # 2. search at full width against projection + search at d = 512
    gal = torch.empty((a.N, D), dtype=torch.bfloat16, device=dev)
    for lo in range(0, a.N, 20000):
        gal[lo:lo + 20000] = unit(min(20000, a.N - lo), P)
    pos = torch.randint(0, a.N, (B,), device=dev, generator=g)
    q = torch.nn.functional.normalize(gal[pos].float() + 0.004 * torch.randn(B, D, device=dev, generator=g), dim=1).to(torch.bfloat16)
    proj = DescriptorProjection(P.float().cpu(), torch.zeros(D, dtype=torch.float64), torch.ones(512, dtype=torch.float64), whiten=False)
    from vpr_amd import gallery as G
    res["search"] = {}
    for fmt in ("bf16", "e4m3"):
        if fmt == "bf16":
            full = ShardedGallery(gal, a.N)
        else:
            rows8 = torch.empty((a.N, D), dtype=torch.uint8, device=dev)
            sc = torch.empty((a.N,), dtype=torch.float32, device=dev)
            for lo in range(0, a.N, 20000):
                rows8[lo:lo + 20000], sc[lo:lo + 20000] = ops.quantize_fp8_rows(gal[lo:lo + 20000].float())
            full = ShardedGallery(rows8, a.N, scales=sc)
        prow, pscale = G.project_gallery(gal, proj, fp8=fmt == "e4m3")
        narrow = ShardedGallery(prow, a.N, scales=pscale, projection=proj)
        qp = proj.apply(q)
        same = (full.search(q, a.k)[1][:, 0] == narrow.search(q, a.k)[1][:, 0]).float().mean().item()
        it = max(a.iters // 4, 10)
        full_us, projected_us, only_us = events([lambda: full.search(q, a.k), lambda: narrow.search(q, a.k),
                                                 lambda: narrow.search(qp, a.k)], it)
        res["search"][fmt] = {"full_us": round(full_us, 2), "projected_us": round(projected_us, 2), "search_only_us": round(only_us, 2),
                              "full_over_projected": round(full_us / projected_us, 2), "same_top1": same,
                              "uncertified": full.uncertified_queries() + narrow.uncertified_queries()}
        del full, narrow
    finish()


if __name__ == "__main__":
    main()
