"""Local re-ranking verified under a similarity transform on one MI355X: ops.local_rerank_similarity
(include/vpr_amd_similarity.h) beside the shift-vote call (ops.local_rerank_spatial) and the plain call of the same shape
(ops.local_rerank / local_rerank_fp8 at n <= 256, their _hires forms beyond), and the two verify launches alone
(vpr_similarity_verify / vpr_spatial_verify on the match list of the same pairs), by the method of
scripts/spatial_rerank_bench.py: medians of `iters`, every form taking turns inside one timed loop after a warm-up (the timing
helpers of scripts/local_match_bench.py are imported).  Needs a GPU.
Usage: python scripts/similarity_rerank_bench.py [--B 64] [--N 4096] [--kc 16 32] [--n 256 529 1369] [--l 128] [--k 10] [--tol 1]
                                                [--iters 100] [--out FILE]

One row per (n, kc, element); times in us:
  sim_us       one call of ops.local_rerank_similarity on a preallocated workspace, events around the call
  shift_us     ops.local_rerank_spatial and
  plain_us     the plain op of the same shape and element, in the same loop; sim/plain and sim/shift are the ratios
  sim_chain    the raw C call of the similarity form 10 times in one HIP graph, per call: match, verify and order without the host
  sh_chain, pl_chain   the same for the shift-vote and the plain form; extra_us = sim_chain - pl_chain, what verification adds
  sim_ver_us   vpr_similarity_verify alone on the [B * kc, n] match list of these pairs, 10 times in one HIP graph, per call
  sh_ver_us    vpr_spatial_verify alone on the same list, likewise
  M            the mean number of matches per pair: the hypothesis loop runs 256 * M inlier tests per pair
  first        fraction of the queries whose planted image (the query zoomed by 3/2 about the grid's centre) comes back first
               under the similarity call / under the shift-vote call"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from local_match_bench import events, graph_chain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--kc", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--n", type=int, nargs="+", default=[256, 529, 1369])
    ap.add_argument("--l", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--tol", type=int, default=1)
    ap.add_argument("--min-sim", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("similarity_rerank_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, device=dev, generator=gen), dim=-1).to(torch.bfloat16)
    lines = [f"# similarity_rerank_bench: library {os.path.basename(_lib.library_path())}, B {a.B}, N {a.N}, l {a.l}, k {a.k}, tol {a.tol}, "
             f"min_sim {a.min_sim}, iters {a.iters}",
             "%5s %4s %5s %9s %9s %9s %9s %9s %10s %9s %9s %9s %11s %10s %7s %10s" % (
                 "n", "kc", "elem", "sim_us", "shift_us", "plain_us", "sim/plain", "sim/shift", "sim_chain", "sh_chain", "pl_chain",
                 "extra_us", "sim_ver_us", "sh_ver_us", "M", "first")]
    for n in a.n:
        gw = int(round(n ** 0.5))
        if gw * gw != n:
            sys.exit(f"similarity_rerank_bench: n = {n} is not a square grid")
        hires = n > _lib.LOCAL_MAX_N
        g16 = torch.cat([unit(min(256, a.N - lo), n, a.l) for lo in range(0, a.N, 256)])
        q16 = unit(a.B, n, a.l)
        # image b is query b zoomed by 3/2: its patch at (x, y) is the query's at floor(1.5 (x - c) + c + 0.5) per axis where that exists
        x = torch.arange(gw, device=dev)
        src = (3 * (2 * x - (gw - 1)) + 2 * (gw - 1) + 2) // 4
        on = x[(src >= 0) & (src < gw)]
        grid = q16.view(a.B, gw, gw, a.l)
        g16[:a.B].view(a.B, gw, gw, a.l)[:, on[:, None], on[None, :]] = grid[:, src[on][:, None], src[on][None, :]]
        g8, q8 = ops.quantize_patch_fp8(g16), ops.quantize_patch_fp8(q16)
        for kc in a.kc:
            k = min(a.k, kc)
            idx = torch.randint(0, a.N, (a.B, kc), device=dev, generator=gen, dtype=torch.int32)
            idx[:, 0] = torch.arange(a.B, device=dev, dtype=torch.int32)
            need = _lib.lib().vpr_similarity_workspace_bytes(a.B, kc, n)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            vals = torch.empty((a.B, k), dtype=torch.float32, device=dev)
            out = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            cnt = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            null = ops._ptr(None)
            head = lambda q, g: (ops._ptr(q), n, ops._ptr(idx), a.B, kc, ops._ptr(g), n, a.l, a.N, 0, a.min_sim, k, ops._ptr(vals),
                                 ops._ptr(out), ops._ptr(cnt))
            raw_v = lambda entry, q, g, fp8: (lambda: ops._call(entry, *head(q, g), *[null] * 6, fp8, gw, gw, a.tol,
                                                                ops._ptr(ws), ws.numel(), ops._stream()))
            raw_pl = lambda entry, q, g: (lambda: ops._call(entry, *head(q, g), *[null] * 4, ops._ptr(ws), ws.numel(), ops._stream()))
            plain16 = ops.local_rerank_hires if hires else ops.local_rerank
            plain8 = ops.local_rerank_fp8_hires if hires else ops.local_rerank_fp8
            entry16 = "vpr_hires_local_rerank" if hires else "vpr_local_rerank"
            entry8 = "vpr_hires_patch_rerank_fp8" if hires else "vpr_patch_rerank_fp8"
            sm16 = lambda: ops.local_rerank_similarity(q16, idx, g16, gw, gw, a.tol, 0, k, a.min_sim, ws)
            sm8 = lambda: ops.local_rerank_similarity(q8, idx, g8, gw, gw, a.tol, 0, k, a.min_sim, ws)
            sh16 = lambda: ops.local_rerank_spatial(q16, idx, g16, gw, gw, a.tol, 0, k, a.min_sim, ws)
            sh8 = lambda: ops.local_rerank_spatial(q8, idx, g8, gw, gw, a.tol, 0, k, a.min_sim, ws)
            pl16 = lambda: plain16(q16, idx, g16, 0, k, a.min_sim, ws)
            pl8 = lambda: plain8(q8, idx, g8, 0, k, a.min_sim, ws)
            first = [float((fn()[1][:, 0] == idx[:, 0]).float().mean()) for fn in (sm16, sm8, sh16, sh8)]
            t = events([sm16, sm8, sh16, sh8, pl16, pl8], a.iters)
            chain = lambda fn: graph_chain([fn] * 10, a.iters)
            sm_chain = [chain(raw_v("vpr_similarity_local_rerank", q16, g16, 0)), chain(raw_v("vpr_similarity_local_rerank", q8, g8, 1))]
            sh_chain = [chain(raw_v("vpr_spatial_local_rerank", q16, g16, 0)), chain(raw_v("vpr_spatial_local_rerank", q8, g8, 1))]
            pl_chain = [chain(raw_pl(entry16, q16, g16)), chain(raw_pl(entry8, q8, g8))]
            for e, (name, q, g) in enumerate((("bf16", q16, g16), ("e4m3", q8, g8))):
                dbg = ops.local_rerank_similarity(q, idx, g, gw, gw, a.tol, 0, k, a.min_sim, ws, debug=True)[3]
                col = dbg.col_nn.view(a.B * kc, n)
                back = torch.gather(dbg.row_nn.view(a.B * kc, n), 1, col.clamp(min=0).long())
                partner = torch.where((col >= 0) & (back == torch.arange(n, device=dev, dtype=torch.int32)), col,
                                      torch.full_like(col, -1)).contiguous()              # the mutual pairs: the list's partners
                sim = torch.full((a.B * kc, n), 0.5, dtype=torch.float32, device=dev)
                res = [torch.empty(a.B * kc, dtype=torch.float32, device=dev)] + [torch.empty(a.B * kc * 6, dtype=torch.int32, device=dev)
                                                                                   for _ in range(3)]
                raw = lambda entry: (lambda: ops._call(entry, ops._ptr(partner), ops._ptr(sim), a.B * kc, n, gw, n, gw, a.tol,
                                                       *[ops._ptr(r) for r in res], null, ops._stream()))
                ver = [chain(raw("vpr_similarity_verify")), chain(raw("vpr_spatial_verify"))]
                lines.append("%5d %4d %5s %9.1f %9.1f %9.1f %9.3f %9.3f %10.1f %9.1f %9.1f %9.1f %11.1f %10.1f %7.1f  %4.2f/%4.2f" % (
                    n, kc, name, t[e], t[2 + e], t[4 + e], t[e] / t[4 + e], t[e] / t[2 + e], sm_chain[e], sh_chain[e], pl_chain[e],
                    sm_chain[e] - pl_chain[e], ver[0], ver[1], float(dbg.pair_matches.float().mean()), first[e], first[2 + e]))
        del g16, g8, q16, q8
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
