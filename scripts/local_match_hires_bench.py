"""Local-feature re-ranking beyond 256 patches on one MI355X: ops.local_rerank_hires / local_rerank_fp8_hires
(include/vpr_amd_local_hires.h) beside the PyTorch form a caller would have written without them, by the method of
scripts/local_match_bench.py (whose timing helpers and PyTorch form are imported): medians of `iters`, every form taking turns
inside one timed loop after a warm-up, the PyTorch forms with their gather inside the timed region.  At n <= 256 the 256-patch
ops join the loop, for the ratio that keeps them the route there.  Needs a GPU.
Usage: python scripts/local_match_hires_bench.py [--B 64] [--kc 16 32] [--n 256 529 1369] [--l 128] [--k 10] [--iters 100] [--out FILE]

One row per (n, kc, element); times in us:
  op_us        one call of the hires op on a preallocated workspace, events around the call
  op_chain_us  the raw C call 10 times in one HIP graph, per call: the two kernels without the host between them
  torch_us     the PyTorch form on the bf16 features (bf16 bmm: similarities rounded to bf16); the same number on both rows
  torch_f32_us the same with the operands widened to f32 before the bmm: f32 similarities, as the kernels have them
  f32/op       torch_f32_us / op_us
  GFLOP        2 * B * kc * n * n * l
  mfma_frac    GFLOP / op_chain_us over the dense MFMA peak of the element (2.5 PFLOP/s bf16, 5 PFLOP/s e4m3)
  gather_MB    B * kc * n * l * bytes per element, the scattered candidate features
  gather_frac  gather_MB / op_chain_us over the 8 TB/s HBM peak (N is chosen so that the gallery of either element is larger
               than the 256 MB Infinity Cache, and every candidate list is random)
  op256_us     n <= 256 only: the 256-patch op of the same element in the same loop; hires/256 = op_us / op256_us
  agree_f32    fraction of (query, position) pairs of the k-lists at which the op and the f32 PyTorch form name the same image
               (for e4m3: on the quantised features the f32 form does not see, so near-ties among distractors differ)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from local_match_bench import HBM_PEAK, MFMA_PEAK, events, graph_chain, torch_local_rerank  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--kc", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--n", type=int, nargs="+", default=[256, 529, 1369])
    ap.add_argument("--l", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--min-sim", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("local_match_hires_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, device=dev, generator=gen), dim=-1).to(torch.bfloat16)
    lines = [f"# local_match_hires_bench: library {os.path.basename(_lib.library_path())}, B {a.B}, l {a.l}, k {a.k}, "
             f"min_sim {a.min_sim}, iters {a.iters}",
             "%5s %4s %5s %6s %10s %12s %10s %13s %7s %8s %10s %10s %12s %10s %10s %10s" % (
                 "n", "kc", "elem", "N", "op_us", "op_chain_us", "torch_us", "torch_f32_us", "f32/op", "GFLOP", "mfma_frac", "gather_MB",
                 "gather_frac", "op256_us", "hires/256", "agree_f32")]
    for n in a.n:
        N = 1
        while N * n * a.l < 256 * 2 ** 20:                                # the e4m3 gallery alone exceeds the Infinity Cache
            N *= 2
        g16 = torch.cat([unit(min(256, N - lo), n, a.l) for lo in range(0, N, 256)])
        q16 = unit(a.B, n, a.l)
        g16[:a.B] = q16[:, torch.randperm(n, device=dev, generator=gen)]  # image b shares query b's patches
        g8, q8 = ops.quantize_patch_fp8(g16), ops.quantize_patch_fp8(q16)
        for kc in a.kc:
            k = min(a.k, kc)
            idx = torch.randint(0, N, (a.B, kc), device=dev, generator=gen, dtype=torch.int32)
            idx[:, 0] = torch.arange(a.B, device=dev, dtype=torch.int32)
            ws = torch.empty(_lib.lib().vpr_hires_local_workspace_bytes(a.B, kc), dtype=torch.uint8, device=dev)
            vals = torch.empty((a.B, k), dtype=torch.float32, device=dev)
            out = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            mt = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            null = ops._ptr(None)
            raw = lambda entry, q, g: (lambda: ops._call(entry, ops._ptr(q), n, ops._ptr(idx), a.B, kc, ops._ptr(g), n, a.l, N, 0, a.min_sim,
                                                         k, ops._ptr(vals), ops._ptr(out), ops._ptr(mt), null, null, null, null,
                                                         ops._ptr(ws), ws.numel(), ops._stream()))
            hip16 = lambda: ops.local_rerank_hires(q16, idx, g16, 0, k, a.min_sim, ws)
            hip8 = lambda: ops.local_rerank_fp8_hires(q8, idx, g8, 0, k, a.min_sim, ws)
            ref = lambda: torch_local_rerank(q16, idx, g16, k, a.min_sim)
            ref32 = lambda: torch_local_rerank(q16, idx, g16, k, a.min_sim, True)
            fns = [hip16, hip8, ref, ref32]
            if n <= _lib.LOCAL_MAX_N:
                fns += [lambda: ops.local_rerank(q16, idx, g16, 0, k, a.min_sim, ws), lambda: ops.local_rerank_fp8(q8, idx, g8, 0, k, a.min_sim, ws)]
            want = ref32()[1]
            agree = [float((fn()[1] == want).float().mean()) for fn in (hip16, hip8)]
            assert all(bool((fn()[1][:, 0] == idx[:, 0]).all()) for fn in (hip16, hip8))      # the planted image comes back first
            t = events(fns, a.iters)
            chains = [graph_chain([raw("vpr_hires_local_rerank", q16, g16)] * 10, a.iters),
                      graph_chain([raw("vpr_hires_patch_rerank_fp8", q8, g8)] * 10, a.iters)]
            flop = 2.0 * a.B * kc * n * n * a.l
            for e, (name, es, peak) in enumerate((("bf16", 2, MFMA_PEAK), ("e4m3", 1, 2 * MFMA_PEAK))):
                gather = a.B * kc * n * a.l * float(es)
                old = "%10.1f %10.2f" % (t[4 + e], t[e] / t[4 + e]) if len(t) > 4 else "%10s %10s" % ("-", "-")
                lines.append("%5d %4d %5s %6d %10.1f %12.1f %10.1f %13.1f %7.2f %8.2f %10.4f %10.1f %12.4f %s %10.4f" % (
                    n, kc, name, N, t[e], chains[e], t[2], t[3], t[3] / t[e], flop / 1e9, flop / (chains[e] * 1e-6) / peak, gather / 1e6,
                    gather / (chains[e] * 1e-6) / HBM_PEAK, old, agree[e]))
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
