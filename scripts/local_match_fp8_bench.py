"""Local-feature re-ranking on e4m3 patch features beside the bf16 form on one MI355X: vpr_patch_rerank_fp8 and
vpr_local_rerank on the same features (the e4m3 store is the device quantiser's output for them), the two ops alternating in
one timed loop (HIP events on torch's stream; needs a GPU).  The yardstick is the bf16 op in the same run.
Usage: python scripts/local_match_fp8_bench.py [--N 4096] [--B 64] [--kc 16 32 64] [--n 256] [--l 128] [--k 10] [--iters 100] [--out FILE]

Columns (times in us, medians of --iters; after a warm-up of every shape):
  bf16_us / fp8_us        one ops.local_rerank / ops.local_rerank_fp8 call on a preallocated workspace, events around the call
  bf16_chain / fp8_chain  the raw C call 10 times in one HIP graph, per call: the two kernels without the host between them
  fp8/bf16                fp8_chain / bf16_chain (below 1: the e4m3 form is faster)
  MB_bf16 / MB_fp8        B * kc * n * l * element size, the scattered candidate features a call gathers
  hbm_bf16 / hbm_fp8      those bytes / chain time over the 8 TB/s HBM peak
  mfma_bf16 / mfma_fp8    2 * B * kc * n * n * l / chain time over each element type's dense MFMA peak (2.5 PFLOP/s bf16, 5 PFLOP/s
                          block-scaled e4m3)
  agree@1 / agree@k       fraction of queries whose first place / of (query, position) pairs of the k-lists at which the two
                          ops name the same image
  quant_us                ops.quantize_patch_fp8 of the B queries' bf16 features (what a search with bf16 query features adds)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from local_match_bench import events, graph_chain  # noqa: E402  (scripts/ is sys.path[0]: the bf16 bench's timing loops)

MFMA_PEAK_BF16, MFMA_PEAK_FP8, HBM_PEAK = 2.5e15, 5.0e15, 8.0e12


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
        sys.exit("local_match_fp8_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, device=dev, generator=g), dim=-1)
    gal32 = [unit(min(512, a.N - lo), a.n, a.l) for lo in range(0, a.N, 512)]
    q32 = unit(a.B, a.n, a.l)
    lines = [f"# local_match_fp8_bench: library {os.path.basename(_lib.library_path())}, B {a.B}, N {a.N}, n {a.n}, l {a.l}, k {a.k}, "
             f"min_sim {a.min_sim}, iters {a.iters}; gallery {a.N * a.n * a.l * 2 / 1e6:.0f} MB bf16, {a.N * a.n * a.l / 1e6:.0f} MB e4m3",
             "%4s %9s %9s %11s %10s %9s %8s %7s %9s %8s %10s %9s %8s %8s %9s" % (
                 "kc", "bf16_us", "fp8_us", "bf16_chain", "fp8_chain", "fp8/bf16", "MB_bf16", "MB_fp8", "hbm_bf16", "hbm_fp8",
                 "mfma_bf16", "mfma_fp8", "agree@1", "agree@k", "quant_us")]
    for kc in a.kc:
        k = min(a.k, kc)
        idx = torch.randint(0, a.N, (a.B, kc), device=dev, generator=g, dtype=torch.int32)
        idx[:, 0] = torch.arange(a.B, device=dev, dtype=torch.int32)         # one candidate per query shares its patches
        gal32[0][:a.B] = q32[:, torch.randperm(a.n, device=dev, generator=g)]
        # both stores from the same f32 features, each in one rounding
        g16, q16 = torch.cat([t.to(torch.bfloat16) for t in gal32]), q32.to(torch.bfloat16)
        g8, q8 = torch.cat([ops.quantize_patch_fp8(t) for t in gal32]), ops.quantize_patch_fp8(q32)
        null = ops._ptr(None)
        forms = []
        for entry, ws_entry, op, qf, gf in (("vpr_local_rerank", "vpr_local_workspace_bytes", ops.local_rerank, q16, g16),
                                            ("vpr_patch_rerank_fp8", "vpr_patch_workspace_bytes_fp8", ops.local_rerank_fp8, q8, g8)):
            ws = torch.empty(getattr(_lib.lib(), ws_entry)(a.B, kc), dtype=torch.uint8, device=dev)
            vals = torch.empty((a.B, k), dtype=torch.float32, device=dev)
            out = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            mt = torch.empty((a.B, k), dtype=torch.int32, device=dev)
            raw = lambda entry=entry, qf=qf, gf=gf, ws=ws, vals=vals, out=out, mt=mt: ops._call(
                entry, ops._ptr(qf), a.n, ops._ptr(idx), a.B, kc, ops._ptr(gf), a.n, a.l, a.N, 0, a.min_sim, k, ops._ptr(vals),
                ops._ptr(out), ops._ptr(mt), null, null, null, null, ops._ptr(ws), ws.numel(), ops._stream())
            call = lambda op=op, qf=qf, gf=gf, ws=ws: op(qf, idx, gf, 0, k, a.min_sim, ws)
            forms.append((raw, call))
        (raw16, hip16), (raw8, hip8) = forms
        i16, i8 = hip16()[1], hip8()[1]
        assert bool((i16[:, 0] == idx[:, 0]).all()) and bool((i8[:, 0] == idx[:, 0]).all())     # the planted image comes back first
        agree1, agreek = float((i16[:, 0] == i8[:, 0]).float().mean()), float((i16 == i8).float().mean())
        us16, us8, quant_us = events([hip16, hip8, lambda: ops.quantize_patch_fp8(q16)], a.iters)
        chain16, chain8 = graph_chain([raw16] * 10, a.iters), graph_chain([raw8] * 10, a.iters)
        flop, elems = 2.0 * a.B * kc * a.n * a.n * a.l, float(a.B * kc * a.n * a.l)
        lines.append("%4d %9.1f %9.1f %11.1f %10.1f %9.3f %8.1f %7.1f %9.4f %8.4f %10.4f %9.4f %8.4f %8.4f %9.1f" % (
            kc, us16, us8, chain16, chain8, chain8 / chain16, 2 * elems / 1e6, elems / 1e6, 2 * elems / (chain16 * 1e-6) / HBM_PEAK,
            elems / (chain8 * 1e-6) / HBM_PEAK, flop / (chain16 * 1e-6) / MFMA_PEAK_BF16, flop / (chain8 * 1e-6) / MFMA_PEAK_FP8,
            agree1, agreek, quant_us))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
