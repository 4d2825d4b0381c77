"""The backbone's row kernels on one MI355X (csrc/backbone_rows.h: LayerNorm row pass, skinny GEMM, the fused launch; HIP
events on torch's stream; needs a GPU).  Every number is the per-call time in us of 20 calls captured back to back in one HIP
graph, median over `iters` replays: without the launch gap, which is what a change to a kernel's code can move.
Usage: python scripts/backbone_rows_bench.py [--iters 200] [--out FILE]
       VPR_AMD_LIBRARY=/path/to/other/libvpr_amd.so python scripts/backbone_rows_bench.py     (A/B against another build)

Numbers (ViT-L sizes: C = 1024, 64 images of 257 tokens = 16448 rows, 64 cls rows):
  ln_{plain,add,bias}_{16448,64}    vpr_layernorm_bf16 / vpr_add_layernorm_bf16 / vpr_bias_layernorm_bf16 on [M, 1024], bf16 parameters
  skinny_{qkv,proj,fc1,fc2}         vpr_skinny_linear_bf16 on the 64 cls rows as the backbone calls it: qkv (N, K) = (3072, 1024)
                                    mode 0 (bias), proj (1024, 1024) mode 2 (accumulate), fc1 (4096, 1024) mode 1 (bias + tanh-GELU),
                                    fc2 (1024, 4096) mode 2
  fused_{qkv,fc1}                   vpr_bias_layernorm_cls_linear_bf16 on [16448 + 64, 1024] with the 64 cls rows' qkv (N = 3072) /
                                    fc1 (N = 4096, GELU) linear in the same launch"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def graph_chain(fn, iters, reps=20):
    """Per-call time (us) of `reps` calls of fn captured back to back in one HIP graph (median over `iters` replays)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(reps):
            fn()
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record(); graph.replay(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("backbone_rows_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    bf = torch.bfloat16
    rnd = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=g) * std
    C, Mp, B, eps = 1024, 16448, 64, 1e-6
    gamma, beta, pb = (1 + 0.2 * rnd(C)).to(bf), (0.1 * rnd(C)).to(bf), rnd(C, std=0.5)
    res = {"library": _lib.library_path(), "iters": a.iters}
    for M in (Mp, B):
        x, r = rnd(M, C).to(bf), rnd(M, C, std=0.5).to(bf)
        res[f"ln_plain_{M}"] = graph_chain(lambda: ops.layernorm_bf16(x, gamma, beta, eps), a.iters)
        res[f"ln_add_{M}"] = graph_chain(lambda: ops.add_layernorm_bf16(x, r, gamma, beta, eps), a.iters)
        res[f"ln_bias_{M}"] = graph_chain(lambda: ops.bias_layernorm_bf16(x, pb, gamma, beta, eps), a.iters)
    w = {}
    for name, N, K, mode in (("qkv", 3072, 1024, 0), ("proj", 1024, 1024, 2), ("fc1", 4096, 1024, 1), ("fc2", 1024, 4096, 2)):
        inp, w[name] = rnd(B, K).to(bf), rnd(N, K, std=0.02).to(bf)
        bias, out = (None if mode == 2 else rnd(N).to(bf)), rnd(B, N).to(bf)
        res[f"skinny_{name}"] = graph_chain(lambda: ops.skinny_linear_bf16(inp, w[name], bias, out, mode), a.iters)
    x = rnd(Mp + B, C).to(bf)
    rs = torch.empty((C // 16, B, 2), dtype=torch.float32, device=dev)
    ops.skinny_linear_bf16(rnd(B, 64).to(bf), torch.zeros(C, 64, dtype=bf, device=dev), None, x[Mp:], 2, pb, rs)   # the cls rows' partials
    for name, gelu in (("qkv", False), ("fc1", True)):
        N = w[name].shape[0]
        consts = ops.ClsLinearConsts.build(w[name], rnd(N).to(bf), gamma, beta, pb)
        out = torch.empty((B, N), dtype=bf, device=dev)
        res[f"fused_{name}"] = graph_chain(
            lambda: ops.bias_layernorm_cls_linear_bf16(x, pb, gamma, beta, eps, Mp, rs, consts, out, gelu=gelu), a.iters)
    text = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
