"""The MFMA tile kernels on one MI355X (csrc/gemm_nt.hip, csrc/gemm256.hip, the score kernel of csrc/knn.hip; HIP events on
torch's stream; needs a GPU).  Every number is the per-call time in us of 20 calls captured back to back in one HIP graph,
median over `iters` replays: without the launch gap, which is what a change to a kernel's code can move.
Usage: python scripts/gemm_tiles_bench.py [--iters 200] [--out FILE]
       VPR_AMD_LIBRARY=/path/to/other/libvpr_amd.so python scripts/gemm_tiles_bench.py     (A/B against another build)

Numbers (SALAD on ViT-L tokens: 64 images x 256 patch tokens = 16384 rows, C = 1024, hidden = 512; kNN at D = 8448):
  salad_l1_gemm256          vpr_gemm256_nt_bf16, layer 1 of the score + cluster MLPs: [16384, 1024] x [1024, 1024]^T + bias, ReLU, bf16 out
  salad_l2_group{0,1}       vpr_gemm_nt_group_bf16, the two second layers ([16384, 512] x [64, 512]^T and x [128, 512]^T, f32 out) in
                            one launch, VPR_GEMM_GROUP_VARIANT = 0 (128 x 128 tiles) / 1 (128 x 64 tiles, 3-deep ring: the default)
  salad_mlps_fused          vpr_salad_stage_mlps: layer 1 with both second layers in the tile epilogue (gemm256_fuse2_kernel)
  salad_mlps_unfused        the same stage under VPR_SALAD_VARIANT=1: layer 1 on 256 x 256 tiles + the grouped second layers
  knn_{bf16,fp8}_BxN        the score stage of vpr_knn_topk* (vpr_knn_topk_scores_stage) of B queries against N gallery rows:
                            64 x 100000 the streaming kernel, 150 x 50000 and 320 x 25000 the 128-row tile, 512 x 12500 the
                            256 x 256 tile with split K (one rank of the 8-GPU form of bench config 5); "kernels" names what ran"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.backbone_rows_bench import graph_chain  # noqa: E402

KNN_SHAPES = ((64, 100000), (150, 50000), (320, 25000), (512, 12500))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemm_tiles_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    bf = torch.bfloat16
    rnd = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=g) * std
    B, n, C, hidden, m, l, t = 64, 256, 1024, 512, 64, 128, 256
    M = B * n
    res = {"library": _lib.library_path(), "iters": a.iters, "kernels": {}}

    # ---- SALAD MLPs
    w = ops.SaladWeights(rnd(2 * hidden, C, std=C ** -0.5).to(bf), rnd(2 * hidden, std=0.1),
                         rnd(m, hidden, std=hidden ** -0.5).to(bf), rnd(m, std=0.1), rnd(l, hidden, std=hidden ** -0.5).to(bf), rnd(l, std=0.1),
                         rnd(hidden, C, std=C ** -0.5).to(bf), rnd(hidden, std=0.1), rnd(t, hidden, std=hidden ** -0.5).to(bf), rnd(t, std=0.1))
    x = rnd(M, C).to(bf)
    H = torch.empty((M, 2 * hidden), dtype=bf, device=dev)
    res["salad_l1_gemm256"] = graph_chain(lambda: ops.gemm_nt_bf16(x, w.w1_sc, w.b1_sc, True, tile256=True, out=H), a.iters)
    S, F = torch.empty((M, m), device=dev), torch.empty((M, l), device=dev)
    layer2 = [dict(a=H[:, :hidden], w=w.w2_s, bias=w.b2_s, out=S), dict(a=H[:, hidden:], w=w.w2_c, bias=w.b2_c, out=F)]
    for variant in (0, 1):
        _lib.tuning_set("VPR_GEMM_GROUP_VARIANT", variant)
        res[f"salad_l2_group{variant}"] = graph_chain(lambda: ops.gemm_nt_group_bf16(layer2), a.iters)
    _lib.tuning_set("VPR_GEMM_GROUP_VARIANT", None)
    _, ws, _, _ = ops._salad_setup(w, B, n, dev)
    cw = w.c_struct()
    mlps = lambda: ops._call("vpr_salad_stage_mlps", ops._ptr(x), n * C, B, n, C, ctypes.byref(cw), m, l, t, hidden, ops._ptr(ws),
                             ws.numel(), ops._stream())
    res["salad_mlps_fused"] = graph_chain(mlps, a.iters)
    _lib.tuning_set("VPR_SALAD_VARIANT", 1)
    res["salad_mlps_unfused"] = graph_chain(mlps, a.iters)
    _lib.tuning_set("VPR_SALAD_VARIANT", None)
    del x, H, S, F, ws

    # ---- kNN score stage
    D, k = 8448, 10
    name = _lib.lib().vpr_knn_scores_kernel_name
    gal = torch.nn.functional.normalize(rnd(KNN_SHAPES[0][1], D), dim=1)
    qry = torch.nn.functional.normalize(rnd(KNN_SHAPES[-1][0], D), dim=1)
    for fp8 in (False, True):
        (G, gs), (Q, qs) = (ops.quantize_fp8_rows(gal), ops.quantize_fp8_rows(qry)) if fp8 else ((gal.to(bf), None), (qry.to(bf), None))
        for Bq, N in KNN_SHAPES:
            q, qsc, gv, gsc = Q[:Bq], (qs[:Bq] if fp8 else None), G[:N], (gs[:N] if fp8 else None)
            kws = ops.knn_workspace(Bq, N, D, k, dev)
            stage = lambda: ops._call("vpr_knn_topk_scores_stage", ops._ptr(q), ops._ptr(qsc), ops._ptr(gv), ops._ptr(gsc), int(fp8),
                                      Bq, N, D, k, ops._ptr(kws), kws.numel(), ops._stream())
            key = f"knn_{'fp8' if fp8 else 'bf16'}_{Bq}x{N}"
            res[key] = graph_chain(stage, a.iters)
            res["kernels"][key] = name(int(fp8), Bq, N).decode()
    text = json.dumps({k_: (round(v, 3) if isinstance(v, float) else v) for k_, v in res.items()})
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
