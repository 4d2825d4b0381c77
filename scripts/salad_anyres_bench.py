"""SALAD aggregation at other token counts on one MI355X (include/vpr_amd_salad_anyres.h; HIP events on torch's stream; needs a
GPU): (a) what the run-time-n stage-A kernel costs against the fixed n = 256 kernel, (b) the whole vpr_salad_aggregate_n call at
322 px (n = 529) and where its time goes, (c) the same aggregation written in PyTorch f32, which is what a caller would write
without it.
Usage: python scripts/salad_anyres_bench.py [--B 64] [--n 529] [--C 1024] [--iters 200] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/salad_anyres_bench.py --trace
           (a run of its own: the whole call 100 times, nothing timed)
       python scripts/salad_anyres_bench.py --trace-summary OUT      (per-kernel medians of that trace by stage; no GPU needed)

Numbers (times in us, medians over `iters`, the forms of one group taking turns within one loop):
  a_new256_us / a_old256_us       stage A alone at n = 256 on the same dense scores / feats: vpr_salad_sinkhorn_aggregate_n against
                                  vpr_salad_sinkhorn_aggregate, events around each call
  a_new256_chain_us / a_old256_chain_us   the same, 20 calls in one HIP graph, per call: without the launch gap
  a_new_us / a_new_chain_us       the run-time-n kernel at --n
  a_bytes / a_new_GBps            scores + feats + tokfeat read and both outputs written at --n, over a_new_chain_us
  call_us                         the whole vpr_salad_aggregate_n call (token MLP, unfused score / cluster MLPs, stage A), bf16 tokens
                                  [B, 1+n, C] in the hub layout
  call256_us                      ops.salad_aggregate_split at n = 256 and the same B, C (fused MLP kernel): per token, the other side
                                  of the unfused route's cost
  stage_t_us                      the token MLP alone (vpr_salad_stage_token: it does not depend on n)
  stage_m_derived_us              call_us - stage_t_us - a_new_us: derived, not measured; the kernel trace has the measured split
  torch_f32_us                    the same aggregation in PyTorch f32 on this GPU (f32 matmuls, log-domain Sinkhorn, einsum,
                                  F.normalize) from the same bf16 tokens; max_abs_diff_torch = its distance from the HIP descriptor"""
import argparse
import csv
import glob
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = (("T token MLP", ("skinny",)), ("M score / cluster MLPs", ("gemm",)), ("A sinkhorn + aggregation", ("sinkhorn",)))


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
    return events([graph.replay], iters)[0] / reps


def torch_salad(tokens, w, dustbin, iters):
    """What a caller writes today: the published algorithm in PyTorch f32 on the device."""
    x, cls = tokens[:, 1:].float(), tokens[:, 0].float()
    hidden = w["w1_sc"].shape[0] // 2
    H = torch.relu(x @ w["w1_sc"].T + w["b1_sc"])
    S = (H[..., :hidden] @ w["w2_s"].T + w["b2_s"]).transpose(1, 2)           # [B, m, n]
    Fm = (H[..., hidden:] @ w["w2_c"].T + w["b2_c"]).transpose(1, 2)          # [B, l, n]
    g = torch.relu(cls @ w["w1_t"].T + w["b1_t"]) @ w["w2_t"].T + w["b2_t"]
    B, m, n = S.shape
    M = torch.cat([S, S.new_full((B, 1, n), dustbin)], 1)
    norm = -math.log(n + m)
    log_a = S.new_full((B, m + 1), norm)
    log_a[:, -1] += math.log(n - m)
    log_b = S.new_full((B, n), norm)
    u, v = torch.zeros_like(log_a), torch.zeros_like(log_b)
    for _ in range(iters):
        u = log_a - torch.logsumexp(M + v.unsqueeze(1), dim=2)
        v = log_b - torch.logsumexp(M + u.unsqueeze(2), dim=1)
    P = torch.exp(M + u.unsqueeze(2) + v.unsqueeze(1) - norm)[:, :-1]
    V = torch.nn.functional.normalize(torch.einsum("bln,bmn->blm", Fm, P), dim=1)
    return torch.nn.functional.normalize(torch.cat([torch.nn.functional.normalize(g, dim=-1), V.flatten(1)], -1), dim=-1)


def trace_summary(directory):
    """Median duration per kernel name of a rocprofv3 --kernel-trace CSV, grouped by the stage the kernel belongs to."""
    f = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)[0]
    by = {}
    for r in csv.DictReader(open(f)):
        by.setdefault(r["Kernel_Name"][:100], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for stage, keys in STAGES:
        total = 0.0
        for name, d in sorted(by.items()):
            if any(k in name for k in keys):
                d.sort()
                total += d[len(d) // 2]
                print("  %-102s n=%4d median %8.1f us  p10 %8.1f  p90 %8.1f" % (name, len(d), d[len(d) // 2], d[len(d) // 10], d[len(d) * 9 // 10]))
        print("%s: sum of the kernel medians %.1f us" % (stage, total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n", type=int, default=529)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", action="store_true", help="only run the whole call 100 times (for a kernel trace)")
    ap.add_argument("--trace-summary", default="", help="print per-kernel medians of a kernel-trace directory and exit")
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    if not torch.cuda.is_available():
        sys.exit("salad_anyres_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=g) * std
    B, n, C, hidden = a.B, a.n, a.C, 512
    w32 = dict(w1_sc=rnd(2 * hidden, C, std=0.02), b1_sc=rnd(2 * hidden, std=0.02), w2_s=rnd(64, hidden, std=0.02), b2_s=rnd(64, std=0.02),
               w2_c=rnd(128, hidden, std=0.02), b2_c=rnd(128, std=0.02), w1_t=rnd(hidden, C, std=0.02), b1_t=rnd(hidden, std=0.02),
               w2_t=rnd(256, hidden, std=0.02), b2_t=rnd(256, std=0.02))
    w32 = {k: (v.to(torch.bfloat16).float() if k.startswith("w") else v) for k, v in w32.items()}      # both sides see the same values
    w = ops.SaladWeights(**{k: (v.to(torch.bfloat16).contiguous() if k.startswith("w") else v) for k, v in w32.items()}, dustbin=1.0)
    tokens = rnd(B, 1 + n, C).to(torch.bfloat16)
    call = lambda: ops.salad_aggregate_n(tokens, w, 3, want_bf16=True)
    if a.trace:
        for _ in range(100):
            call()
        torch.cuda.synchronize()
        return
    res = {"library": os.path.basename(_lib.library_path()), "B": B, "n": n, "C": C, "iters": a.iters}
    # (a) stage A at n = 256, both kernels on the same inputs, and the run-time-n kernel at n
    s256, f256, t256 = rnd(B, 256, 64, std=2.0), rnd(B, 256, 128), rnd(B, 256)
    sn, fn_ = rnd(B, n, 64, std=2.0), rnd(B, n, 128)
    new256 = lambda: ops.salad_sinkhorn_aggregate_n(s256, f256, t256, 1.0, 3, want_bf16=True)
    old256 = lambda: ops.salad_sinkhorn_aggregate(s256, f256, t256, 1.0, 3, want_bf16=True)
    newn = lambda: ops.salad_sinkhorn_aggregate_n(sn, fn_, t256, 1.0, 3, want_bf16=True)
    res["a_256_max_abs_diff"] = float((new256()[0] - old256()[0]).abs().max())
    res["a_new256_us"], res["a_old256_us"], res["a_new_us"] = (round(t, 2) for t in events([new256, old256, newn], a.iters))
    res["a_new256_chain_us"] = round(graph_chain(new256, a.iters), 2)
    res["a_old256_chain_us"] = round(graph_chain(old256, a.iters), 2)
    res["a_new_chain_us"] = round(graph_chain(newn, a.iters), 2)
    res["a_bytes"] = B * (n * (64 + 128) * 4 + 256 * 4 + 8448 * 6)
    res["a_new_GBps"] = round(res["a_bytes"] / res["a_new_chain_us"] / 1e3, 1)
    # (b) the whole call at n, beside the n = 256 call of the same batch, and (c) PyTorch f32
    tokens256 = rnd(B, 257, C).to(torch.bfloat16)
    patch256, cls256 = tokens256[:, 1:].contiguous(), tokens256[:, 0].contiguous()
    call256 = lambda: ops.salad_aggregate_split(patch256, cls256, w, 3, True)
    stage_t = lambda: ops.salad_stage_token(cls256, w, 256, ops._raw_stream())
    torch_f32 = lambda: torch_salad(tokens, w32, 1.0, 3)
    res["max_abs_diff_torch"] = float((call()[0] - torch_f32()).abs().max())
    res["call_us"], res["call256_us"], res["stage_t_us"], res["torch_f32_us"] = (
        round(t, 2) for t in events([call, call256, stage_t, torch_f32], max(a.iters // 2, 10)))
    res["stage_m_derived_us"] = round(res["call_us"] - res["stage_t_us"] - res["a_new_us"], 2)
    res["torch_f32_over_call"] = round(res["torch_f32_us"] / res["call_us"], 2)
    res["call_over_call256_per_token"] = round(res["call_us"] / n / (res["call256_us"] / 256), 3)
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
