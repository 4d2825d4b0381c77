"""SALAD aggregation at 448 / 518 px on one MI355X (include/vpr_amd_salad_hires.h; HIP events on torch's stream; needs a GPU),
with the timing method of scripts/salad_anyres_bench.py (its events() / graph_chain() / torch_salad()):
(a) the price of the high-resolution stage-A layout — K recomputed from the scores on every pass instead of held in LDS —
    where the other stage-A kernels are defined: n = 256 (all three kernels), 529 and 576 (against the run-time-n kernel);
(b) the whole vpr_salad_aggregate_hires call at n = 1024 and 1369 and where its time goes (T / M / A);
(c) the same aggregation written in PyTorch f32 on the same GPU.
Usage: python scripts/salad_hires_bench.py [--B 64] [--C 1024] [--iters 100] [--out profiles/salad_hires_bench.txt]

Numbers (times in us, medians over `iters`, the forms of one group taking turns within one loop):
  a[n].hires_us / n_us / fixed_us         stage A alone on the same dense scores / feats through vpr_salad_sinkhorn_aggregate_hires,
                                          vpr_salad_sinkhorn_aggregate_n and (n = 256) vpr_salad_sinkhorn_aggregate; events around each call
  a[n].*_chain_us                         the same, 20 calls in one HIP graph, per call: without the launch gap
  a[n].max_abs_diff                       between the hires descriptor and the other kernel's
  b[n].call_us                            the whole vpr_salad_aggregate_hires call, bf16 tokens [B, 1+n, C] in the hub layout
  b[n].stage_t_us                         the token MLP alone (vpr_salad_stage_token: it does not depend on n)
  b[n].stage_a_us / stage_a_chain_us      the high-resolution stage A alone at n on dense inputs
  b[n].stage_m_derived_us                 call_us - stage_t_us - stage_a_us: derived, not measured
  b[n].torch_f32_us                       (c): PyTorch f32 from the same bf16 tokens; max_abs_diff_torch = its distance from the HIP descriptor"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from salad_anyres_bench import events, graph_chain, torch_salad  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("salad_hires_bench: needs a GPU (there is nothing to measure without one)")
    from vpr_amd import _lib, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s, std=1.0: torch.randn(*s, device=dev, generator=g) * std
    B, C, hidden = a.B, a.C, 512
    w32 = dict(w1_sc=rnd(2 * hidden, C, std=0.02), b1_sc=rnd(2 * hidden, std=0.02), w2_s=rnd(64, hidden, std=0.02), b2_s=rnd(64, std=0.02),
               w2_c=rnd(128, hidden, std=0.02), b2_c=rnd(128, std=0.02), w1_t=rnd(hidden, C, std=0.02), b1_t=rnd(hidden, std=0.02),
               w2_t=rnd(256, hidden, std=0.02), b2_t=rnd(256, std=0.02))
    w32 = {k: (v.to(torch.bfloat16).float() if k.startswith("w") else v) for k, v in w32.items()}      # both sides see the same values
    w = ops.SaladWeights(**{k: (v.to(torch.bfloat16).contiguous() if k.startswith("w") else v) for k, v in w32.items()}, dustbin=1.0)
    res = {"library": os.path.basename(_lib.library_path()), "B": B, "C": C, "iters": a.iters, "a": {}, "b": {}}
    tok = rnd(B, 256)
    # (a) stage A alone, every kernel that is defined at n, on the same inputs
    for n in (256, 529, 576):
        s, f = rnd(B, n, 64, std=2.0), rnd(B, n, 128)
        forms = {"hires": lambda s=s, f=f: ops.salad_sinkhorn_aggregate_hires(s, f, tok, 1.0, 3, want_bf16=True),
                 "n": lambda s=s, f=f: ops.salad_sinkhorn_aggregate_n(s, f, tok, 1.0, 3, want_bf16=True)}
        if n == 256:
            forms["fixed"] = lambda s=s, f=f: ops.salad_sinkhorn_aggregate(s, f, tok, 1.0, 3, want_bf16=True)
        r = {"max_abs_diff": max(float((forms["hires"]()[0] - fn()[0]).abs().max()) for k, fn in forms.items() if k != "hires")}
        for k, t in zip(forms, events(list(forms.values()), a.iters)):
            r[k + "_us"] = round(t, 2)
        for k, fn in forms.items():
            r[k + "_chain_us"] = round(graph_chain(fn, a.iters), 2)
        res["a"][str(n)] = r
    # (b) the whole call with its stages, and (c) PyTorch f32
    cls256 = rnd(B, C).to(torch.bfloat16)
    stage_t = lambda: ops.salad_stage_token(cls256, w, 256, ops._raw_stream())
    for n in (1024, 1369):
        tokens = rnd(B, 1 + n, C).to(torch.bfloat16)
        s, f = rnd(B, n, 64, std=2.0), rnd(B, n, 128)
        call = lambda: ops.salad_aggregate_hires(tokens, w, 3, want_bf16=True)
        stage_a = lambda: ops.salad_sinkhorn_aggregate_hires(s, f, tok, 1.0, 3, want_bf16=True)
        torch_f32 = lambda: torch_salad(tokens, w32, 1.0, 3)
        r = {"max_abs_diff_torch": float((call()[0] - torch_f32()).abs().max())}
        r["call_us"], r["stage_t_us"], r["stage_a_us"], r["torch_f32_us"] = (
            round(t, 2) for t in events([call, stage_t, stage_a, torch_f32], max(a.iters // 2, 10)))
        r["stage_a_chain_us"] = round(graph_chain(stage_a, a.iters), 2)
        r["stage_m_derived_us"] = round(r["call_us"] - r["stage_t_us"] - r["stage_a_us"], 2)
        r["torch_f32_over_call"] = round(r["torch_f32_us"] / r["call_us"], 2)
        r["a_bytes"] = B * (n * (64 * (2 + 3) + 128) * 4 + 256 * 4 + 8448 * 6)      # the scores are read on each of the 2 + 3 passes
        res["b"][str(n)] = r
        del tokens, s, f
        torch.cuda.empty_cache()
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
