"""Train-mode SALAD cost (B = 64, n = 256, C = 1024): the eval aggregation (salad_aggregate_split) against the training-mode
one (salad_aggregate_train: Dropout in the score / cluster MLPs, Philox masks in the fused MLP epilogue) at p = 0 and 0.3,
interleaved A/B, HIP events on the launch stream, medians; then one full descriptor refresh of a fine-tuning epoch
(TokenCache.train_descriptors) over --images cached images (6378 = the reference's training set).
Prints one JSON line; --out also writes it to a file."""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpr_amd import ops  # noqa: E402
from vpr_amd.finetune import TokenCache  # noqa: E402
from vpr_amd.modules import SaladAggregator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--images", type=int, default=6378)
    ap.add_argument("--refresh-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    agg = SaladAggregator(a.C).to(dev)
    w = agg.pack()
    g = torch.Generator(device=dev).manual_seed(0)
    tok = torch.randn(a.B, 257, a.C, device=dev, generator=g).to(torch.bfloat16)
    patch, cls = tok[:, 1:].contiguous(), tok[:, 0].contiguous()
    calls = {
        "eval_split": lambda: ops.salad_aggregate_split(patch, cls, w, 3, True),
        "train_p0": lambda: ops.salad_aggregate_train((patch, cls), w, 0.0, 1, 0),
        "train_p0.3": lambda: ops.salad_aggregate_train((patch, cls), w, 0.3, 1, 0),
    }
    for fn in calls.values():                    # warm-up: module load, workspaces, fragment copies
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.iters):                     # interleaved: one call of each per round
        for k, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record()
            times[k].append((s, e))
    torch.cuda.synchronize()
    med = {}
    for k, evs in times.items():
        ts = sorted(s.elapsed_time(e) * 1e3 for s, e in evs)
        med[k] = {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1)}
    res = {"B": a.B, "C": a.C, "iters": a.iters, "calls": med,
           "train_over_eval_p0.3": round(med["train_p0.3"]["median_us"] / med["eval_split"]["median_us"], 3),
           "train_over_eval_p0": round(med["train_p0"]["median_us"] / med["eval_split"]["median_us"], 3)}
    del tok, patch, cls

    # one epoch's refresh of every cached descriptor (the tokens are random: the cost does not depend on their values)
    N = a.images
    cache = TokenCache(torch.empty((N, 256, a.C), dtype=torch.bfloat16, device=dev).normal_(generator=g),
                       torch.empty((N, a.C), dtype=torch.bfloat16, device=dev).normal_(generator=g), agg)
    X = torch.empty((N, 8448), dtype=torch.float32, device=dev)
    cache.train_descriptors(X, 7, 0)
    torch.cuda.synchronize()
    ref = []
    for it in range(a.refresh_iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); cache.train_descriptors(X, 7, it + 1); e.record()
        torch.cuda.synchronize()
        ref.append(s.elapsed_time(e))
    ref.sort()
    res["refresh"] = {"images": N, "calls": -(-N // TokenCache.CHUNK), "p": agg.dropout_p(),
                      "median_ms": round(ref[len(ref) // 2], 2), "min_ms": round(ref[0], 2),
                      "token_cache_gb": round((cache.patch.numel() + cache.cls.numel()) * 2 / 1e9, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
