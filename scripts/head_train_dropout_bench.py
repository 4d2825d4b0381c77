"""Cost of dropout in the head-only training step: vpr_head_train_epoch (p = 0) against vpr_head_train_epoch_dropout
(p = 0.3, the _2 scripts' Dropout: dinov2salad_finetuning_2.py:113-122, swin_attempt_2.py:114-123) at the reference's shape
(D = 8448, hidden = 512, n_out = 2, B = 16).  The two are timed alternately, one 64-batch epoch call per sample, so drift on
the box falls on both; prints one JSON line with the per-step medians and spreads (device events)."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vpr_amd import ops

dev = torch.device("cuda:0")
D, hidden, n_out, B, N = 8448, 512, 2, 16, 1024
g = torch.Generator(device=dev).manual_seed(0)
X = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
Y = torch.randn(N, n_out, device=dev, generator=g)
order = torch.randperm(N, device=dev, generator=g).to(torch.int32)
nb = N // B
state = {}
for p in (0.0, 0.3):
    W = [torch.randn(hidden, D, device=dev, generator=g) * 0.01, torch.zeros(hidden, device=dev),
         torch.randn(n_out, hidden, device=dev, generator=g) * 0.04, torch.zeros(n_out, device=dev)]
    state[p] = [W, *ops.head_train_state(W[0], W[2]), 1]


def epoch(p):
    W, m, v, step = state[p]
    ops.head_train_epoch(X, Y, order, B, *W, m, v, step, dropout_p=p, dropout_seed=7)
    state[p][3] = step + nb


def timed(p):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    epoch(p)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / nb


for p in state:
    for _ in range(3):
        epoch(p)
torch.cuda.synchronize()
samples = {p: [] for p in state}
for _ in range(40):
    for p in state:
        samples[p].append(timed(p))
med = {p: float(torch.tensor(s).median()) for p, s in samples.items()}
row = {"shape": f"D={D} hidden={hidden} n_out={n_out} B={B}", "samples_per_p": 40, "steps_per_sample": nb,
       "p0_us_per_step_median": round(med[0.0], 2), "p0_us_per_step_min_max": [round(min(samples[0.0]), 2), round(max(samples[0.0]), 2)],
       "p03_us_per_step_median": round(med[0.3], 2), "p03_us_per_step_min_max": [round(min(samples[0.3]), 2), round(max(samples[0.3]), 2)],
       "dropout_cost_us_per_step": round(med[0.3] - med[0.0], 2)}
print(json.dumps(row), flush=True)
