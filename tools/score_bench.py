#!/usr/bin/env python
"""Scoring of multiple-choice items on the 7B decoder (random weights, no plugins): `loglikelihood()` against the reference-shaped
loop, and the scoring kernel next to the cross-entropy kernel.  Two modes, one process each, every GPU step under its own time limit:

    timeout -k 10 900 python tools/score_bench.py items [n_items=16] && timeout -k 10 300 python tools/score_bench.py kernel

`items`: 4-choice items (context 80 tokens, endings 20-40 tokens, seeded) scored (a) by one `loglikelihood()` call over all choices
and (b) the way the reference's submission scripts do it, built only from the model's plain forward: one `model(ids)` per choice,
`out.logits.cpu().float()`, `torch.log_softmax`, `gather` at rows [-n-1:-1].  Both warmed up, then 5 timed loops each, alternating in
one process; items/s from the median, the spread of (b) as (max - min) / median, and the largest difference of the sums.
`kernel`: `dllm_score_rows` (with lse, rank and four candidates) and `dllm_cross_entropy` (loss only) on the same fp32 rows, R = 128 and
4096 at V = 32000: microseconds per launch from device events around 50 launches, median of 5."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreamllm_amd import ops  # noqa: E402
from dreamllm_amd.factory import VICUNA_7B, build_dreamllm  # noqa: E402

MODE = sys.argv[1] if len(sys.argv) > 1 else "items"
assert torch.cuda.is_available(), "score_bench.py measures on the GPU only"

if MODE == "kernel":
    V = 32000
    for R in (128, 4096):
        g = torch.Generator().manual_seed(R)
        x = (torch.randn(R, V, generator=g) * 4).cuda()
        tg = torch.randint(0, V, (R,), generator=g).cuda()
        runs = {"dllm_score_rows": lambda: ops.score_rows(x, tg, cand_ids=[319, 350, 315, 360], want_lse=True, want_rank=True),
                "dllm_score_rows (logprob / argmax / greedy only)": lambda: ops.score_rows(x, tg),
                "dllm_cross_entropy": lambda: ops.cross_entropy_rows(x, tg)}
        med = {}
        for name, fn in runs.items():
            for _ in range(10):
                fn()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) / 50 * 1e3)
            med[name] = statistics.median(ts)
            print(f"R {R} V {V} [{name}]: {med[name]:.1f} us per launch ({R * V * 4 / med[name] / 1e6:.2f} TB/s of logits), "
                  f"runs {[round(t, 1) for t in ts]}", flush=True)
        print(f"R {R}: dllm_score_rows / dllm_cross_entropy = {med['dllm_score_rows'] / med['dllm_cross_entropy']:.3f}", flush=True)
    sys.exit(0)

N_ITEMS = int(sys.argv[2]) if len(sys.argv) > 2 else 16
model = build_dreamllm(VICUNA_7B, device="cuda", with_clip=False, with_sd=False).eval()
g = torch.Generator().manual_seed(0)
requests = []
for _ in range(N_ITEMS):
    ctx = [1] + torch.randint(3, 32000, (79,), generator=g).tolist()
    for _ in range(4):
        requests.append((ctx, torch.randint(3, 32000, (int(torch.randint(20, 41, (1,), generator=g)),), generator=g).tolist()))


def ours():
    out = model.loglikelihood(requests)
    return out.sum_logprob.cpu()


@torch.no_grad()
def reference_shaped():
    sums = []
    for ctx, cont in requests:
        ids = torch.tensor([ctx + cont], device="cuda")
        logits = model(input_ids=ids).logits.cpu().float()
        n = len(cont)
        lp = torch.log_softmax(logits[0, -n - 1:-1], dim=-1).gather(-1, torch.tensor(cont)[:, None])
        sums.append(lp.sum())
    return torch.stack(sums)


a, b = ours(), reference_shaped()
torch.cuda.synchronize()
print(f"{N_ITEMS} items x 4 choices, {sum(len(c) for _, c in requests)} scored tokens; largest |sum difference| between the two paths "
      f"{float((a - b).abs().max()):.3e} (sums around {float(b.mean()):.1f})", flush=True)
ts = {"loglikelihood": [], "reference-shaped loop": []}
for _ in range(5):
    for name, fn in (("loglikelihood", ours), ("reference-shaped loop", reference_shaped)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts[name].append(time.perf_counter() - t0)
med = {k: statistics.median(v) for k, v in ts.items()}
for name, v in ts.items():
    print(f"[{name}]: {N_ITEMS / med[name]:.1f} items/s ({med[name] * 1e3:.1f} ms per loop, spread {(max(v) - min(v)) / med[name]:.1%}), "
          f"runs {[round(t * 1e3, 1) for t in v]} ms", flush=True)
print(f"loglikelihood / reference-shaped loop = {med['reference-shaped loop'] / med['loglikelihood']:.2f} x", flush=True)
