#!/usr/bin/env python
"""Batch-1 greedy decode of the 7B decoder alone (no plugins): tokens/s and the weight-stream rate; run under
`rocprofv3 --kernel-trace --stats` for the per-kernel table of a token step.   python tools/decode_bench.py [new_tokens=64] [ctx=514] [ab]
`ab`: both session forms in one process, interleaved -- the split-KV partials merged inside the o projection's GEMV (round 6, 5 launches per
layer) against the separate combine launch (6 per layer).
`sample`: greedy against sampled sessions (`SampledDecodeSession`: the VQA setting T 0.2 / top-k 50 and the language-eval setting
T 0.8 / top-p 0.95), interleaved in one process, at batch 1 and 8."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreamllm_amd.decode import GreedyDecodeSession, SampledDecodeSession  # noqa: E402
from dreamllm_amd.factory import VICUNA_7B, build_dreamllm  # noqa: E402

NEW = int(sys.argv[1]) if len(sys.argv) > 1 else 64
CTX = int(sys.argv[2]) if len(sys.argv) > 2 else 514
model = build_dreamllm(VICUNA_7B, device="cuda", with_clip=False, with_sd=False).eval()
ids = torch.randint(3, 32000, (1, CTX), device="cuda")
AB = len(sys.argv) > 3 and sys.argv[3] == "ab"
if len(sys.argv) > 3 and sys.argv[3] == "sample":
    settings = {"greedy": None, "T0.2 top-k 50": (0.2, 50, 1.0), "T0.8 top-p 0.95": (0.8, 0, 0.95)}
    for B in (1, 8):
        idsb = torch.randint(3, 32000, (B, CTX), device="cuda")
        sess = {name: (GreedyDecodeSession(model, B, CTX + NEW + 16) if st is None else
                       SampledDecodeSession(model, B, CTX + NEW + 16, *st)) for name, st in settings.items()}
        for s_ in sess.values():
            s_.prefill(idsb)
            s_.generate(4)
        ts = {k: [] for k in sess}
        for _ in range(5):
            for name, s_ in sess.items():
                s_.prefill(idsb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s_.generate(NEW)
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) / NEW)
        g = sorted(ts["greedy"])[2]
        for name, v in ts.items():
            t = sorted(v)[2]
            print(f"batch {B} [{name}]: {B / t:.1f} tok/s ({1 / t:.1f} steps/s, {t * 1e3:.3f} ms/step), {g / t:.4f} x greedy, "
                  f"runs {[round(x * 1e3, 3) for x in v]}", flush=True)
        del sess
    sys.exit(0)
wbytes = sum(p.numel() for n, p in model.named_parameters() if n.startswith("model.layers") or n.startswith("lm_head") or n == "model.norm.weight") * 2
sessions = {"merged in o-proj" if m else "combine launch": GreedyDecodeSession(model, 1, CTX + 2 * NEW + 16, merge_in_oproj=m)
            for m in ((True, False) if AB else (True,))}
for sess in sessions.values():
    sess.prefill(ids)
    sess.generate(4)
ts = {k: [] for k in sessions}
for _ in range(3):
    for name, sess in sessions.items():
        sess.prefill(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.generate(NEW)
        torch.cuda.synchronize()
        ts[name].append((time.perf_counter() - t0) / NEW)
for name, v in ts.items():
    t = sorted(v)[1]
    print(f"decode [{name}]: {1 / t:.1f} tok/s, {t * 1e3:.3f} ms/token, weight stream {wbytes / t / 1e9:.0f} GB/s ({wbytes / t / 8e12 * 100:.1f} % of 8 TB/s), runs {[round(x * 1e3, 3) for x in v]}")
