#!/usr/bin/env python
"""Batch-1 greedy decode of the 7B decoder alone (no plugins): tokens/s and the weight-stream rate; run under
`rocprofv3 --kernel-trace --stats` for the per-kernel table of a token step.   python tools/decode_bench.py [new_tokens=64] [ctx=514] [mode]
`sample`: greedy against sampled sessions (`SampledDecodeSession`: the VQA setting T 0.2 / top-k 50 and the language-eval setting
T 0.8 / top-p 0.95), interleaved in one process, at batch 1 and 8.
`beam`: beam search at the VQA shape (`BeamDecodeSession`, batch 1 x 5 beams, a 320-token prompt = 256 image patches + text; run as
`decode_bench.py 0 320 beam`) against a greedy session of batch 5 at the same context, for 256 and 1024 new tokens, interleaved in one
process; then the beam-step kernel alone (64 launches in one graph, with the row-map update at a 1344-slot context)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreamllm_amd.decode import BeamDecodeSession, GreedyDecodeSession, SampledDecodeSession  # noqa: E402
from dreamllm_amd.factory import VICUNA_7B, build_dreamllm  # noqa: E402

NEW = int(sys.argv[1]) if len(sys.argv) > 1 else 64
CTX = int(sys.argv[2]) if len(sys.argv) > 2 else 514
model = build_dreamllm(VICUNA_7B, device="cuda", with_clip=False, with_sd=False).eval()
ids = torch.randint(3, 32000, (1, CTX), device="cuda")
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
if len(sys.argv) > 3 and sys.argv[3] == "beam":
    from dreamllm_amd import ops
    B, NB = 1, 5
    idsb = torch.randint(3, 32000, (B, CTX), device="cuda")
    ids5 = idsb.expand(B * NB, CTX).contiguous()
    for new in (256, 1024):
        sess = {"greedy batch 5": GreedyDecodeSession(model, B * NB, CTX + new + 2, vocab_limit=None),
                "beam 1 x 5": BeamDecodeSession(model, B, NB, CTX + new + 2, eos=None, max_new=new)}
        for name, s_ in sess.items():
            s_.prefill(ids5 if name.startswith("greedy") else idsb)
            s_.generate(4)
        ts = {k: [] for k in sess}
        for _ in range(3):
            for name, s_ in sess.items():
                s_.prefill(ids5 if name.startswith("greedy") else idsb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s_.generate(new - 1)
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) / (new - 1))
        g = sorted(ts["greedy batch 5"])[1]
        for name, v in ts.items():
            t = sorted(v)[1]
            print(f"ctx {CTX} + {new} new [{name}]: {1 / t:.1f} steps/s ({t * 1e3:.3f} ms/step), {g / t:.4f} x greedy batch 5, "
                  f"runs {[round(x * 1e3, 3) for x in v]}", flush=True)
        del sess
    V, C = model.config.vocab_size, CTX + 1024
    logits = torch.randn(B * NB, V, device="cuda") * 4
    state = ops.BeamState(B, NB, 8, "cuda")
    kv_len = torch.full((B * NB,), C - 1, dtype=torch.int32, device="cuda")
    row_map = torch.zeros(B * NB, C, dtype=torch.int32, device="cuda")
    for use_map in (False, True):
        kw = dict(kv_len=kv_len, row_map=row_map) if use_map else {}
        ops.beam_step(logits, state, eos=2, **kw)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(64):
                ops.beam_step(logits, state, eos=2, **kw)
        graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        t = (time.perf_counter() - t0) / 640
        print(f"beam-step kernel, {B} x {NB} rows, V {V}{', row map of ' + str(C) + ' slots' if use_map else ''}: "
              f"{t * 1e6:.1f} us per launch (64 launches per graph)", flush=True)
        del graph
    sys.exit(0)
wbytes = sum(p.numel() for n, p in model.named_parameters() if n.startswith("model.layers") or n.startswith("lm_head") or n == "model.norm.weight") * 2
sess = GreedyDecodeSession(model, 1, CTX + 2 * NEW + 16)
sess.prefill(ids)
sess.generate(4)
ts = []
for _ in range(3):
    sess.prefill(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.generate(NEW)
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) / NEW)
t = sorted(ts)[1]
print(f"decode: {1 / t:.1f} tok/s, {t * 1e3:.3f} ms/token, weight stream {wbytes / t / 1e9:.0f} GB/s ({wbytes / t / 8e12 * 100:.1f} % of 8 TB/s), runs {[round(x * 1e3, 3) for x in ts]}")
