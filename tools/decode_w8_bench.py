#!/usr/bin/env python
"""FP8 weight-only decoding against the bf16 token step on the 7B decoder alone (synthetic Vicuna-7B weights, no plugins).

    python tools/decode_w8_bench.py [new_tokens=64] [ctx=514] [reps=3]

For batch 1 and batch 8, in one process: the legs bf16 / fp8 / bf16, each on its own warmed-up session (prefill + captured graph),
`reps` timed runs of `new_tokens` graph replays per leg, median per leg.  Reported per leg: tokens/s, ms per token step and the
weight-stream rate (the bytes a token step must read -- decoder Linear weights in the leg's format + scales + norms + the bf16 lm_head
-- over the step time).  The verdict at batch 1: fp8 beats BOTH bf16 legs by more than twice the spread between them.

Then the four GEMV launches of a layer on their own, bf16 and fp8: 32 launches per graph, one per layer (so every launch streams
its weights from HBM: the 32 layers' copies of a matrix are 0.5 - 5.8 GB, far beyond the 256 MB of infinity cache), median of 5
timed replays of that graph, per launch."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreamllm_amd import ops  # noqa: E402
from dreamllm_amd.decode import DecodeWeightsFP8, GreedyDecodeSession  # noqa: E402
from dreamllm_amd.factory import VICUNA_7B, build_dreamllm  # noqa: E402

NEW = int(sys.argv[1]) if len(sys.argv) > 1 else 64
CTX = int(sys.argv[2]) if len(sys.argv) > 2 else 514
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3

if not torch.cuda.is_available():
    sys.exit("decode_w8_bench: needs the GPU (no CPU fallback, no CPU timing)")

model = build_dreamllm(VICUNA_7B, device="cuda", with_clip=False, with_sd=False).eval()
t0 = time.perf_counter()
weights = DecodeWeightsFP8.from_model(model)
torch.cuda.synchronize()
print(f"quantised {len(weights.layers)} layers in {time.perf_counter() - t0:.1f} s: {weights.nbytes() / 1e9:.2f} GB of codes and scales "
      f"next to the bf16 weights", flush=True)

layer_bf16 = sum(p.numel() * 2 for n, p in model.named_parameters() if n.startswith("model.layers") and "layernorm" not in n)
rest = sum(p.numel() * 2 for n, p in model.named_parameters() if n.startswith("lm_head") or n == "model.norm.weight" or "layernorm" in n)
BYTES = {"bf16": layer_bf16 + rest, "fp8": weights.nbytes() + rest}
print(f"bytes per token step: bf16 {BYTES['bf16'] / 1e9:.2f} GB, fp8 {BYTES['fp8'] / 1e9:.2f} GB (lm_head, norms: {rest / 1e9:.2f} GB bf16 in both)",
      flush=True)


def median(v):
    return sorted(v)[len(v) // 2]


result = {"new_tokens": NEW, "ctx": CTX}
for B in (1, 8):
    ids = torch.randint(3, 32000, (B, CTX), device="cuda")
    sess = {"bf16": GreedyDecodeSession(model, B, CTX + NEW + 16), "fp8": GreedyDecodeSession(model, B, CTX + NEW + 16, weights=weights)}
    for s_ in sess.values():  # warm-up: code objects, graph capture
        s_.prefill(ids)
        s_.generate(4)
    legs = []
    for kind in ("bf16", "fp8", "bf16"):
        ts = []
        for _ in range(REPS):
            sess[kind].prefill(ids)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sess[kind].generate(NEW)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / NEW)
        t = median(ts)
        legs.append((kind, t))
        print(f"batch {B} leg {len(legs)} [{kind}]: {B / t:.1f} tok/s, {t * 1e3:.3f} ms/step, weight stream {BYTES[kind] / t / 1e9:.0f} GB/s "
              f"({BYTES[kind] / t / 8e12 * 100:.1f} % of 8 TB/s), runs {[round(x * 1e3, 3) for x in ts]}", flush=True)
    a, f, b = legs[0][1], legs[1][1], legs[2][1]
    spread = abs(a - b)
    gain = min(a, b) - f
    ok = gain > 2 * spread
    print(f"batch {B}: bf16 legs {a * 1e3:.3f} / {b * 1e3:.3f} ms (spread {spread * 1e3:.3f} ms), fp8 {f * 1e3:.3f} ms: "
          f"{min(a, b) / f:.3f} x the faster bf16 leg, gain {gain * 1e3:.3f} ms {'>' if ok else '<='} 2 x spread", flush=True)
    result[f"b{B}"] = {"bf16_ms": [a * 1e3, b * 1e3], "fp8_ms": f * 1e3, "speedup": min(a, b) / f, "beats_2x_spread": ok,
                       "bf16_tok_s": B / min(a, b), "fp8_tok_s": B / f, "bf16_GBps": BYTES["bf16"] / min(a, b) / 1e9,
                       "fp8_GBps": BYTES["fp8"] / f / 1e9}
    del sess

# ---- the four GEMV launches of a layer on their own ------------------------------------------------------------------------------
cfg = model.config
d, F = cfg.hidden_size, cfg.intermediate_size
eps = cfg.rms_norm_eps
L = len(weights.layers)


def launch_table(B):
    x = torch.randn(B, d, device="cuda").bfloat16()
    a = torch.randn(B, F, device="cuda").bfloat16()
    layers = model.model.layers
    return {
        "q|k|v": (3 * d * d,
                  lambda i: ops.gemv_fused(x, (layers[i].self_attn.q_proj.weight, layers[i].self_attn.k_proj.weight,
                                               layers[i].self_attn.v_proj.weight), norm_w=layers[i].input_layernorm.weight, eps=eps),
                  lambda i: ops.gemv_fused_w8(x, weights.layers[i]["qkv_parts"], weights.layers[i]["qkv_scale_parts"],
                                              norm_w=layers[i].input_layernorm.weight, eps=eps)),
        "o": (d * d,
              lambda i: ops.gemv(x, layers[i].self_attn.o_proj.weight, residual=x),
              lambda i: ops.gemv_w8(x, weights.layers[i]["o"], weights.layers[i]["o_scale"], residual=x)),
        "gate|up": (2 * d * F,
                    lambda i: ops.gemv_fused(x, (layers[i].mlp.gate_proj.weight, layers[i].mlp.up_proj.weight),
                                             norm_w=layers[i].post_attention_layernorm.weight, eps=eps, swiglu=True),
                    lambda i: ops.gemv_fused_w8(x, (weights.layers[i]["gate"], weights.layers[i]["up"]),
                                                (weights.layers[i]["gate_scale"], weights.layers[i]["up_scale"]),
                                                norm_w=layers[i].post_attention_layernorm.weight, eps=eps, swiglu=True)),
        "down": (d * F,
                 lambda i: ops.gemv(a, layers[i].mlp.down_proj.weight, residual=x),
                 lambda i: ops.gemv_w8(a, weights.layers[i]["down"], weights.layers[i]["down_scale"], residual=x)),
    }


def time_graph(fn):
    for i in range(L):
        fn(i)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(L):
            fn(i)
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(4):
            graph.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / (4 * L))
    return median(ts)


for B in (1, 8):
    for name, (elems, f_bf16, f_fp8) in launch_table(B).items():
        tb, tf, tb2 = time_graph(f_bf16), time_graph(f_fp8), time_graph(f_bf16)
        print(f"batch {B} launch {name:8s}: bf16 {tb * 1e6:6.1f} / {tb2 * 1e6:6.1f} us ({elems * 2 / min(tb, tb2) / 1e9:5.0f} GB/s), "
              f"fp8 {tf * 1e6:6.1f} us ({elems / tf / 1e9:5.0f} GB/s), {min(tb, tb2) / tf:.2f} x", flush=True)
        result[f"b{B}_{name}_us"] = {"bf16": [tb * 1e6, tb2 * 1e6], "fp8": tf * 1e6}
print(json.dumps(result))
