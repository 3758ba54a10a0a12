"""Denoising-loop speed of `pipeline` per scheduler / guidance, graphed loop against the plain loop (`use_graph=False`).

    python tools/denoise_bench.py                 # every leg
    python tools/denoise_bench.py --legs A,B,E    # a subset
    python tools/denoise_bench.py --runs ddpm:50,dpm:50,ddim:50,dpm:25,dpm:20 --batch 1,8    # chosen scheduler:steps pairs

Legs (one MI355X, real SD-2.1 / SDXL dimensions, random-init weights, prompt embeddings of 64 / 196 dream queries):
  A  control: DDIM eta 0, CFG 7.5, 50 steps, B_img 1 and 8  (the original graphed path, `dllm_cfg_ddim_step`)
  B  the reference's default: DDPM, CFG 7.5 and 3.5, 50 steps, generator=None, B_img 1 and 8
  C  the COCO eval recipe: DDPM, CFG 2.0, 150 steps, B 24 at 512 px (also images/s)
  D  SDXL (projects/dreamllm_sdxl/inf.py): DDPM, guidance_scale 0.0 (no CFG), 100 steps, 1024 px, B_img 1
  E  DDIM, CFG 7.5 + guidance_rescale 0.7, 50 steps, B_img 1
--runs replaces the legs by leg "R": SD-2.1 at 512 px, CFG 7.5 (--guidance), a seeded generator, one configuration per
scheduler:steps pair and batch size; schedulers: ddpm, ddim, dpm (DPM-Solver++ 2M, graph mode "multistep"), dpm-sde.  It times a
sampler at the step count it is run at beside another (DPM at 20 or 25 steps beside DDIM at 50): step counts, not image quality.
Per configuration: one warm-up call of each loop (graph capture), then graph and plain loop alternate, median of --reps whole
loops each.  Prints one JSON line per configuration: steps/s and ms/step of both loops, and the rel-L2 between their final
latents on the same seed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
BF = torch.bfloat16


def _heads(need_sd21, need_sdxl):
    from dreamllm_amd.modeling_plugins import StableDiffusionHead
    from dreamllm_amd.modeling_plugins_sdxl import StableDiffusionXLHead
    torch.manual_seed(0)
    out = {}
    with torch.device(DEV):
        if need_sd21:
            out["sd21"] = StableDiffusionHead("sd21-base", embed_hidden_size=4096).to(DEV, BF).eval()
        if need_sdxl:
            out["sdxl"] = StableDiffusionXLHead("sdxl-base", embed_hidden_size=4096).to(DEV, BF).eval()
    return out


def _configs():
    from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler
    c = []
    for b in (1, 8):
        c.append(dict(leg="A", head="sd21", sched=DDIMScheduler, gs=7.5, phi=0.0, steps=50, B=b, px=512, gen="seed"))
    for gs in (7.5, 3.5):
        for b in (1, 8):
            c.append(dict(leg="B", head="sd21", sched=DDPMScheduler, gs=gs, phi=0.0, steps=50, B=b, px=512, gen="none"))
    c.append(dict(leg="C", head="sd21", sched=DDPMScheduler, gs=2.0, phi=0.0, steps=150, B=24, px=512, gen="none"))
    c.append(dict(leg="D", head="sdxl", sched=DDPMScheduler, gs=0.0, phi=0.0, steps=100, B=1, px=1024, gen="seed"))
    c.append(dict(leg="E", head="sd21", sched=DDIMScheduler, gs=7.5, phi=0.7, steps=50, B=1, px=512, gen="seed"))
    return c


def _scheduler(name):
    from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    if name == "dpm-sde":
        def DPMSolverSDE():
            return DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
        return DPMSolverSDE
    return dict(ddpm=DDPMScheduler, ddim=DDIMScheduler, dpm=DPMSolverMultistepScheduler)[name]


def _run_configs(runs, batches, guidance):
    c = []
    for pair in runs.split(","):
        name, steps = pair.split(":")
        for b in batches:
            c.append(dict(leg="R", head="sd21", sched=_scheduler(name), gs=guidance, phi=0.0, steps=int(steps), B=b, px=512, gen="seed"))
    return c


def _run(head, cfg, use_graph, steps=None):
    nq = 196 if cfg["head"] == "sdxl" else 64
    g = torch.Generator().manual_seed(42)
    pe = (torch.randn(cfg["B"], nq, 4096, generator=g) * 0.5).to(DEV, BF)
    ne = (torch.randn(cfg["B"], nq, 4096, generator=g) * 0.5).to(DEV, BF) if cfg["gs"] > 1.0 else None
    if cfg["gen"] == "none":
        torch.manual_seed(7)
        gen = None
    else:
        gen = torch.Generator().manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = head.pipeline(height=cfg["px"], width=cfg["px"], num_inference_steps=steps or cfg["steps"], guidance_scale=cfg["gs"],
                        guidance_rescale=cfg["phi"], prompt_embeds=pe, negative_prompt_embeds=ne, generator=gen, output_type="latent",
                        scheduler=cfg["sched"](), use_graph=use_graph)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="A,B,C,D,E")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", default=None, help="scheduler:steps pairs (ddpm, ddim, dpm, dpm-sde), e.g. dpm:20,ddim:50; replaces --legs")
    ap.add_argument("--batch", default="1", help="batch sizes of --runs, e.g. 1,8")
    ap.add_argument("--guidance", type=float, default=7.5, help="guidance scale of --runs")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    if a.runs:
        cfgs = _run_configs(a.runs, [int(b) for b in a.batch.split(",")], a.guidance)
    else:
        cfgs = [c for c in _configs() if c["leg"] in legs]
    heads = _heads(any(c["head"] == "sd21" for c in cfgs), any(c["head"] == "sdxl" for c in cfgs))
    from dreamllm_amd.modeling_plugins import graph_denoise_mode
    for cfg in cfgs:
        head = heads[cfg["head"]]
        mode = graph_denoise_mode(True, cfg["sched"](), cfg["gs"], cfg["phi"], 0.0, None, 1, 4)
        for use_graph in (True, False):  # warm-up: graph capture, lazy caches
            _run(head, cfg, use_graph, steps=2)
        t = {True: [], False: []}
        outs = {}
        for _ in range(a.reps):
            for use_graph in (True, False):
                dt, out = _run(head, cfg, use_graph)
                t[use_graph].append(dt)
                outs.setdefault(use_graph, out)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        n = cfg["steps"]
        d = (outs[True].double() - outs[False].double()).norm() / outs[False].double().norm()
        res = dict(leg=cfg["leg"], head=cfg["head"], scheduler=cfg["sched"].__name__, guidance_scale=cfg["gs"],
                   guidance_rescale=cfg["phi"], steps=n, batch_images=cfg["B"], px=cfg["px"], generator=cfg["gen"], graph_mode=mode,
                   graph_steps_s=round(n / med[True], 3), graph_ms_step=round(1e3 * med[True] / n, 3),
                   loop_steps_s=round(n / med[False], 3), loop_ms_step=round(1e3 * med[False] / n, 3),
                   speedup=round(med[False] / med[True], 3), rel_l2_graph_vs_loop=float(d),
                   graph_loop_s=[round(x, 4) for x in t[True]], plain_loop_s=[round(x, 4) for x in t[False]])
        if cfg["leg"] == "C":
            res["graph_images_s"] = round(cfg["B"] / med[True], 4)
            res["loop_images_s"] = round(cfg["B"] / med[False], 4)
        print(json.dumps(res), flush=True)
        del outs
        head._graph_cache = {}
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
