"""Host-side driver of the heads' sampling pipelines (`StableDiffusionHead.pipeline`, `StableDiffusionXLHead.pipeline`): the choice
of loop, the graphed loop (hipGraph replay of the UNet + one fused step kernel per step), the plain per-step loop and the output
tail.  The heads build the conditioning, the scheduler and the initial latents and call `denoise` and `decode_output`; the graph
and time-bias caches live on the head (`head._graph_cache`, `head._time_bias_cache`).  No kernels of its own."""
from __future__ import annotations

import torch

from . import ops
from .utils import randn_tensor


def graph_denoise_mode(use_graph, sched, guidance_scale, guidance_rescale, eta, callback, num_images_per_prompt, in_channels):
    """Which denoising loop `pipeline` runs (both heads; host logic only):
      "ddim"  -- deterministic DDIM + CFG, no rescale, no callback: hipGraph replay + `dllm_cfg_ddim_step` (the original fast path);
      "sched" -- any scheduler with `step_coeffs` (DDPM, DDIM with eta), with or without CFG / rescale / callback: hipGraph replay +
                 `dllm_cfg_sched_step`;
      "multistep" -- a scheduler with `multistep_coeffs` (DPM-Solver++), same freedom: hipGraph replay + `dllm_cfg_dpm_step`, the
                 previous step's data prediction kept in a device buffer;
      None    -- the plain per-step loop (`use_graph=False`, a scheduler with neither `step_coeffs` nor `multistep_coeffs`,
                 num_images_per_prompt != 1, an inpainting-style UNet)."""
    if not (use_graph and num_images_per_prompt == 1 and in_channels == 4):
        return None
    if (guidance_scale > 1.0 and guidance_rescale == 0.0 and eta == 0.0 and hasattr(sched, "step_cfg_fused_")
            and callback is None):
        return "ddim"
    if hasattr(sched, "step_coeffs"):
        return "sched"
    return "multistep" if hasattr(sched, "multistep_coeffs") else None


def predraw_step_noise(shape, coeffs, generator, device):
    """The plain loop's ancestral draws, made ahead of a graphed loop: one `randn_tensor(shape, generator, device, fp32)` (NCHW, as
    `scheduler.step` draws it) per step whose coefficients draw, in step order -> fp32 [n, B, H, W, C] (NHWC) on `device`, or None
    when no step draws.  Seeded CPU generators, lists of generators, `generator=None` (the device's default generator: the UNet
    draws nothing) and `utils.replay_draws` give the plain loop's values bit for bit."""
    n = sum(1 for c in coeffs if c.draws)
    if n == 0:
        return None
    B, C, H, W = shape
    out = torch.empty(n, B, H, W, C, dtype=torch.float32, device=device)
    k = 0
    for c in coeffs:
        if c.draws:
            out[k].copy_(randn_tensor(shape, generator=generator, device=device, dtype=torch.float32).permute(0, 2, 3, 1))
            k += 1
    return out


def _time_bias_table(head, ts_host, n, addk):
    """Everything that depends on the timestep only (sinusoid, time-embedding MLP, every ResBlock's time_emb_proj: ~38 tiny launches
    per step) for ALL steps, one GEMM per ResBlock; the captured forward reads one row of it.  Without micro-conditioning the table
    depends on (schedule, batch) only and is kept across calls."""
    # every parameter the table is computed from -- time-embedding MLP, each ResBlock's time_emb_proj weight AND bias -- with its
    # storage pointer, dtype and device beside identity / version: `module.to()` swaps `.data` without touching either
    def _sig(p):
        return (id(p), p._version, p.data_ptr(), p.dtype, str(p.device))
    w_sig = tuple(_sig(p) for p in head.unet.time_embedding.parameters()) + \
        tuple(_sig(p) for r in head.unet._resnets() for p in r.time_emb_proj.parameters())
    tb_key = (ts_host, n, w_sig)
    tb_cache = getattr(head, "_time_bias_cache", None)
    if addk is None and tb_cache is not None and tb_cache[0] == tb_key:
        return tb_cache[1]
    tb_table = head.unet.precompute_time_bias(list(ts_host), n, addk)
    head._time_bias_cache = (tb_key, tb_table) if addk is None else None
    return tb_table


def _graphed_unet(head, key, ctx_embeds, ctx_now, tb_row, device):
    """The cached entry of `head._graph_cache` for `key` = (B, H, W, ctx shape, has_added_cond, G): one UNet forward captured on
    static NHWC buffers (input, time-bias row, the cross-attention K/V of the conditioning tokens, prediction)."""
    cache = getattr(head, "_graph_cache", None)
    if cache is None:
        cache = head._graph_cache = {}
    ent = cache.get(key)
    if ent is not None:
        return ent
    B, H, W, G = key[0], key[1], key[2], key[-1]
    x_in = torch.zeros(G * B, H, W, 8, dtype=head.dtype, device=device)
    tb_static = tb_row.clone()
    ctx_static = {k: [t.clone() for t in v] for k, v in ctx_now.items()}
    emb_static = ctx_embeds.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside capture (lazy caches, kernel attributes)
        for _ in range(2):
            head.unet(x_in, None, emb_static, context_cache=ctx_static, nhwc_io=True, return_dict=False, time_bias=tb_static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    # capture ON the warm-up stream: the per-(device, stream) buffers of the operators (GroupNorm meeting slots, stream-K
    # workspace, split-K counters) were allocated by the warm-up calls above, outside the capture -- a different capture
    # stream would allocate new ones from the graph's private pool
    with torch.cuda.graph(graph, stream=side):
        pred = head.unet(x_in, None, emb_static, context_cache=ctx_static, nhwc_io=True, return_dict=False, time_bias=tb_static)[0]
    ent = cache[key] = dict(graph=graph, x_in=x_in, tb=tb_static, ctx=ctx_static, pred=pred, stream=side)  # (keeps the stream's handle alive)
    return ent


def _fused_step(mode, sched, timesteps, pred, lat, x_in, shape, guidance_scale, guidance_rescale, eta, generator):
    """`step(i)`: the ONE fused kernel of step i (CFG combine + scheduler update + next UNet input), in place on `lat` and `x_in`.
    mode "ddim": `dllm_cfg_ddim_step`, the schedule from the host floats, no noise and no history.  mode "sched" / "multistep":
    `dllm_cfg_sched_step` / `dllm_cfg_dpm_step` from the scheduler's coefficients, the ancestral noise drawn here, ahead of the
    loop, in the plain loop's order; the multistep history buffer (the previous step's data prediction) is allocated here, per call."""
    if mode == "ddim":
        ts_host = [float(t) for t in timesteps]  # host floats: no per-step device read of the schedule
        return lambda i: sched.step_cfg_fused_(pred, ts_host[i], lat, x_in, guidance_scale)
    if sched.config.prediction_type not in ("epsilon", "v_prediction"):
        raise ValueError(sched.config.prediction_type)
    vpred = sched.config.prediction_type == "v_prediction"
    if mode == "multistep":
        coeffs = [sched.multistep_coeffs(i) for i in range(len(timesteps))]
        hist = torch.empty_like(lat)  # first read on the first second-order step, after the step before has written it
    else:
        coeffs = [sched.step_coeffs(t, eta) for t in timesteps]
    noise = predraw_step_noise(shape, coeffs, generator, lat.device)
    rows = iter(noise if noise is not None else ())
    zs = [next(rows) if c.draws else None for c in coeffs]
    phi = guidance_rescale if guidance_scale > 1.0 else 0.0  # the reference rescales only with CFG (:829)
    if mode == "multistep":
        return lambda i: ops.cfg_dpm_step_(pred, lat, hist, zs[i], x_in, guidance_scale, phi, coeffs[i], vpred)
    return lambda i: ops.cfg_sched_step_(pred, lat, zs[i], x_in, guidance_scale, phi, coeffs[i], vpred)


def _graph_loop(head, mode, latents, ctx_embeds, sched, guidance_scale, guidance_rescale, eta, generator, callback, callback_steps,
                added_cond_kwargs):
    """The loop body (modeling_plugins.py:809-839) as: [copy the step's time-bias row] -> hipGraph replay of one UNet forward on
    static NHWC buffers -> ONE fused kernel (`_fused_step`) -> `callback(i, t, latents)` as the plain loop.  ~600 kernel launches per
    step collapse into one graph launch, which is what the loop is bound by at B_img = 1.  The graph is cached per shape and CFG
    factor G (G = 1 without CFG: the UNet captured at batch B) and is the same one for every mode (see `graph_denoise_mode`)."""
    B, C, H, W = latents.shape
    G = 2 if (mode == "ddim" or guidance_scale > 1.0) else 1
    dev = latents.device
    timesteps = sched.timesteps.tolist()
    ctx_now = head.unet.prepare_context(ctx_embeds)
    addk = None if added_cond_kwargs is None else {k: v.to(dev) for k, v in added_cond_kwargs.items()}
    # ONE host conversion of the schedule (a device tensor would cost a sync per element)
    tb_table = _time_bias_table(head, tuple(float(t) for t in timesteps), G * B, addk)
    ent = _graphed_unet(head, (B, H, W, tuple(ctx_embeds.shape), added_cond_kwargs is not None, G), ctx_embeds, ctx_now, tb_table[0],
                        dev)
    for k, v in ctx_now.items():
        for dst, src in zip(ent["ctx"][k], v):
            dst.copy_(src)
    lat = latents.permute(0, 2, 3, 1).contiguous().float()  # NHWC fp32 master copy
    x_in = ent["x_in"]
    x_in.zero_()
    for g in range(G):
        x_in[g * B:(g + 1) * B, ..., :4] = lat.to(head.dtype)
    step = _fused_step(mode, sched, timesteps, ent["pred"], lat, x_in, latents.shape, guidance_scale, guidance_rescale, eta, generator)
    for i, t in enumerate(timesteps):
        ent["tb"].copy_(tb_table[i])
        ent["graph"].replay()
        step(i)
        if callback is not None and i % callback_steps == 0:
            callback(i, t, lat.permute(0, 3, 1, 2).contiguous())
    return lat.permute(0, 3, 1, 2).contiguous()


def _plain_loop(head, latents, prompt_embeds, sched, guidance_scale, guidance_rescale, eta, generator, callback, callback_steps,
                added_cond_kwargs):
    """The reference's per-step loop (modeling_plugins.py:809-839; dreamllm_sdxl :395-430 with `added_cond_kwargs`)."""
    do_cfg = guidance_scale > 1.0
    ctx = head.unet.prepare_context(prompt_embeds)  # cross-attention K/V of the dream tokens: once, not per step
    for i, t in enumerate(sched.timesteps.tolist()):
        model_in = torch.cat([latents] * 2) if do_cfg else latents
        model_in = sched.scale_model_input(model_in, t)
        noise_pred = head.unet(model_in.to(head.dtype), t, encoder_hidden_states=prompt_embeds, context_cache=ctx,
                               added_cond_kwargs=added_cond_kwargs, return_dict=False)[0].float()
        if do_cfg:
            noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
            noise_pred = noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
            if guidance_rescale > 0.0:
                noise_pred = head._rescale_noise_cfg(noise_pred, noise_pred_text, guidance_rescale=guidance_rescale)
        latents = sched.step(noise_pred, t, latents, eta=eta, generator=generator)
        if callback is not None and i % callback_steps == 0:
            callback(i, t, latents)
    return latents


@torch.no_grad()
def denoise(head, latents, prompt_embeds, sched, *, guidance_scale, guidance_rescale=0.0, eta=0.0, generator=None, callback=None,
            callback_steps=1, num_images_per_prompt=1, use_graph=True, added_cond_kwargs=None):
    """fp32 NCHW `latents` through every timestep of `sched` (after `set_timesteps`) under the projected `prompt_embeds` (with CFG:
    [negative, positive]) and, for SDXL, `added_cond_kwargs` -> the final fp32 NCHW latents."""
    mode = graph_denoise_mode(use_graph, sched, guidance_scale, guidance_rescale, eta, callback, num_images_per_prompt,
                              head.unet.config.in_channels)
    rest = (prompt_embeds, sched, guidance_scale, guidance_rescale, eta, generator, callback, callback_steps, added_cond_kwargs)
    return _plain_loop(head, latents, *rest) if mode is None else _graph_loop(head, mode, latents, *rest)


@torch.no_grad()
def decode_output(head, latents, output_type):
    """The pipelines' tail (modeling_plugins.py:841-850): "latent" as is, else VAE-decode to [0, 1] -> "pt" / "np" / "pil"."""
    if output_type == "latent":
        return latents
    image = head.vae.decode((latents / head.vae.config.scaling_factor).to(head.dtype))
    image = (image.float() / 2 + 0.5).clamp(0, 1)
    if output_type == "pt":
        return image
    image = image.permute(0, 2, 3, 1).cpu().numpy()
    if output_type == "np":
        return image
    import PIL.Image
    return [PIL.Image.fromarray((im * 255).round().astype("uint8")) for im in image]
