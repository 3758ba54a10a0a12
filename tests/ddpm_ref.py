"""The reference's denoising loop with its own ancestral scheduler (modeling_plugins.py:768-839 with diffusers 0.24 `DDPMScheduler`,
variance_type fixed_small), restated on oracle.sched_ref: the fp32 / bf16 yard-stick of the graphed DDPM loop at full size."""
import math

import torch

from oracle import sched_ref


def ddpm_step(eps, t, x, n, ac, z, T=1000):
    prev = t - T // n
    a_t, a_p = ac[t], (ac[prev] if prev >= 0 else 1.0)
    beta = 1 - a_t / a_p
    x0 = (x - math.sqrt(1 - a_t) * eps) / math.sqrt(a_t)
    mean = math.sqrt(a_p) * beta / (1 - a_t) * x0 + math.sqrt(a_t / a_p) * (1 - a_p) / (1 - a_t) * x
    if t > 0:
        mean = mean + math.sqrt(max((1 - a_p) / (1 - a_t) * beta, 1e-20)) * z
    return mean


def ddpm_loop(unet_fn, latents, ctx_uncond, ctx_text, n_steps, guidance, noises):
    """CFG + DDPM over the leading timesteps; noises[i]: the NCHW draw of step i.  Returns the final fp32 latents."""
    ac = sched_ref.alphas_cumprod()
    x = latents.float()
    ctx = torch.cat([ctx_uncond, ctx_text])
    for i, t in enumerate(sched_ref.leading_timesteps(n_steps)):
        pred = unet_fn(torch.cat([x, x]), t, ctx).float()
        eu, ec = pred.chunk(2)
        x = ddpm_step(sched_ref.cfg(eu, ec, guidance), t, x, n_steps, ac, noises[i].float())
    return x
