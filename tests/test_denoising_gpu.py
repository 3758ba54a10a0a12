"""`-m gpu`: properties of the heads' sampling pipelines that hold across samplers and across both heads, on the tiny SD and SDXL
heads of the executed-reference fixtures: one captured UNet graph serves every graphed mode without carrying state from one mode to
the next, the deterministic DDIM mode draws nothing inside the loop, and every `output_type` is the same tail of the same latents."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
B, QUERIES = 2, 8


def _head(golden, xl):
    from test_diffusion_gpu import _fixture_head
    g = golden(("sdxl_head" if xl else "sd_head") + ".pt")
    return _fixture_head(g, xl), g["embed"]


def _run(head, embed, sched, steps, seed=7, **kw):
    """B = 2 prompts of 8 dream queries, latents drawn from a seeded CPU generator at the UNet's own (tiny) sample size."""
    g = torch.Generator().manual_seed(3)
    pe, ne = ((torch.randn(B, QUERIES, embed, generator=g) * 0.5).to(BF).to(DEV) for _ in range(2))
    kw = dict(dict(guidance_scale=7.5, output_type="latent"), **kw)
    return head.pipeline(num_inference_steps=steps, prompt_embeds=pe, negative_prompt_embeds=ne,
                         generator=torch.Generator().manual_seed(seed), scheduler=sched, **kw)


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_one_captured_graph_serves_every_mode(golden, xl):
    """3 steps each of "ddim", "sched" (DDPM, CFG 7.5) and "multistep" on one head: one cache entry, the same graph and input
    buffer throughout, and each result bit for bit that of a head which has run nothing else (copies made before the first call)."""
    from dreamllm_amd.modeling_plugins import graph_denoise_mode
    from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    head, embed = _head(golden, xl)
    modes = [("ddim", DDIMScheduler), ("sched", DDPMScheduler), ("multistep", DPMSolverMultistepScheduler)]
    fresh = [copy.deepcopy(head) for _ in modes]
    graph = x_in = None
    for (mode, new), other in zip(modes, fresh):
        assert graph_denoise_mode(True, new(), 7.5, 0.0, 0.0, None, 1, 4) == mode
        out = _run(head, embed, new(), 3)
        assert len(head._graph_cache) == 1
        (ent,) = head._graph_cache.values()
        if graph is None:
            graph, x_in = ent["graph"], ent["x_in"]
        assert ent["graph"] is graph and ent["x_in"] is x_in
        assert torch.isfinite(out).all()
        assert torch.equal(out, _run(other, embed, new(), 3)), mode


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_ddim_mode_draws_nothing_in_the_loop(golden, xl):
    """DDIM eta = 0 with CFG: the generator is left where the single draw of `prepare_latents` leaves it."""
    from dreamllm_amd.modeling_plugins import graph_denoise_mode
    from dreamllm_amd.schedulers import DDIMScheduler
    from dreamllm_amd.utils import randn_tensor
    head, embed = _head(golden, xl)
    assert graph_denoise_mode(True, DDIMScheduler(), 7.5, 0.0, 0.0, None, 1, 4) == "ddim"
    g = torch.Generator().manual_seed(7)
    pe, ne = (torch.zeros(B, QUERIES, embed, dtype=BF, device=DEV) for _ in range(2))
    out = head.pipeline(num_inference_steps=3, guidance_scale=7.5, eta=0.0, prompt_embeds=pe, negative_prompt_embeds=ne, generator=g,
                        scheduler=DDIMScheduler(), output_type="latent")
    g2 = torch.Generator().manual_seed(7)
    randn_tensor(tuple(out.shape), generator=g2, device=torch.device(DEV), dtype=torch.float32)
    assert torch.equal(g.get_state(), g2.get_state())
    assert not torch.equal(g.get_state(), torch.Generator().manual_seed(7).get_state())


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_both_heads_share_one_output_tail(golden, xl):
    """2 steps, one seed: "pt" is the decoded latent mapped to [0, 1], "np" is "pt" channels-last on the host, "pil" is "np" rounded
    to bytes -- all exact."""
    from dreamllm_amd.schedulers import DDIMScheduler
    head, embed = _head(golden, xl)
    lat, pt, arr, pil = (_run(head, embed, DDIMScheduler(), 2, output_type=t) for t in ("latent", "pt", "np", "pil"))
    with torch.no_grad():
        want = (head.vae.decode((lat / head.vae.config.scaling_factor).to(head.dtype)).float() / 2 + 0.5).clamp(0, 1)
    assert pt.shape[0] == B and pt.dtype == torch.float32 and torch.equal(pt, want)
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, pt.permute(0, 2, 3, 1).cpu().numpy())
    assert isinstance(pil, list) and len(pil) == B
    for im, a in zip(pil, arr):
        assert np.array_equal(np.asarray(im), (a * 255).round().astype("uint8"))
