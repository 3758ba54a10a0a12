"""`-m gpu`: the graphed denoising loop for every scheduler -- the fused step kernel `dllm_cfg_sched_step` against the plain loop's
arithmetic, the executed-reference goldens that the original graphed loop (deterministic DDIM + CFG only) left to the plain loop,
the DDPM loop at the real SD-2.1 size against an fp32 oracle, callbacks, and the model-level entry points."""
import pytest
import torch
import torch.nn.functional as F

from conftest import bound, check_tensor, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _plain_step(pred_nchw, x, sched, t, eta, guidance, phi, G, z):
    """The plain loop's arithmetic (modeling_plugins.py:824-833) in fp32 torch, NCHW."""
    from dreamllm_amd.modeling_plugins import StableDiffusionHead
    from dreamllm_amd.utils import replay_draws
    e = pred_nchw.float()
    if G == 2:
        eu, ec = e.chunk(2)
        e = eu + guidance * (ec - eu)
        if phi > 0:
            e = StableDiffusionHead._rescale_noise_cfg(None, e, ec, guidance_rescale=phi)
    with replay_draws([("randn", z)] if sched.step_coeffs(t, eta).draws else []):
        return sched.step(e, t, x, eta=eta)


@pytest.mark.parametrize("kind", ["ddpm", "ddim_eta"])
@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("G", [2, 1])
def test_cfg_sched_step_kernel(kind, pred_type, phi, G):
    from dreamllm_amd import ops
    from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler
    sched = (DDPMScheduler if kind == "ddpm" else DDIMScheduler)(prediction_type=pred_type)
    sched.set_timesteps(50)
    eta = 0.5 if kind == "ddim_eta" else 0.0
    for B in (1, 3, 24):
        for S in (8, 64, 128):
            t = sched.timesteps.tolist()[17]
            g = torch.Generator().manual_seed(B * 1000 + S)
            pred = torch.randn(G * B, 4, S, S, generator=g).to(BF)
            x = torch.randn(B, 4, S, S, generator=g)
            z = torch.randn(B, 4, S, S, generator=g)
            ref = _plain_step(pred, x, sched, t, eta, 7.5, phi, G, z)
            c = sched.step_coeffs(t, eta)
            nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().to(DEV)  # noqa: E731
            outs = []
            for _ in range(2):
                lat = nhwc(x)
                nxt = torch.full((G * B, S, S, 8), 3.0, dtype=BF, device=DEV)
                ops.cfg_sched_step_(nhwc(pred), lat, nhwc(z) if c.draws else None, nxt, 7.5, phi, c, pred_type == "v_prediction")
                outs.append((lat, nxt))
            lat, nxt = outs[0]
            err = rel_l2(lat.permute(0, 3, 1, 2), ref)
            assert err <= 1e-5, (B, S, err)
            for gi in range(G):
                half = nxt[gi * B:(gi + 1) * B]
                assert torch.equal(half[..., :4], lat.to(BF)), (B, S, gi)
                assert torch.count_nonzero(half[..., 4:]) == 0
            assert torch.equal(outs[1][0], lat) and torch.equal(outs[1][1], nxt)  # two launches: the same bits


def test_cfg_sched_step_rejects_bad_shapes():
    from dreamllm_amd import ops
    from dreamllm_amd.schedulers import DDPMScheduler
    sched = DDPMScheduler()
    sched.set_timesteps(10)
    c = sched.step_coeffs(sched.timesteps.tolist()[0])
    lat = torch.zeros(2, 8, 8, 4, device=DEV)
    with pytest.raises(ValueError):  # pred is 3 x latents: neither CFG nor no-CFG
        ops.cfg_sched_step_(torch.zeros(6, 8, 8, 4, dtype=BF, device=DEV), lat, torch.zeros_like(lat), None, 7.5, 0.0, c)
    with pytest.raises(ValueError):  # sigma != 0 without noise: the library's DLLM_ERR_SHAPE
        ops.cfg_sched_step_(torch.zeros(4, 8, 8, 4, dtype=BF, device=DEV), lat, None, None, 7.5, 0.0, c)


# ----------------------------------------------------------------------------- executed-reference goldens on the graph
_GRAPH_CASES = ["ddim_10_rescale", "ddim_4_nocfg", "ddpm_10", "ddpm_5_pt_randlat", "ddim_4_vpred_eta"]


def _count_sched_steps(monkeypatch):
    from dreamllm_amd import ops
    calls = []
    real = ops.cfg_sched_step_

    def counted(pred, *a, **k):
        calls.append(pred.shape[0])
        return real(pred, *a, **k)

    monkeypatch.setattr(ops, "cfg_sched_step_", counted)
    return calls


@pytest.mark.parametrize("xl,name", [(xl, n) for xl in (False, True) for n in _GRAPH_CASES])
def test_graph_pipeline_vs_executed_reference(golden, xl, name, monkeypatch):
    """The five pipeline cases of tests/golden/{sd,sdxl}_head.pt that the DDIM-only graphed loop left to the plain loop (rescale,
    no CFG, the head's own DDPM scheduler with a generator, v-prediction with eta > 0) on the graphed loop, same rule as
    test_sd_head_pipeline_vs_executed_reference."""
    from test_diffusion_gpu import _case, _fixture_head
    from dreamllm_amd.modeling_plugins import graph_denoise_mode
    from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler
    from dreamllm_amd.utils import replay_draws
    tag = "sdxl_head" if xl else "sd_head"
    g = golden(tag + ".pt")
    c = _case(g, "pipeline", name)
    kw = dict(c["kwargs"])
    head = _fixture_head(g, xl, prediction_type=c["prediction_type"])
    sched = {"DDIMScheduler": DDIMScheduler, "DDPMScheduler": DDPMScheduler}[c["scheduler"]](prediction_type=c["prediction_type"])
    cfg = kw["guidance_scale"] > 1.0
    assert graph_denoise_mode(True, sched, kw["guidance_scale"], kw["guidance_rescale"], kw["eta"], None, 1, 4) == "sched"
    calls = _count_sched_steps(monkeypatch)
    with replay_draws(c["draws"]):
        out = head.pipeline(latents=None if c["latents"] is None else c["latents"].float().clone(),
                            prompt_embeds=c["prompt_embeds"].to(BF).to(DEV),
                            negative_prompt_embeds=c["negative_prompt_embeds"].to(BF).to(DEV) if cfg else None,
                            generator=torch.Generator().manual_seed(c["gen_seed"]), scheduler=sched, use_graph=True, **kw)
    assert sched.timesteps.tolist() == c["timesteps"]
    # the graphed loop ran: one fused step per timestep on the captured UNet's output, a graph cached for this CFG factor
    B = c["prompt_embeds"].shape[0]
    G = 2 if cfg else 1
    assert calls == [G * B] * c["steps"]
    assert any(k[-1] == G and k[0] == B for k in head._graph_cache)
    ref = c["out"].float()
    check_tensor(f"{tag}.pipeline.{name}.graph", out, ref, rel_l2(c["out_bf16"].float(), ref))


def test_graph_callback_matches_plain_loop(golden):
    """callback(i, t, latents) at the same (i, t) as the plain loop; the latents it receives are copies of the graph's latents
    at that step (the last one is the result, bit for bit)."""
    from test_diffusion_gpu import _case, _fixture_head
    from dreamllm_amd.schedulers import DDPMScheduler
    from dreamllm_amd.utils import replay_draws
    g = golden("sd_head.pt")
    c = _case(g, "pipeline", "ddpm_10")
    kw = dict(c["kwargs"])
    head = _fixture_head(g, False, prediction_type=c["prediction_type"])
    res = {}
    for use_graph in (True, False):
        seen = []
        with replay_draws(c["draws"]):
            out = head.pipeline(latents=c["latents"].float().clone(), prompt_embeds=c["prompt_embeds"].to(BF).to(DEV),
                                negative_prompt_embeds=c["negative_prompt_embeds"].to(BF).to(DEV),
                                generator=torch.Generator().manual_seed(c["gen_seed"]), scheduler=DDPMScheduler(),
                                use_graph=use_graph, callback=lambda i, t, x: seen.append((i, t, x.clone())), callback_steps=3,
                                **kw)
        res[use_graph] = (out, seen)
    (out_g, seen_g), (out_l, seen_l) = res[True], res[False]
    assert [(i, t) for i, t, _ in seen_g] == [(i, t) for i, t, _ in seen_l] == [(i, c["timesteps"][i]) for i in (0, 3, 6, 9)]
    assert all(type(t) is type(tl) for (_, t, _), (_, tl, _) in zip(seen_g, seen_l))
    assert torch.equal(seen_g[-1][2], out_g)
    assert not torch.equal(seen_g[0][2], out_g)
    err_ref = rel_l2(c["out_bf16"].float(), c["out"].float())
    for (_, _, xg), (_, _, xl_) in zip(seen_g, seen_l):
        assert xg.shape == xl_.shape == out_l.shape and xg.dtype == torch.float32
        assert rel_l2(xg, xl_) <= bound(err_ref)


# ----------------------------------------------------------------------------- full size: SD-2.1 at 512 px, DDPM
def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(BF).float()


@pytest.fixture(scope="module")
def sd21():
    from dreamllm_amd.modeling_plugins import StableDiffusionHead
    from oracle import unet_ref
    torch.manual_seed(0)
    with torch.device(DEV):
        head = StableDiffusionHead("sd21-base", embed_hidden_size=4096)
    ucfg = dict(unet_ref.SD21_BASE)
    usd = {k: v.to(BF).float() for k, v in unet_ref.random_state_dict(ucfg, seed=21, device=DEV).items()}
    head.unet.load_state_dict(usd, strict=True)
    pw = _randn(1024, 4096, seed=23, scale=0.02)
    head.projector.projector.weight.data = pw.clone()
    yield dict(head=head.to(DEV, BF), ucfg=ucfg, usd=usd, pw=pw)
    del head
    torch.cuda.empty_cache()


@pytest.mark.parametrize("gen", ["cpu", "none"])
def test_ddpm_graph_full_size_vs_oracle(sd21, gen):
    """SD-2.1 at 512 px, the head's DDPM scheduler, CFG 3.5, 10 steps, 2 images: graph and plain loop each within the contract of
    the fp32 oracle DDPM loop (yard-stick: the same loop with the UNet in bf16), and graph-to-loop below that yard-stick."""
    from ddpm_ref import ddpm_loop
    from dreamllm_amd.schedulers import DDPMScheduler
    from oracle import unet_ref
    h, n, B, s = sd21, 10, 2, 3.5
    pe, ne = _randn(B, 64, 4096, seed=31, scale=0.5), _randn(B, 64, 4096, seed=32, scale=0.5)
    lat0 = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(42)).to(DEV)
    shape = (B, 4, 64, 64)

    def generator():
        if gen == "cpu":
            return torch.Generator().manual_seed(5)
        torch.manual_seed(5)  # generator=None: the default device generator, as the COCO eval recipe after set_seed
        return None

    g0 = generator()
    noises = [(torch.randn(shape, generator=g0).to(DEV) if g0 is not None else torch.randn(shape, device=DEV)) for _ in range(n)]

    def oracle(dtype):
        usd, pw = {k: v.to(dtype) for k, v in h["usd"].items()}, h["pw"].to(dtype)
        with torch.no_grad():
            return ddpm_loop(lambda x, t, ctx: unet_ref.unet_forward(x.to(dtype), torch.tensor([t], device=DEV), ctx, usd, h["ucfg"]),
                             lat0, F.linear(ne.to(dtype), pw), F.linear(pe.to(dtype), pw), n, s, noises)

    ref, yard = oracle(torch.float32), oracle(BF)
    e_ref = rel_l2(yard, ref)
    outs = {}
    for use_graph in (True, False):
        outs[use_graph] = h["head"].pipeline(num_inference_steps=n, guidance_scale=s, latents=lat0.clone(), prompt_embeds=pe.to(BF),
                                             negative_prompt_embeds=ne.to(BF), output_type="latent", generator=generator(),
                                             scheduler=DDPMScheduler(), use_graph=use_graph)
        assert outs[use_graph].shape == shape and outs[use_graph].dtype == torch.float32
        check_tensor(f"fullsize.ddpm_{n}.{gen}.{'graph' if use_graph else 'loop'}", outs[use_graph], ref, e_ref)
    assert rel_l2(outs[True], outs[False]) < e_ref


# ----------------------------------------------------------------------------- model-level entry points
def _ids(B, n, seed):
    return torch.randint(3, 32000, (B, n), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _entry_point(m, monkeypatch, **kw):
    calls = _count_sched_steps(monkeypatch)
    out = {}
    for use_graph in (True, False):
        out[use_graph] = m.stable_diffusion_pipeline(generator=torch.Generator().manual_seed(11), output_type="latent",
                                                     use_graph=use_graph, **kw)
        if use_graph:
            assert len(calls) == kw["num_inference_steps"]  # the graphed loop ran
    assert len(calls) == kw["num_inference_steps"]          # ... and the plain loop did not use it
    return out


def test_model_stable_diffusion_pipeline_takes_the_graph(monkeypatch):
    """`DreamLLMForCausalMLM.stable_diffusion_pipeline` as the reference's callers use it: the head's own DDPM scheduler, CFG 3.5."""
    from dreamllm_amd.factory import TINY, TINY_DIFFUSION, build_dreamllm
    m = build_dreamllm(TINY, device=DEV, dtype=BF, with_clip=False, diffusion=TINY_DIFFUSION, num_dream_queries=8).eval()
    out = _entry_point(m, monkeypatch, prompt_ids=_ids(2, 12, 1), negative_prompt_ids=_ids(2, 12, 2), guidance_scale=3.5,
                       num_inference_steps=8)
    assert out[True].shape == out[False].shape == (2, 4, 16, 16)
    assert rel_l2(out[True], out[False]) < 1e-2


def test_sdxl_model_pipeline_without_cfg_takes_the_graph(monkeypatch):
    """The SDXL model's entry with guidance_scale=0.0 (projects/dreamllm_sdxl/inf.py): no CFG, the UNet captured at batch B."""
    from dreamllm_amd.factory import TINY, build_dreamllm_sdxl
    from oracle import unet_ref
    sd = dict(unet=unet_ref.tiny_config(64, sdxl=True), vae=dict(block_out_channels=(32, 64, 64, 64), layers_per_block=1))
    m = build_dreamllm_sdxl(TINY, device=DEV, dtype=BF, with_clip=False, diffusion=sd, num_dream_queries=8,
                            global_condition_hidden_size=40).eval()
    out = _entry_point(m, monkeypatch, prompt_ids=_ids(1, 12, 3), negative_prompt_ids=None, guidance_scale=0.0, num_inference_steps=6)
    assert any(k[-1] == 1 for k in m.stable_diffusion_head._graph_cache)
    assert rel_l2(out[True], out[False]) < 1e-2
