"""`-m gpu`: DPM-Solver++ on the graphed denoising loop -- the fused multistep kernel `dllm_cfg_dpm_step` against the update in fp32
torch and against the plain loop's `step()` over a trajectory, the graphed loop (mode "multistep") against the plain loop on the tiny
SD and SDXL heads under the bound tests/test_denoise_graph_gpu.py holds the "sched" loop to, and one run at the real SD-2.1 size
against the fp32 oracle loop (tests/dpm_ref.py on oracle.unet_ref)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import bound, check_tensor, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (algorithm_type, solver_type, step of a 20-step schedule): first-order (step 0) and second-order steps of both algorithm types
_KINDS = {"det_o1": ("dpmsolver++", "midpoint", 0), "det_o2_midpoint": ("dpmsolver++", "midpoint", 5),
          "det_o2_heun": ("dpmsolver++", "heun", 19), "sde_o1": ("sde-dpmsolver++", "midpoint", 0),
          "sde_o2_midpoint": ("sde-dpmsolver++", "midpoint", 11), "sde_o2_heun": ("sde-dpmsolver++", "heun", 5)}


def _nhwc(a):
    return a.permute(0, 2, 3, 1).contiguous().to(DEV)


def _guided(pred_nchw, guidance, phi, G):
    """The plain loop's CFG combine and rescale (modeling_plugins.py:824-830) in fp32 torch, NCHW."""
    from dreamllm_amd.modeling_plugins import StableDiffusionHead
    e = pred_nchw.float()
    if G == 2:
        eu, ec = e.chunk(2)
        e = eu + guidance * (ec - eu)
        if phi > 0:
            e = StableDiffusionHead._rescale_noise_cfg(None, e, ec, guidance_rescale=phi)
    return e


def _update(c, e, x, m1, z, vpred):
    """The multistep update from its coefficients in fp32 torch: (x_next, m0)."""
    m0 = c.sqrt_at * x - c.sqrt_1mat * e if vpred else (x - c.sqrt_1mat * e) / c.sqrt_at
    out = c.k_x * x + c.k_m0 * m0
    if c.k_m1 != 0.0:
        out = out + c.k_m1 * m1
    if c.sigma != 0.0:
        out = out + c.sigma * z
    return out, m0


def _check_next_in(nxt, lat, G, B, where):
    for gi in range(G):
        half = nxt[gi * B:(gi + 1) * B]
        assert torch.equal(half[..., :4], lat.to(BF)), (where, gi)
        assert torch.count_nonzero(half[..., 4:]) == 0


@pytest.mark.parametrize("kind", sorted(_KINDS))
@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("G", [2, 1])
def test_cfg_dpm_step_kernel(kind, pred_type, phi, G):
    """One launch against the fp32 torch restatement on the same bf16 inputs; bound and shapes of test_cfg_sched_step_kernel."""
    from dreamllm_amd import ops
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    algo, solver, i = _KINDS[kind]
    sched = DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type)
    sched.set_timesteps(20)
    c = sched.multistep_coeffs(i)
    assert (c.k_m1 != 0.0) == ("_o2" in kind) and c.draws == (algo == "sde-dpmsolver++")
    vpred = pred_type == "v_prediction"
    for B in (1, 3, 24):
        for S in (8, 64, 128):
            g = torch.Generator().manual_seed(B * 1000 + S)
            pred = torch.randn(G * B, 4, S, S, generator=g).to(BF)
            x, z, m1 = (torch.randn(B, 4, S, S, generator=g) for _ in range(3))
            ref, ref_m0 = _update(c, _guided(pred, 7.5, phi, G), x, m1, z, vpred)
            outs = []
            for _ in range(2):
                lat, hist = _nhwc(x), _nhwc(m1)
                nxt = torch.full((G * B, S, S, 8), 3.0, dtype=BF, device=DEV)
                ops.cfg_dpm_step_(_nhwc(pred), lat, hist, _nhwc(z) if c.draws else None, nxt, 7.5, phi, c, vpred)
                outs.append((lat, hist, nxt))
            lat, hist, nxt = outs[0]
            err, err_m0 = rel_l2(lat.permute(0, 3, 1, 2), ref), rel_l2(hist.permute(0, 3, 1, 2), ref_m0)
            assert err <= 1e-5 and err_m0 <= 1e-5, (B, S, err, err_m0)
            _check_next_in(nxt, lat, G, B, (B, S))
            assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))  # two launches: the same bits


@pytest.mark.parametrize("algo,solver", [("dpmsolver++", "midpoint"), ("dpmsolver++", "heun"), ("sde-dpmsolver++", "midpoint"),
                                         ("sde-dpmsolver++", "heun")])
@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("phi,G", [(0.0, 2), (0.7, 2), (0.0, 1)])
def test_cfg_dpm_step_trajectory_carries_the_history(algo, solver, pred_type, phi, G):
    """A whole short schedule: the kernel launch after launch on one history buffer (uninitialised at the start, as the loop leaves
    it) against the plain loop's arithmetic with the stateful `step()`, on the same bf16 predictions at every step."""
    from dreamllm_amd import ops
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    from dreamllm_amd.utils import replay_draws
    n, B, S = 7, 3, 32
    sched = DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type)
    sched.set_timesteps(n)
    coeffs = [sched.multistep_coeffs(i) for i in range(n)]
    assert [c.k_m1 != 0.0 for c in coeffs] == [False] + [True] * (n - 2) + [False]
    g = torch.Generator().manual_seed(n)
    preds = [torch.randn(G * B, 4, S, S, generator=g).to(BF) for _ in range(n)]
    zs = [torch.randn(B, 4, S, S, generator=g) for _ in range(n)]
    x = torch.randn(B, 4, S, S, generator=g)
    lat = _nhwc(x)
    hist = torch.full_like(lat, float("nan"))
    nxt = torch.zeros(G * B, S, S, 8, dtype=BF, device=DEV)
    with replay_draws([("randn", z) for z in zs] if coeffs[0].draws else []):
        for i, t in enumerate(sched.timesteps.tolist()):
            x = sched.step(_guided(preds[i], 7.5, phi, G), t, x)
            ops.cfg_dpm_step_(_nhwc(preds[i]), lat, hist, _nhwc(zs[i]) if coeffs[i].draws else None, nxt, 7.5, phi, coeffs[i],
                              pred_type == "v_prediction")
            err = rel_l2(lat.permute(0, 3, 1, 2), x)
            assert err <= 1e-5, (i, err)
            _check_next_in(nxt, lat, G, B, i)
    assert torch.isfinite(hist).all()


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_cfg_dpm_step_first_step_does_not_read_the_history(phi):
    """k_m1 == 0: a NaN-filled history buffer gives the bits of a zeroed one, and is overwritten with m0."""
    from dreamllm_amd import ops
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    sched = DPMSolverMultistepScheduler()
    sched.set_timesteps(20)
    c = sched.multistep_coeffs(0)
    assert c.k_m1 == 0.0
    g = torch.Generator().manual_seed(1)
    pred, x = torch.randn(4, 64, 64, 4, generator=g).to(BF).to(DEV), torch.randn(2, 64, 64, 4, generator=g).to(DEV)
    res = []
    for fill in (float("nan"), 0.0):
        lat, hist = x.clone(), torch.full_like(x, fill)
        nxt = torch.zeros(4, 64, 64, 8, dtype=BF, device=DEV)
        ops.cfg_dpm_step_(pred, lat, hist, None, nxt, 7.5, phi, c)
        assert torch.isfinite(lat).all() and torch.isfinite(hist).all() and torch.isfinite(nxt.float()).all()
        res.append((lat, hist, nxt))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_cfg_dpm_step_rejects_bad_arguments():
    from dreamllm_amd import _lib, ops
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    det, sde = DPMSolverMultistepScheduler(), DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    det.set_timesteps(10)
    sde.set_timesteps(10)
    c, cs = det.multistep_coeffs(1), sde.multistep_coeffs(1)
    lat = torch.ones(2, 8, 8, 4, device=DEV)
    hist, pred = torch.zeros_like(lat), torch.zeros(4, 8, 8, 4, dtype=BF, device=DEV)
    with pytest.raises(ValueError):  # pred is 3 x latents: neither CFG nor no-CFG
        ops.cfg_dpm_step_(torch.zeros(6, 8, 8, 4, dtype=BF, device=DEV), lat, hist, None, None, 7.5, 0.0, c)
    with pytest.raises(ValueError):  # history of another shape
        ops.cfg_dpm_step_(pred, lat, torch.zeros(2, 8, 4, 4, device=DEV), None, None, 7.5, 0.0, c)
    with pytest.raises(ValueError):  # history in bf16
        ops.cfg_dpm_step_(pred, lat, hist.to(BF), None, None, 7.5, 0.0, c)
    with pytest.raises(ValueError):  # no history
        ops.cfg_dpm_step_(pred, lat, None, None, None, 7.5, 0.0, c)
    with pytest.raises(ValueError):  # next_in of the wrong size
        ops.cfg_dpm_step_(pred, lat, hist, None, torch.zeros(4, 8, 8, 4, dtype=BF, device=DEV), 7.5, 0.0, c)
    with pytest.raises(ValueError):  # sigma != 0 without noise: the library's DLLM_ERR_SHAPE
        ops.cfg_dpm_step_(pred, lat, hist, None, None, 7.5, 0.0, cs)
    # the library's own checks, below the Python validation: a null history and misaligned pointers return the error, nothing runs
    vp, st = ops._vp, ops._stream()
    tail = (2, 64, 2, 7.5, 0.0, 0, c.sqrt_at, c.sqrt_1mat, c.k_x, c.k_m0, c.k_m1, c.sigma, st)
    p = {k: v.data_ptr() for k, v in dict(pred=pred, lat=lat, hist=hist).items()}
    assert _lib.call("dllm_cfg_dpm_step", vp(p["pred"]), vp(p["lat"]), None, None, None, *tail) == -1
    assert _lib.call("dllm_cfg_dpm_step", vp(p["pred"]), vp(p["lat"]), vp(p["hist"] + 4), None, None, *tail) == -4
    assert _lib.call("dllm_cfg_dpm_step", vp(p["pred"]), vp(p["lat"] + 8), vp(p["hist"]), None, None, *tail) == -4
    assert _lib.call("dllm_cfg_dpm_step", vp(p["pred"] + 2), vp(p["lat"]), vp(p["hist"]), None, None, *tail) == -4
    assert _lib.call("dllm_cfg_dpm_step", vp(p["pred"]), vp(p["lat"]), vp(p["hist"]), None, None, 2, 64, 3, *tail[3:]) == -1
    torch.cuda.synchronize()
    assert torch.equal(lat, torch.ones_like(lat)) and torch.count_nonzero(hist) == 0


# ----------------------------------------------------------------------------- the graphed loop against the plain loop
def _count_dpm_steps(monkeypatch):
    from dreamllm_amd import ops
    calls = []
    real = ops.cfg_dpm_step_

    def counted(pred, *a, **k):
        calls.append(pred.shape[0])
        return real(pred, *a, **k)

    monkeypatch.setattr(ops, "cfg_dpm_step_", counted)
    return calls


def _pipeline(head, c, sched, use_graph, gen_seed=None, **extra):
    kw = dict(c["kwargs"], **extra)
    cfg = kw["guidance_scale"] > 1.0
    return head.pipeline(latents=c["latents"].float().clone(), prompt_embeds=c["prompt_embeds"].to(BF).to(DEV),
                         negative_prompt_embeds=c["negative_prompt_embeds"].to(BF).to(DEV) if cfg else None,
                         generator=None if gen_seed is None else torch.Generator().manual_seed(gen_seed), scheduler=sched,
                         use_graph=use_graph, **kw)


# inputs, guidance settings, step counts and yard-sticks of the executed-reference pipeline cases (tests/golden/{sd,sdxl}_head.pt);
# only the scheduler is replaced
_LOOP_CASES = [("ddpm_10", "dpmsolver++", "midpoint"), ("ddpm_10", "sde-dpmsolver++", "midpoint"), ("ddim_10_rescale", "dpmsolver++", "heun"),
               ("ddim_10_rescale", "sde-dpmsolver++", "heun"), ("ddim_4_nocfg", "dpmsolver++", "midpoint"),
               ("ddim_4_nocfg", "sde-dpmsolver++", "midpoint"), ("ddim_4_vpred_eta", "dpmsolver++", "heun")]


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
@pytest.mark.parametrize("name,algo,solver", _LOOP_CASES)
def test_graph_multistep_vs_plain_loop(golden, xl, name, algo, solver, monkeypatch):
    """Deterministic and SDE (a seeded CPU generator), CFG / no CFG / rescale / v-prediction: the graphed loop within
    bound(err_ref) of the plain loop (err_ref: the executed reference in bf16 against itself in fp32 on the same case -- the rule of
    test_graph_callback_matches_plain_loop), through the multistep kernel once per step, and the same bits on a second call."""
    from test_diffusion_gpu import _case, _fixture_head
    from dreamllm_amd.modeling_plugins import graph_denoise_mode
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    g = golden(("sdxl_head" if xl else "sd_head") + ".pt")
    c = _case(g, "pipeline", name)
    kw = c["kwargs"]
    head = _fixture_head(g, xl, prediction_type=c["prediction_type"])
    new = lambda: DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=c["prediction_type"])  # noqa: E731
    assert graph_denoise_mode(True, new(), kw["guidance_scale"], kw["guidance_rescale"], kw["eta"], None, 1, 4) == "multistep"
    calls = _count_dpm_steps(monkeypatch)
    sched = new()
    out_g = _pipeline(head, c, sched, True, gen_seed=c["gen_seed"])
    B, G = c["prompt_embeds"].shape[0], 2 if kw["guidance_scale"] > 1.0 else 1
    assert calls == [G * B] * c["steps"] and len(sched.timesteps) == c["steps"]
    assert any(k[-1] == G and k[0] == B and k[-2] == xl for k in head._graph_cache)  # (the SDXL head: with added_cond_kwargs)
    out_g2 = _pipeline(head, c, new(), True, gen_seed=c["gen_seed"])
    assert torch.equal(out_g, out_g2)
    out_l = _pipeline(head, c, new(), False, gen_seed=c["gen_seed"])
    assert len(calls) == 2 * c["steps"]  # the plain loop goes through step(), not the kernel
    assert out_g.shape == out_l.shape == c["out"].shape and out_g.dtype == torch.float32
    assert torch.isfinite(out_g).all()
    err, err_ref = rel_l2(out_g, out_l), rel_l2(c["out_bf16"].float(), c["out"].float())
    assert err <= bound(err_ref), f"{name} {algo} {solver}: graph vs plain loop {err:.3e} > bound({err_ref:.3e}) = {bound(err_ref):.3e}"
    if algo == "sde-dpmsolver++":  # the noise matters: another seed, another image
        assert rel_l2(_pipeline(head, c, new(), True, gen_seed=c["gen_seed"] + 1), out_g) > bound(err_ref)


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_graph_multistep_callback_matches_plain_loop(golden, xl, algo):
    """callback(i, t, latents) as test_graph_callback_matches_plain_loop: the same (i, t), latents within bound(err_ref)."""
    from test_diffusion_gpu import _case, _fixture_head
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    g = golden(("sdxl_head" if xl else "sd_head") + ".pt")
    c = _case(g, "pipeline", "ddpm_10")
    head = _fixture_head(g, xl, prediction_type=c["prediction_type"])
    res = {}
    for use_graph in (True, False):
        seen = []
        sched = DPMSolverMultistepScheduler(algorithm_type=algo)
        out = _pipeline(head, c, sched, use_graph, gen_seed=c["gen_seed"], callback=lambda i, t, x: seen.append((i, t, x.clone())),
                        callback_steps=3)
        res[use_graph] = (out, seen, sched.timesteps.tolist())
    (out_g, seen_g, ts), (out_l, seen_l, _) = res[True], res[False]
    assert [(i, t) for i, t, _ in seen_g] == [(i, t) for i, t, _ in seen_l] == [(i, ts[i]) for i in (0, 3, 6, 9)]
    assert all(type(t) is type(tl) for (_, t, _), (_, tl, _) in zip(seen_g, seen_l))
    assert torch.equal(seen_g[-1][2], out_g)
    assert not torch.equal(seen_g[0][2], out_g)
    err_ref = rel_l2(c["out_bf16"].float(), c["out"].float())
    for (_, _, xg), (_, _, xl_) in zip(seen_g, seen_l):
        assert xg.shape == xl_.shape == out_l.shape and xg.dtype == torch.float32
        assert rel_l2(xg, xl_) <= bound(err_ref)


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "sdxl"])
def test_multistep_reuses_the_graph_a_ddpm_call_captured(golden, xl):
    from test_diffusion_gpu import _case, _fixture_head
    from dreamllm_amd.schedulers import DDPMScheduler, DPMSolverMultistepScheduler
    from dreamllm_amd.utils import replay_draws
    g = golden(("sdxl_head" if xl else "sd_head") + ".pt")
    c = _case(g, "pipeline", "ddpm_10")
    head = _fixture_head(g, xl, prediction_type=c["prediction_type"])
    with replay_draws(c["draws"]):
        _pipeline(head, c, DDPMScheduler(), True, gen_seed=c["gen_seed"])
    assert len(head._graph_cache) == 1
    (key, ent), = head._graph_cache.items()
    graph, x_in = ent["graph"], ent["x_in"]
    out = _pipeline(head, c, DPMSolverMultistepScheduler(), True)
    assert list(head._graph_cache) == [key] and head._graph_cache[key]["graph"] is graph and head._graph_cache[key]["x_in"] is x_in
    assert rel_l2(out, _pipeline(head, c, DPMSolverMultistepScheduler(), False)) <= bound(rel_l2(c["out_bf16"].float(), c["out"].float()))


# ----------------------------------------------------------------------------- full size: SD-2.1 at 512 px
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


def test_dpm_graph_full_size_vs_oracle(sd21):
    """SD-2.1 at 512 px, DPM-Solver++ (midpoint, linspace), CFG 7.5, 20 steps: the graphed loop and the plain loop each within the
    contract of the fp32 oracle loop (tests/dpm_ref.py over oracle.unet_ref; yard-stick: the same loop with the UNet in bf16), as
    test_config3_pipeline_latents_full_size holds the DDIM loops."""
    import dpm_ref
    from dreamllm_amd.schedulers import DPMSolverMultistepScheduler
    from oracle import sched_ref, unet_ref
    h, n, s = sd21, 20, 7.5
    pe, ne = _randn(1, 64, 4096, seed=31, scale=0.5), _randn(1, 64, 4096, seed=32, scale=0.5)
    lat0 = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(42)).to(DEV)

    def oracle(dtype):
        usd, pw = {k: v.to(dtype) for k, v in h["usd"].items()}, h["pw"].to(dtype)
        ctx = torch.cat([F.linear(ne.to(dtype), pw), F.linear(pe.to(dtype), pw)])

        def model(i, t, x):
            x = x.float()  # the reference keeps fp32 latents and feeds the UNet in its dtype
            eu, ec = unet_ref.unet_forward(torch.cat([x, x]).to(dtype), torch.tensor([t], device=DEV), ctx, usd, h["ucfg"]).float().chunk(2)
            return sched_ref.cfg(eu, ec, s)

        with torch.no_grad():
            return dpm_ref.dpm_trajectory(model, lat0, n)[-1].float()

    ref, yard = oracle(torch.float32), oracle(BF)
    e_ref = rel_l2(yard, ref)
    for use_graph in (True, False):
        sched = DPMSolverMultistepScheduler()
        out = h["head"].pipeline(num_inference_steps=n, guidance_scale=s, latents=lat0.clone(), prompt_embeds=pe.to(BF),
                                 negative_prompt_embeds=ne.to(BF), output_type="latent", scheduler=sched, use_graph=use_graph)
        assert sched.timesteps.tolist() == dpm_ref.timesteps(n, "linspace")
        assert out.shape == (1, 4, 64, 64) and out.dtype == torch.float32
        check_tensor(f"fullsize.dpm_{n}.{'graph' if use_graph else 'loop'}", out, ref, e_ref)
