"""CPU: `DPMSolverMultistepScheduler` -- coefficient identities, exactness for a constant data prediction, order 1 against DDIM,
`step()` and `multistep_coeffs` against the fp64 restatement tests/dpm_ref.py, the order schedule and the timesteps, and the choice
of loop (`graph_denoise_mode`).  No kernels are launched.

Yard-sticks.  The fp64 restatements run on the scheduler's own (fp32-rounded) table of cumulative alphas, so that a comparison
measures the step arithmetic alone.  `step()` is a handful of fp32 operations per step, like the existing DDIM and DDPM steps; its
error against fp64 may be at most twice theirs on inputs of the same shape, plus 1e-6 relative."""
import math
import sys

import pytest
import torch

import ddpm_ref
import dpm_ref
from dreamllm_amd import utils
from dreamllm_amd.modeling_plugins import graph_denoise_mode, predraw_step_noise
from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, MultistepCoeffs

EPS64 = sys.float_info.epsilon
SHAPE = (2, 4, 8, 8)
ALGOS = ["dpmsolver++", "sde-dpmsolver++"]
SOLVERS = ["midpoint", "heun"]
PREDS = ["epsilon", "v_prediction"]
SPACINGS = ["linspace", "leading", "trailing"]


def _table(sched):
    return sched.alphas_cumprod.double().tolist()


def _rand(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(SHAPE, generator=g) for _ in range(n)]


def _apply(c, e, x, m1, z, vpred):
    """x_next and m0 from the coefficients, as dllm_cfg_dpm_step computes them (fp32)."""
    m0 = c.sqrt_at * x - c.sqrt_1mat * e if vpred else (x - c.sqrt_1mat * e) / c.sqrt_at
    out = c.k_x * x + c.k_m0 * m0
    if c.k_m1 != 0.0:
        out = out + c.k_m1 * m1
    if c.sigma != 0.0:
        out = out + c.sigma * z
    return out, m0


def _run_step(sched, outs, x, n, noises=None):
    sched.set_timesteps(n)
    traj = []
    with utils.replay_draws([("randn", z) for z in noises] if noises is not None else []):
        for e, t in zip(outs, sched.timesteps.tolist()):
            x = sched.step(e, t, x)
            traj.append(x)
    return traj


def _run_coeffs(sched, outs, x, n, noises=None):
    sched.set_timesteps(n)
    vpred = sched.config.prediction_type == "v_prediction"
    traj, m1 = [], None
    for i, e in enumerate(outs):
        c = sched.multistep_coeffs(i)
        x, m1 = _apply(c, e, x, m1, noises[i] if noises is not None else None, vpred)
        traj.append(x)
    return traj


def _ddpm_yardstick(n, seed):
    """The existing DDPM `step()` over a whole trajectory against tests/ddpm_ref.py in fp64, on inputs of the same shape."""
    sched = DDPMScheduler()
    sched.set_timesteps(n)
    ac = _table(sched)
    outs, noises, (x0,) = _rand(n, seed), _rand(n, seed + 1), _rand(1, seed + 2)
    x, xr, got, ref = x0, x0.double(), [], []
    with utils.replay_draws([("randn", z) for z in noises]):  # (the last step, t = 1 > 0, draws too)
        for e, z, t in zip(outs, noises, sched.timesteps.tolist()):
            x = sched.step(e, t, x)
            xr = ddpm_ref.ddpm_step(e.double(), t, xr, n, ac, z.double())
            got.append(x)
            ref.append(xr)
    return dpm_ref.traj_err(got, ref)


# ------------------------------------------------------------------------------------------------ 1. coefficient identities
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pred_type", PREDS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_coefficient_identities(algo, solver, pred_type, spacing):
    """The update maps alpha_s x0 + sigma_s eps (with m0 = m1 = x0) onto alpha_t x0 + sigma_t eps':
      deterministic  k_x sigma_s = sigma_t                       k_x alpha_s + k_m0 + k_m1 = alpha_t
      SDE            k_x^2 sigma_s^2 + sigma^2 = sigma_t^2       k_x alpha_s + k_m0 + k_m1 = alpha_t
    Tolerance: every coefficient is a product of at most ~10 correctly rounded fp64 operations (sqrt, log, exp, expm1, * and /), so
    each side carries at most 16 eps relative to the magnitude of its largest term; the largest term is alpha_t (sigma_t) itself
    except on second-order steps, where k_m0 and k_m1 carry the cancelling pair +-w/r0 of D1 and the sum is exact only to that pair's
    rounding.  Hence 64 eps times max(alpha_t, |k_x| alpha_s + |k_m0| + |k_m1|), and 64 eps relative for the sigma identities."""
    sched = DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type, timestep_spacing=spacing)
    ac = _table(sched)
    for n in (1, 2, 7, 20, 50):
        sched.set_timesteps(n)
        ts = sched.timesteps.tolist()
        for i, s in enumerate(ts):
            c = sched.multistep_coeffs(i)
            assert isinstance(c, MultistepCoeffs) and all(type(v) is float for v in c[:6]) and type(c.draws) is bool
            ab_s, ab_t = ac[s], ac[ts[i + 1]] if i + 1 < n else ac[0]
            al_s, sg_s, al_t, sg_t = math.sqrt(ab_s), math.sqrt(1 - ab_s), math.sqrt(ab_t), math.sqrt(1 - ab_t)
            assert c.sqrt_at == al_s and c.sqrt_1mat == sg_s
            assert (c.k_m1 == 0.0) == (sched.order_at(i) == 1), (n, i)
            mag = max(al_t, abs(c.k_x) * al_s + abs(c.k_m0) + abs(c.k_m1))
            d_alpha = abs(c.k_x * al_s + c.k_m0 + c.k_m1 - al_t)
            assert d_alpha <= 64 * EPS64 * mag, (n, i, d_alpha, mag)
            if algo == "dpmsolver++":
                assert c.sigma == 0.0 and c.draws is False
                d_sigma = abs(c.k_x * sg_s - sg_t) / sg_t
            else:
                assert c.sigma > 0.0 and c.draws is True
                d_sigma = abs(c.k_x**2 * sg_s**2 + c.sigma**2 - sg_t**2) / sg_t**2
            assert d_sigma <= 64 * EPS64, (n, i, d_sigma)


# ------------------------------------------------------------------------------------------------ 2. constant data prediction
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pred_type", PREDS)
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", [1, 2, 7, 20, 50])
def test_constant_data_prediction_is_exact(solver, pred_type, spacing, n):
    """A model whose data prediction is x0* at every step: the deterministic solver lands on alpha_0 x0* + sigma_0 eps, eps being
    the noise of the initial latents -- at order 2 too (D1 = 0).  DDIM has the same property, so its own fp32 `step()` on the same
    problem is the yard-stick: at most twice its error against the closed form, plus 1e-6."""
    (x0s, eps) = _rand(2, 100 + n)

    def run(sched):
        sched.set_timesteps(n)
        ac = _table(sched)
        ts = sched.timesteps.tolist()
        x = (math.sqrt(ac[ts[0]]) * x0s.double() + math.sqrt(1 - ac[ts[0]]) * eps.double()).float()
        for t in ts:
            a, s = math.sqrt(ac[t]), math.sqrt(1 - ac[t])
            xd = x.double()
            out = (xd - a * x0s.double()) / s if pred_type == "epsilon" else (a * xd - x0s.double()) / s
            x = sched.step(out.float(), t, x)
        want = math.sqrt(ac[0]) * x0s.double() + math.sqrt(1 - ac[0]) * eps.double()
        return ((x.double() - want).norm() / want.norm()).item()

    err = run(DPMSolverMultistepScheduler(solver_type=solver, prediction_type=pred_type, timestep_spacing=spacing))
    err_ddim = run(DDIMScheduler(prediction_type=pred_type))
    assert err <= 2 * err_ddim + 1e-6, f"DPM {err:.3e} vs closed form; DDIM step on the same problem {err_ddim:.3e}"


# ------------------------------------------------------------------------------------------------ 3. order 1 is DDIM
@pytest.mark.parametrize("pred_type", PREDS)
@pytest.mark.parametrize("n", [10, 25, 50, 80])
def test_order_one_is_ddim(pred_type, n):
    outs, (x,) = _rand(n, n), _rand(1, n + 7)
    dpm = DPMSolverMultistepScheduler(solver_order=1, timestep_spacing="leading", prediction_type=pred_type)
    ddim = DDIMScheduler(prediction_type=pred_type)
    ddim.set_timesteps(n)
    dpm.set_timesteps(n)
    assert dpm.timesteps.tolist() == ddim.timesteps.tolist()
    ac = _table(dpm)
    ref = dpm_ref.dpm_trajectory(lambda i, t, x_: outs[i], x, n, solver_order=1, spacing="leading", prediction_type=pred_type, ac=ac)
    ref_ddim = dpm_ref.ddim_trajectory(outs, x, n, pred_type, ac=ac)
    assert dpm_ref.traj_err(ref, ref_ddim) <= 1e-12  # the two fp64 restatements: one trajectory
    got = _run_step(dpm, outs, x, n)
    xd, got_ddim = x, []
    for e, t in zip(outs, ddim.timesteps.tolist()):
        xd = ddim.step(e, t, xd, eta=0.0)
        got_ddim.append(xd)
    err, err_ddim = dpm_ref.traj_err(got, ref), dpm_ref.traj_err(got_ddim, ref)
    assert err <= 2 * err_ddim + 1e-6, f"DPM order 1 vs fp64 {err:.3e}; DDIM step vs fp64 {err_ddim:.3e}"
    assert dpm_ref.traj_err(got, [g.double() for g in got_ddim]) <= err + err_ddim + 1e-6


# ------------------------------------------------------------------------------------------------ 4. fp64 restatement
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pred_type", PREDS)
@pytest.mark.parametrize("n", [2, 7, 14, 15, 25])
def test_step_and_coeffs_agree_with_fp64_restatement(algo, solver, pred_type, n):
    outs, (x,) = _rand(n, 10 * n), _rand(1, 10 * n + 1)
    noises = _rand(n, 10 * n + 2) if algo == "sde-dpmsolver++" else None
    err_yard = _ddpm_yardstick(n, 10 * n + 3)
    for spacing in SPACINGS:
        sched = DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type, timestep_spacing=spacing)
        ref = dpm_ref.dpm_trajectory(lambda i, t, x_: outs[i], x, n, algorithm_type=algo, solver_type=solver, spacing=spacing,
                                     prediction_type=pred_type, noises=noises, ac=_table(sched))
        e_step = dpm_ref.traj_err(_run_step(sched, outs, x, n, noises), ref)
        e_coef = dpm_ref.traj_err(_run_coeffs(sched, outs, x, n, noises), ref)
        msg = f"{spacing}: step {e_step:.3e}, coefficients {e_coef:.3e} vs fp64; DDPM step vs its fp64 restatement {err_yard:.3e}"
        assert e_step <= 2 * err_yard + 1e-6, msg
        assert e_coef <= 2 * err_yard + 1e-6, msg


def test_predraw_fits_multistep_coeffs():
    """`predraw_step_noise` reads `.draws` only: one draw per SDE step, none for the deterministic solver."""
    for algo, want in (("dpmsolver++", None), ("sde-dpmsolver++", 5)):
        sched = DPMSolverMultistepScheduler(algorithm_type=algo)
        sched.set_timesteps(5)
        noise = predraw_step_noise(SHAPE, [sched.multistep_coeffs(i) for i in range(5)], torch.Generator().manual_seed(3), "cpu")
        if want is None:
            assert noise is None
            continue
        assert noise.shape == (5, 2, 8, 8, 4)
        g = torch.Generator().manual_seed(3)
        want_draws = [torch.randn(SHAPE, generator=g) for _ in range(5)]  # what step() draws, in order, from the same seed
        assert all(torch.equal(noise[k].permute(0, 3, 1, 2), want_draws[k]) for k in range(5))
        g, x, xr = torch.Generator().manual_seed(3), torch.ones(SHAPE), torch.ones(SHAPE)
        with utils.replay_draws([("randn", z) for z in want_draws]):
            for t in sched.timesteps.tolist():
                xr = sched.step(torch.zeros(SHAPE), t, xr)
        sched.set_timesteps(5)
        for t in sched.timesteps.tolist():
            x = sched.step(torch.zeros(SHAPE), t, x, generator=g)
        assert torch.equal(x, xr)


# ------------------------------------------------------------------------------------------------ 5. orders and timesteps
def test_order_schedule():
    def orders(n, **kw):
        s = DPMSolverMultistepScheduler(**kw)
        s.set_timesteps(n)
        return [s.order_at(i) for i in range(n)]

    assert orders(1) == [1]
    assert orders(2) == [1, 1]
    assert orders(14) == [1] + [2] * 12 + [1]
    assert orders(15) == [1] + [2] * 14
    assert orders(50) == [1] + [2] * 49
    assert orders(2, lower_order_final=False) == [1, 2]
    assert orders(14, lower_order_final=False) == [1] + [2] * 13
    for n in (1, 2, 14, 15, 50):
        assert orders(n, solver_order=1) == [1] * n
        assert dpm_ref.orders(n) == orders(n)


_TIMESTEPS = {
    ("linspace", 1): [999],
    ("linspace", 2): [999, 500],
    ("linspace", 14): [999, 928, 856, 785, 714, 642, 571, 500, 428, 357, 285, 214, 143, 71],
    ("linspace", 15): [999, 932, 866, 799, 733, 666, 599, 533, 466, 400, 333, 266, 200, 133, 67],
    ("linspace", 50): [999, 979, 959, 939, 919, 899, 879, 859, 839, 819, 799, 779, 759, 739, 719, 699, 679, 659, 639, 619, 599, 579, 559,
                       539, 519, 500, 480, 460, 440, 420, 400, 380, 360, 340, 320, 300, 280, 260, 240, 220, 200, 180, 160, 140, 120, 100,
                       80, 60, 40, 20],
    ("trailing", 1): [999],
    ("trailing", 2): [999, 499],
    ("trailing", 14): [999, 928, 856, 785, 713, 642, 570, 499, 428, 356, 285, 213, 142, 70],
    ("trailing", 15): [999, 932, 866, 799, 732, 666, 599, 532, 466, 399, 332, 266, 199, 132, 66],
    ("trailing", 50): list(range(999, 0, -20)),
    ("leading", 1): [1],
    ("leading", 2): [501, 1],
    ("leading", 14): list(range(924, 0, -71)),
    ("leading", 15): list(range(925, 0, -66)),
    ("leading", 50): list(range(981, 0, -20)),
}


@pytest.mark.parametrize("spacing,n", sorted(_TIMESTEPS))
def test_timesteps(spacing, n):
    sched = DPMSolverMultistepScheduler(timestep_spacing=spacing)
    sched.set_timesteps(n)
    assert sched.timesteps.dtype == torch.long
    assert sched.timesteps.tolist() == _TIMESTEPS[(spacing, n)]
    assert dpm_ref.timesteps(n, spacing) == _TIMESTEPS[(spacing, n)]
    if spacing == "leading":  # the base class's schedule, steps_offset included
        base = DDIMScheduler()
        base.set_timesteps(n)
        assert sched.timesteps.tolist() == base.timesteps.tolist()
        off0 = DPMSolverMultistepScheduler(timestep_spacing="leading", steps_offset=0)
        off0.set_timesteps(n)
        assert off0.timesteps.tolist() == [t - 1 for t in _TIMESTEPS[(spacing, n)]]


# ------------------------------------------------------------------------------------------------ 6. routing and config
class _Foreign:
    def step(self, *a, **k):
        raise NotImplementedError


def test_graph_denoise_mode_multistep():
    cb = lambda i, t, x: None  # noqa: E731
    for dpm in (DPMSolverMultistepScheduler(), DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", solver_type="heun")):
        assert not hasattr(dpm, "step_coeffs") and not hasattr(dpm, "step_cfg_fused_")
        #        use_graph, sched, cfg, rescale, eta, callback, n, in_ch -> mode
        table = [
            ((True, dpm, 7.5, 0.0, 0.0, None, 1, 4), "multistep"),
            ((True, dpm, 1.0, 0.0, 0.0, None, 1, 4), "multistep"),   # no CFG
            ((True, dpm, 0.0, 0.0, 0.0, None, 1, 4), "multistep"),
            ((True, dpm, 7.5, 0.7, 0.0, None, 1, 4), "multistep"),   # guidance rescale
            ((True, dpm, 7.5, 0.0, 0.0, cb, 1, 4), "multistep"),     # callback
            ((True, dpm, 1.0, 0.7, 0.5, cb, 1, 4), "multistep"),     # (eta is ignored)
            ((False, dpm, 7.5, 0.0, 0.0, None, 1, 4), None),         # use_graph=False
            ((True, dpm, 7.5, 0.0, 0.0, None, 2, 4), None),          # num_images_per_prompt > 1
            ((True, dpm, 7.5, 0.0, 0.0, None, 1, 9), None),          # inpainting-style UNet input
        ]
        for args, want in table:
            assert graph_denoise_mode(*args) == want, (args, want)
    ddim, ddpm, foreign = DDIMScheduler(), DDPMScheduler(), _Foreign()
    for args, want in [((True, ddim, 7.5, 0.0, 0.0, None, 1, 4), "ddim"), ((True, ddim, 7.5, 0.0, 0.5, None, 1, 4), "sched"),
                       ((True, ddim, 7.5, 0.0, 0.0, cb, 1, 4), "sched"), ((True, ddpm, 7.5, 0.0, 0.0, None, 1, 4), "sched"),
                       ((True, ddpm, 0.0, 0.0, 0.0, None, 1, 4), "sched"), ((True, foreign, 7.5, 0.0, 0.0, None, 1, 4), None),
                       ((True, foreign, 1.0, 0.0, 0.0, None, 1, 4), None), ((False, ddpm, 7.5, 0.0, 0.0, None, 1, 4), None)]:
        assert graph_denoise_mode(*args) == want, (args, want)


@pytest.mark.parametrize("key,value", [("solver_order", 3), ("solver_order", 0), ("algorithm_type", "dpmsolver"),
                                       ("algorithm_type", "sde-dpmsolver"), ("solver_type", "bh2"), ("lower_order_final", "yes"),
                                       ("timestep_spacing", "karras"), ("thresholding", True), ("use_karras_sigmas", True)])
def test_unsupported_config_raises(key, value):
    with pytest.raises(ValueError) as ei:
        DPMSolverMultistepScheduler(**{key: value})
    assert key in str(ei.value) and repr(value) in str(ei.value)
    with pytest.raises(ValueError, match=key):
        DPMSolverMultistepScheduler.from_name_or_path({"scheduler": {key: value}})


def test_config_defaults_and_loading(tmp_path):
    import json
    from dreamllm_amd import schedulers
    c = DPMSolverMultistepScheduler().config
    assert (c.solver_order, c.algorithm_type, c.solver_type, c.lower_order_final, c.timestep_spacing) == \
        (2, "dpmsolver++", "midpoint", True, "linspace")
    assert (c.num_train_timesteps, c.beta_schedule, c.prediction_type, c.steps_offset) == (1000, "scaled_linear", "epsilon", 1)
    assert torch.equal(DPMSolverMultistepScheduler().alphas_cumprod, DDIMScheduler().alphas_cumprod)
    # a scheduler_config.json: the DPM keys are read for this class ...
    (tmp_path / "scheduler").mkdir()
    raw = dict(prediction_type="v_prediction", timestep_spacing="trailing", solver_order=1, algorithm_type="sde-dpmsolver++",
               solver_type="heun", lower_order_final=False, _class_name="DPMSolverMultistepScheduler")
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(raw))
    c = DPMSolverMultistepScheduler.from_name_or_path(str(tmp_path)).config
    assert (c.prediction_type, c.timestep_spacing, c.solver_order, c.algorithm_type, c.solver_type, c.lower_order_final) == \
        ("v_prediction", "trailing", 1, "sde-dpmsolver++", "heun", False)
    # ... and what the two existing classes load is what it was: SD21_SCHED's keys only
    d = schedulers._load_cfg(str(tmp_path))
    assert d == dict(schedulers.SD21_SCHED, prediction_type="v_prediction", timestep_spacing="trailing")
    assert list(d) == list(schedulers.SD21_SCHED)
    assert vars(DDIMScheduler.from_name_or_path(str(tmp_path)).config) == d
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(dict(raw, use_karras_sigmas=True)))
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        DPMSolverMultistepScheduler.from_name_or_path(str(tmp_path))
    # add_noise / get_velocity are the base class's
    g = torch.Generator().manual_seed(0)
    x, e, ts = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g), torch.tensor([3, 700])
    assert torch.equal(DPMSolverMultistepScheduler().add_noise(x, e, ts), DDPMScheduler().add_noise(x, e, ts))
    assert torch.equal(DPMSolverMultistepScheduler().get_velocity(x, e, ts), DDPMScheduler().get_velocity(x, e, ts))


@pytest.mark.parametrize("algo", ALGOS)
def test_set_timesteps_resets_the_history(algo):
    n = 7
    outs, (x,) = _rand(n, 5), _rand(1, 6)
    noises = _rand(n, 7) if algo == "sde-dpmsolver++" else None
    sched = DPMSolverMultistepScheduler(algorithm_type=algo)
    a = _run_step(sched, outs, x, n, noises)
    b = _run_step(sched, outs, x, n, noises)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    fresh = _run_step(DPMSolverMultistepScheduler(algorithm_type=algo), outs, x, n, noises)
    assert all(torch.equal(p, q) for p, q in zip(a, fresh))
    # out of order: the history would be wrong, so step() says so
    sched.set_timesteps(n)
    with pytest.raises(ValueError):
        sched.step(outs[0], sched.timesteps.tolist()[1], x)
