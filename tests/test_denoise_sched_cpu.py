"""CPU: the host side of the graphed denoising loop for every scheduler -- `step_coeffs` against `step()`, the ancestral noise
drawn ahead of the loop against the plain loop's draws, and the choice of loop (`graph_denoise_mode`).  No kernels are launched."""
import pytest
import torch

from dreamllm_amd import utils
from dreamllm_amd.modeling_plugins import graph_denoise_mode, predraw_step_noise
from dreamllm_amd.schedulers import DDIMScheduler, DDPMScheduler


def _apply(c, e, x, z, vpred):
    """x_prev from the coefficients, as dllm_cfg_sched_step computes it (fp32)."""
    if vpred:
        x0, eps = c.sqrt_at * x - c.sqrt_1mat * e, c.sqrt_at * e + c.sqrt_1mat * x
    else:
        x0, eps = (x - c.sqrt_1mat * e) / c.sqrt_at, e
    out = c.k_x0 * x0 + c.k_eps * eps + c.k_x * x
    return out + c.sigma * z if c.draws else out


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [1, 10, 50, 150])
def test_step_coeffs_reproduce_step(kind, pred_type, n):
    cls = DDPMScheduler if kind == "ddpm" else DDIMScheduler
    sched = cls(prediction_type=pred_type)
    sched.set_timesteps(n)
    g = torch.Generator().manual_seed(n)
    e, x, z = (torch.randn(2, 4, 8, 8, generator=g) for _ in range(3))
    etas = [0.0] if kind == "ddpm" else [0.0, 0.3, 1.0]
    for eta in etas:
        for t in sched.timesteps.tolist():
            c = sched.step_coeffs(t, eta)
            assert all(isinstance(v, float) for v in c[:6]) and isinstance(c.draws, bool)
            assert c.draws == (t > 0 if kind == "ddpm" else eta > 0)
            # the same fixed noise for the step's one draw; replay_draws fails if step() draws where the coefficients say it
            # does not (or the other way round: an unconsumed draw)
            with utils.replay_draws([("randn", z)] if c.draws else []):
                ref = sched.step(e, t, x, eta=eta)
            ours = _apply(c, e, x, z, pred_type == "v_prediction")
            assert _rel(ours, ref) <= 1e-6, (kind, pred_type, n, eta, t, _rel(ours, ref))


class _Recorder:
    """Stand-in for `utils.draws` that records every draw (shape, dtype, device, generator, values) and makes it for real."""

    def __init__(self):
        self.log = []

    def randn(self, shape, generator=None, device=None, dtype=None):
        out = torch.randn(shape, generator=generator, device=device, dtype=dtype)
        self.log.append((tuple(shape), dtype, str(device), id(generator) if generator is not None else None, out.clone()))
        return out


def _record(fn, monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(utils, "draws", rec)
    fn()
    return rec.log


@pytest.mark.parametrize("gen_kind", ["cpu", "list", "none"])
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.5), ("ddim", 0.0)])
def test_predraw_makes_the_plain_loops_draws(monkeypatch, gen_kind, kind, eta):
    B, shape = 2, (2, 4, 8, 8)
    sched = (DDPMScheduler if kind == "ddpm" else DDIMScheduler)()
    sched.set_timesteps(6)
    ts = sched.timesteps.tolist()

    def gens():
        if gen_kind == "cpu":
            return torch.Generator().manual_seed(7)
        if gen_kind == "list":
            return [torch.Generator().manual_seed(7 + b) for b in range(B)]
        torch.manual_seed(7)  # generator=None: the default generator
        return None

    e = torch.randn(shape, generator=torch.Generator().manual_seed(1))

    def plain():  # the plain loop's draws: inside scheduler.step, once per step
        g, x = gens(), torch.zeros(shape)
        for t in ts:
            x = sched.step(e, t, x, eta=eta, generator=g)

    box = {}

    def graphed():
        box["noise"] = predraw_step_noise(shape, [sched.step_coeffs(t, eta) for t in ts], gens(), "cpu")

    log_plain = _record(plain, monkeypatch)
    log_pre = _record(graphed, monkeypatch)
    n_draw = sum(sched.step_coeffs(t, eta).draws for t in ts)
    per_step = B if gen_kind == "list" else 1
    assert len(log_plain) == len(log_pre) == n_draw * per_step
    for a, b in zip(log_plain, log_pre):
        assert a[:3] == b[:3]                                        # shape, dtype, device, in order
        assert (a[3] is None) == (b[3] is None)
        assert torch.equal(a[4], b[4])                               # the same values
    noise = box["noise"]
    if n_draw == 0:
        assert noise is None
        return
    assert noise.shape == (n_draw, 2, 8, 8, 4) and noise.dtype == torch.float32
    for k in range(n_draw):
        step_draw = torch.cat([r[4] for r in log_plain[k * per_step:(k + 1) * per_step]])
        assert torch.equal(noise[k].permute(0, 3, 1, 2), step_draw)  # NHWC layout of the step's NCHW draw


class _Foreign:
    """A scheduler object the graphed loop does not know: no step_coeffs, no fused step."""

    def step(self, *a, **k):
        raise NotImplementedError


def test_graph_denoise_mode_table():
    ddim, ddpm, foreign = DDIMScheduler(), DDPMScheduler(), _Foreign()
    cb = lambda i, t, x: None  # noqa: E731
    #        use_graph, sched, cfg, rescale, eta, callback, n, in_ch -> mode
    table = [
        ((True, ddim, 7.5, 0.0, 0.0, None, 1, 4), "ddim"),     # the original fast path, unchanged
        ((True, ddpm, 7.5, 0.0, 0.0, None, 1, 4), "sched"),    # the reference's own scheduler
        ((True, ddpm, 3.5, 0.0, 0.7, None, 1, 4), "sched"),    # DDPM ignores eta
        ((True, ddim, 1.0, 0.0, 0.0, None, 1, 4), "sched"),    # no CFG
        ((True, ddpm, 0.0, 0.0, 0.0, None, 1, 4), "sched"),    # guidance_scale 0 (dreamllm_sdxl/inf.py)
        ((True, ddim, 7.5, 0.7, 0.0, None, 1, 4), "sched"),    # guidance rescale
        ((True, ddim, 7.5, 0.0, 0.5, None, 1, 4), "sched"),    # DDIM with eta
        ((True, ddim, 7.5, 0.0, 0.0, cb, 1, 4), "sched"),      # callback
        ((True, ddpm, 7.5, 0.0, 0.0, cb, 1, 4), "sched"),
        ((True, ddpm, 7.5, 0.0, 0.0, None, 2, 4), None),       # num_images_per_prompt > 1
        ((True, ddim, 7.5, 0.0, 0.0, None, 2, 4), None),
        ((True, ddpm, 7.5, 0.0, 0.0, None, None, 4), None),
        ((True, foreign, 7.5, 0.0, 0.0, None, 1, 4), None),    # a foreign scheduler object
        ((True, foreign, 1.0, 0.0, 0.0, None, 1, 4), None),
        ((False, ddim, 7.5, 0.0, 0.0, None, 1, 4), None),      # use_graph=False
        ((False, ddpm, 7.5, 0.0, 0.0, None, 1, 4), None),
        ((True, ddpm, 7.5, 0.0, 0.0, None, 1, 9), None),       # inpainting-style UNet input
    ]
    for args, want in table:
        assert graph_denoise_mode(*args) == want, (args, want)
