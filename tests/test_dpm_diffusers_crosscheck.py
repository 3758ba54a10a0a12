"""Cross-check of `DPMSolverMultistepScheduler` and of its fp64 restatement tests/dpm_ref.py against the real
`diffusers.DPMSolverMultistepScheduler` (the "dpm" branch of omni/utils/block_utils.py:34-47; diffusers==0.24.0, pyproject.toml:74).

`diffusers` is not installed where this suite is written and run, so every test here is SKIPPED there, in the manner of
tests/test_diffusers_crosscheck.py; on any box that has diffusers they run.  The 'linspace' and 'trailing' schedules are compared
with diffusers' own; the 'leading' schedule is the project's base-class schedule (shared with DDIM / DDPM) and is pinned by
tests/test_dpm_sched_cpu.py; the step arithmetic is the same on every spacing."""
import pytest
import torch

from conftest import rel_l2

diffusers = pytest.importorskip("diffusers")

import dpm_ref  # noqa: E402
from dreamllm_amd.schedulers import DPMSolverMultistepScheduler  # noqa: E402

TOL = 1e-5   # fp32 vs fp32, the same update written in another order
KW = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)
SHAPE = (2, 4, 8, 8)


def _theirs(algo, solver, pred_type, spacing, **extra):
    return diffusers.DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type,
                                                 timestep_spacing=spacing, solver_order=2, lower_order_final=True, **KW, **extra)


@pytest.mark.parametrize("spacing", ["linspace", "trailing"])
@pytest.mark.parametrize("n", [1, 2, 14, 15, 20, 25, 50])
def test_timesteps_equal_diffusers(spacing, n):
    theirs = _theirs("dpmsolver++", "midpoint", "epsilon", spacing)
    theirs.set_timesteps(n)
    ours = DPMSolverMultistepScheduler(timestep_spacing=spacing)
    ours.set_timesteps(n)
    assert ours.timesteps.tolist() == [int(t) for t in theirs.timesteps] == dpm_ref.timesteps(n, spacing)
    assert torch.allclose(ours.alphas_cumprod, theirs.alphas_cumprod, rtol=1e-6, atol=0)


@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
@pytest.mark.parametrize("solver", ["midpoint", "heun"])
@pytest.mark.parametrize("pred_type", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("spacing", ["linspace", "trailing"])
@pytest.mark.parametrize("n", [2, 14, 15, 25])
def test_trajectory_equals_diffusers(algo, solver, pred_type, spacing, n):
    g = torch.Generator().manual_seed(n)
    outs = [torch.randn(SHAPE, generator=g) for _ in range(n)]
    x0 = torch.randn(SHAPE, generator=g)
    theirs = _theirs(algo, solver, pred_type, spacing)
    theirs.set_timesteps(n)
    ours = DPMSolverMultistepScheduler(algorithm_type=algo, solver_type=solver, prediction_type=pred_type, timestep_spacing=spacing)
    ours.set_timesteps(n)
    ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    xa, xb, noises = x0, x0, []
    for e, t in zip(outs, theirs.timesteps):
        xa = theirs.step(e, t, xa, generator=ga).prev_sample
        xb = ours.step(e, int(t), xb, generator=gb)
        assert rel_l2(xb, xa) < TOL, (int(t), rel_l2(xb, xa))
    if algo == "sde-dpmsolver++":
        gc = torch.Generator().manual_seed(5)
        noises = [torch.randn(SHAPE, generator=gc) for _ in range(n)]
    ref = dpm_ref.dpm_trajectory(lambda i, t, x: outs[i], x0, n, algorithm_type=algo, solver_type=solver, spacing=spacing,
                                 prediction_type=pred_type, noises=noises or None, ac=ours.alphas_cumprod.double().tolist())
    assert rel_l2(ref[-1], xa) < TOL
