"""DPM-Solver++ multistep sampling (diffusers 0.24 `DPMSolverMultistepScheduler`, algorithm types "dpmsolver++" and
"sde-dpmsolver++", orders 1 and 2, solver types "midpoint" and "heun") restated in fp64 over plain Python floats, written from the
update formulas and not from dreamllm_amd/schedulers.py: the yard-stick of `DPMSolverMultistepScheduler.step` / `multistep_coeffs`.

`ac` is the table of cumulative alphas the trajectory is computed on (a list of floats; default: oracle.sched_ref's fp64 table).  The
tests pass the scheduler's own table so that the comparison measures the step arithmetic and not the rounding of the fp32 table."""
import math

import torch

from oracle import sched_ref


def timesteps(n, spacing, T=1000, offset=1):
    if spacing == "leading":
        return sched_ref.leading_timesteps(n, T, offset)
    if spacing == "linspace":  # linspace(0, T - 1, n + 1).round()[::-1][:-1]; Python's round is half-to-even, as numpy's
        return [round(i * ((T - 1) / n)) for i in range(n, 0, -1)]
    if spacing == "trailing":  # round(arange(T, 0, -T / n)) - 1; numpy's arange fills with T + i * ((T - T / n) - T)
        return [round(T + i * ((T - T / n) - T)) - 1 for i in range(n)]
    raise ValueError(spacing)


def orders(n, solver_order=2, lower_order_final=True):
    return [1 if (i == 0 or solver_order == 1 or (i == n - 1 and lower_order_final and n < 15)) else 2 for i in range(n)]


def _lam(ab):
    return math.log(math.sqrt(ab)) - math.log(math.sqrt(1 - ab))


def data_prediction(out, x, ab, prediction_type):
    a, s = math.sqrt(ab), math.sqrt(1 - ab)
    if prediction_type == "epsilon":
        return (x - s * out) / a
    if prediction_type == "v_prediction":
        return a * x - s * out
    raise ValueError(prediction_type)


def dpm_trajectory(model_fn, x, n, *, algorithm_type="dpmsolver++", solver_type="midpoint", solver_order=2, lower_order_final=True,
                   spacing="linspace", prediction_type="epsilon", noises=None, ac=None):
    """model_fn(i, t, x) -> the model output at step i (a list of outputs works through `outputs.__getitem__`-style lambdas);
    noises[i]: the draw of step i (SDE only).  Returns [x after step 0, ..., x after step n - 1], fp64."""
    ac = sched_ref.alphas_cumprod() if ac is None else ac
    ts = timesteps(n, spacing)
    order = orders(n, solver_order, lower_order_final)
    sde = algorithm_type == "sde-dpmsolver++"
    assert sde or algorithm_type == "dpmsolver++"
    assert solver_type in ("midpoint", "heun")
    x = x.double()
    traj, m1 = [], None
    for i, s in enumerate(ts):
        ab_s, ab_t = ac[s], ac[ts[i + 1]] if i + 1 < n else ac[0]
        al_t, sg_t, sg_s = math.sqrt(ab_t), math.sqrt(1 - ab_t), math.sqrt(1 - ab_s)
        h = _lam(ab_t) - _lam(ab_s)
        m0 = data_prediction(model_fn(i, s, x).double(), x, ab_s, prediction_type)
        if sde:
            x = sg_t / sg_s * math.exp(-h) * x + al_t * (1 - math.exp(-2 * h)) * m0 + sg_t * math.sqrt(1 - math.exp(-2 * h)) * noises[i].double()
        else:
            x = sg_t / sg_s * x - al_t * (math.exp(-h) - 1) * m0
        if order[i] == 2:
            r0 = (_lam(ab_s) - _lam(ac[ts[i - 1]])) / h
            d1 = (m0 - m1) / r0
            if sde and solver_type == "midpoint":
                x = x + 0.5 * al_t * (1 - math.exp(-2 * h)) * d1
            elif sde:
                x = x + al_t * ((1 - math.exp(-2 * h)) / (-2 * h) + 1) * d1
            elif solver_type == "midpoint":
                x = x - 0.5 * al_t * (math.exp(-h) - 1) * d1
            else:
                x = x + al_t * ((math.exp(-h) - 1) / h + 1) * d1
        m1 = m0
        traj.append(x)
    return traj


def ddim_trajectory(outputs, x, n, prediction_type="epsilon", ac=None):
    """Deterministic DDIM over the leading timesteps on the same table, fp64 (oracle.sched_ref.ddim_step, plus v-prediction)."""
    ac = sched_ref.alphas_cumprod() if ac is None else ac
    x = x.double()
    traj = []
    for i, t in enumerate(sched_ref.leading_timesteps(n)):
        prev = t - 1000 // n
        a_t, a_p = ac[t], (ac[prev] if prev >= 0 else ac[0])
        out = outputs[i].double()
        x0 = data_prediction(out, x, a_t, prediction_type)
        eps = out if prediction_type == "epsilon" else math.sqrt(a_t) * out + math.sqrt(1 - a_t) * x
        x = math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps
        traj.append(x)
    return traj


def traj_err(got, ref):
    """max over the steps of rel-L2(got[i], ref[i])."""
    return max(((g.double() - r).norm() / r.norm()).item() for g, r in zip(got, ref))
