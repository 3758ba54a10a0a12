"""DDPM / DDIM scheduler arithmetic -- restated from diffusers==0.24 `DDPMScheduler` / `DDIMScheduler` as the reference
uses them (omni/models/dreamllm/modeling_plugins.py:379-381,534-536,551,787-788,812,833; `_compute_snr` :468-491).
SD-2.1 scheduler_config: scaled_linear betas 0.00085 -> 0.012 over 1000 steps, steps_offset 1, clip_sample False,
set_alpha_to_one False, "leading" timestep spacing.  Host-side tables + tiny latent updates; the
denoising loop's per-step update runs as the fused HIP kernel `dllm_cfg_ddim_step` (see `DDIMScheduler.step_cfg_fused_`), or,
for every other graphed loop, `dllm_cfg_sched_step` on the coefficients of `step_coeffs`.
`DPMSolverMultistepScheduler` (the `"dpm"` branch of omni/utils/block_utils.py:34-47) restates diffusers==0.24's class of that name
for the `++` algorithm types at order 1 and 2; its graphed step is `dllm_cfg_dpm_step` on the coefficients of `multistep_coeffs`.
"""
from __future__ import annotations

import json
import math
import os
from types import SimpleNamespace
from typing import NamedTuple

import torch

from .utils import randn_tensor

SD21_SCHED = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                  prediction_type="epsilon", steps_offset=1, clip_sample=False, set_alpha_to_one=False,
                  timestep_spacing="leading", variance_type="fixed_small")


class StepCoeffs(NamedTuple):
    """`step()` at one timestep as plain floats (the operands of the fused HIP step `dllm_cfg_sched_step`):
    x0 = (x - sqrt_1mat e) / sqrt_at, eps = e  (epsilon)  or  x0 = sqrt_at x - sqrt_1mat e, eps = sqrt_at e + sqrt_1mat x  (v);
    x_prev = k_x0 x0 + k_eps eps + k_x x + sigma z, with z ~ N(0, 1) drawn (randn_tensor, NCHW) iff `draws`."""
    sqrt_at: float
    sqrt_1mat: float
    k_x0: float
    k_eps: float
    k_x: float
    sigma: float
    draws: bool


class MultistepCoeffs(NamedTuple):
    """One step of `DPMSolverMultistepScheduler` as plain floats (the operands of the fused HIP step `dllm_cfg_dpm_step`):
    m0 = (x - sqrt_1mat e) / sqrt_at  (epsilon)  or  m0 = sqrt_at x - sqrt_1mat e  (v);  m1: the m0 of the step before;
    x_next = k_x x + k_m0 m0 + k_m1 m1 + sigma z, with z ~ N(0, 1) drawn (randn_tensor, NCHW) iff `draws`.  k_m1 == 0 on a
    first-order step: m1 is not read there."""
    sqrt_at: float
    sqrt_1mat: float
    k_x: float
    k_m0: float
    k_m1: float
    sigma: float
    draws: bool


# DPMSolverMultistepScheduler's own keys (diffusers 0.24 defaults) on top of SD21_SCHED; the last two are read only to be refused
DPM_SCHED = dict(solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                 timestep_spacing="linspace", thresholding=False, use_karras_sigmas=False)


def _load_cfg(name_or_path, extra=None):
    d = dict(SD21_SCHED)
    if extra:
        d.update(extra)
    if isinstance(name_or_path, dict):
        d.update(name_or_path.get("scheduler", {}))
    elif isinstance(name_or_path, str):
        fp = os.path.join(name_or_path, "scheduler", "scheduler_config.json")
        if os.path.isfile(fp):
            with open(fp) as f:
                raw = json.load(f)
            d.update({k: raw[k] for k in d if k in raw})
    return d


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **cfg):
        d = dict(SD21_SCHED, **cfg)
        self.config = SimpleNamespace(**d)
        T = d["num_train_timesteps"]
        if d["beta_schedule"] == "scaled_linear":
            betas = torch.linspace(d["beta_start"] ** 0.5, d["beta_end"] ** 0.5, T, dtype=torch.float32) ** 2
        elif d["beta_schedule"] == "linear":
            betas = torch.linspace(d["beta_start"], d["beta_end"], T, dtype=torch.float32)
        else:
            raise ValueError(f"unsupported beta_schedule {d['beta_schedule']}")
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if d["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.timesteps = torch.arange(T - 1, -1, -1)
        self.num_inference_steps = None

    @classmethod
    def from_name_or_path(cls, name_or_path):
        return cls(**_load_cfg(name_or_path))

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        """'leading' spacing: t_i = i * (T // N) + steps_offset, descending."""
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        ts = (torch.arange(0, num_inference_steps) * ratio).round().flip(0).long() + self.config.steps_offset
        self.timesteps = ts.to(device) if device is not None else ts

    def _ab(self, x, timesteps):
        ac = self.alphas_cumprod.to(device=x.device)
        a = ac[timesteps].float() ** 0.5
        b = (1 - ac[timesteps].float()) ** 0.5
        while a.dim() < x.dim():
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        return a, b

    def add_noise(self, original_samples, noise, timesteps):
        """x_t = sqrt(abar_t) x_0 + sqrt(1 - abar_t) eps   (modeling_plugins.py:534-536)."""
        a, b = self._ab(original_samples, timesteps)
        return (a * original_samples.float() + b * noise.float()).to(original_samples.dtype)

    def get_velocity(self, sample, noise, timesteps):
        """v = sqrt(abar_t) eps - sqrt(1 - abar_t) x_0   (modeling_plugins.py:551)."""
        a, b = self._ab(sample, timesteps)
        return (a * noise.float() - b * sample.float()).to(sample.dtype)

    def _x0_eps(self, model_output, t, sample):
        a_t = self.alphas_cumprod[t].item()
        if self.config.prediction_type == "epsilon":
            eps = model_output
            x0 = (sample - (1 - a_t) ** 0.5 * eps) / a_t**0.5
        elif self.config.prediction_type == "v_prediction":
            x0 = a_t**0.5 * sample - (1 - a_t) ** 0.5 * model_output
            eps = a_t**0.5 * model_output + (1 - a_t) ** 0.5 * sample
        else:
            raise ValueError(self.config.prediction_type)
        return x0, eps, a_t


class DDPMScheduler(_SchedulerBase):
    """Ancestral sampling step, variance_type fixed_small (the reference head's own scheduler, modeling_plugins.py:833)."""

    def step(self, model_output, t, sample, eta=0.0, generator=None):
        t = int(t)
        T = self.config.num_train_timesteps
        prev_t = t - T // (self.num_inference_steps or T)
        x0, _, a_t = self._x0_eps(model_output.float(), t, sample.float())
        a_prev = self.alphas_cumprod[prev_t].item() if prev_t >= 0 else 1.0
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        mean = (a_prev**0.5 * cur_beta) / (1 - a_t) * x0 + cur_alpha**0.5 * (1 - a_prev) / (1 - a_t) * sample.float()
        if t > 0:
            var = max((1 - a_prev) / (1 - a_t) * cur_beta, 1e-20)
            noise = randn_tensor(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)
            mean = mean + var**0.5 * noise
        return mean.to(sample.dtype)

    def step_coeffs(self, t, eta=0.0):
        """`step()` at timestep t as StepCoeffs, from the same `.item()` floats (`eta` is ignored, as in `step()`)."""
        t = int(t)
        T = self.config.num_train_timesteps
        prev_t = t - T // (self.num_inference_steps or T)
        a_t = self.alphas_cumprod[t].item()
        a_prev = self.alphas_cumprod[prev_t].item() if prev_t >= 0 else 1.0
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        sigma = max((1 - a_prev) / (1 - a_t) * cur_beta, 1e-20) ** 0.5 if t > 0 else 0.0
        return StepCoeffs(a_t**0.5, (1 - a_t) ** 0.5, (a_prev**0.5 * cur_beta) / (1 - a_t), 0.0,
                          cur_alpha**0.5 * (1 - a_prev) / (1 - a_t), sigma, t > 0)


class DDIMScheduler(_SchedulerBase):
    """Deterministic DDIM (eta = 0) as installed by the benchmark (BASELINE config 3: "50 DDIM steps")."""

    def alphas_for(self, t):
        t = int(t)
        T = self.config.num_train_timesteps
        prev_t = t - T // self.num_inference_steps
        a_t = self.alphas_cumprod[t].item()
        a_prev = self.alphas_cumprod[prev_t].item() if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def step(self, model_output, t, sample, eta=0.0, generator=None):
        x0, eps, a_t = self._x0_eps(model_output.float(), int(t), sample.float())
        _, a_prev = self.alphas_for(t)
        var = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
        std = eta * var**0.5
        prev = a_prev**0.5 * x0 + max(1 - a_prev - std**2, 0.0) ** 0.5 * eps
        if eta > 0:
            prev = prev + std * randn_tensor(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)
        return prev.to(sample.dtype)

    def step_coeffs(self, t, eta=0.0):
        """`step()` at timestep t as StepCoeffs, from the same `.item()` floats; noise is drawn only when eta > 0."""
        a_t, a_prev = self.alphas_for(t)
        var = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
        std = eta * var**0.5
        return StepCoeffs(a_t**0.5, (1 - a_t) ** 0.5, a_prev**0.5, max(1 - a_prev - std**2, 0.0) ** 0.5, 0.0, std, eta > 0)

    def step_cfg_fused_(self, noise_pred_nhwc, t, latents_nhwc, next_in, guidance_scale):
        """CFG combine + eta=0 update + next UNet input in ONE kernel (in place on the fp32 NHWC latents)."""
        from . import ops
        a_t, a_prev = self.alphas_for(t)
        return ops.cfg_ddim_step_(noise_pred_nhwc, latents_nhwc, next_in, guidance_scale, a_t, a_prev,
                                  self.config.prediction_type == "v_prediction")


class DPMSolverMultistepScheduler(_SchedulerBase):
    """DPM-Solver++ multistep, orders 1 and 2 (diffusers 0.24 `DPMSolverMultistepScheduler` with `algorithm_type` "dpmsolver++" or
    "sde-dpmsolver++", `solver_type` "midpoint" or "heun", no thresholding, no Karras sigmas).  With abar = alphas_cumprod,
    alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln alpha - ln sigma, s the current timestep, t the next entry of
    `timesteps` (training timestep 0 after the last one), m0 / m1 the data predictions at s and at the step before (timestep s1),
    h = lambda_t - lambda_s, r0 = (lambda_s - lambda_s1) / h and D1 = (m0 - m1) / r0:
      deterministic  x_t = (sigma_t / sigma_s) x - alpha_t (e^-h - 1) m0   [- 1/2 alpha_t (e^-h - 1) D1            midpoint]
                                                                             [+ alpha_t ((e^-h - 1) / h + 1) D1       heun]
      SDE            x_t = (sigma_t / sigma_s) e^-h x + alpha_t (1 - e^-2h) m0 + sigma_t sqrt(1 - e^-2h) z
                                                                             [+ 1/2 alpha_t (1 - e^-2h) D1            midpoint]
                                                                             [+ alpha_t ((1 - e^-2h) / (-2h) + 1) D1  heun]
    The bracketed term is there on second-order steps only (`order_at`).  `step()` keeps m1 on the object for the plain loop; the
    graphed loop keeps it in a device buffer of its own and takes the step as `multistep_coeffs(i)`."""

    def __init__(self, **cfg):
        super().__init__(**dict(DPM_SCHED, **cfg))
        c = self.config
        allowed = dict(solver_order=(1, 2), algorithm_type=("dpmsolver++", "sde-dpmsolver++"), solver_type=("midpoint", "heun"),
                       lower_order_final=(True, False), timestep_spacing=("linspace", "leading", "trailing"),
                       thresholding=(False,), use_karras_sigmas=(False,))
        for key, ok in allowed.items():
            v = getattr(c, key)
            if isinstance(v, bool) != isinstance(ok[0], bool) or v not in ok:
                raise ValueError(f"DPMSolverMultistepScheduler: unsupported {key}={v!r} (supported: {', '.join(map(repr, ok))})")
        self._reset()

    @classmethod
    def from_name_or_path(cls, name_or_path):
        return cls(**_load_cfg(name_or_path, DPM_SCHED))

    def _reset(self):
        self._ts = None        # the schedule as host ints
        self._step_index = 0   # state of the stateful `step()`: which entry of `timesteps` comes next ...
        self._m1 = None        # ... and the data prediction of the step before

    def set_timesteps(self, num_inference_steps, device=None):
        """Descending schedule of N steps; also forgets the multistep history.  'leading': the base class's; 'linspace':
        linspace(0, T - 1, N + 1).round()[::-1][:-1]; 'trailing': round(arange(T, 0, -T / N)) - 1 (rounding half to even)."""
        T, N = self.config.num_train_timesteps, num_inference_steps
        spacing = self.config.timestep_spacing
        if spacing == "leading":
            super().set_timesteps(N, device)
        else:
            if spacing == "linspace":
                step = (T - 1) / N
                vals = [round(i * step) for i in range(N, 0, -1)]
            else:
                delta = (T - T / N) - T  # numpy's arange: the difference of its first two entries, N entries
                vals = [round(T + i * delta) - 1 for i in range(N)]
            self.num_inference_steps = N
            ts = torch.tensor(vals, dtype=torch.long)
            self.timesteps = ts.to(device) if device is not None else ts
        self._reset()
        self._ts = [int(v) for v in self.timesteps.tolist()]

    def order_at(self, i):
        """Order of the update at step i of N: 1 on the first step (no history), with solver_order 1, and on the last step of a
        short schedule (lower_order_final, N < 15); else 2."""
        N = len(self._ts)
        if i == 0 or self.config.solver_order == 1 or (i == N - 1 and self.config.lower_order_final and N < 15):
            return 1
        return 2

    def _terms(self, i):
        """Step i as host floats, all from `alphas_cumprod[.].item()`: (alpha_s, sigma_s, alpha_t, sigma_t, h, r0); r0 is None on a
        first-order step."""
        if self._ts is None:
            raise ValueError("DPMSolverMultistepScheduler: call set_timesteps() first")
        ab_s = self.alphas_cumprod[self._ts[i]].item()
        ab_t = self.alphas_cumprod[self._ts[i + 1] if i + 1 < len(self._ts) else 0].item()
        lam = lambda ab: 0.5 * (math.log(ab) - math.log(1 - ab))  # noqa: E731
        h = lam(ab_t) - lam(ab_s)
        r0 = None
        if self.order_at(i) == 2:
            r0 = (lam(ab_s) - lam(self.alphas_cumprod[self._ts[i - 1]].item())) / h
        return ab_s**0.5, (1 - ab_s) ** 0.5, ab_t**0.5, (1 - ab_t) ** 0.5, h, r0

    def _weights(self, i):
        """(k_x, w_m0, w_d1, sigma) of x_t = k_x x + w_m0 m0 + w_d1 D1 + sigma z at step i (w_d1 = 0.0 at order 1)."""
        _, s_s, a_t, s_t, h, r0 = self._terms(i)
        if self.config.algorithm_type == "dpmsolver++":
            em1 = math.expm1(-h)                  # e^-h - 1
            k_x, w_m0, sigma = s_t / s_s, -a_t * em1, 0.0
            w_d1 = -0.5 * a_t * em1 if self.config.solver_type == "midpoint" else a_t * (em1 / h + 1.0)
        else:
            om = -math.expm1(-2.0 * h)            # 1 - e^-2h
            k_x, w_m0, sigma = s_t / s_s * math.exp(-h), a_t * om, s_t * om**0.5
            w_d1 = 0.5 * a_t * om if self.config.solver_type == "midpoint" else a_t * (om / (-2.0 * h) + 1.0)
        return k_x, w_m0, (w_d1 if r0 is not None else 0.0), sigma

    def step(self, model_output, t, sample, eta=0.0, generator=None):
        """One step of the plain loop, in `timesteps` order (`eta` is ignored; `set_timesteps` starts a new trajectory)."""
        i = self._step_index
        if self._ts is None or i >= len(self._ts) or int(t) != self._ts[i]:
            raise ValueError(f"DPMSolverMultistepScheduler.step: timestep {int(t)} is not entry {i} of the schedule set by "
                             "set_timesteps() (the multistep history follows `timesteps` in order)")
        x = sample.float()
        m0, _, _ = self._x0_eps(model_output.float(), int(t), x)
        k_x, w_m0, w_d1, sigma = self._weights(i)
        out = k_x * x + w_m0 * m0
        if w_d1 != 0.0:
            out = out + w_d1 * ((m0 - self._m1) / self._terms(i)[5])
        if sigma != 0.0:
            out = out + sigma * randn_tensor(sample.shape, generator=generator, device=sample.device, dtype=torch.float32)
        self._m1 = m0
        self._step_index = i + 1
        return out.to(sample.dtype)

    def multistep_coeffs(self, i):
        """Step i of the schedule as MultistepCoeffs, from the same `.item()` floats as `step()` (D1 folded into m0 and m1)."""
        a_s, s_s, _, _, _, r0 = self._terms(i)
        k_x, w_m0, w_d1, sigma = self._weights(i)
        d = w_d1 / r0 if r0 is not None else 0.0
        return MultistepCoeffs(a_s, s_s, k_x, w_m0 + d, -d, sigma, self.config.algorithm_type == "sde-dpmsolver++")
