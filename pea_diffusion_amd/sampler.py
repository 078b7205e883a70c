"""Inference denoise loop on the HIP UNet: the scheduler object and loop body that
`StableDiffusionTest.__call__` drives (tests/test_sdxl_zh.py:350-406; ControlNet variant
tests/test_sdxl_zh_controlnet.py:437-553).  `DPMSolverMultistep` exposes the four members the reference touches --
`set_timesteps`, `timesteps`, `scale_model_input`, `step(...)[0]` -- with the configuration the reference loads
(:145, DPMSolverMultistepScheduler on the SDXL scheduler config: scaled-linear betas, epsilon prediction, "leading"
spacing with offset 1, dpmsolver++ 2M midpoint, lower_order_final).  The schedule's scalars are host float64; the
latent update, the CFG combine and `rescale_noise_cfg` are HIP kernels (csrc/sampler.hip).  `LCMScheduler` is the few-step
sampler of the LCM-LoRA program (tests/test_sdxl_zh_lcm.py:178) on the same surface."""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from . import ops


class DPMSolverMultistep:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 timestep_spacing: str = "leading", steps_offset: int = 1, solver_order: int = 2,
                 lower_order_final: bool = True, final_sigma: str = "sigma_min"):
        if solver_order not in (1, 2):
            raise ValueError("solver_order 1 or 2")
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.num_train_timesteps = num_train_timesteps
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset
        self.solver_order, self.lower_order_final, self.final_sigma = solver_order, lower_order_final, final_sigma
        self.timesteps = None

    # ------------------------------------------------------------------ schedule (host)
    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, num_inference_steps
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif self.timestep_spacing == "trailing":
            ts = (np.arange(T, 0, -T / n).round() - 1).astype(np.int64)
        else:
            raise ValueError(f"timestep_spacing {self.timestep_spacing!r}")
        sig = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        last = {"sigma_min": sig[0], "zero": 0.0, "repeat": sigmas[-1]}[self.final_sigma]
        self.sigmas = np.concatenate([sigmas, [last]])
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = n
        self._i = 0
        self._lower = 0
        self._x0_prev = None
        return self.timesteps

    def set_begin_index(self, begin_index: int = 0):
        """Start the solver at position `begin_index` of the schedule (img2img / inpainting with strength < 1 run
        `timesteps[t_start:]`): as diffusers 0.23 derives the step index from the timestep's position in the FULL schedule, the
        coefficients are those of that position, the first step is first order (no earlier data prediction exists) and the
        lower_order_final test keeps using the full length."""
        if self.timesteps is None:
            raise ValueError("set_begin_index: call set_timesteps first")
        if not 0 <= begin_index < len(self.timesteps):
            raise ValueError(f"set_begin_index: {begin_index} outside the {len(self.timesteps)}-step schedule")
        self._i = int(begin_index)
        self._lower = 0
        self._x0_prev = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    @staticmethod
    def _alpha_sigma(sigma):
        a = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return a, sigma * a

    def _coefficients(self, i: int, order: int):
        lam = lambda a, s: (math.log(a) - math.log(s)) if s > 0 else float("inf")
        a_t, s_t = self._alpha_sigma(self.sigmas[i + 1])
        a_s, s_s = self._alpha_sigma(self.sigmas[i])
        h = lam(a_t, s_t) - lam(a_s, s_s)
        em = math.expm1(-h) if math.isfinite(h) else -1.0
        c_s = s_t / s_s
        if order == 1:
            return a_s, s_s, c_s, -a_t * em, 0.0
        a_p, s_p = self._alpha_sigma(self.sigmas[i - 1])
        r0 = (lam(a_s, s_s) - lam(a_p, s_p)) / h
        return a_s, s_s, c_s, -a_t * em * (1.0 + 0.5 / r0), 0.5 * a_t * em / r0

    # ------------------------------------------------------------------ one step (device)
    def step(self, model_output, timestep, sample, return_dict: bool = False, **kwargs):
        """`latents = scheduler.step(noise_pred, t, latents, return_dict=False)[0]` (:406).  fp32 CUDA tensors;
        `sample` is updated IN PLACE and returned."""
        order, (a_s, s_s, c_s, c0, c1) = self.next_step_plan()
        if sample.dtype != torch.float32 or not sample.is_contiguous():
            sample = sample.float().contiguous()
        eps = model_output.float().contiguous()
        if self._x0_prev is None:
            self._x0_prev = torch.zeros_like(sample)
        ops.dpm_update_(sample, eps, self._x0_prev, a_s, s_s, c_s, c0, c1)
        self._advance()
        return (sample,)

    def next_step_plan(self):
        """host side of the next `step`: (order, (alpha_s, sigma_s, c_s, c_0, c_1))"""
        i, n = self._i, len(self.timesteps)
        final = (i == n - 1) and self.lower_order_final and n < 15
        order = 1 if (self.solver_order == 1 or self._lower < 1 or final) else 2
        return order, self._coefficients(i, order)

    def _advance(self):
        if self._lower < self.solver_order:
            self._lower += 1
        self._i += 1


class LCMScheduler:
    """`LCMScheduler.from_config(pipe.scheduler.config)` of the LCM-LoRA program (tests/test_sdxl_zh_lcm.py:178; 5 steps at
    guidance_scale 0, :335-336) as diffusers 0.23 configures it from the SDXL scheduler config: scaled-linear betas,
    epsilon prediction, no clipping or thresholding, original_inference_steps 50, boundary scalings with sigma_data 0.5 and
    timestep scaling 10.  Host scalars are float64; the tensor work of a step is one HIP kernel (ops.lcm_update_).
    `step` draws its noise as diffusers' randn_tensor does -- on the generator's device, so a CPU generator draws on the CPU
    and the draw is copied over -- in fp32, or takes it as `noise=`.  The guidance-embedding UNets (`time_cond_proj`) of
    fully distilled LCM checkpoints are not built here: LCM-LoRA on a plain UNet is the supported form."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 original_inference_steps: int = 50, timestep_scaling: float = 10.0, sigma_data: float = 0.5):
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.final_alpha_cumprod = self.alphas_cumprod[0]          # set_alpha_to_one = False
        self.num_train_timesteps = num_train_timesteps
        self.original_inference_steps = original_inference_steps
        self.timestep_scaling, self.sigma_data = timestep_scaling, sigma_data
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        n, orig = num_inference_steps, self.original_inference_steps
        if not 1 <= n <= orig <= self.num_train_timesteps:
            raise ValueError(f"LCMScheduler: {n} steps outside 1..{orig} (original_inference_steps)")
        origin = np.arange(1, orig + 1) * (self.num_train_timesteps // orig) - 1
        ts = origin[::-(orig // n)][:n].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)
        self.num_inference_steps = n
        self._i = 0
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def boundary_scalings(self, t):
        """(c_skip, c_out) of the consistency parameterisation at timestep t"""
        st, sd2 = self.timestep_scaling * float(t), self.sigma_data ** 2
        return sd2 / (st * st + sd2), st / math.sqrt(st * st + sd2)

    def next_step_plan(self):
        """host side of the next `step`: (last, (sqrt(a_t), sqrt(1 - a_t), c_skip, c_out, sqrt(a_prev), sqrt(1 - a_prev)))"""
        i, n = self._i, len(self.timesteps)
        if i >= n:
            raise ValueError("LCMScheduler.step: past the end of the schedule; call set_timesteps")
        t = int(self.timesteps[i])
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[int(self.timesteps[i + 1])] if i + 1 < n else self.final_alpha_cumprod
        c_skip, c_out = self.boundary_scalings(t)
        return i == n - 1, (math.sqrt(a_t), math.sqrt(1.0 - a_t), c_skip, c_out, math.sqrt(a_prev), math.sqrt(1.0 - a_prev))

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = False, noise=None, **kwargs):
        """-> (prev_sample, denoised).  fp32 CUDA tensors; `sample` is updated IN PLACE and returned."""
        last, (sa, sb, c_skip, c_out, sp, sn) = self.next_step_plan()
        if sample.dtype != torch.float32 or not sample.is_contiguous():
            sample = sample.float().contiguous()
        eps = model_output.float().contiguous()
        if last:
            noise = None
        elif noise is None:
            dev = generator.device if generator is not None else sample.device
            noise = torch.randn(sample.shape, generator=generator, device=dev, dtype=torch.float32)
        if noise is not None:
            noise = noise.to(sample.device, torch.float32).contiguous()
        denoised = torch.empty_like(sample)
        ops.lcm_update_(sample, eps, noise, c_out / sa + c_skip, -c_out * sb / sa, 1.0 if last else sp, sn, denoised)
        self._i += 1
        return (sample, denoised)


def denoise(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps: int = 30,
            guidance_scale: float = 7.5, guidance_rescale: float = 0.0,
            residual_fn: Optional[Callable] = None, callback: Optional[Callable] = None, generator=None,
            timestep_cond=None):
    """Steps 4-7 of the reference pipeline call (tests/test_sdxl_zh.py:350-406): timesteps, CFG batch doubling, UNet,
    guidance (+ rescale), scheduler step.  `unet` is a `HipUNet` built for batch 2B when guidance_scale > 1.
    `residual_fn(latent_model_input, t) -> (down_residuals, mid_residual)` is where a ControlNet plugs in
    (tests/test_sdxl_zh_controlnet.py:510-535).  Returns the final latents (fp32, the VAE decode stays outside).
    `generator` goes to `scheduler.step` (the LCMScheduler draws noise between steps, tests/test_sdxl_zh_lcm.py:398; with
    guidance_scale <= 1, the LCM-LoRA case, the loop runs at batch B without the CFG kernels).  `timestep_cond`, the
    guidance embedding of fully distilled LCM UNets (`time_cond_proj`), is refused: those UNets are not built here."""
    if timestep_cond is not None:
        raise ValueError("denoise: timestep_cond (guidance-embedding LCM UNets) is not supported; use LCM-LoRA on a plain UNet")
    do_cfg = guidance_scale > 1.0
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    for i, t in enumerate(timesteps):
        x = torch.cat([latents] * 2) if do_cfg else latents
        x = scheduler.scale_model_input(x, t)
        kw = {}
        if residual_fn is not None:
            down, mid = residual_fn(x, t)
            kw = dict(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        noise_pred = unet(x, t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                          return_dict=False, **kw)[0]
        if do_cfg:
            noise_pred = ops.cfg_combine(noise_pred.float(), guidance_scale, guidance_rescale)
        latents = scheduler.step(noise_pred, t, latents, return_dict=False, generator=generator)[0]
        if callback is not None:
            callback(i, t, latents)
    return latents
