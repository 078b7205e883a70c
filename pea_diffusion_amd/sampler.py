"""Inference denoise loop on the HIP UNet: the scheduler object and loop body that
`StableDiffusionTest.__call__` drives (tests/test_sdxl_zh.py:350-406; ControlNet variant
tests/test_sdxl_zh_controlnet.py:437-553).  `DPMSolverMultistep` exposes the four members the reference touches --
`set_timesteps`, `timesteps`, `scale_model_input`, `step(...)[0]` -- with the configuration the reference loads
(:145, DPMSolverMultistepScheduler on the SDXL scheduler config: scaled-linear betas, epsilon prediction, "leading"
spacing with offset 1, dpmsolver++ 2M midpoint, lower_order_final).  The schedule's scalars are host float64; the
latent update, the CFG combine and `rescale_noise_cfg` are HIP kernels (csrc/sampler.hip).  `LCMScheduler` is the few-step
sampler of the LCM-LoRA program (tests/test_sdxl_zh_lcm.py:178) on the same surface; `EulerDiscrete` (plain SDXL checkpoints)
and `EulerAncestralDiscrete` (SDXL-Turbo, README "Sampling Acceleration") are the sigma-space schedulers, whose step kernel
also writes the next UNet input."""
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

    def model_input_scale(self) -> float:
        """the factor `scale_model_input` applies at the current position: 1 (alpha-space)"""
        return 1.0

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
    and the draw is copied over -- in fp32, or takes it as `noise=`.  Fully distilled LCM checkpoints (LCM-SDXL) take the guidance
    scale as `timestep_cond` instead: `guidance_scale_embedding` -> `denoise(..., timestep_cond=)` on a `lcm_sdxl_config()` UNet."""
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

    def model_input_scale(self) -> float:
        """the factor `scale_model_input` applies at the current position: 1 (alpha-space)"""
        return 1.0

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


class EulerDiscrete:
    """`EulerDiscreteScheduler` as diffusers 0.23 configures it from the SDXL scheduler config (what plain SDXL checkpoints
    ship with; the reference's demo scripts import it next to DPM-Solver): scaled-linear betas, epsilon prediction, linear
    sigma interpolation, no Karras sigmas, s_churn 0; the default is SDXL base ("leading" spacing, offset 1).  It works in
    sigma space: `init_noise_sigma != 1` and the UNet reads `sample / sqrt(sigma^2 + 1)`.  Host scalars are float64; a step
    is one HIP kernel (ops.euler_update_) that also writes the NEXT step's scaled (and, for CFG, doubled) model input, which
    `scale_model_input` hands out when it is given that step's result -- the identical tensor object, not modified in
    between; anything else gets the entry form of the same kernel.  `dup=2` asks for the CFG-doubled batch
    (`cat([x] * 2)` of the loop) from the kernel instead of from torch.cat."""
    order = 1
    init_noise_sigma = None            # known after set_timesteps
    fused_model_input = True           # denoise(): scale_model_input(latents, t, dup=) replaces cat + scale
    ancestral = False

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 timestep_spacing: str = "leading", steps_offset: int = 1):
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(f"timestep_spacing {timestep_spacing!r}")
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas)
        self.num_train_timesteps = num_train_timesteps
        self.timestep_spacing, self.steps_offset = timestep_spacing, steps_offset
        self.timesteps = None
        self._dup, self._ready, self._buf = 1, None, None

    # ------------------------------------------------------------------ schedule (host)
    def set_timesteps(self, num_inference_steps: int, device=None):
        T, n = self.num_train_timesteps, num_inference_steps
        if not 1 <= n <= T:
            raise ValueError(f"{type(self).__name__}: {n} steps outside 1..{T}")
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float64) + self.steps_offset
        elif self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n, dtype=np.float64)[::-1].copy()
        else:
            ts = np.arange(T, 0, -T / n).round() - 1
        sig = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = np.concatenate([sigmas, [0.0]])
        smax = float(sigmas.max())
        self.init_noise_sigma = smax if self.timestep_spacing in ("linspace", "trailing") else math.sqrt(smax * smax + 1.0)
        # integral for "leading" / "trailing"; "linspace" keeps its fractional timesteps
        self.timesteps = torch.from_numpy(ts if self.timestep_spacing == "linspace" else ts.astype(np.int64))
        self.num_inference_steps = n
        self._i = 0
        self._ready = None
        return self.timesteps

    def set_begin_index(self, begin_index: int = 0):
        """start at position `begin_index` of the schedule (img2img / inpainting with strength < 1 run `timesteps[t_start:]`)"""
        if self.timesteps is None:
            raise ValueError("set_begin_index: call set_timesteps first")
        if not 0 <= begin_index < len(self.timesteps):
            raise ValueError(f"set_begin_index: {begin_index} outside the {len(self.timesteps)}-step schedule")
        self._i = int(begin_index)
        self._ready = None

    def _step_sigmas(self, sigma_from: float, sigma_to: float):
        """(sigma_down, sigma_up)"""
        return sigma_to, 0.0

    def next_step_plan(self):
        """host side of the next `step`: (draws noise, (sigma, sigma_to, sigma_down, sigma_up, k_s)); the kernel's scalars are
        k_e = sigma_down - sigma, k_n = sigma_up and k_s = 1 / sqrt(sigma_to^2 + 1), the next model input's scale"""
        if self.timesteps is None or self._i >= len(self.timesteps):
            raise ValueError(f"{type(self).__name__}.step: past the end of the schedule; call set_timesteps")
        sigma, sigma_to = float(self.sigmas[self._i]), float(self.sigmas[self._i + 1])
        down, up = self._step_sigmas(sigma, sigma_to)
        return up > 0.0, (sigma, sigma_to, down, up, 1.0 / math.sqrt(sigma_to * sigma_to + 1.0))

    # ------------------------------------------------------------------ device
    def _model_in(self, x, dup):
        shape = (dup * x.shape[0],) + tuple(x.shape[1:])
        if self._buf is None or tuple(self._buf.shape) != shape or self._buf.device != x.device:
            self._buf = torch.empty(shape, device=x.device, dtype=torch.float32)
        return self._buf

    def model_input_scale(self) -> float:
        """the factor `scale_model_input` applies at the current position, 1 / sqrt(sigma^2 + 1), as the fp32 value its kernel
        multiplies by"""
        if self.timesteps is None:
            raise ValueError("model_input_scale: call set_timesteps first")
        sigma = float(self.sigmas[min(self._i, len(self.sigmas) - 1)])
        return float(np.float32(1.0 / math.sqrt(sigma * sigma + 1.0)))

    def scale_model_input(self, sample, timestep=None, dup: int = 1):
        """`sample / sqrt(sigma^2 + 1)`, [dup * B, ...] fp32: the buffer the previous `step` filled when `sample` is that
        step's result, else one launch of the entry form.  The buffer is reused from call to call."""
        if self.timesteps is None:
            raise ValueError("scale_model_input: call set_timesteps first")
        if self._ready is not None and sample is self._ready[0] and dup == self._dup:
            model_in, self._ready = self._ready[1], None
            return model_in
        self._dup, self._ready = int(dup), None
        x = sample if sample.dtype == torch.float32 and sample.is_contiguous() else sample.float().contiguous()
        sigma = float(self.sigmas[min(self._i, len(self.sigmas) - 1)])
        model_in = self._model_in(x, self._dup)
        ops.euler_update_(x, None, None, model_in, 0.0, 0.0, 1.0 / math.sqrt(sigma * sigma + 1.0), self._dup)
        return model_in

    def step(self, model_output, timestep, sample, generator=None, return_dict: bool = False, noise=None, **kwargs):
        """-> (prev_sample,).  fp32 CUDA tensors; `sample` is updated IN PLACE and returned.  The ancestral form draws its
        noise as `LCMScheduler.step` does (on the generator's device, fp32) or takes it as `noise=`; none when sigma_up is 0."""
        draws, (sigma, sigma_to, down, up, k_s) = self.next_step_plan()
        if sample.dtype != torch.float32 or not sample.is_contiguous():
            sample = sample.float().contiguous()
        eps = model_output.float().contiguous()
        if not draws:
            noise = None
        elif noise is None:
            dev = generator.device if generator is not None else sample.device
            noise = torch.randn(sample.shape, generator=generator, device=dev, dtype=torch.float32)
        if noise is not None:
            noise = noise.to(sample.device, torch.float32).contiguous()
        last = self._i == len(self.timesteps) - 1
        model_in = None if last else self._model_in(sample, self._dup)
        ops.euler_update_(sample, eps, noise, model_in, down - sigma, up, k_s, self._dup)
        self._i += 1
        self._ready = None if last else (sample, model_in)
        return (sample,)

    def add_noise(self, original_samples, noise, begin_index: int = 0):
        """`original + sigma * noise` at position `begin_index` of the schedule (the start of a strength < 1 run), fp32"""
        x = original_samples.float().contiguous().clone()
        z = noise.to(x.device, torch.float32).contiguous()
        return ops.euler_update_(x, z, None, None, float(self.sigmas[begin_index]), 0.0, 1.0)


class EulerAncestralDiscrete(EulerDiscrete):
    """`EulerAncestralDiscreteScheduler` (diffusers 0.23) on the same config; the default is what SDXL-Turbo ships with:
    "trailing" spacing, run for 1-4 steps at guidance_scale 0 and 512 x 512.  Each step goes down to sigma_down and adds
    sigma_up of fresh noise, sigma_up^2 + sigma_down^2 = sigma_to^2; the last step (sigma_to = 0) adds none."""
    ancestral = True

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 timestep_spacing: str = "trailing", steps_offset: int = 0):
        super().__init__(num_train_timesteps, beta_start, beta_end, timestep_spacing, steps_offset)

    def _step_sigmas(self, sigma_from: float, sigma_to: float):
        up = math.sqrt(sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2)
        return math.sqrt(sigma_to ** 2 - up ** 2), up


def guidance_scale_embedding(w, embedding_dim: int = 256) -> torch.Tensor:
    """`get_guidance_scale_embedding` of the reference's loop (tests/test_sdxl_zh_inpaint.py:721-745; the LCM pipelines call it
    with w = guidance_scale - 1): [B, embedding_dim] float64 = [sin | cos] of 1000 w * exp(-ln(10000) / (half - 1) * i),
    zero-padded by one column when embedding_dim is odd.  Neither the order nor the divisor of the timestep embedding."""
    w = np.atleast_1d(np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float64))
    if w.ndim != 1:
        raise ValueError(f"guidance_scale_embedding: w must be a scalar or [B], got shape {w.shape}")
    half = embedding_dim // 2
    if half < 2:
        raise ValueError(f"guidance_scale_embedding: embedding_dim={embedding_dim} < 4")
    freq = np.exp(np.arange(half, dtype=np.float64) * -(math.log(10000.0) / (half - 1)))
    arg = (1000.0 * w)[:, None] * freq[None, :]
    emb = np.concatenate([np.sin(arg), np.cos(arg)], axis=1)
    if embedding_dim % 2:
        emb = np.pad(emb, ((0, 0), (0, 1)))
    return torch.from_numpy(emb)


def check_timestep_cond(unet, timestep_cond, do_cfg: bool):
    """`timestep_cond` as the UNet call takes it, or a ValueError for a UNet that has no guidance embedding"""
    if timestep_cond is None:
        return None
    if getattr(unet, "time_cond_proj_dim", None) is None:
        raise ValueError("denoise: timestep_cond needs a guidance-embedded UNet (a config with time_cond_proj_dim, e.g. "
                         "lcm_sdxl_config()); this one has none -- use LCM-LoRA on a plain UNet")
    if do_cfg and timestep_cond.shape[0] * 2 == getattr(unet, "B", 0):
        timestep_cond = torch.cat([timestep_cond] * 2)
    return timestep_cond


def denoise(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps: int = 30,
            guidance_scale: float = 7.5, guidance_rescale: float = 0.0,
            residual_fn: Optional[Callable] = None, callback: Optional[Callable] = None, generator=None,
            timestep_cond=None):
    """Steps 4-7 of the reference pipeline call (tests/test_sdxl_zh.py:350-406): timesteps, CFG batch doubling, UNet,
    guidance (+ rescale), scheduler step.  `unet` is a `HipUNet` built for batch 2B when guidance_scale > 1.
    `residual_fn(latent_model_input, t) -> (down_residuals, mid_residual)` is where a ControlNet plugs in
    (tests/test_sdxl_zh_controlnet.py:510-535).  Returns the final latents (fp32, the VAE decode stays outside).
    `generator` goes to `scheduler.step` (the LCMScheduler draws noise between steps, tests/test_sdxl_zh_lcm.py:398; with
    guidance_scale <= 1, the LCM-LoRA case, the loop runs at batch B without the CFG kernels).  `timestep_cond`
    ([B, time_cond_proj_dim], `guidance_scale_embedding`) goes to a guidance-embedded UNet (one whose config has a
    `time_cond_proj_dim`: fully distilled LCM checkpoints) with every call and is refused for any other.
    With the Euler schedulers (`fused_model_input`) the scaled -- and for CFG doubled -- model input of every step after
    the first comes out of the previous step's kernel: no separate scale launch and no torch.cat."""
    do_cfg = guidance_scale > 1.0
    timestep_cond = check_timestep_cond(unet, timestep_cond, do_cfg)
    ukw = {} if timestep_cond is None else dict(timestep_cond=timestep_cond)
    fused = getattr(scheduler, "fused_model_input", False)
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    for i, t in enumerate(timesteps):
        if fused:
            x = scheduler.scale_model_input(latents, t, dup=2 if do_cfg else 1)
        else:
            x = torch.cat([latents] * 2) if do_cfg else latents
            x = scheduler.scale_model_input(x, t)
        kw = dict(ukw)
        if residual_fn is not None:
            down, mid = residual_fn(x, t)
            kw.update(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        noise_pred = unet(x, t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                          return_dict=False, **kw)[0]
        if do_cfg:
            noise_pred = ops.cfg_combine(noise_pred.float(), guidance_scale, guidance_rescale)
        latents = scheduler.step(noise_pred, t, latents, return_dict=False, generator=generator)[0]
        if callback is not None:
            callback(i, t, latents)
    return latents
