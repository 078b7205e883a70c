"""Self-Attention Guidance (Hong, Lee, Jang, Kim 2023, "Improving Sample Quality of Diffusion Models Using Self-Attention
Guidance"): a second guidance term that needs no training and no weights.  Per denoising step the model's data prediction is
blurred where one self-attention layer looks most, the model is called once more on that degraded input, and the difference
of the two predictions is added to the (classifier-free) guidance.

Per step, with the scheduler's data prediction x0 = c_x x + c_e eps:
  1. the ordinary UNet call; the chosen self-attention layer keeps A[b][k] = sum_q mean_h softmax(scale Q_h K_h^T)[q][k]
     (`HipUNet.enable_sag`; under CFG of the unconditional half only),
  2. the mask m = A > 1 on the layer's grid, brought to the latent grid by nearest-neighbour indexing,
  3. x0_deg = m ? gaussian9x9(x0) : x0 and the degraded model input o_b x0_deg + o_e eps (`ops.sag_degrade`, one launch),
  4. a second UNet call on it at batch B (the unconditional conditioning under CFG),
  5. eps_out = u + g (t - u) + s (u - eps_deg), or eps + s (eps - eps_deg) without CFG (`ops.cfg_sag_combine`),
then the scheduler's ordinary step.  The arithmetic is a restatement (unpinned); tests/sag_ref.py says
it again in plain torch.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import ops
from . import sampler as _sampler
from ._lib import PeaError


def sag_coefficients(scheduler, i: int) -> Tuple[float, float, float, float]:
    """(c_x, c_e, o_b, o_e) at position i of the schedule, host float64: x0 = c_x x + c_e eps is the scheduler's data
    prediction, o_b x0' + o_e eps the model input that belongs to a data prediction x0'.  Alpha-space schedulers
    (`DPMSolverMultistep`, `LCMScheduler`): c_x = 1 / alpha_t, c_e = -sigma_t / alpha_t, o_b = alpha_t, o_e = sigma_t.
    Sigma-space (`EulerDiscrete`, `EulerAncestralDiscrete`): c_x = 1, c_e = -sigma, o_b = k, o_e = sigma k with
    k = 1 / sqrt(sigma^2 + 1), the scheduler's own model-input scale.  With an unchanged x0 the model input is
    `scale_model_input(x)`."""
    if scheduler.timesteps is None:
        raise PeaError("sag_coefficients: call set_timesteps first")
    n = len(scheduler.timesteps)
    if not 0 <= i < n:
        raise PeaError(f"sag_coefficients: step {i} outside the {n}-step schedule")
    if isinstance(scheduler, _sampler.EulerDiscrete):                 # (EulerAncestralDiscrete is one)
        sigma = float(scheduler.sigmas[i])
        k = 1.0 / math.sqrt(sigma * sigma + 1.0)
        return 1.0, -sigma, k, sigma * k
    if isinstance(scheduler, _sampler.DPMSolverMultistep):
        sigma = float(scheduler.sigmas[i])
        alpha_t = 1.0 / math.sqrt(sigma * sigma + 1.0)
        sigma_t = sigma * alpha_t
    elif isinstance(scheduler, _sampler.LCMScheduler):
        a = float(scheduler.alphas_cumprod[int(scheduler.timesteps[i])])
        alpha_t, sigma_t = math.sqrt(a), math.sqrt(1.0 - a)
    else:
        raise PeaError(f"sag_coefficients: no rule for {type(scheduler).__name__} (DPMSolverMultistep, LCMScheduler, "
                       "EulerDiscrete, EulerAncestralDiscrete)")
    return 1.0 / alpha_t, -sigma_t / alpha_t, alpha_t, sigma_t


def nearest_tables(h: int, w: int, H: int, W: int):
    """Source row of every latent row and source column of every latent column for bringing an h x w map to H x W by
    nearest-neighbour indexing, int32 [H] and [W] on the host: `F.interpolate(mode="nearest")`,
    src = min(floor(dst * (float)in / out), in - 1) with the ratio and the product in fp32."""
    def table(n_in, n_out):
        if n_in < 1 or n_out < 1:
            raise PeaError(f"nearest_tables: {n_in} -> {n_out}")
        scale = np.float32(n_in) / np.float32(n_out)
        src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
        return torch.from_numpy(np.minimum(src, n_in - 1).astype(np.int32))
    return table(h, H), table(w, W)


def denoise_sag(unet, unet_sag, scheduler, latents, prompt_embeds, added_cond_kwargs, sag_scale: float = 0.75,
                num_inference_steps: int = 30, guidance_scale: float = 7.5, guidance_rescale: float = 0.0,
                residual_fn: Optional[Callable] = None, callback: Optional[Callable] = None, generator=None,
                timestep_cond=None, sag_layer=None, residual_fn_sag: Optional[Callable] = None):
    """`sampler.denoise` with self-attention guidance.  `unet` is the `HipUNet` of `sampler.denoise` (batch 2B when
    guidance_scale > 1); `unet_sag` is a batch-B `HipUNet(..., share_weights_from=unet)` for the degraded pass (without CFG it
    may be `unet` itself: the capture is then switched off around the second call).  sag_layer: `HipUNet.enable_sag`'s layer
    (None: the mid block's first transformer block).  residual_fn_sag(x_deg, t): the ControlNet residuals of the degraded pass
    at batch B, none when omitted.  guidance_rescale > 0 is refused: no pipeline combines it with this guidance.  With the
    Euler schedulers the degraded input is already the scaled model input and does not go through `scale_model_input`."""
    if guidance_rescale > 0.0:
        raise PeaError("denoise_sag: guidance_rescale > 0 cannot be combined with self-attention guidance")
    do_cfg = guidance_scale > 1.0
    B = latents.shape[0]
    if unet.B != (2 * B if do_cfg else B) or unet_sag.B != B:
        raise PeaError(f"denoise_sag: latents of batch {B} need a UNet of batch {2 * B if do_cfg else B} (has {unet.B}) and a "
                       f"degraded-pass UNet of batch {B} (has {unet_sag.B})")
    timestep_cond = _sampler.check_timestep_cond(unet, timestep_cond, do_cfg)
    ukw = {} if timestep_cond is None else dict(timestep_cond=timestep_cond)
    ukw_sag = {} if timestep_cond is None else dict(timestep_cond=timestep_cond[:B])
    # the conditioning of the degraded pass: the unconditional half under CFG
    embeds_sag = prompt_embeds[:B] if do_cfg else prompt_embeds
    added_sag = None if added_cond_kwargs is None else {
        k: (v[:B] if do_cfg and torch.is_tensor(v) else v) for k, v in added_cond_kwargs.items()}
    fused = getattr(scheduler, "fused_model_input", False)
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    H, W = latents.shape[-2:]
    unet.enable_sag(sag_layer, samples=(0, B))
    try:
        tables = None
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
                              return_dict=False, **kw)[0].float().contiguous()
            part = unet.sag_colsum()
            if tables is None:
                h, w = unet._grid_of(part.shape[2])
                iy, ix = nearest_tables(h, w, H, W)
                tables = (h, w, iy.to(latents.device), ix.to(latents.device))
            h, w, iy, ix = tables
            x_deg = ops.sag_degrade(latents, noise_pred[:B], part, (h, w), iy, ix, *sag_coefficients(scheduler, scheduler._i))
            kw = dict(ukw_sag)
            if residual_fn_sag is not None:
                down, mid = residual_fn_sag(x_deg, t)
                kw.update(down_block_additional_residuals=down, mid_block_additional_residual=mid)
            if unet_sag is unet:
                unet.disable_sag()
            eps_deg = unet_sag(x_deg, t, encoder_hidden_states=embeds_sag, added_cond_kwargs=added_sag, return_dict=False,
                               **kw)[0].float()
            if unet_sag is unet:
                unet.enable_sag(sag_layer, samples=(0, B))
            noise_pred = ops.cfg_sag_combine(noise_pred, eps_deg, guidance_scale, sag_scale, do_cfg)
            latents = scheduler.step(noise_pred, t, latents, return_dict=False, generator=generator)[0]
            if callback is not None:
                callback(i, t, latents)
    finally:
        unet.disable_sag()
    return latents
