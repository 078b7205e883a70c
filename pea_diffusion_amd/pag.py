"""Perturbed-Attention Guidance (Ahn, Cho, Min, Jang, Kim, Kim, Park, Jin, Kim 2024, "Self-Rectifying Diffusion Sampling with
Perturbed-Attention Guidance") and its successor, Smoothed Energy Guidance (Hong 2024, "Smoothed Energy Guidance: Guiding
Diffusion Models with Reduced Energy Curvature of Attention"): a guidance term that needs no training and no weights, from a
sample whose self-attention is perturbed in a few layers.

Unlike self-attention guidance (sag.py) there is no second UNet call: with n latents the UNet runs ONE batch
[uncond | cond | perturbed] of 3n (or [cond | perturbed] of 2n without classifier-free guidance).  The perturbed samples get the
conditional embeddings; in the chosen self-attention layers (default: the mid block) and for those samples only
  "pag":  O = V                                   (the softmax replaced by the identity),
  "seg":  O = softmax(scale blur(Q) K^T) V        (the projected queries blurred over the h x w token grid, per channel),
and every other sample and layer is untouched (`HipUNet.set_attention_perturbation`).  Then
  eps = u + g (t - u) + s_t (t - p)        (t + s_t (t - p) without CFG),   s_t = max(0, scale - adaptive_scale (1000 - timestep)),
`rescale_noise_cfg` when guidance_rescale > 0 (`ops.cfg_pag_combine`), and the scheduler's ordinary step.

The SEG blur is a separable Gaussian with reflect padding, size k = ceil(6 sigma) + 1 - ceil(6 sigma) % 2 clamped per axis of
length m to m - (m % 2 - 1), taps exp(-0.5 (x / sigma)^2) on linspace(-(k - 1) / 2, (k - 1) / 2, k), normalised; sigma above 9999
(the authors' default is "infinite") is the mean over the grid.  `blur_matrix` folds all of that into one dense matrix per axis.

The arithmetic is a restatement of the papers and the authors' public code (unpinned);
tests/pag_ref.py says it again in plain torch.  Not built: PAG's other perturbations (random or additive masks) and layers
outside the UNet's self-attention.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import numpy as np
import torch

from . import ops
from . import sampler as _sampler
from ._lib import PeaError

INFINITE_SIGMA = 9999.0


def blur_kernel_size(m: int, sigma: float) -> int:
    """the (odd) tap count along an axis of length m"""
    c = int(math.ceil(6.0 * sigma))
    return min(c + 1 - c % 2, m - (m % 2 - 1))


def blur_matrix(m: int, sigma: float) -> np.ndarray:
    """fp32 [m, m], row-stochastic: row i holds the weight every source position has in blurred position i along an axis of
    length m -- the Gaussian taps with reflect padding (no edge repeat) folded in; sigma > 9999: 1 / m everywhere.  Built in
    float64.  A grid is blurred as Mh . X . Mw^T."""
    m = int(m)
    if m < 1 or not sigma > 0.0:
        raise PeaError(f"blur_matrix: an axis of {m} positions, sigma {sigma}")
    if sigma > INFINITE_SIGMA:
        return np.full((m, m), 1.0 / m, dtype=np.float64).astype(np.float32)
    k = blur_kernel_size(m, float(sigma))
    x = np.linspace(-(k - 1) / 2.0, (k - 1) / 2.0, k, dtype=np.float64)
    taps = np.exp(-0.5 * (x / float(sigma)) ** 2)
    taps /= taps.sum()
    M = np.zeros((m, m), dtype=np.float64)
    r = k // 2
    for i in range(m):
        for d in range(-r, r + 1):
            j = abs(i + d)
            j = 2 * m - 2 - j if j >= m else j
            M[i, j] += taps[d + r]
    return M.astype(np.float32)


def perturbed_scale(scale: float, adaptive_scale: float, t) -> float:
    """s_t = max(0, scale - adaptive_scale (1000 - t)): the guidance weight at timestep t (diffusers' `pag_adaptive_scale`)"""
    return max(0.0, float(scale) - float(adaptive_scale) * (1000.0 - float(t)))


def _append_cond(v, n):
    """a batched conditioning tensor with its conditional (last) n samples once more at the end"""
    return torch.cat([v, v[-n:]]) if torch.is_tensor(v) else v


def denoise_perturbed(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, mode: str = "pag", scale: float = 3.0,
                      adaptive_scale: float = 0.0, blur_sigma: float = float("inf"), layers=None, num_inference_steps: int = 30,
                      guidance_scale: float = 7.5, guidance_rescale: float = 0.0, residual_fn: Optional[Callable] = None,
                      callback: Optional[Callable] = None, generator=None, timestep_cond=None):
    """`sampler.denoise` with perturbed-attention (mode "pag") or smoothed-energy (mode "seg") guidance.  latents [n, ...];
    `unet` is a `HipUNet` of batch 3n when guidance_scale > 1, else 2n.  prompt_embeds / added_cond_kwargs / timestep_cond are
    what `sampler.denoise` takes (batch 2n under CFG, unconditional half first, else n): the perturbed samples' copies of the
    conditional ones are appended here.  layers: `HipUNet.set_attention_perturbation`'s (None: the mid block).
    residual_fn(x, t) sees the whole batch.  The perturbation is switched on for the loop and cleared behind it."""
    if mode not in ("pag", "seg"):
        raise PeaError(f"denoise_perturbed: mode {mode!r} ('pag' or 'seg')")
    if scale < 0.0 or adaptive_scale < 0.0:
        raise PeaError(f"denoise_perturbed: scale {scale}, adaptive_scale {adaptive_scale} (both >= 0)")
    if not blur_sigma > 0.0:
        raise PeaError(f"denoise_perturbed: blur_sigma {blur_sigma} (> 0; above {INFINITE_SIGMA:g}: the mean over the grid)")
    do_cfg = guidance_scale > 1.0
    n = latents.shape[0]
    k = 3 if do_cfg else 2
    if getattr(unet, "B", None) != k * n:
        raise PeaError(f"denoise_perturbed: latents of batch {n} need a UNet of batch {k * n} "
                       f"({'[uncond | cond | perturbed]' if do_cfg else '[cond | perturbed]'}; has {getattr(unet, 'B', None)})")
    if prompt_embeds.shape[0] != (k - 1) * n:
        raise PeaError(f"denoise_perturbed: prompt_embeds of batch {prompt_embeds.shape[0]}, expected {(k - 1) * n}")
    timestep_cond = _sampler.check_timestep_cond(unet, timestep_cond, False)
    ukw = {}
    if timestep_cond is not None:
        if timestep_cond.shape[0] == n:
            timestep_cond = torch.cat([timestep_cond] * (k - 1))
        ukw = dict(timestep_cond=_append_cond(timestep_cond, n))
    embeds = _append_cond(prompt_embeds, n)
    added = None if added_cond_kwargs is None else {key: _append_cond(v, n) for key, v in added_cond_kwargs.items()}
    fused = getattr(scheduler, "fused_model_input", False)
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    unet.set_attention_perturbation(mode, layers=layers, samples=n, blur_sigma=blur_sigma)
    try:
        for i, t in enumerate(timesteps):
            # (the Euler kernel writes one or two copies of the next model input; the third is torch's)
            x = scheduler.scale_model_input(latents, t, dup=1) if fused else scheduler.scale_model_input(latents, t)
            x = torch.cat([x] * k)
            kw = dict(ukw)
            if residual_fn is not None:
                down, mid = residual_fn(x, t)
                kw.update(down_block_additional_residuals=down, mid_block_additional_residual=mid)
            noise_pred = unet(x, t, encoder_hidden_states=embeds, added_cond_kwargs=added, return_dict=False, **kw)[0]
            noise_pred = ops.cfg_pag_combine(noise_pred.float(), guidance_scale, perturbed_scale(scale, adaptive_scale, t),
                                             guidance_rescale, do_cfg)
            latents = scheduler.step(noise_pred, t, latents, return_dict=False, generator=generator)[0]
            if callback is not None:
                callback(i, t, latents)
    finally:
        unet.clear_attention_perturbation()
    return latents
