"""Semantic Guidance (Brack, Friedrich, Hintersdorf, Struppek, Schramowski, Kersting 2023, "SEGA: Instructing Text-to-Image Models
using Semantic Guidance"): concept-level edits ("add glasses", "remove the crowd") steered during sampling, with no training, no
weights and no second pass.

As with perturbed-attention guidance (pag.py) there is no second UNet call: with n latents and K edit concepts the UNet runs ONE
batch [uncond | cond | edit_1 .. edit_K] of (2 + K) n, the edit samples conditioned on the edit prompts' embeddings.  Then, per
concept c with its signed scale s_c (negative: `reverse_editing_direction`, steer away from the concept),
  d_c = s_c (e_c - u),    m_c = d_c where |d_c| >= quantile_{q_c}(|d_c|) over the h x w positions of its channel, else 0
(only the upper tail of each channel acts: the edit stays local), and with the momentum `mom` (zero before the first step)
  E_all = sum_c w_c m_c,  E_warm = sum_c warm_c w_c m_c,  used = E_all + mu mom,
  eps = u + g (t - u) + (any warm ? E_warm + mu mom : 0),   mom <- beta mom + (1 - beta) used
(`ops.cfg_sega_combine`: an exact radix select per channel and one elementwise pass, two launches), and the scheduler's ordinary
step.  The momentum builds up during a concept's warm-up steps, the edit acts from `edit_warmup_steps` on, and from
`edit_cooldown_steps` on the concept contributes nothing (its weight is 0: the kernels skip it).  `step_plan` is that schedule.

The arithmetic is a restatement of the paper and of diffusers' `SemanticStableDiffusionPipeline` (unpinned);
tests/sega_ref.py says it again in plain torch.  Not built: diffusers' renormalised concept weights while only some concepts are
warm (here a warm concept simply acts and a cold one does not), `guidance_rescale` together with SEGA, SEGA without
classifier-free guidance, LEDITS++ inversion of real images, latents of more than 16384 positions.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import ops
from . import sampler as _sampler
from ._lib import PeaError

MAX_CONCEPTS = 8


def _per_concept(name, v, K, kind=float):
    """a scalar broadcast over the K concepts, or a list of K"""
    if isinstance(v, (list, tuple)):
        if len(v) != K:
            raise PeaError(f"step_plan: {name} has {len(v)} entries for {K} concepts")
        return [None if a is None else kind(a) for a in v]
    return [None if v is None else kind(v)] * K


def step_plan(i: int, K: int, edit_guidance_scale=5.0, edit_threshold=0.9, reverse_editing_direction=False, edit_warmup_steps=10,
              edit_cooldown_steps=None, edit_weights=1.0):
    """The four K-lists `ops.cfg_sega_combine` takes at step i (counted from 0): (edit_scale, quantile, weight, warm).  Each
    argument is one value for every concept or a list of K.  edit_scale[c] = -edit_guidance_scale when the concept's direction
    is reversed; weight[c] = 0 from step edit_cooldown_steps on (None: never); warm[c] = 1 from step edit_warmup_steps on."""
    K = int(K)
    if not 1 <= K <= MAX_CONCEPTS:
        raise PeaError(f"step_plan: K={K} edit concepts (1 .. {MAX_CONCEPTS})")
    scale = _per_concept("edit_guidance_scale", edit_guidance_scale, K)
    thr = _per_concept("edit_threshold", edit_threshold, K)
    rev = _per_concept("reverse_editing_direction", reverse_editing_direction, K, bool)
    warmup = _per_concept("edit_warmup_steps", edit_warmup_steps, K, int)
    cool = _per_concept("edit_cooldown_steps", edit_cooldown_steps, K, int)
    wts = _per_concept("edit_weights", edit_weights, K)
    for c in range(K):
        if not scale[c] >= 0.0 or not wts[c] >= 0.0 or warmup[c] < 0 or (cool[c] is not None and cool[c] < 0):
            raise PeaError(f"step_plan: concept {c}: edit_guidance_scale {scale[c]}, weight {wts[c]}, warm-up {warmup[c]}, cool-down {cool[c]} "
                           "(none negative; the direction is `reverse_editing_direction`)")
        if not 0.0 <= thr[c] < 1.0:
            raise PeaError(f"step_plan: concept {c}: edit_threshold {thr[c]} outside [0, 1)")
    i = int(i)
    return ([-scale[c] if rev[c] else scale[c] for c in range(K)], thr,
            [0.0 if cool[c] is not None and i >= cool[c] else wts[c] for c in range(K)],
            [1 if i >= warmup[c] else 0 for c in range(K)])


def denoise_semantic(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, edit_prompt_embeds, edit_added_cond_kwargs,
                     edit_guidance_scale=5.0, edit_threshold=0.9, reverse_editing_direction=False, edit_warmup_steps=10,
                     edit_cooldown_steps=None, edit_weights=1.0, edit_momentum_scale: float = 0.1, edit_mom_beta: float = 0.4,
                     num_inference_steps: int = 30, guidance_scale: float = 7.5, residual_fn: Optional[Callable] = None,
                     callback: Optional[Callable] = None, generator=None, timestep_cond=None):
    """`sampler.denoise` with semantic guidance.  latents [n, ...]; `unet` is a `HipUNet` of batch (2 + K) n.  prompt_embeds /
    added_cond_kwargs / timestep_cond are what `sampler.denoise` takes under CFG (batch 2n, unconditional half first);
    edit_prompt_embeds [K n, L, D] and the tensors of edit_added_cond_kwargs [K n, ...] are concept-major (concept 0's n samples
    first) and are appended behind them.  The edit arguments are `step_plan`'s.  residual_fn(x, t) sees the whole batch.
    One momentum buffer and one workspace serve every step."""
    n = latents.shape[0]
    if not guidance_scale > 1.0:
        raise PeaError(f"denoise_semantic: guidance_scale {guidance_scale} (> 1: semantic guidance is built on classifier-free guidance)")
    if edit_prompt_embeds is None or edit_prompt_embeds.dim() != 3 or edit_prompt_embeds.shape[0] % n or edit_prompt_embeds.shape[0] < n:
        raise PeaError(f"denoise_semantic: edit_prompt_embeds {None if edit_prompt_embeds is None else tuple(edit_prompt_embeds.shape)}, "
                       f"expected [K * {n}, L, D], concept-major")
    K = edit_prompt_embeds.shape[0] // n
    step_plan(0, K, edit_guidance_scale, edit_threshold, reverse_editing_direction, edit_warmup_steps, edit_cooldown_steps, edit_weights)
    if not 0.0 <= edit_mom_beta <= 1.0 or edit_momentum_scale < 0.0:
        raise PeaError(f"denoise_semantic: edit_mom_beta {edit_mom_beta} (0 .. 1), edit_momentum_scale {edit_momentum_scale} (>= 0)")
    if getattr(unet, "B", None) != (2 + K) * n:
        raise PeaError(f"denoise_semantic: latents of batch {n} and {K} edit concepts need a UNet of batch {(2 + K) * n} "
                       f"([uncond | cond | edit_1 .. edit_{K}]; has {getattr(unet, 'B', None)})")
    if prompt_embeds.shape[0] != 2 * n:
        raise PeaError(f"denoise_semantic: prompt_embeds of batch {prompt_embeds.shape[0]}, expected {2 * n}")
    if (added_cond_kwargs is None) != (edit_added_cond_kwargs is None):
        raise PeaError("denoise_semantic: added_cond_kwargs and edit_added_cond_kwargs come together or not at all")
    added = None
    if added_cond_kwargs is not None:
        added = {}
        for key, v in added_cond_kwargs.items():
            e = edit_added_cond_kwargs.get(key)
            if e is None or e.shape[0] != K * n or v.shape[0] != 2 * n:
                raise PeaError(f"denoise_semantic: added_cond_kwargs[{key!r}] of batch {v.shape[0]} with an edit part of batch "
                               f"{None if e is None else e.shape[0]}, expected {2 * n} and {K * n}")
            added[key] = torch.cat([v, e.to(v.dtype)])
    timestep_cond = _sampler.check_timestep_cond(unet, timestep_cond, False)
    ukw = {}
    if timestep_cond is not None:
        if timestep_cond.shape[0] not in (n, (2 + K) * n):
            raise PeaError(f"denoise_semantic: timestep_cond of batch {timestep_cond.shape[0]}, expected {n} or {(2 + K) * n}")
        ukw = dict(timestep_cond=torch.cat([timestep_cond] * (2 + K)) if timestep_cond.shape[0] == n else timestep_cond)
    embeds = torch.cat([prompt_embeds, edit_prompt_embeds.to(prompt_embeds.dtype)])
    fused = getattr(scheduler, "fused_model_input", False)
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    momentum = torch.zeros_like(latents)
    workspace = ops.sega_workspace(n, latents.shape[1], K, latents.device)
    for i, t in enumerate(timesteps):
        # (the Euler kernel writes one or two copies of the next model input; the others are torch's)
        x = scheduler.scale_model_input(latents, t, dup=1) if fused else scheduler.scale_model_input(latents, t)
        x = torch.cat([x] * (2 + K))
        kw = dict(ukw)
        if residual_fn is not None:
            down, mid = residual_fn(x, t)
            kw.update(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        noise_pred = unet(x, t, encoder_hidden_states=embeds, added_cond_kwargs=added, return_dict=False, **kw)[0]
        scale, quantile, weight, warm = step_plan(i, K, edit_guidance_scale, edit_threshold, reverse_editing_direction,
                                                  edit_warmup_steps, edit_cooldown_steps, edit_weights)
        noise_pred = ops.cfg_sega_combine(noise_pred.float(), momentum, guidance_scale, scale, quantile, weight, warm,
                                          edit_momentum_scale, edit_mom_beta, workspace=workspace)
        latents = scheduler.step(noise_pred, t, latents, return_dict=False, generator=generator)[0]
        if callback is not None:
            callback(i, t, latents)
    return latents
