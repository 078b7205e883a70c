"""CPU restatement of the sigma-space samplers and of the guidance-embedded UNet, written from the formulas and independent of
pea_diffusion_amd/sampler.py: `EulerDiscreteScheduler` / `EulerAncestralDiscreteScheduler` as diffusers 0.23 configures them
from the SDXL scheduler config (scaled-linear betas 0.00085-0.012 over 1000 steps, epsilon prediction, linear sigma
interpolation, no Karras sigmas, s_churn 0), the generation loop around them (CFG, `timestep_cond`, a start index for
strength < 1), `get_guidance_scale_embedding` of the reference's loop (tests/test_sdxl_zh_inpaint.py:721-745), and the oracle UNet
with `time_embedding.cond_proj`.  Scheduler arithmetic in float64, the UNet in fp32.  Test infrastructure only
(tests/test_turbo_*.py)."""
import math

import torch
import torch.nn as nn

from oracle.unet_ref import UNet2DConditionRef, _st, timestep_embedding


class EulerRef:
    def __init__(self, ancestral=False, spacing=None, offset=None, T=1000, beta_start=0.00085, beta_end=0.012):
        self.ancestral = ancestral
        self.spacing = spacing if spacing is not None else ("trailing" if ancestral else "leading")
        self.offset = offset if offset is not None else (0 if ancestral else 1)
        self.T = T
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float64) ** 2
        ac = torch.cumprod(1.0 - betas, dim=0)
        self.train_sigmas = ((1.0 - ac) / ac).sqrt().tolist()
        self.timesteps = None

    def _sigma_at(self, t):
        """linear interpolation of the training sigmas at a (possibly fractional) timestep"""
        lo = min(int(math.floor(t)), self.T - 1)
        hi = min(lo + 1, self.T - 1)
        f = t - lo
        return (1.0 - f) * self.train_sigmas[lo] + f * self.train_sigmas[hi]

    def set_timesteps(self, n):
        T = self.T
        if self.spacing == "leading":
            ts = [float(round(j * (T // n))) + self.offset for j in range(n)][::-1]
        elif self.spacing == "linspace":
            ts = [(T - 1) * j / (n - 1) if n > 1 else 0.0 for j in range(n)][::-1]
        else:
            ts = [float(round(T - k * (T / n))) - 1.0 for k in range(n)]       # arange(T, 0, -T / n).round() - 1
        self.ts = ts
        self.sigmas = [self._sigma_at(t) for t in ts] + [0.0]
        smax = max(self.sigmas)
        self.init_noise_sigma = smax if self.spacing in ("linspace", "trailing") else math.sqrt(smax * smax + 1.0)
        self.timesteps = torch.tensor(ts, dtype=torch.float64 if self.spacing == "linspace" else torch.int64)
        self.step_index = 0
        return self.timesteps

    def scalars(self, i):
        """(sigma, sigma_to, sigma_down, sigma_up) of step i"""
        s, to = self.sigmas[i], self.sigmas[i + 1]
        if not self.ancestral:
            return s, to, to, 0.0
        up = math.sqrt(to * to * (s * s - to * to) / (s * s))
        return s, to, math.sqrt(to * to - up * up), up

    def scale_model_input(self, sample, timestep=None):
        s = self.sigmas[self.step_index]
        return sample / math.sqrt(s * s + 1.0)

    def step(self, eps, timestep, sample, generator=None, noise=None):
        """-> (prev_sample,) in float64"""
        i = self.step_index
        assert float(timestep) == float(self.timesteps[i])
        s, to, down, up = self.scalars(i)
        x = sample.double() + (down - s) * eps.double()          # derivative (x - x0) / sigma = eps (epsilon prediction)
        if up > 0.0:
            if noise is None:
                noise = torch.randn(sample.shape, generator=generator, dtype=torch.float32)
            x = x + up * noise.double()
        self.step_index += 1
        return (x,)


def guidance_scale_embedding_ref(w, dim=256):
    half = dim // 2
    rows = []
    for wv in w:
        arg = [1000.0 * float(wv) * math.exp(-math.log(10000.0) / (half - 1) * i) for i in range(half)]
        rows.append([math.sin(a) for a in arg] + [math.cos(a) for a in arg] + [0.0] * (dim % 2))
    return torch.tensor(rows, dtype=torch.float64)


def euler_denoise_ref(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps, guidance_scale=0.0,
                      generator=None, timestep_cond=None, t_start=0, scale_init=True, unet_kwargs=None, calls=None):
    """the generation loop: CFG doubling for guidance_scale > 1, one UNet evaluation per step on the scaled input, noise from
    `generator` inside the ancestral steps.  t_start > 0 runs `timesteps[t_start:]` on latents the caller has already noised."""
    do_cfg = guidance_scale > 1.0
    scheduler.set_timesteps(num_inference_steps)
    scheduler.step_index = t_start
    latents = latents.double() * (scheduler.init_noise_sigma if scale_init else 1.0)
    kw = dict(unet_kwargs or {})
    if timestep_cond is not None:
        kw["timestep_cond"] = torch.cat([timestep_cond] * 2) if do_cfg else timestep_cond
    for t in scheduler.timesteps[t_start:]:
        x = scheduler.scale_model_input(latents, t)
        x = torch.cat([x] * 2) if do_cfg else x
        if calls is not None:
            calls.append(x.shape[0])
        eps = unet(x.float(), t, encoder_hidden_states=prompt_embeds, added_cond_kwargs=added_cond_kwargs,
                   return_dict=False, **kw)[0]
        if do_cfg:
            u, c = eps.double().chunk(2)
            eps = u + guidance_scale * (c - u)
        latents = scheduler.step(eps, t, latents, generator=generator)[0]
    return latents


class CondUNetRef(UNet2DConditionRef):
    """the oracle UNet with diffusers' `time_cond_proj_dim`: TimestepEmbedding adds the bias-free `cond_proj(timestep_cond)`
    to the sinusoidal projection in front of linear_1.  `forward(..., timestep_cond=)`; None leaves it out."""

    def __init__(self, cfg, time_cond_proj_dim):
        super().__init__(cfg)
        self.time_embedding.cond_proj = nn.Linear(time_cond_proj_dim, cfg.block_out_channels[0], bias=False)
        self._cond = None

    def embed(self, timesteps, added_cond_kwargs, B):
        cfg = self.config
        t = timesteps
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.int64)
        if t.dim() == 0:
            t = t[None]
        t = t.expand(B)
        te = _st(timestep_embedding(t, cfg.block_out_channels[0]).to(self.dtype))
        if self._cond is not None:
            te = _st(te + self.time_embedding.cond_proj(_st(self._cond.to(self.dtype))))
        emb = _st(self.time_embedding(te))
        if cfg.addition_embed_type == "text_time":
            text_embeds = added_cond_kwargs["text_embeds"]
            time_ids = added_cond_kwargs["time_ids"]
            tid = _st(timestep_embedding(time_ids.flatten(), cfg.addition_time_embed_dim)).reshape(B, -1)
            add = torch.cat([_st(text_embeds), tid.to(text_embeds.dtype)], dim=-1)
            emb = _st(emb + self.add_embedding(add.to(self.dtype)))
        return emb

    def forward(self, sample, timesteps, encoder_hidden_states, added_cond_kwargs=None, timestep_cond=None, **kw):
        self._cond = timestep_cond
        try:
            return super().forward(sample, timesteps, encoder_hidden_states, added_cond_kwargs=added_cond_kwargs, **kw)
        finally:
            self._cond = None


def euler_inpaint_ref(unet9, scheduler, vae, image, mask, prompt_embeds, added_cond_kwargs, num_inference_steps, strength,
                      guidance_scale, noise, vae_noise):
    """the inpainting program (tests/inpaint_ref.py) around a sigma-space scheduler: a strength < 1 run starts from
    `image_latents + sigma * noise` at position t_start and runs `timesteps[t_start:]`.  -> (latents, timesteps run)"""
    from inpaint_ref import get_timesteps_ref, prepare_ref
    do_cfg = guidance_scale > 1.0
    scheduler.set_timesteps(num_inference_steps)
    timesteps, left, t_start = get_timesteps_ref(scheduler.timesteps, num_inference_steps, strength)
    assert left >= 1
    init, masked, lmask = prepare_ref(image, mask)
    sf = vae.config.scaling_factor
    if strength == 1.0:
        latents = noise.double() * scheduler.init_noise_sigma
    else:
        image_latents = vae.encode(init).latent_dist.sample(noise=vae_noise[0]) * sf
        latents = image_latents.double() + scheduler.sigmas[t_start] * noise.double()
    masked_latents = vae.encode(masked).latent_dist.sample(noise=vae_noise[1]) * sf
    m2 = torch.cat([lmask] * 2) if do_cfg else lmask
    ml2 = torch.cat([masked_latents] * 2) if do_cfg else masked_latents
    gathered = lambda x, t, **k: unet9(torch.cat([x, m2, ml2], dim=1), t, **k)
    out = euler_denoise_ref(gathered, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps,
                            guidance_scale=guidance_scale, t_start=t_start, scale_init=False)
    return out, timesteps
