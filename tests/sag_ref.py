"""Test infrastructure: self-attention guidance (Hong et al. 2023) restated in plain fp32 torch.

Nothing here is pinned against another implementation (diffusers is not a dependency): it restates the method as
pea_diffusion_amd/sag.py documents it, with torch's own operators where the method names them --
`F.pad(mode="reflect")` + `F.conv2d` for the blur, `F.interpolate(mode="nearest")` for the mask.

  colsum_ref        kernel level: the column sums of the head-mean softmax, and the fp32 log-sum-exp
  degrade_ref       mask -> latent grid, data prediction, blur, select, degraded model input
  combine_ref       the guidance combine, both forms
  SagAttention      `Attention` that also records its column sums;  attach_sag
  denoise_sag_ref   the loop, on the schedulers of oracle.sampler_ref / tests/turbo_ref.py
"""
import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import Attention, _st


def colsum_ref(q, k, H, scale=0.125):
    """q [B, Sq, H * 64], k [B, Skv, H * 64] (any float dtype) -> (A fp32 [B, Skv], lse fp32 [B, H, Sq]):
    A[b][key] = sum_q mean_h softmax(scale q_h k_h^T)[q][key].  A q that arrives multiplied by scale log2(e) has scale = ln 2."""
    B, Sq, _ = q.shape
    qh = q.float().view(B, Sq, H, 64).transpose(1, 2)
    kh = k.float().view(B, -1, H, 64).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * scale                           # [B, H, Sq, Skv]
    lse = torch.logsumexp(s, -1)
    return torch.exp(s - lse[..., None]).mean(1).sum(1), lse


def gaussian_taps():
    w = torch.exp(-0.5 * torch.arange(-4, 5, dtype=torch.float64) ** 2)
    return (w / w.sum()).float()


def degrade_ref(latents, eps, mask, c_x, c_e, o_b, o_e):
    """latents, eps [B, C, H, W] fp32; mask bool [B, h, w] on the layer's grid -> the degraded model input [B, C, H, W]"""
    B, C, H, W = latents.shape
    m = F.interpolate(mask[:, None].float(), size=(H, W), mode="nearest") > 0.5
    x0 = c_x * latents + c_e * eps
    w = gaussian_taps().to(x0.dtype)
    p = F.pad(x0, (4, 4, 4, 4), mode="reflect")
    p = F.conv2d(p, w.view(1, 1, 1, 9).expand(C, 1, 1, 9), groups=C)            # rows
    blur = F.conv2d(p, w.view(1, 1, 9, 1).expand(C, 1, 9, 1), groups=C)         # columns
    return o_b * torch.where(m, blur, x0) + o_e * eps


def combine_ref(eps, eps_deg, g, s, do_cfg=True):
    if do_cfg:
        u, t = eps.chunk(2)
        return u + g * (t - u) + s * (u - eps_deg)
    return eps + s * (eps - eps_deg)


class SagAttention(Attention):
    """the oracle's self-attention, which also keeps the column sums of its head-mean softmax: `record` is None (off) or a list
    that gets one fp32 [B, S] per forward"""

    def __init__(self, query_dim, heads):
        super().__init__(query_dim, heads, None)
        self.record = None

    def forward(self, x, ctx=None):
        if self.record is not None:
            B, S, C = x.shape
            H = self.heads
            q = _st(self.to_q(x)).view(B, S, H, C // H).transpose(1, 2)
            k = _st(self.to_k(x)).view(B, S, H, C // H).transpose(1, 2)
            a = torch.softmax(q @ k.transpose(-1, -2) * (C // H) ** -0.5, dim=-1)       # fp32: never a bf16 operand
            self.record.append(a.mean(1).sum(1).float().clone())
        return super().forward(x, ctx)


def attach_sag(unet, name):
    """the attn1 module `name` of `unet` becomes a SagAttention with the same weights -> the module"""
    old = unet.get_submodule(name)
    new = SagAttention(old.to_q.weight.shape[0], old.heads)
    new.load_state_dict(old.state_dict())
    for p in new.parameters():
        p.requires_grad_(False)
    setattr(unet.get_submodule(name.rsplit(".", 1)[0]), "attn1", new)
    return new


def coefficients_ref(kind, sigma):
    """(c_x, c_e, o_b, o_e) from the closed forms; kind "alpha" (sigma = sigma_t / alpha_t) or "sigma\""""
    k = 1.0 / math.sqrt(sigma * sigma + 1.0)
    if kind == "alpha":
        return 1.0 / k, -sigma, k, sigma * k
    return 1.0, -sigma, k, sigma * k


def denoise_sag_ref(unet, module, scheduler, latents, prompt_embeds, added, n_steps, guidance_scale, sag_scale, map_hw,
                    kind="alpha", mask_fix=None, masks_out=None, A_out=None, step_kw=None):
    """the loop of pea_diffusion_amd.sag.denoise_sag around the oracle.  module: the SagAttention of `attach_sag`.  kind: the
    scheduler's space.  mask_fix(i, A, mask) -> mask lets a test hand in the device's decision at entries it leaves out."""
    cfg = guidance_scale > 1.0
    B = latents.shape[0]
    scheduler.set_timesteps(n_steps)
    latents = latents * scheduler.init_noise_sigma
    cut = lambda v: v[:B] if cfg else v
    added_u = None if added is None else {k: cut(v) for k, v in added.items()}
    for i, t in enumerate(scheduler.timesteps):
        x = torch.cat([latents] * 2) if cfg else latents
        x = scheduler.scale_model_input(x, t)
        module.record = []
        eps = unet(x.float(), int(t), encoder_hidden_states=prompt_embeds, added_cond_kwargs=added, return_dict=False)[0]
        A = module.record[0][:B]
        module.record = None
        mask = (A > 1.0).view(B, *map_hw)
        if A_out is not None:
            A_out.append(A.clone())
        if mask_fix is not None:
            mask = mask_fix(i, A, mask)
        if masks_out is not None:
            masks_out.append(mask.clone())
        x_deg = degrade_ref(latents.float(), eps[:B], mask, *coefficients_ref(kind, float(scheduler.sigmas[i])))
        eps_deg = unet(x_deg, int(t), encoder_hidden_states=cut(prompt_embeds), added_cond_kwargs=added_u, return_dict=False)[0]
        out = combine_ref(eps, eps_deg, guidance_scale, sag_scale, cfg)
        latents = scheduler.step(out, t, latents, **(step_kw or {}))[0]
    return latents
