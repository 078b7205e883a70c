"""Test infrastructure: perturbed-attention guidance (Ahn et al. 2024) and smoothed-energy guidance (Hong 2024) restated in plain
fp32 torch.

Nothing here is pinned against another implementation (diffusers is not a dependency): it restates the methods as
pea_diffusion_amd/pag.py documents them, with torch's own operators where the methods name them -- `F.pad(mode="reflect")` +
`F.conv2d` for the blur, `Tensor.std` for the rescale.

  blur_taps, blur_ref     the SEG blur of a [n, h w, C] token tensor over its grid
  combine_ref             the three-way guidance combine, both forms, with diffusers' rescale_noise_cfg
  PerturbAttention        `Attention` whose last samples run the perturbed attention;  attach_perturb
  denoise_perturbed_ref   the loop, on the schedulers of oracle.sampler_ref / tests/turbo_ref.py
"""
import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import Attention, _st


def blur_taps(m, sigma):
    """float64 taps along an axis of length m: size ceil(6 sigma) made odd, clamped to m - (m % 2 - 1)"""
    c = int(math.ceil(6.0 * sigma))
    k = min(c + 1 - c % 2, m - (m % 2 - 1))
    x = torch.linspace(-(k - 1) / 2.0, (k - 1) / 2.0, k, dtype=torch.float64)
    w = torch.exp(-0.5 * (x / sigma) ** 2)
    return w / w.sum()


def blur_ref(q, h, w, sigma):
    """q [n, h * w, C] -> the same shape: every channel's h x w grid blurred (sigma > 9999: its mean)"""
    n, S, C = q.shape
    g = q.reshape(n, h, w, C).permute(0, 3, 1, 2)
    if sigma > 9999.0:
        out = g.mean(dim=(2, 3), keepdim=True).expand_as(g)
    else:
        th, tw = blur_taps(h, sigma).to(q.dtype), blur_taps(w, sigma).to(q.dtype)
        rh, rw = th.numel() // 2, tw.numel() // 2
        p = F.pad(g, (rw, rw, rh, rh), mode="reflect")
        p = F.conv2d(p, tw.view(1, 1, 1, -1).expand(C, 1, 1, -1), groups=C)
        out = F.conv2d(p, th.view(1, 1, -1, 1).expand(C, 1, -1, 1), groups=C)
    return out.permute(0, 2, 3, 1).reshape(n, S, C)


def combine_ref(eps, g, s, rescale=0.0, do_cfg=True):
    if not do_cfg:
        t, p = eps.chunk(2)
        return t + s * (t - p)
    u, t, p = eps.chunk(3)
    out = u + g * (t - u) + s * (t - p)
    if rescale > 0.0:
        dims = list(range(1, t.dim()))
        factor = t.std(dim=dims, keepdim=True) / out.std(dim=dims, keepdim=True)
        out = rescale * (out * factor) + (1.0 - rescale) * out
    return out


class PerturbAttention(Attention):
    """the oracle's self-attention whose samples `first` .. B - 1 are perturbed: mode "pag" O = V, mode "seg" the stored query
    blurred over its grid (and stored again, as the device's in-place blur does); mode None: the plain attention"""

    def __init__(self, query_dim, heads):
        super().__init__(query_dim, heads, None)
        self.mode, self.first, self.sigma, self.grid_of = None, 0, float("inf"), None

    def forward(self, x, ctx=None):
        if self.mode is None:
            return super().forward(x, ctx)
        B, S, C = x.shape
        H, f = self.heads, self.first
        q, k, v = _st(self.to_q(x)), _st(self.to_k(x)), _st(self.to_v(x))
        if self.mode == "seg":
            q = torch.cat([q[:f], _st(blur_ref(q[f:], *self.grid_of(S), self.sigma))])
        split = lambda z: z.view(B, S, H, C // H).transpose(1, 2)
        a = torch.softmax(split(q) @ split(k).transpose(-1, -2) * (C // H) ** -0.5, dim=-1)
        o = _st((_st(a) @ split(v)).transpose(1, 2).reshape(B, S, C))
        if self.mode == "pag":
            o = torch.cat([o[:f], v[f:]])
        return self.to_out[0](o)


def attach_perturb(unet, names, grid_of):
    """the attn1 modules `names` of `unet` become PerturbAttention with the same weights (mode None: plain) -> the modules.
    grid_of(S) -> (h, w) of a layer with S tokens."""
    out = []
    for name in names:
        old = unet.get_submodule(name)
        if isinstance(old, PerturbAttention):
            out.append(old)
            continue
        new = PerturbAttention(old.to_q.weight.shape[0], old.heads)
        new.load_state_dict(old.state_dict())
        for p in new.parameters():
            p.requires_grad_(False)
        new.grid_of = grid_of
        setattr(unet.get_submodule(name.rsplit(".", 1)[0]), "attn1", new)
        out.append(new)
    return out


def set_perturb(modules, mode, first=0, sigma=float("inf")):
    for m in modules:
        m.mode, m.first, m.sigma = mode, first, sigma


def denoise_perturbed_ref(unet, scheduler, latents, prompt_embeds, added, n_steps, guidance_scale, scale, adaptive_scale=0.0,
                          rescale=0.0):
    """the loop of pea_diffusion_amd.pag.denoise_perturbed around the oracle, whose PerturbAttention modules the caller has set
    (`set_perturb` with first = the number of unperturbed samples; mode None gives the plain CFG loop)"""
    cfg = guidance_scale > 1.0
    n = latents.shape[0]
    k = 3 if cfg else 2
    scheduler.set_timesteps(n_steps)
    latents = latents * scheduler.init_noise_sigma
    more = lambda v: torch.cat([v, v[-n:]])
    embeds = more(prompt_embeds)
    added = None if added is None else {key: more(v) for key, v in added.items()}
    for t in scheduler.timesteps:
        x = scheduler.scale_model_input(torch.cat([latents] * k), t)
        eps = unet(x.float(), int(t), encoder_hidden_states=embeds, added_cond_kwargs=added, return_dict=False)[0]
        s_t = max(0.0, scale - adaptive_scale * (1000.0 - float(t)))
        latents = scheduler.step(combine_ref(eps, guidance_scale, s_t, rescale, cfg), t, latents)[0]
    return latents
