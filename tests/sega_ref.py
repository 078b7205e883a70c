"""Semantic guidance (Brack et al. 2023) restated in plain torch on the CPU: the masked combine with its momentum, the two order
statistics behind torch.quantile's linear interpolation, and the loop around any UNet callable.  The arithmetic is DESIGN.md
section 2's (unpinned): eps = [u | t | e_1 .. e_K], per concept d_c = s_c (e_c - u), kept where |d_c| reaches the q_c-quantile of
its own channel."""
import math

import torch


def diff_ref(eps, K, c, scale):
    """d_c = s_c (e_c - u) in the dtype of eps: one subtraction, one multiplication"""
    B = eps.shape[0] // (2 + K)
    return torch.tensor(scale, dtype=eps.dtype) * (eps[(2 + c) * B:(3 + c) * B] - eps[:B])


def threshold_ref(d, q):
    """[B, C]: torch.quantile of |d| over the positions of each channel"""
    return torch.quantile(d.abs().flatten(2), q, dim=2)


def rank_ref(q, hw):
    """(k, k + 1 clamped) of torch.quantile: r = q (hw - 1) in fp32, k = floor(r)"""
    r = float(torch.tensor(q, dtype=torch.float32) * torch.tensor(hw - 1, dtype=torch.float32))
    k = min(int(math.floor(r)), hw - 1)
    return k, min(k + 1, hw - 1)


def bounds_ref(eps, edit_scale, quantile):
    """[K, B, C, 2]: v[k] and v[min(k + 1, hw - 1)] of the ascending |d_c| of every group, through torch.sort"""
    K = len(edit_scale)
    out = []
    for c in range(K):
        v = diff_ref(eps, K, c, edit_scale[c]).abs().flatten(2).sort(dim=2).values
        k, k1 = rank_ref(quantile[c], v.shape[2])
        out.append(torch.stack([v[:, :, k], v[:, :, k1]], dim=-1))
    return torch.stack(out)


def combine_ref(eps, mom, g, edit_scale, quantile, weight, warm, mu, beta):
    """-> (out, mom'): the step's arithmetic, literally; mom is not written.  A concept of weight 0 is skipped."""
    K = len(edit_scale)
    B = eps.shape[0] // (2 + K)
    u, t = eps[:B], eps[B:2 * B]
    f = lambda v: torch.tensor(v, dtype=eps.dtype)
    e_all, e_warm = torch.zeros_like(u), torch.zeros_like(u)
    for c in range(K):
        if weight[c] == 0:
            continue
        d = diff_ref(eps, K, c, edit_scale[c])
        thr = threshold_ref(d, quantile[c])
        m = torch.where(d.abs() >= thr[:, :, None, None], d, torch.zeros_like(d))
        e_all = e_all + f(weight[c]) * m
        if warm[c]:
            e_warm = e_warm + f(weight[c]) * m
    used = e_all + f(mu) * mom
    out = u + f(g) * (t - u)
    if any(warm):
        out = out + (e_warm + f(mu) * mom)
    return out, f(beta) * mom + (f(1.0) - f(beta)) * used


def denoise_semantic_ref(unet, scheduler, latents, embeds, added, plan, steps, g, mu=0.1, beta=0.4):
    """The loop around any UNet callable: embeds / added hold the whole batch [uncond | cond | edit_1 .. edit_K]; plan(i) gives the
    four K-lists of step i."""
    timesteps = scheduler.set_timesteps(steps)
    timesteps = scheduler.timesteps if timesteps is None else timesteps
    n = latents.shape[0]
    reps = embeds.shape[0] // n
    latents = latents * scheduler.init_noise_sigma
    mom = torch.zeros_like(latents)
    for i, t in enumerate(timesteps):
        x = scheduler.scale_model_input(torch.cat([latents] * reps), t)
        eps = unet(x, t, embeds, added_cond_kwargs=added)[0].to(latents.dtype)
        out, mom = combine_ref(eps, mom, g, *plan(i), mu, beta)
        latents = scheduler.step(out, t, latents)[0]
    return latents
