"""Regional text prompts ("regional prompter" / "attention couple"): a text prompt per region of the picture.

The R prompts' embeddings lie back to back in ONE context of R * 77 rows (`compose_prompt_embeds`), so the UNet's stacked K|V
projection serves them all, and every cross-attention layer computes

    O[b, q] = sum_r w[b, r, q] * softmax(scale q K_r^T) V_r

in one launch (`ops.attention_fwd_regions`, `HipUNet.set_prompt_regions`).  `region_weights` makes w from the regions' masks
for one layer's grid.  Nothing here touches a sampler: `sampler.denoise` takes the composed context as it takes any other.
Pooled embeds and time ids stay the caller's (the base prompt's); a ControlNet keeps its 77-row context."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._lib import PeaError


def region_weights(masks, weights, h_l: int, w_l: int, device=None) -> torch.Tensor:
    """-> fp32 [Bm, R, h_l * w_l]: what region r weighs at every position of an h_l x w_l layer grid.

    masks[r]: None (everywhere) or [h, w] / [1|B, h, w], values >= 0, at any resolution; reduced to the grid with
    `F.adaptive_avg_pool2d` -- area means keep values in [0, 1] and keep a partition a partition at every level (the bicubic
    rule of the image prompts does neither).  a_r = weights[r] * m_r, w_r = a_r / sum_r a_r where the sum exceeds 1e-6;
    elsewhere (nobody claims the position) region 0 gets 1."""
    masks = list(masks)
    R = len(masks)
    if R < 1:
        raise PeaError("region_weights: no regions")
    weights = [1.0] * R if weights is None else [float(x) for x in weights]
    if len(weights) != R:
        raise PeaError(f"region_weights: {len(weights)} weights for {R} regions")
    if any(not (x >= 0.0) or x == float("inf") for x in weights):
        raise PeaError(f"region_weights: weights {weights} (finite, >= 0)")
    red = []
    for r, m in enumerate(masks):
        if m is None:
            red.append(torch.ones(1, h_l, w_l, dtype=torch.float32, device=device))
            continue
        m = torch.as_tensor(m).to(device=device, dtype=torch.float32)
        m = m[None] if m.dim() == 2 else m
        if m.dim() != 3:
            raise PeaError(f"region_weights: mask {tuple(m.shape)} of region {r}, expected [h, w] or [B, h, w]")
        if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0:
            raise PeaError(f"region_weights: the mask of region {r} has negative or non-finite values")
        red.append(F.adaptive_avg_pool2d(m[:, None], (h_l, w_l))[:, 0])
    Bm = max(m.shape[0] for m in red)
    if any(m.shape[0] not in (1, Bm) for m in red):
        raise PeaError(f"region_weights: mask batches {[m.shape[0] for m in red]} (1 or one common size)")
    a = torch.stack([x * m.expand(Bm, h_l, w_l) for x, m in zip(weights, red)], 1)       # [Bm, R, h_l, w_l]
    tot = a.sum(1, keepdim=True)
    covered = tot > 1e-6
    w = torch.where(covered, a / torch.where(covered, tot, torch.ones_like(tot)), torch.zeros_like(a))
    w[:, :1] = torch.where(covered, w[:, :1], torch.ones_like(tot))
    return w.reshape(Bm, R, h_l * w_l).contiguous()


def compose_prompt_embeds(region_embeds, negative_embeds=None) -> torch.Tensor:
    """region_embeds: R tensors [n, 77, D] (the text encoder's states of each region's prompt) -> the context [n, R * 77, D].
    With negative_embeds [n, 77, D] (classifier-free guidance): [2 n, R * 77, D], the unconditional half first -- the negative
    prompt tiled R times, so that half has the same context length (`set_prompt_regions(..., do_cfg=True)` lets it attend to
    its first copy alone)."""
    region_embeds = list(region_embeds)
    if not region_embeds:
        raise PeaError("compose_prompt_embeds: no regions")
    shape = tuple(region_embeds[0].shape)
    if len(shape) != 3 or any(tuple(e.shape) != shape for e in region_embeds):
        raise PeaError(f"compose_prompt_embeds: region embeddings {[tuple(e.shape) for e in region_embeds]} (all [n, L, D])")
    cond = torch.cat(region_embeds, 1)
    if negative_embeds is None:
        return cond
    if tuple(negative_embeds.shape) != shape:
        raise PeaError(f"compose_prompt_embeds: negative embeddings {tuple(negative_embeds.shape)} != {shape}")
    return torch.cat([negative_embeds.repeat(1, len(region_embeds), 1).to(cond.dtype), cond], 0)
