"""Cross-attention heat maps (DAAM, "What the DAAM: Interpreting Stable Diffusion Using Cross Attention", Tang et al. 2022):
where in the picture each prompt token acts.

The definition restated (unpinned, the `daam` package is not a dependency): for token k the map is the sum,
over every cross-attention layer, head and denoising step, of that layer's softmax probabilities of key k, each layer's
h_l x w_l map upsampled bicubically to one common size.  Here the heads are averaged inside the kernel (`xattn_maps_kernel`
adds the head MEAN of a layer-forward into the accumulator of its latent grid: `HipUNet.enable_attention_maps`), layers of one
grid are summed before the upsampling (the upsampling is linear, so the order does not matter), and the total is divided by
the number of layer-forwards: a mean probability per (token, pixel) instead of DAAM's raw sum, which differs by one constant
per image and keeps maps of runs with different step counts comparable."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._lib import PeaError


def combine(levels, size=None, clamp=True):
    """levels: {(h_l, w_l): (tensor [B, L, h_l, w_l], n_accumulated)} or an iterable of such (tensor, n) pairs -- per latent grid the
    summed head-mean probabilities and the number of layer-forwards in the sum (`HipUNet.attention_maps()`).  Every level is
    upsampled to `size` (default: the largest grid among the levels) with `F.interpolate(mode="bicubic", align_corners=False)`;
    with `clamp` negatives (bicubic overshoot) go to 0, as DAAM does; the levels are summed and divided by the total count.
    -> fp32 [B, L, H, W].  Pure torch: runs on CPU tensors too."""
    pairs = list(levels.values()) if isinstance(levels, dict) else list(levels)
    if not pairs:
        raise PeaError("attention_maps.combine: no levels")
    if size is None:
        size = max((tuple(t.shape[-2:]) for t, _ in pairs), key=lambda hw: hw[0] * hw[1])
    size = (int(size[0]), int(size[1]))
    total, count = None, 0
    for t, n in pairs:
        if t.dim() != 4:
            raise PeaError(f"attention_maps.combine: level {tuple(t.shape)}, expected [B, L, h, w]")
        t = t.to(torch.float32)
        up = t if tuple(t.shape[-2:]) == size else F.interpolate(t, size=size, mode="bicubic", align_corners=False)
        if clamp:
            up = up.clamp(min=0.0)
        total = up if total is None else total + up
        count += int(n)
    if count <= 0:
        raise PeaError("attention_maps.combine: nothing was accumulated (run a forward between enable_attention_maps and the readout)")
    return total / float(count)


def heat_maps(unet, size=None, do_cfg=False, tokens=None):
    """`combine` on the accumulators of `unet` (a `HipUNet` with `enable_attention_maps()` on).  do_cfg: the batch is
    [unconditional | conditional]; keep the conditional half.  tokens: indices of the context rows to keep (there is no
    tokenizer here: the caller knows which rows its words landed in).  -> fp32 [B or B / 2, L or len(tokens), H, W]."""
    m = combine(unet.attention_maps(), size=size)
    if do_cfg:
        if m.shape[0] % 2:
            raise PeaError(f"attention_maps.heat_maps: do_cfg needs an even batch (B={m.shape[0]})")
        m = m[m.shape[0] // 2:]
    if tokens is not None:
        m = m[:, torch.as_tensor(list(tokens), dtype=torch.long, device=m.device)]
    return m
