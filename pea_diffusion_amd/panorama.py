"""MultiDiffusion (Bar-Tal, Yariv, Lipman, Dekel 2023, "MultiDiffusion: Fusing Diffusion Paths for Controlled Image Generation"):
a latent canvas larger than the UNet's window is denoised through overlapping window-sized views with the unchanged fixed-shape
UNet, and the views are reconciled in the overlaps at every step.  It needs no weights and works with every scheduler here.

Canvas fp32 [N, C, Hc, Wc], window h x w (the context's), Hc >= h, Wc >= w.  A view is (n, y0, x0): image n, rows
y0 .. y0 + h - 1, columns (x0 + j) mod Wc for j < w; with `wrap_x` (circular panoramas) a view may straddle the seam, without it
x0 + w <= Wc; there is no wrap in y.  Weights are separable, wy[i] wx[j] at window position (i, j); T[n, Y, X] is the sum of the
weights of the views that cover an element, added in ascending view order in fp32.  One step at scheduler position i:
  1. each view's model input is its crop of the canvas times the scheduler's input scale, doubled to [uncond | text] under CFG
     (`ops.views_gather`, one launch per UNet call),
  2. the UNet runs over the views, `vb` of them per call (a chunk; the last one is padded with a repeat of its last view),
  3. each view's prediction is e_v = u + g (t - u), times its own `rescale_noise_cfg` factor when guidance_rescale > 0,
  4. the canvas prediction is (sum over covering views, ascending, of wy wx e_v) / T (`ops.views_merge_`, one launch per UNet call),
  5. `scheduler.step` runs once, on the canvas; ancestral and LCM noise is drawn once, canvas-shaped.
The arithmetic is a restatement of the paper (unpinned); tests/panorama_ref.py says it again in plain torch.
Stepping every view and averaging the results (diffusers' StableDiffusionPanoramaPipeline) is the same thing for the four
schedulers here, whose step is affine in (x, eps, history) with coefficients that do not depend on the view -- except that
diffusers draws ancestral noise per view and averages it, which loses variance in the overlaps; that is not copied.

Per-view prompts, per-view `time_ids` crop coordinates, ControlNet residuals, inpainting and anything whose state is tied to a
position in the picture (regional prompts, IP region masks, attention maps) are outside this loop.
"""
from __future__ import annotations

import functools
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import ops
from . import sampler as _sampler
from ._lib import PeaError, lib

MAX_VIEW_SLOTS = 16        # view slots of one chunk (the kernels' slot table)


def _origins(size: int, win: int, stride: int, wrap: bool) -> List[int]:
    if win > size:
        raise PeaError(f"views: a window of {win} on a canvas axis of {size}")
    if stride < 1:
        raise PeaError(f"views: stride {stride}")
    if wrap:
        out = list(range(0, size, stride))
    else:
        out = list(range(0, size - win + 1, stride))
        if (size - win) % stride:
            out.append(size - win)                       # flush with the edge: the remainder is covered too
    covered = [False] * size
    for o in out:
        for k in range(win):
            covered[(o + k) % size] = True
    assert all(covered), f"views: stride {stride} leaves part of an axis of {size} outside every window of {win}"
    return out


def views(Hc: int, Wc: int, h: int, w: int, stride: int, wrap_x: bool = False) -> List[Tuple[int, int]]:
    """The views of one image as (y0, x0), in row-major order of the origins.  Per axis the origins are 0, stride, 2 stride, ...
    <= size - win, plus one last origin size - win when that is no multiple of the stride; on a wrapped x axis 0, stride, ... < Wc.
    Every canvas element is covered by at least one view (asserted)."""
    ys, xs = _origins(Hc, h, stride, False), _origins(Wc, w, stride, bool(wrap_x))
    return [(y0, x0) for y0 in ys for x0 in xs]


def view_weights(n: int, kind: str = "uniform", overlap: Optional[int] = None) -> torch.Tensor:
    """One table of the separable view weights, fp32 [n] (evaluated in float64), all positive.  "uniform": ones (the paper).
    "ramp": min(i + 1, n - i, overlap + 1) / (overlap + 1).  "gaussian": exp(-(i - (n - 1) / 2)^2 / (n^2 0.02)) / sqrt(0.02 pi)
    (Mixture of Diffusers, variance 0.01)."""
    i = torch.arange(n, dtype=torch.float64)
    if kind == "uniform":
        t = torch.ones(n, dtype=torch.float64)
    elif kind == "ramp":
        if overlap is None or overlap < 0:
            raise PeaError(f"view_weights: ramp weights need overlap >= 0, got {overlap}")
        t = torch.minimum(torch.minimum(i + 1, n - i), torch.full_like(i, overlap + 1.0)) / (overlap + 1.0)
    elif kind == "gaussian":
        t = torch.exp(-(i - (n - 1) / 2.0) ** 2 / (n * n * 0.02)) / math.sqrt(0.02 * math.pi)
    else:
        raise PeaError(f"view_weights: kind {kind!r} (uniform, ramp, gaussian)")
    return t.float()


def _triples(vs: Sequence, N: int) -> List[Tuple[int, int, int]]:
    """(y0, x0) views of one image -> the (n, y0, x0) of N images, image by image; triples pass through"""
    vs = [tuple(int(a) for a in v) for v in vs]
    if vs and len(vs[0]) == 3:
        return vs
    return [(n, y0, x0) for n in range(N) for (y0, x0) in vs]


def weight_total(views, N: int, Hc: int, Wc: int, wy: torch.Tensor, wx: torch.Tensor, wrap_x: bool = False) -> torch.Tensor:
    """T fp32 [N, Hc, Wc] on the host: the weights wy[i] wx[j] of the covering views, added in ascending view order in fp32.
    `views`: (n, y0, x0) triples, or the (y0, x0) of one image, which every image then has."""
    wy, wx = wy.detach().float().cpu(), wx.detach().float().cpu()
    h, w = wy.numel(), wx.numel()
    plane = wy[:, None] * wx[None, :]
    T = torch.zeros(N, Hc, Wc, dtype=torch.float32)
    for n, y0, x0 in _triples(views, N):
        if not (0 <= n < N and 0 <= y0 <= Hc - h and 0 <= x0 and (x0 < Wc if wrap_x else x0 <= Wc - w)):
            raise PeaError(f"weight_total: view {(n, y0, x0)} outside {N} canvases of {Hc} x {Wc} (wrap_x={bool(wrap_x)})")
        cols = (x0 + torch.arange(w)) % Wc
        Tn = T[n]
        Tn[y0:y0 + h, cols] = Tn[y0:y0 + h, cols] + plane
    assert bool((T > 0).all()), "weight_total: a canvas element outside every view"
    return T


def _chunks(triples, vb):
    return [triples[k:k + vb] for k in range(0, len(triples), vb)]


def _axis_overlap(size, win, stride, overlap, wrap=False):
    """the overlap the ramp weights of an axis run over: none where the axis has a single origin"""
    if len(_origins(size, win, stride, wrap)) == 1:
        return 0
    return max(win - stride, 0) if overlap is None else int(overlap)


@functools.lru_cache(maxsize=8)
def _geometry(N, Hc, Wc, h, w, stride, wrap_x, kind, overlap, f, device):
    """-> (views as triples, wy, wx, T), the tables on the device, everything times f (the decoder's pixels per latent): computed once
    per geometry"""
    triples = [(n, y0 * f, x0 * f) for n, y0, x0 in _triples(views(Hc, Wc, h, w, stride, wrap_x), N)]
    wy = view_weights(h * f, kind, _axis_overlap(Hc, h, stride, overlap) * f)
    wx = view_weights(w * f, kind, _axis_overlap(Wc, w, stride, overlap, wrap_x) * f)
    T = weight_total(triples, N, Hc * f, Wc * f, wy, wx, wrap_x)
    return triples, wy.to(device), wx.to(device), T.to(device)


def denoise_panorama(unet, scheduler, latents, prompt_embeds, added_cond_kwargs, num_inference_steps: int = 30,
                     guidance_scale: float = 7.5, guidance_rescale: float = 0.0, stride: Optional[int] = None,
                     weights: str = "uniform", overlap: Optional[int] = None, wrap_x: bool = False, generator=None,
                     timestep_cond=None, callback: Optional[Callable] = None):
    """`sampler.denoise` on a canvas larger than the UNet's window.  latents [N, C, Hc, Wc] on the device; `prompt_embeds` and the
    tensors of `added_cond_kwargs` are per canvas image, laid out as `sampler.denoise` takes them for batch N ([uncond N | text N]
    when guidance_scale > 1), `timestep_cond` [N, dim]; they are expanded to the context's batch per chunk.  `unet.B` is
    dup * vb with dup = 2 under CFG and vb in 1..16 views per call.  stride (both axes) defaults to w // 2; weights is a
    `view_weights` kind, `overlap` the ramp's (default: window - stride).  Per step and chunk: one gather, the UNet, the two factor
    launches when guidance_rescale > 0, one merge; then the scheduler's step on the canvas.  Returns the canvas latents, fp32."""
    do_cfg = guidance_scale > 1.0
    dup = 2 if do_cfg else 1
    if latents.dim() != 4:
        raise PeaError(f"denoise_panorama: latents {tuple(latents.shape)}, expected [N, C, Hc, Wc]")
    N, C, Hc, Wc = latents.shape
    h, w = unet.H, unet.W
    vb = unet.B // dup
    if unet.B != dup * vb or not 1 <= vb <= MAX_VIEW_SLOTS:
        raise PeaError(f"denoise_panorama: a UNet of batch {unet.B} is not {dup} x vb for vb in 1..{MAX_VIEW_SLOTS} (guidance_scale {guidance_scale})")
    if Hc < h or Wc < w:
        raise PeaError(f"denoise_panorama: a {Hc} x {Wc} canvas is smaller than the UNet's {h} x {w} window")
    stride = int(stride) if stride is not None else w // 2
    dev = latents.device
    triples, wy, wx, T = _geometry(N, Hc, Wc, h, w, stride, bool(wrap_x), weights, overlap, 1, str(dev))
    timestep_cond = _sampler.check_timestep_cond(unet, timestep_cond, False)

    # the conditioning of a chunk: rows of the per-image tensors picked by the slots' image (padded slots repeat the last view)
    cond = {}

    def chunk_cond(chunk):
        ns = tuple([v[0] for v in chunk] + [chunk[-1][0]] * (vb - len(chunk)))
        if ns not in cond:
            idx = torch.tensor(ns, dtype=torch.long)
            idx = torch.cat([idx, idx + N]) if do_cfg else idx
            pick = lambda t: t.index_select(0, idx.to(t.device))
            added = None if added_cond_kwargs is None else {
                k: (pick(v) if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == dup * N else v) for k, v in added_cond_kwargs.items()}
            kw = {}
            if timestep_cond is not None:
                kw["timestep_cond"] = timestep_cond.index_select(0, torch.tensor(ns * dup, dtype=torch.long).to(timestep_cond.device))
            cond[ns] = (pick(prompt_embeds), added, kw)
        return cond[ns]

    if prompt_embeds.shape[0] != dup * N:
        raise PeaError(f"denoise_panorama: prompt_embeds of batch {prompt_embeds.shape[0]} for {N} canvas images (expected {dup * N})")
    chunks = _chunks(triples, vb)
    timesteps = scheduler.set_timesteps(num_inference_steps)
    latents = (latents.float() * scheduler.init_noise_sigma).contiguous()
    eps_canvas = torch.empty_like(latents)
    model_in = torch.empty(dup * vb, C, h, w, device=dev, dtype=torch.float32)
    rescale = do_cfg and guidance_rescale > 0.0
    factor = torch.empty(vb, device=dev, dtype=torch.float32) if rescale else None
    ws = torch.empty(lib().pea_op_cfg_combine_workspace_bytes(vb), device=dev, dtype=torch.uint8) if rescale else None
    for i, t in enumerate(timesteps):
        k_s = scheduler.model_input_scale()
        for ci, chunk in enumerate(chunks):
            embeds, added, kw = chunk_cond(chunk)
            ops.views_gather(latents, chunk, vb, (h, w), k_s, dup, wrap_x, out=model_in)
            eps = unet(model_in, t, encoder_hidden_states=embeds, added_cond_kwargs=added, return_dict=False, **kw)[0]
            if rescale:
                ops.cfg_rescale_factors(eps, guidance_scale, guidance_rescale, out=factor, workspace=ws)
            ops.views_merge_(eps_canvas, eps, chunk, wy, wx, T, dup, guidance_scale, factor, first=ci == 0,
                             last=ci == len(chunks) - 1, wrap_x=wrap_x)
        latents = scheduler.step(eps_canvas, t, latents, return_dict=False, generator=generator)[0]
        if callback is not None:
            callback(i, t, latents)
    return latents


def decode_tiled(decoder, latents, stride: Optional[int] = None, overlap: Optional[int] = None, inv_scaling: float = 1.0):
    """The canvas through the fixed-shape `HipVAEDecoder`: latent tiles of the decoder's h x w over the view geometry of
    `views` (stride in latent units, default w // 2; no wrap), `decoder.B` tiles per call, the decoded pixel tiles merged by
    `ops.views_merge_` with "ramp" weights over the pixel overlap (`overlap` in latent units, default tile - stride; an axis
    with a single tile has uniform weights).  latents [N, C, Hc, Wc] and `inv_scaling` as `decoder.decode` takes them.
    -> fp32 [N, 3, f Hc, f Wc], f the decoder's scale factor.  A canvas of one tile gives `decoder.decode`'s bits.
    As with tiled decoding everywhere, every tile has its own GroupNorm statistics and its own mid-block attention, so tiles
    disagree slightly where they overlap; the ramp blends the seams, it does not remove that difference."""
    if latents.dim() != 4:
        raise PeaError(f"decode_tiled: latents {tuple(latents.shape)}, expected [N, C, Hc, Wc]")
    N, C, Hc, Wc = latents.shape
    h, w, f, B = decoder.h, decoder.w, decoder.scale_factor, decoder.B
    if not 1 <= B <= MAX_VIEW_SLOTS:
        raise PeaError(f"decode_tiled: a decoder of batch {B} (1..{MAX_VIEW_SLOTS} tiles per call)")
    if Hc < h or Wc < w:
        raise PeaError(f"decode_tiled: a {Hc} x {Wc} canvas is smaller than the decoder's {h} x {w} tile")
    stride = int(stride) if stride is not None else w // 2
    dev = decoder.device
    triples = _triples(views(Hc, Wc, h, w, stride), N)
    pixel, wy, wx, T = _geometry(N, Hc, Wc, h, w, stride, False, "ramp", overlap, f, str(dev))
    z = latents.detach().to(dev, torch.float32).contiguous()
    image = torch.empty(N, 3, Hc * f, Wc * f, device=dev, dtype=torch.float32)
    tiles = torch.empty(B, C, h, w, device=dev, dtype=torch.float32)
    lat_chunks, pix_chunks = _chunks(triples, B), _chunks(pixel, B)
    for ci, (lc, pc) in enumerate(zip(lat_chunks, pix_chunks)):
        ops.views_gather(z, lc, B, (h, w), 1.0, 1, out=tiles)
        img = decoder.decode(tiles, inv_scaling=inv_scaling)[0]
        ops.views_merge_(image, img, pc, wy, wx, T, 1, first=ci == 0, last=ci == len(lat_chunks) - 1)
    return image
