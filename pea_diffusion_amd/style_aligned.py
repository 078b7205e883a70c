"""StyleAligned generation (Hertz, Voynov, Fruchter, Cohen-Or 2023, "Style Aligned Image Generation via Shared Attention"):
a batch of N prompts denoised together comes out in one style.  Sample 0 is the style reference; in the self-attention layers
every other sample ("target") moves its queries and keys onto the reference's per-channel statistics (AdaIN) and attends to the
reference's keys and values as well as its own, under one softmax.

There is no denoising loop here: `HipUNet.set_style_aligned(...)` switches the sharing on, `sampler.denoise` with the batch of
prompts is the loop, `HipUNet.clear_style_aligned()` switches it off.  This module holds the host-side bookkeeping: which sample
refers to which, and which self-attention layers share.

The arithmetic is restated from the paper and the authors' public code (their `share_attention=True, adain_queries=True,
adain_keys=True` path with `shared_score_scale` / `shared_score_shift`; see DESIGN.md section 2: unpinned).  Not built:
`share_group_norm`, `share_layer_norm` (both off in the authors' SDXL defaults), `adain_values`, `full_attention_share`.
"""
from __future__ import annotations

from typing import List, Sequence, Union

from . import config as _cfg
from ._lib import PeaError, lib


def reference_index(n: int, do_cfg: bool = False) -> List[int]:
    """ref[b] for a batch of n prompts whose first is the style reference: [-1, 0, 0, ...].  do_cfg: the batch is
    [uncond x n | cond x n] and each half has its own reference, samples 0 and n: [-1, 0, ..., 0, -1, n, ..., n]."""
    n = int(n)
    if n < 1:
        raise PeaError(f"reference_index: n={n} prompts")
    half = [-1] + [0] * (n - 1)
    return half + [-1 if r < 0 else r + n for r in half] if do_cfg else half


def layer_names_of(cfg) -> List[str]:
    """the `attn1` module name of every self-attention layer in the order a forward runs them: down blocks, mid block, up
    blocks (the order of `pea_unet_set_style_aligned`'s switches)"""
    down, up, mid = _cfg.depth_tables(cfg)
    out = []
    for i, kind in enumerate(cfg.down_block_types):
        if kind.startswith("CrossAttn"):
            for j in range(cfg.layers_per_block):
                out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.{t}.attn1" for t in range(down[i][j])]
    if mid >= 0:
        out += [f"mid_block.attentions.0.transformer_blocks.{t}.attn1" for t in range(mid)]
    for i, kind in enumerate(cfg.up_block_types):
        if kind.startswith("CrossAttn"):
            for j in range(cfg.layers_per_block + 1):
                out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.{t}.attn1" for t in range(up[i][j])]
    return out


def layer_names(unet) -> List[str]:
    """`layer_names_of(unet.cfg)`, checked against the number of self-attention launches the context's tape holds"""
    names = layer_names_of(unet.cfg)
    n = int(lib().pea_unet_num_self_attention_layers(unet._h))
    if n != len(names):
        raise PeaError(f"style_aligned.layer_names: the configuration names {len(names)} self-attention layers, the tape has {n}")
    return names


def level_switches(n_layers: int, level: float) -> List[bool]:
    """`level` of the n layers switched on, spread evenly: the switch vector of the authors' `_get_switch_vec`.  0: none, 1: all;
    below one half every (n // int(level n))-th layer is on, above it the complement of the vector for 1 - level.  Their
    `only_self_level = x` (the share of layers that do NOT share) is `layers = 1 - x` here."""
    n, level = int(n_layers), float(level)
    if not 0.0 <= level <= 1.0:
        raise PeaError(f"level_switches: level {level} is outside 0..1")
    if level == 0.0:
        return [False] * n
    if level == 1.0:
        return [True] * n
    flip = level > 0.5
    if flip:
        level = 1.0 - level
    k = int(level * n)
    if k == 0:
        vec = [False] * n
    else:
        vec = [i % (n // k) == 0 for i in range(n)]
    return [not v for v in vec] if flip else vec


def resolve_layers(unet, layers: Union[None, float, Sequence[str], dict]) -> List[float]:
    """One switch (1.0 / 0.0) per self-attention layer in the order of `layer_names(unet)`.  layers: None (all), a number 0..1
    (`level_switches`), a list of names or name prefixes cut at a `.` ("up_blocks.0", "mid_block", "down", "up", "mid"), or a
    dict of such keys to truth values (the longest matching key wins; layers no key names are off).  A key that matches no layer
    is refused."""
    names = layer_names(unet)
    if layers is None:
        return [1.0] * len(names)
    if isinstance(layers, bool):
        return [float(layers)] * len(names)
    if isinstance(layers, (int, float)):
        return [float(v) for v in level_switches(len(names), layers)]
    if isinstance(layers, str):
        layers = [layers]
    spec = dict(layers) if isinstance(layers, dict) else {k: True for k in layers}
    short = {"down": "down_blocks", "up": "up_blocks", "mid": "mid_block"}
    keys = {}
    for k, v in spec.items():
        full = short.get(k, k)
        if not any(n == full or n.startswith(full + ".") for n in names):
            raise PeaError(f"style_aligned.resolve_layers: '{k}' names no self-attention layer of this UNet")
        keys[full] = 1.0 if v else 0.0
    out = []
    for n in names:
        hit = [k for k in keys if n == k or n.startswith(k + ".")]
        out.append(keys[max(hit, key=len)] if hit else 0.0)
    return out
