"""Image prompts (IP-Adapter) for the HIP UNet: reading the published weight files, numbering the cross-attention layers the
way the files do, and the base image projection.  The UNet side -- a second key / value projection per cross-attention
layer and the decoupled attention `softmax(q k^T) v + scale * softmax(q k_ip^T) v_ip` in one launch -- lives behind
`HipUNet.load_ip_adapter / set_ip_tokens` (include/pea_hip.h: pea_unet_ip_*, pea_op_attention_fwd_ip).

A file holds two groups:
  image_proj   `proj.weight` [N * cross_dim, embed_dim], `proj.bias`, `norm.weight`, `norm.bias` [cross_dim]: the base
               ImageProjModel, tokens = LayerNorm(proj(image_embeds).view(B, N, cross_dim))
  ip_adapter   `<i>.to_k_ip.weight`, `<i>.to_v_ip.weight` [C, cross_dim], i = the position of the layer's processor in
               `unet.attn_processors` (see layer_keys)
as a torch pickle of the two nested dicts (`.bin`) or flat with the group name as a prefix (`.safetensors`).  "Plus" files carry a
Resampler instead of `proj` / `norm`; it is not built here -- their tokens can be computed elsewhere and handed to
`HipUNet.set_ip_tokens` directly.  Everything but `IPAdapter.tokens` is host code."""
from __future__ import annotations

import re
from typing import Dict, List, Tuple

import torch

from . import config as _cfg
from ._lib import PeaError

MAX_TOKENS = 32                                 # image keys of one decoupled attention launch
_LAYER = re.compile(r"^(\d+)\.(to_k_ip|to_v_ip)\.weight$")


def _cross_layers(cfg) -> List[Tuple[str, int]]:
    """[(attn2 prefix, channels)] of every cross-attention layer in the order diffusers registers the modules: all of
    `down_blocks`, then all of `up_blocks`, then `mid_block` (UNet2DConditionModel.__init__ creates both ModuleLists before
    the mid block) -- not the down / mid / up order of a forward pass."""
    down, up, mid = _cfg.depth_tables(cfg)
    ch = list(cfg.block_out_channels)
    out = []
    for i, kind in enumerate(cfg.down_block_types):
        if kind.startswith("CrossAttn"):
            for j in range(cfg.layers_per_block):
                out += [(f"down_blocks.{i}.attentions.{j}.transformer_blocks.{t}.attn2", ch[i]) for t in range(down[i][j])]
    for i, kind in enumerate(cfg.up_block_types):
        if kind.startswith("CrossAttn"):
            for j in range(cfg.layers_per_block + 1):
                out += [(f"up_blocks.{i}.attentions.{j}.transformer_blocks.{t}.attn2", ch[len(ch) - 1 - i]) for t in range(up[i][j])]
    if mid >= 0:
        out += [(f"mid_block.attentions.0.transformer_blocks.{t}.attn2", ch[-1]) for t in range(mid)]
    return out


def layer_keys(cfg) -> List[Tuple[int, str]]:
    """[(index, attn2 prefix)]: the number an IP-Adapter file gives each cross-attention layer.  The file numbers the entries of
    `unet.attn_processors`; every transformer block contributes `attn1` then `attn2`, so cross-attention layers get the odd
    numbers (SDXL: 1..139, 49 = the first of up_blocks.0, 121 = the first of the mid block; SD1.5: 1..31)."""
    return [(2 * n + 1, pfx) for n, (pfx, _) in enumerate(_cross_layers(cfg))]


def load_ip_adapter_state_dict(path_or_dict) -> Dict[str, Dict[str, torch.Tensor]]:
    """-> {"image_proj": {...}, "ip_adapter": {"1.to_k_ip.weight": ...}} from that dict itself, a `.bin` / `.pt` pickle of it, or
    the flat `.safetensors` form (`image_proj.proj.weight`, `ip_adapter.1.to_k_ip.weight`)"""
    from .lora import load_lora_state_dict
    sd = load_lora_state_dict(path_or_dict)
    if not (isinstance(sd.get("image_proj"), dict) and isinstance(sd.get("ip_adapter"), dict)):
        nested: Dict[str, Dict[str, torch.Tensor]] = {"image_proj": {}, "ip_adapter": {}}
        for k, v in sd.items():
            grp, _, rest = k.partition(".")
            if grp not in nested or not rest or not torch.is_tensor(v):
                raise PeaError(f"load_ip_adapter_state_dict: unexpected key '{k}' (groups: image_proj, ip_adapter)")
            nested[grp][rest] = v
        sd = nested
    ip = sd["image_proj"]
    if any(k == "latents" or k.startswith(("layers.", "proj_in.", "proj_out.", "norm_out.")) for k in ip):
        raise PeaError("load_ip_adapter_state_dict: this is a 'plus' file (image_proj.latents / image_proj.layers.*): its "
                       "Resampler projection is not built; compute the image tokens elsewhere and pass them to "
                       "HipUNet.set_ip_tokens")
    absent = [k for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias") if k not in ip]
    if absent:
        raise PeaError(f"load_ip_adapter_state_dict: image_proj lacks {absent}")
    return {"image_proj": dict(ip), "ip_adapter": dict(sd["ip_adapter"])}


class IPAdapter:
    """The weights of one base IP-Adapter, checked against a UNet config: `layers` {`<attn2 prefix>.to_k_ip.weight`: tensor} for
    `HipUNet.load_ip_adapter`, and the image projection `tokens()`."""

    def __init__(self, sd, cfg):
        sd = load_ip_adapter_state_dict(sd)
        proj, self.cfg = sd["image_proj"], cfg
        cross = cfg.cross_attention_dim
        w = proj["proj.weight"]
        if w.dim() != 2 or w.shape[0] % cross or tuple(proj["norm.weight"].shape) != (cross,):
            raise PeaError(f"IPAdapter: image_proj.proj.weight {tuple(w.shape)} / norm.weight {tuple(proj['norm.weight'].shape)} do "
                           f"not fit cross_attention_dim {cross}")
        self.n_tokens, self.embed_dim = w.shape[0] // cross, w.shape[1]
        if not 1 <= self.n_tokens <= MAX_TOKENS:
            raise PeaError(f"IPAdapter: {self.n_tokens} image tokens (1..{MAX_TOKENS})")
        if tuple(proj["proj.bias"].shape) != (w.shape[0],) or tuple(proj["norm.bias"].shape) != (cross,):
            raise PeaError("IPAdapter: image_proj bias shapes do not match their weights")
        self._proj = {k: proj[k].detach() for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")}
        self._dev = None
        given, self.layers = dict(sd["ip_adapter"]), {}
        for (idx, pfx), (_, C) in zip(layer_keys(cfg), _cross_layers(cfg)):
            for nm in ("to_k_ip", "to_v_ip"):
                t = given.pop(f"{idx}.{nm}.weight", None)
                if t is None:
                    raise PeaError(f"IPAdapter: the file lacks '{idx}.{nm}.weight' ({pfx})")
                if tuple(t.shape) != (C, cross):
                    raise PeaError(f"IPAdapter: '{idx}.{nm}.weight' is {tuple(t.shape)}, {pfx} needs {(C, cross)}")
                self.layers[f"{pfx}.{nm}.weight"] = t.detach()
        if given:
            raise PeaError(f"IPAdapter: keys this UNet has no layer for: {sorted(given)[:5]}")

    def tokens(self, image_embeds, do_cfg: bool = False):
        """image_embeds [B, embed_dim] (`HipImageEncoder.encode(...)`'s image_embeds) -> fp32 tokens [B, N, cross_dim] on the
        device: LayerNorm(proj(embeds).view(B, N, cross_dim)), eps 1e-5.  do_cfg: [2B, N, cross_dim], the tokens of an all-zero
        embedding (the unconditional half) first."""
        from . import ops
        e = image_embeds.detach()
        if e.dim() != 2 or e.shape[1] != self.embed_dim:
            raise PeaError(f"IPAdapter.tokens: image_embeds {tuple(e.shape)}, expected [B, {self.embed_dim}]")
        if not e.is_cuda:
            e = e.to("cuda")
        if self._dev is None or self._dev[0].device != e.device:
            p = self._proj
            self._dev = (p["proj.weight"].to(e.device, torch.bfloat16).contiguous(),) + tuple(
                p[k].to(e.device, torch.float32).contiguous() for k in ("proj.bias", "norm.weight", "norm.bias"))
        w, b, g, beta = self._dev
        e = e.to(torch.bfloat16)
        if do_cfg:
            e = torch.cat([torch.zeros_like(e), e])
        cross = self.cfg.cross_attention_dim
        y = ops.gemm(e.contiguous(), w, bias=b, out_f32=True).view(-1, cross)
        return ops.layernorm_fwd(y, g, beta, 1e-5)[0].view(e.shape[0], self.n_tokens, cross)
