"""Image prompts (IP-Adapter) for the HIP UNet: reading the published weight files, numbering the cross-attention layers the
way the files do, and both image projections: the base one and the Resampler of the "plus" files.  The UNet side -- a second key / value projection per cross-attention
layer and the decoupled attention `softmax(q k^T) v + scale * softmax(q k_ip^T) v_ip` in one launch -- lives behind
`HipUNet.load_ip_adapter / set_ip_tokens` (include/pea_hip.h: pea_unet_ip_*, pea_op_attention_fwd_ip).

A file holds two groups:
  image_proj   `proj.weight` [N * cross_dim, embed_dim], `proj.bias`, `norm.weight`, `norm.bias` [cross_dim]: the base
               ImageProjModel, tokens = LayerNorm(proj(image_embeds).view(B, N, cross_dim))
  ip_adapter   `<i>.to_k_ip.weight`, `<i>.to_v_ip.weight` [C, cross_dim], i = the position of the layer's processor in
               `unet.attn_processors` (see layer_keys)
as a torch pickle of the two nested dicts (`.bin`) or flat with the group name as a prefix (`.safetensors`).

"Plus" files (`ip-adapter-plus_sdxl_vit-h`, `ip-adapter-plus-face_sdxl_vit-h`, the SD1.5 plus files) carry a Perceiver Resampler
in `image_proj` instead of `proj` / `norm`: `latents` [1, Nq, dim], `proj_in`, `proj_out`, `norm_out`, and per layer L
`layers.L.0.{norm1, norm2, to_q, to_kv, to_out}` (PerceiverAttention) and `layers.L.1.{0, 1, 3}` (LayerNorm, Linear, GELU, Linear).
It consumes the tower's `hidden_states[-2]` (`HipImageEncoder.encode(pixels, hidden_index=-2)`), not `image_embeds`:

    ad = IPAdapterPlus(path, unet.cfg); unet.load_ip_adapter(ad)
    unet.set_ip_tokens(ad.encode(image_encoder, pixels, do_cfg=True))      # [2B, Nq, cross_dim], unconditional half first

`IPAdapterPlus.tokens` runs the Resampler as an op tape on the device (`HipResampler`; include/pea_hip.h: pea_resampler_*, with
pea_op_attention_fwd_fewq for its two-source attention).  Under CFG the plus pipelines resample the tower's states of an all-zero
PIXEL tensor for the unconditional half; the base adapter projects an all-zero embedding.  The two loaders refuse each other's
files.  Everything but the two `tokens` methods is host code."""
from __future__ import annotations

import ctypes
import re
from typing import Dict, List, Tuple

import torch

from . import config as _cfg
from ._lib import PeaError, check, lib, ptr, stream_ptr
from .tape import HipTape

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


def downsample_mask(mask, h_l: int, w_l: int) -> torch.Tensor:
    """A region mask [h, w] or [1|B, h, w] (any resolution, any float or bool dtype) reduced to the h_l x w_l grid of one
    cross-attention layer: `F.interpolate(mode="bicubic", align_corners=False)` without antialiasing, flattened row-major to fp32
    [1|B, h_l * w_l] -- the rule of diffusers' IPAdapterMaskProcessor.downsample as restated in DESIGN.md section 2 (unpinned:
    diffusers is not installed here).  Bicubic taps are negative at distance > 1, so a binary mask comes out below 0 and above 1
    next to its edges; the attention takes the values as they are."""
    m = torch.as_tensor(mask)
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise PeaError(f"downsample_mask: mask {tuple(m.shape)}, expected [h, w] or [1|B, h, w]")
    out = torch.nn.functional.interpolate(m[:, None].to(torch.float32), size=(int(h_l), int(w_l)), mode="bicubic", align_corners=False)
    return out.reshape(m.shape[0], int(h_l) * int(w_l)).contiguous()


BLOCK_SCALE_KEYS = "down | up | mid, `down_blocks.<i>` / `up_blocks.<i>` / `mid_block`, any longer prefix of an attn2 module name, or `default`"


def resolve_layer_scales(cfg, spec) -> List[float]:
    """One adapter's scale as a per-layer vector in the order of `layer_keys(cfg)`.  spec: a number (every layer), or a dict of
    per-block scales (InstantStyle: `{"up": {"block_0": ...}}` is written here as `{"up_blocks.0": ...}`).  Accepted keys:
      "down", "up", "mid"                       every cross-attention layer of the down blocks / up blocks / mid block
      "down_blocks.1", "up_blocks.0", "mid_block", "up_blocks.0.attentions.1", ...
                                                any prefix of the names `_cross_layers(cfg)` lists, cut at a `.`
      "default"                                 layers no other key names (0 when absent: a dict switches off what it leaves out)
    The longest matching key wins.  A key that matches no layer is refused."""
    names = [pfx for pfx, _ in _cross_layers(cfg)]
    if not isinstance(spec, dict):
        return [float(spec)] * len(names)
    short = {"down": "down_blocks", "up": "up_blocks", "mid": "mid_block"}
    keys = {}
    for k, v in spec.items():
        if k == "default":
            continue
        full = short.get(k, k)
        if not any(n == full or n.startswith(full + ".") for n in names):
            raise PeaError(f"resolve_layer_scales: '{k}' names no cross-attention layer of this UNet (keys: {BLOCK_SCALE_KEYS})")
        keys[full] = float(v)
    default = float(spec.get("default", 0.0))
    out = []
    for n in names:
        hit = [k for k in keys if n == k or n.startswith(k + ".")]
        out.append(keys[max(hit, key=len)] if hit else default)
    return out


def _groups(path_or_dict, who: str) -> Dict[str, Dict[str, torch.Tensor]]:
    """the two groups of a file of either kind, from the nested dict itself, a pickle of it, or the flat `.safetensors` form"""
    from .lora import load_lora_state_dict
    sd = load_lora_state_dict(path_or_dict)
    if not (isinstance(sd.get("image_proj"), dict) and isinstance(sd.get("ip_adapter"), dict)):
        nested: Dict[str, Dict[str, torch.Tensor]] = {"image_proj": {}, "ip_adapter": {}}
        for k, v in sd.items():
            grp, _, rest = k.partition(".")
            if grp not in nested or not rest or not torch.is_tensor(v):
                raise PeaError(f"{who}: unexpected key '{k}' (groups: image_proj, ip_adapter)")
            nested[grp][rest] = v
        sd = nested
    return sd


def _is_plus(image_proj) -> bool:
    return any(k == "latents" or k.startswith(("layers.", "proj_in.", "proj_out.", "norm_out.")) for k in image_proj)


def load_ip_adapter_state_dict(path_or_dict) -> Dict[str, Dict[str, torch.Tensor]]:
    """-> {"image_proj": {...}, "ip_adapter": {"1.to_k_ip.weight": ...}} from that dict itself, a `.bin` / `.pt` pickle of it, or
    the flat `.safetensors` form (`image_proj.proj.weight`, `ip_adapter.1.to_k_ip.weight`).  Base files only."""
    sd = _groups(path_or_dict, "load_ip_adapter_state_dict")
    ip = sd["image_proj"]
    if _is_plus(ip):
        raise PeaError("load_ip_adapter_state_dict: this is a 'plus' file (image_proj.latents / image_proj.layers.*): its "
                       "Resampler projection is not part of IPAdapter; open it with IPAdapterPlus, whose tokens() / encode() "
                       "feed HipUNet.set_ip_tokens")
    absent = [k for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias") if k not in ip]
    if absent:
        raise PeaError(f"load_ip_adapter_state_dict: image_proj lacks {absent}")
    return {"image_proj": dict(ip), "ip_adapter": dict(sd["ip_adapter"])}


def load_ip_adapter_plus_state_dict(path_or_dict) -> Dict[str, Dict[str, torch.Tensor]]:
    """the same for a "plus" file: `image_proj` holds the Resampler (`latents`, `proj_in.*`, `layers.L.*`, `proj_out.*`,
    `norm_out.*`).  A base file is refused."""
    sd = _groups(path_or_dict, "load_ip_adapter_plus_state_dict")
    ip = sd["image_proj"]
    if "proj.weight" in ip or "norm.weight" in ip or not _is_plus(ip):
        raise PeaError("load_ip_adapter_plus_state_dict: this is not a 'plus' file (image_proj.proj / image_proj.norm, no "
                       "image_proj.latents): open a base file with IPAdapter / load_ip_adapter_state_dict")
    absent = [k for k in ("latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight",
                          "norm_out.bias", "layers.0.0.to_q.weight") if k not in ip]
    if absent:
        raise PeaError(f"load_ip_adapter_plus_state_dict: image_proj lacks {absent}")
    return {"image_proj": dict(ip), "ip_adapter": dict(sd["ip_adapter"])}


class _LayerMap:
    """what both adapter kinds hand `HipUNet.load_ip_adapter`: `cfg`, `n_tokens` and `layers` {`<attn2 prefix>.to_k_ip.weight`:
    tensor}, every entry of the file's `ip_adapter` group matched to its cross-attention layer and checked for shape"""

    def _map_layers(self, given, cfg, who: str):
        cross = cfg.cross_attention_dim
        given, self.layers = dict(given), {}
        for (idx, pfx), (_, C) in zip(layer_keys(cfg), _cross_layers(cfg)):
            for nm in ("to_k_ip", "to_v_ip"):
                t = given.pop(f"{idx}.{nm}.weight", None)
                if t is None:
                    raise PeaError(f"{who}: the file lacks '{idx}.{nm}.weight' ({pfx})")
                if tuple(t.shape) != (C, cross):
                    raise PeaError(f"{who}: '{idx}.{nm}.weight' is {tuple(t.shape)}, {pfx} needs {(C, cross)}")
                self.layers[f"{pfx}.{nm}.weight"] = t.detach()
        if given:
            raise PeaError(f"{who}: keys this UNet has no layer for: {sorted(given)[:5]}")


class IPAdapter(_LayerMap):
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
        self._map_layers(sd["ip_adapter"], cfg, "IPAdapter")

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


# ---------------------------------------------------------------- the Resampler of the "plus" files
HEAD_DIM = 64                                   # dim_head of every published Resampler


def resampler_keys(rc: "_cfg.ResamplerConfig") -> Dict[str, tuple]:
    """{key under `image_proj.`: shape} of a Resampler with these dimensions, in the file's layout"""
    inner = rc.heads * HEAD_DIM
    out = {"latents": (1, rc.n_queries, rc.dim), "proj_in.weight": (rc.dim, rc.embed_dim), "proj_in.bias": (rc.dim,),
           "proj_out.weight": (rc.out_dim, rc.dim), "proj_out.bias": (rc.out_dim,), "norm_out.weight": (rc.out_dim,),
           "norm_out.bias": (rc.out_dim,)}
    for l in range(rc.depth):
        a, f = f"layers.{l}.0", f"layers.{l}.1"
        for n in ("norm1", "norm2"):
            out[f"{a}.{n}.weight"] = out[f"{a}.{n}.bias"] = (rc.dim,)
        out[f"{a}.to_q.weight"], out[f"{a}.to_kv.weight"], out[f"{a}.to_out.weight"] = (inner, rc.dim), (2 * inner, rc.dim), (rc.dim, inner)
        out[f"{f}.0.weight"] = out[f"{f}.0.bias"] = (rc.dim,)
        out[f"{f}.1.weight"], out[f"{f}.3.weight"] = (rc.ff_inner, rc.dim), (rc.dim, rc.ff_inner)
    return out


def resampler_config_of(image_proj) -> "_cfg.ResamplerConfig":
    """every dimension from the tensor shapes of a plus file's `image_proj` group; the head count from to_q's rows at the fixed
    head width of 64.  Any key missing, left over or of another shape than these dimensions imply is refused."""
    who = "IPAdapterPlus"
    try:
        lat, w_in, w_out = image_proj["latents"], image_proj["proj_in.weight"], image_proj["proj_out.weight"]
        q, ff = image_proj["layers.0.0.to_q.weight"], image_proj["layers.0.1.1.weight"]
    except KeyError as e:
        raise PeaError(f"{who}: image_proj lacks {e.args[0]!r}") from None
    if lat.dim() != 3 or lat.shape[0] != 1 or w_in.dim() != 2 or w_out.dim() != 2 or q.dim() != 2 or ff.dim() != 2:
        raise PeaError(f"{who}: latents {tuple(lat.shape)} / proj_in {tuple(w_in.shape)} / proj_out {tuple(w_out.shape)} are not a Resampler's")
    dim, inner = lat.shape[2], q.shape[0]
    kv = image_proj.get("layers.0.0.to_kv.weight")
    if inner % HEAD_DIM or kv is None or kv.shape[0] != 2 * inner:
        raise PeaError(f"{who}: to_q has {inner} rows, to_kv {None if kv is None else kv.shape[0]}: heads must be {HEAD_DIM} wide")
    depth = 1 + max(int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", k) for k in image_proj) if m)
    rc = _cfg.ResamplerConfig(embed_dim=w_in.shape[1], dim=dim, heads=inner // HEAD_DIM, depth=depth, n_queries=lat.shape[1],
                              ff_inner=ff.shape[0], out_dim=w_out.shape[0])
    want = resampler_keys(rc)
    absent, extra = [k for k in want if k not in image_proj], [k for k in image_proj if k not in want]
    if absent or extra:
        raise PeaError(f"{who}: image_proj lacks {absent[:5]}, has unexpected {extra[:5]}")
    for k, shape in want.items():
        if tuple(image_proj[k].shape) != shape:
            raise PeaError(f"{who}: image_proj.{k} is {tuple(image_proj[k].shape)}, expected {shape} (heads {HEAD_DIM} wide)")
    return rc


def resampler_plan(rc, batch: int = 1, seq: int = 257) -> Dict[str, int]:
    """parameter total and attention census of the Resampler tape (pea_resampler_plan: host only, no device needed)"""
    c = _cfg.resampler_to_c(rc)
    n, a, pre = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
    check(lib().pea_resampler_plan(ctypes.byref(c), batch, seq, ctypes.byref(n), ctypes.byref(a), ctypes.byref(pre)))
    return {"n_params": n.value, "n_attn": a.value, "n_prescaled": pre.value}


def resampler_weight_table(rc, batch: int = 1, seq: int = 257) -> Dict[str, tuple]:
    """{key: shape in the file's layout} of the tape's weight table, without a device (pea_resampler_plan_weight)"""
    c = _cfg.resampler_to_c(rc)
    name = ctypes.create_string_buffer(256)
    numel, kind, d0, d1 = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    out, i = {}, 0
    while lib().pea_resampler_plan_weight(ctypes.byref(c), batch, seq, i, name, 256, ctypes.byref(numel), ctypes.byref(kind),
                                          ctypes.byref(d0), ctypes.byref(d1)) == 0:
        out[name.value.decode()] = (d0.value,) if kind.value == 0 else (d0.value, d1.value)
        i += 1
    if "latents" in out:
        out["latents"] = (1,) + out["latents"]
    return out


class HipResampler(HipTape):
    """The Resampler as an op tape for `batch` samples of `seq` image rows; weights under the file's `image_proj.` key names."""

    def __init__(self, rc, batch: int, seq: int):
        self._open()
        self.cfg, self.B, self.S = rc, batch, seq
        c = _cfg.resampler_to_c(rc)
        check(lib().pea_resampler_create(ctypes.byref(c), batch, seq, ctypes.byref(self._h)))

    def weight_table(self) -> Dict[str, tuple]:
        table = super().weight_table()
        table["latents"] = (1,) + table["latents"]                 # the file's [1, Nq, dim]; the tape holds [Nq, dim]
        return table

    def forward(self, hidden):
        """hidden [B, S, embed_dim] -> fp32 tokens [B, Nq, out_dim] on the device"""
        want = (self.B, self.S, self.cfg.embed_dim)
        if tuple(hidden.shape) != want:
            raise PeaError(f"HipResampler built for hidden states {want}, got {tuple(hidden.shape)}")
        h = hidden.detach().to(self.device, torch.float32).contiguous()
        out = torch.empty(self.B, self.cfg.n_queries, self.cfg.out_dim, device=self.device, dtype=torch.float32)
        check(lib().pea_resampler_forward(self._h, ptr(h), ptr(out), stream_ptr()))
        self._keep = h
        return out

    __call__ = forward


class IPAdapterPlus(_LayerMap):
    """The weights of one "plus" IP-Adapter, checked against a UNet config: `layers` as `IPAdapter.layers`, the Resampler's
    dimensions (`resampler`, read off the tensor shapes) and the image projection `tokens()` / `encode()`."""

    def __init__(self, sd, cfg):
        sd = load_ip_adapter_plus_state_dict(sd)
        self.cfg = cfg
        self._proj = {k: v.detach() for k, v in sd["image_proj"].items()}
        self.resampler = rc = resampler_config_of(self._proj)
        self.n_tokens, self.embed_dim = rc.n_queries, rc.embed_dim
        if not 1 <= self.n_tokens <= MAX_TOKENS:
            raise PeaError(f"IPAdapterPlus: {self.n_tokens} image tokens (1..{MAX_TOKENS})")
        if rc.out_dim != cfg.cross_attention_dim:
            raise PeaError(f"IPAdapterPlus: the Resampler's output_dim {rc.out_dim} is not this UNet's cross_attention_dim "
                           f"{cfg.cross_attention_dim}")
        self._map_layers(sd["ip_adapter"], cfg, "IPAdapterPlus")
        self._tapes: Dict[tuple, HipResampler] = {}

    def _tape(self, batch: int, seq: int) -> HipResampler:
        """the tape for this (batch, rows per image), built and loaded on first use"""
        if (batch, seq) not in self._tapes:
            t = HipResampler(self.resampler, batch, seq)
            t.load_state_dict(self._proj)
            self._tapes[(batch, seq)] = t
        return self._tapes[(batch, seq)]

    def tokens(self, hidden, uncond_hidden=None):
        """hidden [B, S, embed_dim] (`HipImageEncoder.encode(pixels, hidden_index=-2)`'s hidden states) -> fp32 tokens
        [B, Nq, cross_dim] on the device.  uncond_hidden (the same of an all-zero pixel tensor): [2B, Nq, cross_dim], the
        unconditional half first, resampled in the same pass."""
        h = hidden.detach()
        if h.dim() != 3 or h.shape[2] != self.embed_dim:
            raise PeaError(f"IPAdapterPlus.tokens: hidden states {tuple(h.shape)}, expected [B, S, {self.embed_dim}]")
        if uncond_hidden is not None:
            if tuple(uncond_hidden.shape) != tuple(h.shape):
                raise PeaError(f"IPAdapterPlus.tokens: uncond_hidden {tuple(uncond_hidden.shape)} != hidden {tuple(h.shape)}")
            h = torch.cat([uncond_hidden.detach().to(h.device), h])
        return self._tape(h.shape[0], h.shape[1]).forward(h)

    def encode(self, image_encoder, pixels, do_cfg: bool = False):
        """pixels (normalised: `vision.preprocess`) -> the tower's `hidden_states[-2]` -> tokens; do_cfg: the unconditional half
        is the same path on all-zero pixels, and comes first"""
        hid = image_encoder.encode(pixels, hidden_index=-2)[0]
        un = image_encoder.encode(torch.zeros_like(pixels), hidden_index=-2)[0] if do_cfg else None
        return self.tokens(hid, un)
