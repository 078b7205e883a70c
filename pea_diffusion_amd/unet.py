"""`HipUNet`: the UNet plug-in surface of the reference --
`unet(sample, t, encoder_hidden_states, added_cond_kwargs=..., return_dict=False)[0]`
(train_sdxl_zh.py:397,415; tests/test_sdxl_zh.py:384-391) -- backed by the HIP op tape in
libpea_hip.so.  `down_blocks[i]`, `mid_block`, `up_blocks[i]` accept `register_forward_hook`
so the reference's `cast_hook` (train_sdxl_zh.py:79-84) works unchanged."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import torch

from . import config as _cfg
from ._lib import PeaError, check, lib, ptr, stream_ptr
from .tape import HipTape, _staged


class _HookHandle:
    def __init__(self, lst, fn):
        self.lst, self.fn = lst, fn

    def remove(self):
        if self.fn in self.lst:
            self.lst.remove(self.fn)


class _BlockShim:
    """Hook-able stand-in for a diffusers block; `residuals_present` mirrors the `(hidden, res_samples)`
    tuple that down blocks return (reference getActivation, train_sdxl_zh.py:69-77)."""

    def __init__(self, name: str, tap_index: int, residuals_present: bool):
        self.name, self.tap_index, self.residuals_present = name, tap_index, residuals_present
        self._hooks: List = []

    def register_forward_hook(self, fn):
        self._hooks.append(fn)
        return _HookHandle(self._hooks, fn)


class _DeviceF32:
    """a device fp32 buffer of the library, as `torch.as_tensor` reads it (the buffer stays the library's: clone what is kept)"""

    def __init__(self, address: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": "<f4", "data": (int(address), False),
                                         "strides": None, "version": 2}


class _Config:
    def __init__(self, cfg):
        self.__dict__.update(cfg.__dict__)


class HipUNet(HipTape):
    def __init__(self, cfg, batch: int, height: Optional[int] = None, width: Optional[int] = None, ctx_len: int = 77,
                 needs_grad: bool = False, share_weights_from: Optional["HipUNet"] = None,
                 residual_inputs: bool = False, inpaint_inputs: bool = False):
        self._open()
        self.cfg = cfg
        self.config = _Config(cfg)
        self.in_channels = cfg.in_channels
        self.B, self.H, self.W, self.L = batch, height or cfg.sample_size, width or cfg.sample_size, ctx_len
        self.needs_grad = needs_grad
        self.dtype = torch.bfloat16
        c = _cfg.to_c(cfg)
        self.residual_inputs = residual_inputs
        self.inpaint_inputs = inpaint_inputs
        # PEA_UNET_GRAD | PEA_UNET_RESIDUAL_INPUTS | PEA_UNET_INPAINT_INPUTS
        flags = (1 if needs_grad else 0) | (2 if residual_inputs else 0) | (4 if inpaint_inputs else 0)
        self.time_cond_proj_dim = _cfg.time_cond_dim(cfg) or None
        check(lib().pea_unet_create_cond(ctypes.byref(c), self.B, self.H, self.W, self.L, flags, _cfg.time_cond_dim(cfg),
                                         int(share_weights_from is None), ctypes.byref(self._h)))
        if share_weights_from is not None:
            check(lib().pea_unet_share_weights(self._h, share_weights_from._h))
            self._weights_owner = share_weights_from      # keep alive
        n = len(cfg.block_out_channels)
        self.num_taps = lib().pea_unet_num_taps(self._h)
        nm = ctypes.create_string_buffer(16)
        self.tap_names = []
        for k in range(self.num_taps):
            check(lib().pea_unet_tap_name(self._h, k, nm, 16))
            self.tap_names.append(nm.value.decode())
        idx = {name: k for k, name in enumerate(self.tap_names)}
        self.down_blocks = [_BlockShim(f"d{i}", idx[f"d{i}"], True) for i in range(n)]
        # `mid_block_type: null` configs (SSD-1B) have no mid block: diffusers sets `unet.mid_block = None`
        self.mid_block = _BlockShim("m", idx["m"], False) if "m" in idx else None
        self.up_blocks = [_BlockShim(f"u{i}", idx[f"u{i}"], False) for i in range(n)]

    def release_activations(self):
        """free the activation / gradient arenas (weights stay); the next forward allocates them again"""
        check(lib().pea_unet_release_activations(self._h))
        self._tcond = None             # the context's conditioning input comes back zeroed

    # ---------------------------------------------------------------- LoRA
    _fused: tuple = ()         # keys currently loaded as base + LoRA

    def fuse_lora(self, base_state_dict: Dict[str, torch.Tensor], lora, lora_scale: float = 1.0) -> List[str]:
        """`pipe.load_lora_weights(path); pipe.fuse_lora(lora_scale)` (tests/test_sdxl_zh_lcm.py:181-182).  `lora`: a LoRA
        state dict, a `.safetensors` / `.bin` path (lora.load_lora_state_dict), or a list of `(lora, scale)` pairs that
        accumulate into the same weights (LCM-LoRA plus a style LoRA).  Every touched weight is re-loaded as
        base + sum lora_scale * scale * alpha / rank * up @ down, composed in fp32 on the device from `base_state_dict`
        (the packed bf16 weights cannot be un-rounded) and rounded to bf16 once; weights fused by an earlier call and not
        named now go back to the base.  Contexts sharing these weights see the result.  Returns the fused keys."""
        from .lora import load_lora_state_dict, resolve_lora
        if getattr(self, "_weights_owner", None) is not None:
            raise PeaError("fuse_lora: this context borrows its weights; fuse on the context that owns them")
        table = self.weight_table()
        pairs = lora if isinstance(lora, (list, tuple)) else [(lora, 1.0)]
        per_key: Dict[str, list] = {}
        for item, scale in pairs:
            resolved, _ = resolve_lora(load_lora_state_dict(item), table)
            for k, (down, up, alpha) in resolved.items():
                per_key.setdefault(k, []).append((down, up, float(lora_scale) * float(scale) * alpha / down.shape[0]))
        absent = [k for k in list(per_key) + list(self._fused) if k not in base_state_dict]
        if absent:
            raise PeaError(f"fuse_lora: base_state_dict lacks {absent[:5]}")
        for k in self._fused:
            if k not in per_key:
                t = _staged(self.device, k, table[k], base_state_dict[k])
                check(lib().pea_unet_load_weight(self._h, k.encode(), ptr(t), t.numel(), stream_ptr()))
        for k, ads in per_key.items():
            base = _staged(self.device, k, table[k], base_state_dict[k])
            n = len(ads)
            keep = [(d.to(self.device), u.to(self.device)) for d, u, _ in ads]
            downs = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in keep])
            ups = (ctypes.c_void_p * n)(*[u.data_ptr() for _, u in keep])
            ranks = (ctypes.c_int * n)(*[d.shape[0] for d, _ in keep])
            scales = (ctypes.c_float * n)(*[s for _, _, s in ads])
            check(lib().pea_unet_load_weight_lora(self._h, k.encode(), ptr(base), base.numel(), n, downs, ups, ranks,
                                                  scales, stream_ptr()))
        torch.cuda.current_stream().synchronize()      # staging tensors above are freed after this call
        self._fused = tuple(per_key)
        return list(per_key)

    def unfuse_lora(self, base_state_dict: Dict[str, torch.Tensor]) -> List[str]:
        """`pipe.unfuse_lora()`: re-loads the fused keys from the base -- through the same load as any weight, so the UNet is
        bit-identical to one that never fused.  Returns the keys that were restored."""
        if getattr(self, "_weights_owner", None) is not None:
            raise PeaError("unfuse_lora: this context borrows its weights")
        table = self.weight_table()
        absent = [k for k in self._fused if k not in base_state_dict]
        if absent:
            raise PeaError(f"unfuse_lora: base_state_dict lacks {absent[:5]}")
        for k in self._fused:
            t = _staged(self.device, k, table[k], base_state_dict[k])
            check(lib().pea_unet_load_weight(self._h, k.encode(), ptr(t), t.numel(), stream_ptr()))
        torch.cuda.current_stream().synchronize()
        restored, self._fused = list(self._fused), ()
        return restored

    # ---------------------------------------------------------------- forward
    def __call__(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, cross_attention_kwargs=None,
                 return_dict=False, down_block_additional_residuals=None, mid_block_additional_residual=None,
                 timestep_cond=None):
        """`timestep_cond` [B, time_cond_proj_dim]: the guidance-scale embedding of a guidance-embedded UNet
        (`sampler.guidance_scale_embedding`); None, as in diffusers, leaves the projection out of this call."""
        self._route_timestep_cond(timestep_cond)
        if down_block_additional_residuals is not None or mid_block_additional_residual is not None:
            self.set_additional_residuals(down_block_additional_residuals, mid_block_additional_residual)
        elif self.residual_inputs and self._residuals_set:
            self.set_additional_residuals(None, None)        # a call without the kwargs is a plain UNet call
        B = self.B
        self._route_inpaint(sample)
        x = sample.detach().to(self.device, torch.float32).contiguous()
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep])
        t = t.to(self.device, torch.float32).reshape(-1).expand(B).contiguous()
        ehs = encoder_hidden_states.detach().to(self.device)
        if tuple(ehs.shape) != (self.B, self.L, self.cfg.cross_attention_dim):
            raise PeaError(f"encoder_hidden_states {tuple(ehs.shape)} != {(self.B, self.L, self.cfg.cross_attention_dim)}")
        e_dt = 1 if ehs.dtype == torch.bfloat16 else 0
        ehs = ehs.contiguous() if e_dt else ehs.float().contiguous()
        text = tid = None
        t_dt = 0
        if self.cfg.addition_embed_type == "text_time":
            text = added_cond_kwargs["text_embeds"].detach().to(self.device)
            t_dt = 1 if text.dtype == torch.bfloat16 else 0
            text = text.contiguous() if t_dt else text.float().contiguous()
            tid = added_cond_kwargs["time_ids"].detach().to(self.device, torch.float32).contiguous()
        eps = torch.empty(self.B, self.cfg.out_channels, self.H, self.W, device=self.device, dtype=torch.float32)
        check(lib().pea_unet_forward(self._h, ptr(x), ptr(t), ptr(ehs), e_dt, ptr(text), t_dt, ptr(tid), ptr(eps),
                                     stream_ptr()))
        self._keep = (x, t, ehs, text, tid)
        for blk in list(self.down_blocks) + [self.mid_block] + list(self.up_blocks):
            if blk._hooks:
                tap = self.tap(blk.tap_index)
                out = (tap, ()) if blk.residuals_present else tap
                for fn in list(blk._hooks):
                    fn(blk, (), out)
        out = eps.to(sample.dtype) if sample.dtype in (torch.float16, torch.bfloat16) else eps
        return (out,)

    # ---------------------------------------------------------------- guidance embedding
    _tcond = None          # the conditioning last handed to the context (kept alive while the cast may still be queued)

    def _route_timestep_cond(self, timestep_cond):
        if timestep_cond is None:
            if self._tcond is not None:
                check(lib().pea_unet_set_timestep_cond(self._h, None, stream_ptr()))
                self._tcond = None
            return
        if self.time_cond_proj_dim is None:
            raise PeaError("timestep_cond given, but this UNet's config has no time_cond_proj_dim")
        if tuple(timestep_cond.shape) != (self.B, self.time_cond_proj_dim):
            raise PeaError(f"timestep_cond {tuple(timestep_cond.shape)} != {(self.B, self.time_cond_proj_dim)}")
        c = timestep_cond.detach().to(self.device, torch.float32).contiguous()
        check(lib().pea_unet_set_timestep_cond(self._h, ptr(c), stream_ptr()))
        self._tcond = c

    # ---------------------------------------------------------------- FreeU
    freeu = None           # (s1, s2, b1, b2) while the switch is on

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' `pipe.enable_freeu(s1, s2, b1, b2)` (0.23; training-free, no weights): in front of every skip concatenation
        of `up_blocks[0]` (s1, b1) and `up_blocks[1]` (s2, b2) the first half of the hidden channels is multiplied by b and the
        skip tensor's four lowest frequencies by s (`fourier_filter`, threshold 1), inside the concat's own launch plus one
        reduction.  A switch of THIS context (one sharing its weights carries its own); every later call runs with it until
        `disable_freeu()`; calling again replaces the factors.  Inference contexts only."""
        check(lib().pea_unet_set_freeu(self._h, float(s1), float(s2), float(b1), float(b2), stream_ptr()))
        self.freeu = (float(s1), float(s2), float(b1), float(b2))

    def disable_freeu(self):
        """diffusers' `pipe.disable_freeu()`: the plain concat launches again, bit for bit"""
        check(lib().pea_unet_clear_freeu(self._h))
        self.freeu = None

    # ---------------------------------------------------------------- inpainting condition
    _inp = None            # (mask, masked_latents) fp32 on the device, as last handed to the context
    _inp_lat_b = 0
    _inp_live = False      # the context currently gathers (a plain 9-channel call clears it until the next latents-only call)

    def set_inpaint_cond(self, mask, masked_latents, latent_batch: Optional[int] = None):
        """The per-generation inputs of the inpainting UNet (tests/test_sdxl_zh_inpaint.py: `mask`, `masked_image_latents` of
        the per-step `torch.cat([latent_model_input, mask, masked_image_latents], dim=1)`), copied into the context once.
        mask [cb,1,H,W], masked_latents [cb,C,H,W] (C = out_channels), cb dividing the UNet batch (with CFG: the images
        WITHOUT the CFG doubling, cb = B/2).  Afterwards `__call__` also takes the latents alone, [lb,C,H,W] with lb dividing B
        (default latent_batch: cb); image b reads latents[b % lb] and mask / masked_latents[b % cb]."""
        if not self.inpaint_inputs:
            raise PeaError("HipUNet was created without inpaint_inputs=True")
        C = self.cfg.out_channels
        cb = mask.shape[0]
        if tuple(mask.shape) != (cb, 1, self.H, self.W) or tuple(masked_latents.shape) != (cb, C, self.H, self.W):
            raise PeaError(f"set_inpaint_cond: mask {tuple(mask.shape)} / masked_latents {tuple(masked_latents.shape)}, expected "
                           f"[cb,1,{self.H},{self.W}] / [cb,{C},{self.H},{self.W}]")
        m = mask.detach().to(self.device, torch.float32).contiguous()
        ml = masked_latents.detach().to(self.device, torch.float32).contiguous()
        lb = cb if latent_batch is None else int(latent_batch)
        check(lib().pea_unet_set_inpaint_cond(self._h, ptr(m), ptr(ml), cb, lb, stream_ptr()))
        self._inp, self._inp_lat_b, self._inp_live = (m, ml), lb, True

    def clear_inpaint_cond(self):
        """back to the plain call: `sample` is the full [B, in_channels, H, W] input again"""
        check(lib().pea_unet_clear_inpaint_cond(self._h))
        self._inp, self._inp_lat_b, self._inp_live = None, 0, False

    def _route_inpaint(self, sample):
        shp = tuple(sample.shape)
        if shp == (self.B, self.in_channels, self.H, self.W):
            if self._inp_live:              # the reference's own concatenated input: the plain conv_in reads it
                check(lib().pea_unet_clear_inpaint_cond(self._h))
                self._inp_live = False
            return
        C = self.cfg.out_channels
        if self._inp is not None and len(shp) == 4 and shp[1:] == (C, self.H, self.W) and shp[0] > 0 and self.B % shp[0] == 0:
            if not self._inp_live or shp[0] != self._inp_lat_b:
                check(lib().pea_unet_set_inpaint_cond(self._h, ptr(self._inp[0]), ptr(self._inp[1]), self._inp[0].shape[0],
                                                      shp[0], stream_ptr()))
                self._inp_lat_b, self._inp_live = shp[0], True
            return
        want = f"{(self.B, self.in_channels, self.H, self.W)}"
        if self._inp is not None:
            want += f" or latents [lb, {C}, {self.H}, {self.W}] with lb dividing {self.B}"
        raise PeaError(f"HipUNet built for {want}, got {shp}")

    # ---------------------------------------------------------------- image prompts (IP-Adapter)
    _ip = None             # the loaded ip_adapter.IPAdapter / IPAdapterPlus, or the list of them (the list form)
    _ips = ()              # ... always as a sequence, one entry per set of the context
    _ip_tokens = None      # the tokens last handed to the context (kept alive while the cast may still be queued)

    def load_ip_adapter(self, adapter_or_sd):
        """Give every cross-attention layer the `to_k_ip` / `to_v_ip` projections of an IP-Adapter (an `ip_adapter.IPAdapter` or
        `IPAdapterPlus`, or the state dict or file path of a base adapter), or of up to four of them: a list, one entry per
        adapter, base and plus files mixed as needed, with at most 32 image tokens together (4 + 16, 16 + 16, 4 + 4 + 16).  The
        UNet's own weights -- `weight_table()`, `load_state_dict` -- do not change, and neither does any launch until
        `set_ip_tokens`.  Returns the adapter (its `.tokens()` is the image projection), or the list of them."""
        from .ip_adapter import IPAdapter, _LayerMap
        many = isinstance(adapter_or_sd, (list, tuple))
        ads = [a if isinstance(a, _LayerMap) else IPAdapter(a, self.cfg) for a in (adapter_or_sd if many else [adapter_or_sd])]
        for ad in ads:
            if ad.cfg.cross_attention_dim != self.cfg.cross_attention_dim:
                raise PeaError(f"load_ip_adapter: adapter built for cross_attention_dim {ad.cfg.cross_attention_dim}, UNet has "
                               f"{self.cfg.cross_attention_dim}")
        if many:
            n = (ctypes.c_int * max(len(ads), 1))(*[ad.n_tokens for ad in ads])
            check(lib().pea_unet_ip_create_sets(self._h, len(ads), n))
        else:
            check(lib().pea_unet_ip_create(self._h, ads[0].n_tokens))
        try:
            for j, ad in enumerate(ads):
                for k, t in ad.layers.items():
                    t = t.to(self.device, torch.float32).contiguous()
                    if many:
                        check(lib().pea_unet_ip_load_weight_set(self._h, j, k.encode(), ptr(t), t.numel(), stream_ptr()))
                    else:
                        check(lib().pea_unet_ip_load_weight(self._h, k.encode(), ptr(t), t.numel(), stream_ptr()))
            torch.cuda.current_stream().synchronize()      # staging tensors above are freed after this call
        except PeaError:
            self.unload_ip_adapter()
            raise
        self._ips, self._ip_tokens = list(ads), [None] * len(ads)
        self._ip = list(ads) if many else ads[0]
        return self._ip

    def _per_adapter(self, what, value):
        """`value` as one entry per loaded adapter: a list is taken as it is, anything else is the entry of every adapter"""
        if not self._ips:
            raise PeaError(f"{what}: call load_ip_adapter first")
        if isinstance(value, (list, tuple)):
            if len(value) != len(self._ips):
                raise PeaError(f"{what}: {len(value)} entries for {len(self._ips)} adapters")
            return list(value)
        return [value] * len(self._ips)

    def set_ip_tokens(self, tokens):
        """tokens [B, N, cross_dim] (`IPAdapter.tokens(image_embeds, do_cfg=...)`, or `IPAdapterPlus.tokens / encode`):
        projected to every layer's image keys / values once; every call reads them until `clear_ip_tokens()`.  With several
        adapters: a list with one such tensor per adapter; `None` leaves that adapter's tokens as they are."""
        if not self._ips:
            raise PeaError("set_ip_tokens: call load_ip_adapter first")
        if not isinstance(tokens, (list, tuple)):
            if len(self._ips) != 1:
                raise PeaError(f"set_ip_tokens: one tensor for {len(self._ips)} adapters; pass a list with one entry per adapter")
            tokens = [tokens]
        for j, (ad, tok) in enumerate(zip(self._ips, self._per_adapter("set_ip_tokens", list(tokens)))):
            if tok is None:
                continue
            want = (self.B, ad.n_tokens, self.cfg.cross_attention_dim)
            if tuple(tok.shape) != want:
                raise PeaError(f"set_ip_tokens: tokens {tuple(tok.shape)} != {want}" + (f" (adapter {j})" if len(self._ips) > 1 else ""))
            t = tok.detach().to(self.device, torch.float32).contiguous()
            if len(self._ips) == 1:
                check(lib().pea_unet_ip_set_tokens(self._h, ptr(t), stream_ptr()))
            else:
                check(lib().pea_unet_ip_set_tokens_set(self._h, j, ptr(t), stream_ptr()))
            self._ip_tokens[j] = t

    def set_ip_adapter_scale(self, scale):
        """the weight of the image branch (default 1; 0 runs the plain attention).  A number, or a dict of per-block scales
        (`ip_adapter.resolve_layer_scales`: keys `down` / `up` / `mid`, `up_blocks.0`, `up_blocks.0.attentions.1`, ..., `default`;
        layers a dict does not name get 0), or a list with one such entry per adapter.  One entry for several adapters goes to
        each of them."""
        from .ip_adapter import resolve_layer_scales
        for j, sc in enumerate(self._per_adapter("set_ip_adapter_scale", scale)):
            if isinstance(sc, dict):
                vec = resolve_layer_scales(self.cfg, sc)
                arr = (ctypes.c_float * len(vec))(*vec)
                check(lib().pea_unet_ip_set_layer_scales(self._h, j, arr, len(vec)))
                check(lib().pea_unet_ip_set_scale_set(self._h, j, 1.0))
            else:
                check(lib().pea_unet_ip_set_layer_scales(self._h, j, None, 0))
                check(lib().pea_unet_ip_set_scale_set(self._h, j, float(sc)))

    def ip_query_counts(self):
        """the distinct query counts of this context's cross-attention layers (host only), e.g. [4096, 1024] for SDXL at 1024^2"""
        n = ctypes.c_int()
        check(lib().pea_unet_ip_query_counts(self._h, None, 0, ctypes.byref(n)))
        out = (ctypes.c_int * max(n.value, 1))()
        check(lib().pea_unet_ip_query_counts(self._h, out, n.value, ctypes.byref(n)))
        return list(out[:n.value])

    def _grid_of(self, count: int):
        """(h, w) of the layers with `count` queries: the latent grid halved (n -> ceil(n / 2), a stride-2 convolution)"""
        h, w = self.H, self.W
        while h * w > count and (h > 1 or w > 1):
            h, w = (h + 1) // 2, (w + 1) // 2
        if h * w != count:
            raise PeaError(f"no level of a {self.H} x {self.W} latent has {count} positions")
        return h, w

    def set_ip_adapter_masks(self, masks):
        """Confine adapters to regions of the picture: a list with, per adapter, `None` (everywhere) or a mask `[h, w]` /
        `[1|B, h, w]` at any resolution, 1 inside the region.  Every cross-attention layer multiplies that adapter's output by the
        mask reduced to its own grid with `ip_adapter.downsample_mask` (bicubic, the values are used as they come out)."""
        from .ip_adapter import downsample_mask
        counts = None
        for j, m in enumerate(self._per_adapter("set_ip_adapter_masks", list(masks) if isinstance(masks, (list, tuple)) else masks)):
            if m is None:
                check(lib().pea_unet_ip_set_mask(self._h, j, 0, None, 0, stream_ptr()))
                continue
            m = torch.as_tensor(m)
            m = m[None] if m.dim() == 2 else m
            if m.dim() != 3 or m.shape[0] not in (1, self.B):
                raise PeaError(f"set_ip_adapter_masks: mask {tuple(m.shape)} of adapter {j}, expected [h, w] or [1|{self.B}, h, w]")
            counts = self.ip_query_counts() if counts is None else counts
            for c in counts:
                d = downsample_mask(m.to(self.device), *self._grid_of(c))
                check(lib().pea_unet_ip_set_mask(self._h, j, c, ptr(d), d.shape[0], stream_ptr()))
            torch.cuda.current_stream().synchronize()      # the library copies on the stream; `d` is freed after this call

    def set_prompt_regions(self, masks, weights=None, do_cfg=False):
        """Regional text prompts: the context of this UNet holds R prompts of L / R tokens (`regional.compose_prompt_embeds`), and
        `masks` says where each of them applies: a list with, per prompt, `None` (everywhere) or a mask `[h, w]` / `[1|B, h, w]` at
        any resolution, values >= 0.  Every cross-attention layer then runs R softmaxes in one launch and mixes their outputs with
        `regional.region_weights(masks, weights, h_l, w_l)` of its own grid (area means, normalised per position; uncovered
        positions go to prompt 0).  `weights`: one factor per prompt (default 1).  do_cfg: the first half of the batch (the
        unconditional half) attends to prompt 0 alone.  Holds until `clear_prompt_regions()`."""
        from .regional import region_weights
        masks = list(masks)
        R = len(masks)
        self.clear_prompt_regions()
        try:
            for c in self.ip_query_counts():
                w = region_weights(masks, weights, *self._grid_of(c), device=self.device)         # [Bm, R, c]
                if w.shape[0] not in (1, self.B):
                    raise PeaError(f"set_prompt_regions: masks with batch {w.shape[0]}, expected 1 or {self.B}")
                if do_cfg:
                    if self.B % 2:
                        raise PeaError(f"set_prompt_regions: do_cfg needs an even batch (B={self.B})")
                    w = w.expand(self.B, -1, -1).clone()
                    w[: self.B // 2] = 0.0
                    w[: self.B // 2, 0] = 1.0
                w = w.contiguous()
                check(lib().pea_unet_set_prompt_regions(self._h, R, c, ptr(w), w.shape[0], stream_ptr()))
            torch.cuda.current_stream().synchronize()          # the library copies on the stream; `w` is freed after this call
        except Exception:
            self.clear_prompt_regions()
            raise

    def clear_prompt_regions(self):
        """back to one softmax over the whole context"""
        check(lib().pea_unet_clear_prompt_regions(self._h))

    def enable_attention_maps(self, layers=None):
        """Cross-attention heat maps (DAAM): from now on every selected cross-attention layer adds its head-mean softmax
        probabilities to an fp32 accumulator [B, L, h_l * w_l] of its latent grid, in one extra launch per layer; the forward's own
        results do not change.  layers: None (every cross-attention layer) or a spec in the vocabulary of
        `ip_adapter.resolve_layer_scales` (`{"up": 1.0}`, `{"down_blocks.2": 1.0, "mid": 1.0}`, ...; non-zero = capture).  Enable
        before a denoising loop and read `attention_maps()` / `attention_maps.heat_maps(unet)` after it: the sums then run over
        layers and steps.  Accumulators start at zero; `reset_attention_maps()` zeroes them again."""
        if layers is None:
            check(lib().pea_unet_enable_attention_maps(self._h, None, 0))
            return
        from .ip_adapter import resolve_layer_scales
        vec = resolve_layer_scales(self.cfg, layers)
        arr = (ctypes.c_float * len(vec))(*vec)
        check(lib().pea_unet_enable_attention_maps(self._h, arr, len(vec)))

    def disable_attention_maps(self):
        """stop capturing and free the accumulators"""
        check(lib().pea_unet_disable_attention_maps(self._h))

    def reset_attention_maps(self):
        """zero the accumulators and their counters (on the current stream)"""
        check(lib().pea_unet_reset_attention_maps(self._h, stream_ptr()))

    def attention_maps(self):
        """-> {(h_l, w_l): (fp32 tensor [B, L, h_l, w_l], n_accumulated)}: per latent grid the sum of the head-mean cross-attention
        probabilities over every layer-forward since the last reset, and how many layer-forwards that is (a host counter).  The
        tensors are copies made on the current stream."""
        out = {}
        for c in self.ip_query_counts():
            p, n = ctypes.c_void_p(), ctypes.c_longlong()
            check(lib().pea_unet_attention_maps(self._h, c, ctypes.byref(p), ctypes.byref(n)))
            h, w = self._grid_of(c)
            t = torch.as_tensor(_DeviceF32(p.value, (self.B, self.L, h, w)), device=self.device).clone()
            out[(h, w)] = (t, int(n.value))
        return out

    def set_prompt_edit(self, edit, do_cfg=False):
        """Prompt-to-prompt editing (`prompt2prompt.PromptEdit`): the batch of this UNet holds N prompts denoised from the same
        latents, and sample b with edit.src[b] >= 0 takes its cross-attention probabilities partly from that source (word swap,
        refinement, re-weighting) and, in the first steps, its self-attention probabilities in the layers with at most
        edit.self_max_tokens queries.  do_cfg: the batch is [uncond x N | cond x N]; the tables of an edit composed without it are
        laid out for it here.  The step is set with `set_prompt_edit_step`; holds until `clear_prompt_edit()`."""
        if do_cfg:
            edit = edit.with_cfg()
        B, L = self.B, edit.Mt.shape[-1]
        if L != self.L:                                        # the library copies B * L * L and T * 2 * B * L elements by ITS L
            raise PeaError(f"set_prompt_edit: tables for a context of {L} rows, this UNet has {self.L} (compose the edit with "
                           f"L = ctx_len, not the number of tokens)")
        if edit.src.numel() != B or tuple(edit.Mt.shape) != (B, L, L) or tuple(edit.cd.shape[1:]) != (2, B, L):
            raise PeaError(f"set_prompt_edit: tables for a batch of {edit.src.numel()} (Mt {tuple(edit.Mt.shape)}, cd "
                           f"{tuple(edit.cd.shape)}), this UNet has batch {B}")
        src = (ctypes.c_int * B)(*[int(x) for x in edit.src.tolist()])
        Mt = edit.Mt.to(device=self.device, dtype=torch.bfloat16).contiguous()
        cd = edit.cd.to(device=self.device, dtype=torch.float32).contiguous()
        check(lib().pea_unet_set_prompt_edit(self._h, src, ptr(Mt), ptr(cd), int(edit.cd.shape[0]), int(edit.self_until),
                                             int(edit.self_max_tokens), stream_ptr()))

    def set_prompt_edit_step(self, i):
        """the denoising step the next forward belongs to (a host integer: nothing is transferred)"""
        check(lib().pea_unet_set_prompt_edit_step(self._h, int(i)))

    def clear_prompt_edit(self):
        """back to plain attention; a forward then gives the bits it gave before"""
        check(lib().pea_unet_clear_prompt_edit(self._h))

    def set_style_aligned(self, ref=None, layers=None, adain_queries=True, adain_keys=True, shared_score_scale=1.0,
                          shared_score_shift=0.0, do_cfg=False):
        """StyleAligned generation (Hertz et al. 2023): the batch of this UNet holds N prompts denoised together, and in the
        self-attention layers every target sample moves its queries and keys onto its reference's per-channel statistics (AdaIN)
        and attends to the reference's keys and values as well as its own, under one softmax.  ref: None (sample 0 is the
        reference of all others; with do_cfg the batch is [uncond x n | cond x n] and each half has its own, see
        `style_aligned.reference_index`) or B ints, ref[b] >= 0 the reference of b, negative = plain.  layers: None (every
        self-attention layer), a fraction 0..1 of them (`style_aligned.level_switches`), or names / prefixes of
        `style_aligned.layer_names(self)`.  Reference logits are shared_score_scale * logit + shared_score_shift.  Holds until
        `clear_style_aligned()`; `sampler.denoise` over the batch is the generation loop."""
        from . import style_aligned as sa
        if ref is None:
            if do_cfg and self.B % 2:
                raise PeaError(f"set_style_aligned: do_cfg needs an even batch (B={self.B})")
            ref = sa.reference_index(self.B // 2 if do_cfg else self.B, do_cfg)
        ref = [int(x) for x in (ref.tolist() if hasattr(ref, "tolist") else ref)]
        if len(ref) != self.B:
            raise PeaError(f"set_style_aligned: {len(ref)} references for a batch of {self.B}")
        href = (ctypes.c_int * self.B)(*ref)
        arr, n = None, 0
        if layers is not None:
            vec = sa.resolve_layers(self, layers)
            arr, n = (ctypes.c_float * len(vec))(*vec), len(vec)
        check(lib().pea_unet_set_style_aligned(self._h, href, arr, n, int(bool(adain_queries)), int(bool(adain_keys)),
                                               float(shared_score_scale), float(shared_score_shift), stream_ptr()))

    def clear_style_aligned(self):
        """back to plain self-attention; a forward then gives the bits it gave before"""
        check(lib().pea_unet_clear_style_aligned(self._h))

    def set_attention_perturbation(self, mode, layers=None, samples=None, blur_sigma=float("inf")):
        """Perturbed-attention guidance (mode "pag"; Ahn et al. 2024) or smoothed-energy guidance (mode "seg"; Hong 2024) in one
        UNet call (`pag.denoise_perturbed` is the loop): the last `samples` samples of the batch are the perturbed ones, and in
        the chosen self-attention layers their attention is the identity, O = V ("pag"), or runs on queries blurred over the
        token grid with a Gaussian of `blur_sigma` ("seg"; above 9999: the mean over the grid).  layers: as
        `set_style_aligned`'s names / prefixes / fraction; None = the mid block.  samples: how many; None = the last third of a
        batch that divides by 3.  Every other sample keeps its bits.  Holds until `clear_attention_perturbation()`."""
        import numpy as np
        from . import pag
        from . import style_aligned as sa
        modes = {"pag": 1, "seg": 2}
        if mode not in modes:
            raise PeaError(f"set_attention_perturbation: mode {mode!r} ('pag' or 'seg')")
        if samples is None:
            if self.B % 3:
                raise PeaError(f"set_attention_perturbation: a batch of {self.B} is no [uncond | cond | perturbed]; say how many "
                               "samples at its end are perturbed")
            samples = self.B // 3
        names = sa.layer_names(self)
        if layers is None and not any(n.startswith("mid_block.") for n in names):
            raise PeaError("set_attention_perturbation: this UNet has no mid-block attention; name the layers "
                           "(style_aligned.layer_names)")
        vec = sa.resolve_layers(self, ["mid_block"] if layers is None else layers)
        arr = (ctypes.c_float * len(vec))(*vec)
        grids, tables = [], []
        if mode == "seg":
            top = len(self.cfg.down_block_types) - 1
            for name, on in zip(names, vec):
                block, idx = name.split(".")[0], name.split(".")[1]
                level = int(idx) if block == "down_blocks" else top if block == "mid_block" else top - int(idx)
                h, w = self.H, self.W
                for _ in range(level):
                    h, w = (h + 1) // 2, (w + 1) // 2
                if on and (h, w) not in grids:
                    grids.append((h, w))
                    tables += [pag.blur_matrix(h, blur_sigma).reshape(-1), pag.blur_matrix(w, blur_sigma).reshape(-1)]
        gh = (ctypes.c_int * max(len(grids), 1))(*[g[0] for g in grids])
        gw = (ctypes.c_int * max(len(grids), 1))(*[g[1] for g in grids])
        flat = np.ascontiguousarray(np.concatenate(tables) if tables else np.zeros(1), dtype=np.float32)
        check(lib().pea_unet_set_attn_perturb(self._h, modes[mode], self.B - int(samples), arr, len(vec), len(grids), gh, gw,
                                              ctypes.c_void_p(flat.ctypes.data), stream_ptr()))

    def clear_attention_perturbation(self):
        """back to plain self-attention; a forward then gives the bits it gave before"""
        check(lib().pea_unet_clear_attn_perturb(self._h))

    def enable_sag(self, layer=None, samples=None):
        """Self-attention guidance capture (Hong et al. 2023; `sag.denoise_sag` is the loop): while enabled, one self-attention
        layer's launch also stores its lse and is followed by one column-sum launch, `sag_colsum()`.  layer: an index or a name
        of `style_aligned.layer_names(self)`; None = the mid block's first transformer block (a UNet without mid-block attention
        needs an index).  samples: (first, count) of the batch to capture; None = all (under CFG `(0, B // 2)` is the
        unconditional half).  A forward's output does not change.  Holds until `disable_sag()`."""
        from . import style_aligned as sa
        names = sa.layer_names(self)
        if layer is None:
            mid = [i for i, n in enumerate(names) if n.startswith("mid_block.")]
            if not mid:
                raise PeaError("enable_sag: this UNet has no mid-block attention; name a self-attention layer by index "
                               f"(0..{len(names) - 1}, style_aligned.layer_names)")
            layer = mid[0]
        elif isinstance(layer, str):
            if layer not in names:
                raise PeaError(f"enable_sag: '{layer}' names no self-attention layer of this UNet")
            layer = names.index(layer)
        first, count = (0, self.B) if samples is None else (int(samples[0]), int(samples[1]))
        check(lib().pea_unet_enable_sag(self._h, int(layer), first, count))
        self._sag = (int(layer), first, count)

    def disable_sag(self):
        """stop capturing and free the buffers; a forward then gives the bits it gave before"""
        check(lib().pea_unet_disable_sag(self._h))
        self._sag = None

    def sag_colsum(self):
        """-> fp32 [n_samples, G, S]: the partial column sums of the captured layer's last forward (`part.sum(1)` in ascending g
        is the mass every key received); a copy made on the current stream"""
        p, G, S = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        check(lib().pea_unet_sag_colsum(self._h, ctypes.byref(p), ctypes.byref(G), ctypes.byref(S)))
        n = self._sag[2]
        return torch.as_tensor(_DeviceF32(p.value, (n, G.value, S.value)), device=self.device).clone()

    def clear_ip_tokens(self, index=None):
        """back to plain cross-attention launches (index: for that adapter alone); the adapters' weights stay loaded"""
        if index is None:
            check(lib().pea_unet_ip_clear(self._h))
            self._ip_tokens = [None] * len(self._ips)
        else:
            check(lib().pea_unet_ip_clear_set(self._h, int(index)))
            self._ip_tokens[index] = None

    def unload_ip_adapter(self, index=None):
        """drop every adapter, or (index) that one: the others are loaded again into a new state, WITHOUT their tokens, scales
        and masks -- set them again"""
        rest = [] if index is None else [ad for j, ad in enumerate(self._ips) if j != int(index)]
        if index is not None and not 0 <= int(index) < len(self._ips):
            raise PeaError(f"unload_ip_adapter: adapter {index} of {len(self._ips)}")
        check(lib().pea_unet_ip_destroy(self._h))
        self._ip, self._ips, self._ip_tokens = None, (), None
        if rest:
            self.load_ip_adapter(rest)

    def ip_kv(self):
        """parity instrumentation: the packed image K|V of every layer, fp32 [B * N, cols] with N the image tokens of all adapters
        together, adapter j in rows off_j .. off_j + N_j of every sample (columns: pea_unet_stacked_layout(which=0))"""
        rows, cols = ctypes.c_longlong(), ctypes.c_int()
        check(lib().pea_unet_ip_export_kv(self._h, None, ctypes.byref(rows), ctypes.byref(cols), None))
        out = torch.empty(rows.value, cols.value, device=self.device, dtype=torch.float32)
        check(lib().pea_unet_ip_export_kv(self._h, ptr(out), None, None, stream_ptr()))
        return out

    # ---------------------------------------------------------------- ControlNet residual inputs
    _residuals_set = False

    def residual_shapes(self):
        """[(C, H, W)] of `down_block_additional_residuals` followed by `mid_block_additional_residual` (last)."""
        n = lib().pea_unet_num_residuals(self._h)
        out = []
        for i in range(n):
            c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            check(lib().pea_unet_residual_info(self._h, i, ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)))
            out.append((c.value, h.value, w.value))
        return out

    def set_additional_residuals(self, down, mid, scale: float = 1.0):
        """`down_block_additional_residuals=..., mid_block_additional_residual=...` of the UNet call
        (tests/test_sdxl_zh_controlnet.py:534-535): NCHW tensors as a torch ControlNet returns them."""
        if not self.residual_inputs:
            raise PeaError("HipUNet was created without residual_inputs=True")
        shapes = self.residual_shapes()
        items = (list(down) if down is not None else [None] * (len(shapes) - 1)) + [mid]
        if len(items) != len(shapes):
            raise PeaError(f"{len(items) - 1} down residuals given, the UNet has {len(shapes) - 1}")
        keep, ptrs = [], (ctypes.c_void_p * len(items))()
        dts = {t.dtype for t in items if t is not None}
        dt = torch.bfloat16 if dts == {torch.bfloat16} else torch.float32
        for i, (t, (C, H, W)) in enumerate(zip(items, shapes)):
            if t is None:
                ptrs[i] = None
                continue
            if tuple(t.shape) != (self.B, C, H, W):
                raise PeaError(f"residual {i}: {tuple(t.shape)} != {(self.B, C, H, W)}")
            t = t.detach().to(self.device, dt).contiguous()
            keep.append(t)
            ptrs[i] = t.data_ptr()
        check(lib().pea_unet_set_residuals(self._h, len(items), ptrs, 1 if dt == torch.bfloat16 else 0, float(scale),
                                           stream_ptr()))
        self._keep_res = keep
        self._residuals_set = any(t is not None for t in items)

    def clear_residuals(self):
        self.set_additional_residuals(None, None)

    def tap(self, k: int, grad: bool = False) -> torch.Tensor:
        """feature tap k (cast_hook order) as an NCHW fp32 tensor"""
        B, H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().pea_unet_tap_info(self._h, k, None, None, ctypes.byref(B), ctypes.byref(H), ctypes.byref(W),
                                      ctypes.byref(C)))
        out = torch.empty(B.value, C.value, H.value, W.value, device=self.device, dtype=torch.float32)
        check(lib().pea_unet_tap_export_nchw(self._h, k, int(grad), ptr(out), stream_ptr()))
        return out

    def set_tap_grad(self, k: int, seed: torch.Tensor):
        """write a gradient seed (NCHW, the tap's shape) into tap k's gradient buffer in its storage layout; pass bit k in
        `backward(..., tap_seed_mask)` afterwards"""
        s = seed.detach().to(self.device, torch.float32).contiguous()
        check(lib().pea_unet_tap_import_grad_nchw(self._h, k, ptr(s), stream_ptr()))

    def tap_layout(self, k: int) -> int:
        """0 = NHWC, 1 = depth-to-space (include/pea_hip.h: pea_unet_tap_layout)"""
        return int(lib().pea_unet_tap_layout(self._h, k))

    def tap_pointers(self, k: int):
        """-> (data ptr, grad ptr, (B, H, W, C), layout); layout as `tap_layout` -- the pointers of a depth-to-space tap are
        only handed out once the layout has been asked for (pea_unet_tap_info)"""
        layout = self.tap_layout(k)
        d, g = ctypes.c_void_p(), ctypes.c_void_p()
        B, H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib().pea_unet_tap_info(self._h, k, ctypes.byref(d), ctypes.byref(g), ctypes.byref(B), ctypes.byref(H),
                                      ctypes.byref(W), ctypes.byref(C)))
        return d.value, g.value, (B.value, H.value, W.value, C.value), layout

    # ---------------------------------------------------------------- backward (data gradients only)
    def backward(self, d_eps: Optional[torch.Tensor], tap_seed_mask: int = 0):
        """-> (d_encoder_hidden_states [B,L,cross] fp32, d_text_embeds [B,pooled] fp32 or None)"""
        de = d_eps.detach().to(self.device, torch.float32).contiguous() if d_eps is not None else None
        check(lib().pea_unet_backward(self._h, ptr(de), tap_seed_mask, stream_ptr()))
        pe, pt = ctypes.c_void_p(), ctypes.c_void_p()
        check(lib().pea_unet_input_grads(self._h, ctypes.byref(pe), ctypes.byref(pt)))
        d_ehs = d_text = None
        if pe.value:
            d_ehs = torch.empty(self.B, self.L, self.cfg.cross_attention_dim, device=self.device)
            check(lib().pea_op_cast_bf16_f32(pe, ptr(d_ehs), d_ehs.numel(), stream_ptr()))
        if pt.value:
            d_text = torch.empty(self.B, self.cfg.pooled_dim, device=self.device)
            check(lib().pea_op_cast_bf16_f32(pt, ptr(d_text), d_text.numel(), stream_ptr()))
        return d_ehs, d_text
