"""`HipImageEncoder`: the CLIP vision towers (HF `CLIPVisionModelWithProjection` state-dict keys) on the HIP op tape, with the
image preprocessing in front of them and the CLIPScore behind them -- what turns `HipVAEDecoder`'s pixels into "is this
checkpoint's image closer to its prompt than the last one's?" without leaving the device.  ViT-B/32, ViT-L/14 (head_dim 64)
and ViT-H/14 (head_dim 80: the image tower of Chinese-CLIP ViT-H/14 and of xlm-roberta-large-ViT-H-14, the pairs the student
text towers belong to).

    enc = HipImageEncoder(config.clip_vit_h14_config(), batch=8); enc.load_state_dict(clip_state_dict, strict=False)
    scores = clip_score_images(enc, vae.decode(latents), text_embeds)        # device [8], no host sync

`preprocess` resamples with the definition of `torch.nn.functional.interpolate(mode="bicubic", antialias=True)`; the
per-coordinate tap tables are built here on the host in float64 (`resample_taps`) and cached on the device per input shape."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import config as _cfg
from . import ops as _ops
from ._lib import PeaError, check, lib, ptr, stream_ptr
from .tape import HipTape


# ---------------------------------------------------------------- resampling tables (host, float64)
@dataclass
class AxisTaps:
    """output coordinate i = sum_k weights[i, k] * source[first[i] + k], k < count[i] (weights past count[i] are zero)"""
    first: np.ndarray      # int32 [n]
    count: np.ndarray      # int32 [n]
    weights: np.ndarray    # float64 [n, taps]
    in_size: int

    def dense(self) -> np.ndarray:
        """the same map as a float64 [n, in_size] matrix"""
        m = np.zeros((len(self.first), self.in_size))
        for i, (f, c) in enumerate(zip(self.first, self.count)):
            m[i, f:f + c] = self.weights[i, :c]
        return m


def _keys(x: float, a: float = -0.5) -> float:
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def axis_taps(in_size: int, out_size: int, lo: int = 0, n: int = None) -> AxisTaps:
    """taps of output coordinates lo .. lo + n - 1 of an antialiased bicubic resize in_size -> out_size (align_corners=False):
    Keys kernel a = -0.5 stretched by max(scale, 1), support 2 max(scale, 1), weights normalised to sum 1; exact zeros at
    either end of a window are dropped (the identity resize is a single tap of weight 1)"""
    n = out_size - lo if n is None else n
    scale = in_size / out_size
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    rows = []
    for i in range(lo, lo + n):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [_keys((j - center + 0.5) * inv) for j in range(xmin, xmax)]
        total = sum(w)
        w = [v / total for v in w]
        while len(w) > 1 and w[0] == 0.0:
            w.pop(0)
            xmin += 1
        while len(w) > 1 and w[-1] == 0.0:
            w.pop()
        rows.append((xmin, w))
    taps = max(len(w) for _, w in rows)
    weights = np.zeros((n, taps))
    for i, (_, w) in enumerate(rows):
        weights[i, :len(w)] = w
    return AxisTaps(np.array([f for f, _ in rows], np.int32), np.array([len(w) for _, w in rows], np.int32), weights, in_size)


def resized_shape(H: int, W: int, size: int) -> Tuple[int, int]:
    """shorter side -> `size`, the longer one scaled by the same ratio and truncated (torchvision / HF `resize(size)`)"""
    return (size, int(size * W / H)) if H <= W else (int(size * H / W), size)


def resample_taps(H: int, W: int, size: int) -> Tuple[AxisTaps, AxisTaps]:
    """(rows, columns) taps of resize-shorter-side-to-`size` + centre crop to size x size, the crop folded into the tables"""
    Hr, Wr = resized_shape(H, W, size)
    top, left = int(round((Hr - size) / 2.0)), int(round((Wr - size) / 2.0))
    return axis_taps(H, Hr, top, size), axis_taps(W, Wr, left, size)


_TILES = ((8, 32), (8, 16), (4, 16), (4, 8), (2, 8), (1, 4))
_LDS_LIMIT = 64 * 1024


def _window(t: AxisTaps, tile: int, align: int) -> int:
    """largest source extent any tile of `tile` consecutive outputs reads (its start rounded down, its length up, to `align`)"""
    ext = 0
    for i0 in range(0, len(t.first), tile):
        lo = int(t.first[i0:i0 + tile].min()) // align * align
        hi = int((t.first[i0:i0 + tile] + t.count[i0:i0 + tile]).max())
        ext = max(ext, -(-(hi - lo) // align) * align)
    return ext


def plan_tiles(ty: AxisTaps, tx: AxisTaps) -> Tuple[int, int, int, int]:
    """(tile_h, tile_w, win_h, win_w) of pea_op_preprocess: the largest output tile whose source window fits the LDS budget"""
    for th, tw in _TILES:
        wh, ww = _window(ty, th, 1), _window(tx, tw, 4)
        if 4 * (wh * ww + wh * tw + tw * tx.weights.shape[1] + th * ty.weights.shape[1]) <= _LDS_LIMIT:
            return th, tw, wh, ww
    raise PeaError(f"preprocess: a {ty.in_size}x{tx.in_size} source is too large a reduction to {len(ty.first)} (no tile fits the LDS)")


_tables: Dict[tuple, tuple] = {}


def _device_tables(H: int, W: int, size: int, device):
    key = (H, W, size, str(device))
    if key not in _tables:
        ty, tx = resample_taps(H, W, size)
        dev = []
        for t in (ty, tx):
            dev += [torch.from_numpy(t.first).to(device), torch.from_numpy(t.count).to(device),
                    torch.from_numpy(t.weights.astype(np.float32)).contiguous().to(device), t.weights.shape[1]]
        _tables[key] = (tuple(dev), plan_tiles(ty, tx))
    return _tables[key]


def preprocess(images, size: int, mean: Sequence[float], std: Sequence[float], value_range=(-1.0, 1.0), quantize: bool = True):
    """images fp32 [B,3,H,W] in `value_range` (as `HipVAEDecoder` returns them) -> fp32 [B,3,size,size]: map to [0,1] and
    clamp, with `quantize` round to the 8-bit grid a saved image holds, resize the shorter side to `size` (antialiased bicubic,
    the float definition of `F.interpolate(..., antialias=True)` -- PIL additionally rounds its output to 8 bits), centre
    crop, `(x - mean[c]) / std[c]`.  The tap tables of an input shape are built and uploaded on its first use."""
    if images.dim() != 4 or images.shape[1] != 3:
        raise PeaError(f"preprocess: images {tuple(images.shape)}, expected [B,3,H,W]")
    x = images.detach().to(torch.float32).contiguous()
    B, _, H, W = x.shape
    (yf, yc, yw, yt, xf, xc, xw, xt), (th, tw, wh, ww) = _device_tables(H, W, int(size), x.device)
    out = torch.empty(B, 3, size, size, device=x.device, dtype=torch.float32)
    lo, hi = float(value_range[0]), float(value_range[1])
    check(lib().pea_op_preprocess(ptr(x), B, H, W, lo, hi, int(bool(quantize)), ptr(yf), ptr(yc), ptr(yw), yt, ptr(xf), ptr(xc),
                                  ptr(xw), xt, int(size), th, tw, wh, ww, float(mean[0]), float(mean[1]), float(mean[2]),
                                  float(std[0]), float(std[1]), float(std[2]), ptr(out), stream_ptr()))
    return out


def patchify(pixels, patch_size: int):
    """pixels fp32 [B,3,S,S] -> the patch GEMM's A operand, bf16 [B*(S/P)^2, Kpad]: column (c, py, px), zero-padded from 3 P P
    to the next multiple of 64 (pea_op_patchify; the tower runs the same kernel internally)"""
    x = pixels.detach().to(torch.float32).contiguous()
    B, _, S, _ = x.shape
    kpad = -(-3 * patch_size * patch_size // 64) * 64
    rows = torch.empty(B * (S // patch_size) ** 2, kpad, device=x.device, dtype=torch.bfloat16)
    check(lib().pea_op_patchify(ptr(x), ptr(rows), B, S, patch_size, kpad, stream_ptr()))
    return rows


# ---------------------------------------------------------------- the tower
class _HiddenStates:
    def __init__(self, enc, pixels):
        self._enc, self._px = enc, pixels

    def __getitem__(self, k: int):
        return self._enc.encode(self._px, hidden_index=k)[0]


class _Output:
    """the fields of HF's `CLIPVisionModelOutput` that callers read"""

    def __init__(self, enc, pixels, last, pooled, embeds):
        self.last_hidden_state, self.pooler_output, self.image_embeds = last, pooled, embeds
        self.hidden_states = _HiddenStates(enc, pixels)


class HipImageEncoder(HipTape):
    """`load_state_dict` is strict by default; strict=False skips a full CLIP checkpoint's `text_model.*`, `logit_scale`"""

    def __init__(self, cfg, batch: int):
        self._open()
        self.cfg, self.config = cfg, cfg
        self.B, self.L = batch, cfg.num_tokens
        self.dtype = torch.bfloat16
        c = _cfg.vision_to_c(cfg)
        check(lib().pea_vision_create(ctypes.byref(c), self.B, ctypes.byref(self._h)))

    def encode(self, pixels, hidden_index: int = -1):
        """pixels fp32 [B,3,S,S] (normalised: `preprocess`) -> (hidden fp32 [B, Np+1, width], pooler_output fp32 [B, width],
        image_embeds fp32 [B, proj]).  hidden_index: -1 the last state before `post_layernorm` (HF `last_hidden_state`),
        -2 = `hidden_states[-2]`, k >= 0 = `hidden_states[k]`."""
        S = self.cfg.image_size
        if tuple(pixels.shape) != (self.B, 3, S, S):
            raise PeaError(f"HipImageEncoder built for pixels {(self.B, 3, S, S)}, got {tuple(pixels.shape)}")
        px = pixels.detach().to(self.device, torch.float32).contiguous()
        hid = torch.empty(self.B, self.L, self.cfg.hidden_size, device=self.device, dtype=torch.float32)
        pooled = torch.empty(self.B, self.cfg.hidden_size, device=self.device, dtype=torch.float32)
        emb = torch.empty(self.B, self.cfg.projection_dim, device=self.device, dtype=torch.float32)
        check(lib().pea_vision_forward(self._h, ptr(px), int(hidden_index), ptr(hid), ptr(pooled), ptr(emb), stream_ptr()))
        self._keep = px
        return hid, pooled, emb

    def __call__(self, pixel_values, output_hidden_states: bool = False, **kw):
        last, pooled, emb = self.encode(pixel_values, hidden_index=-1)
        return _Output(self, pixel_values, last, pooled, emb)


def plan(cfg, batch: int = 1) -> Dict[str, int]:
    """parameter total, tokens per image and attention ops of the tower (pea_vision_plan: host only, no device needed)"""
    c = _cfg.vision_to_c(cfg)
    n, t, a = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
    check(lib().pea_vision_plan(ctypes.byref(c), batch, ctypes.byref(n), ctypes.byref(t), ctypes.byref(a)))
    return {"n_params": n.value, "n_tokens": t.value, "n_attn": a.value}


def clip_score_images(image_encoder: HipImageEncoder, images, text_embeds, w: float = 2.5, value_range=(-1.0, 1.0),
                      quantize: bool = True):
    """CLIPScore of decoded images against their prompts' embeddings: preprocess -> tower -> score, all on the current stream,
    -> device fp32 [B].  `images` fp32 [B,3,H,W] in `value_range`; `text_embeds` [B, proj]: `HipTextEncoder`'s `text_embeds`
    for a CLIP-flavour tower with a projection (INTEGRATION.md shows the projected CLS state of the BERT / XLM-R towers)."""
    cfg = image_encoder.cfg
    px = preprocess(images, cfg.image_size, cfg.image_mean, cfg.image_std, value_range, quantize)
    emb = image_encoder.encode(px)[2]
    return _ops.clip_score(emb, text_embeds, w)
