"""LoRA files for the HIP UNet: reading them and resolving their keys against a UNet's weight table -- the host half of
`pipe.load_lora_weights(path)` / `pipe.fuse_lora()` (tests/test_sdxl_zh_lcm.py:181-182; the `DOWNSTREAM == "LoRA"` switch of
tests/test_sdxl_zh.py:148-149).  Pure host code (no GPU, no library needed); `HipUNet.fuse_lora` does the device work.

Three key spellings are understood, for a module `m` (a diffusers state-dict key without its `.weight`):
  kohya      lora_unet_<m with '_' for '.'>.lora_down.weight / .lora_up.weight / .alpha
  diffusers  unet.<m>.lora.down.weight / .lora.up.weight, also the attention-processor spelling
             unet.<attn>.processor.to_q_lora.down.weight (to_q / to_k / to_v, to_out_lora -> to_out.0)
  PEFT       [base_model.model.][unet.]<m>.lora_A.weight / .lora_B.weight (an adapter name may sit before `.weight`)
`down` is [rank][Cin] or [rank][Cin][3][3], `up` is [Cout][rank] or [Cout][rank][1][1]; the fused weight is
W + lora_scale * alpha / rank * up @ down, alpha = rank when the file carries none.  Text-encoder keys are skipped: the PEA
adapter replaces the text encoders on this path."""
from __future__ import annotations

import re
from typing import Dict, List, Tuple

import torch

from ._lib import PeaError

MAX_RANK = 256                                  # pea_op_lora_compose
# module suffixes of the LCM-LoRA target set: attention and feed-forward projections, the transformers' proj_in / proj_out,
# resnet convolutions and time_emb_proj, the down / up sampler convolutions
LCM_LORA_TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "proj_in", "proj_out", "ff.net.0.proj", "ff.net.2", "conv1", "conv2",
                    "conv_shortcut", "downsamplers.0.conv", "upsamplers.0.conv", "time_emb_proj")
_TEXT_PREFIXES = ("lora_te1_", "lora_te2_", "lora_te_", "text_encoder.", "text_encoder_2.")
_KOHYA = "lora_unet_"
_PROC = re.compile(r"^(.*)\.processor\.(to_q|to_k|to_v|to_out)_lora\.(down|up)\.weight$")
_DIFF = re.compile(r"^(.*)\.lora\.(down|up)\.weight$")
_PEFT = re.compile(r"^(.*)\.lora_(A|B)(?:\.[^.]+)?\.weight$")
_ALPHA = re.compile(r"^(.*?)(?:\.lora)?\.alpha$")


def load_lora_state_dict(path_or_dict) -> Dict[str, torch.Tensor]:
    """a dict of tensors as it is, a `.safetensors` file, or a torch pickle (`.bin` / `.pt`)"""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    path = str(path_or_dict)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    sd = torch.load(path, map_location="cpu")
    if not isinstance(sd, dict):
        raise PeaError(f"load_lora_state_dict: {path} holds a {type(sd).__name__}, not a state dict")
    return sd


def kohya_names(weight_table) -> Dict[str, str]:
    """{kohya module name: weight key} of every `*.weight` key of the table; the '.' -> '_' image must be injective"""
    image = {}
    for key in weight_table:
        if not key.endswith(".weight"):
            continue
        name = key[:-len(".weight")].replace(".", "_")
        assert name not in image, f"kohya names collide: {image[name]} and {key} both spell {name}"
        image[name] = key
    return image


def _parse(key: str, kohya: Dict[str, str]):
    """-> (module or None, part) with part in down / up / alpha, or None for a key that is no LoRA entry of the UNet"""
    if key.startswith(_KOHYA):
        name, _, tail = key[len(_KOHYA):].partition(".")
        part = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}.get(tail)
        if part is None:
            return None
        wkey = kohya.get(name)
        return (wkey[:-len(".weight")] if wkey else None), part
    k = key
    for prefix in ("base_model.model.", "unet."):
        if k.startswith(prefix):
            k = k[len(prefix):]
    m = _PROC.match(k)
    if m:
        return f"{m.group(1)}.{'to_out.0' if m.group(2) == 'to_out' else m.group(2)}", m.group(3)
    m = _DIFF.match(k)
    if m:
        return m.group(1), m.group(2)
    m = _PEFT.match(k)
    if m:
        return m.group(1), "down" if m.group(2) == "A" else "up"
    m = _ALPHA.match(k)
    if m:
        return m.group(1), "alpha"
    return None


def check_factors(key: str, shape, down: torch.Tensor, up: torch.Tensor) -> int:
    """rank of a factor pair for the weight `key` of torch shape `shape`; raises on any size that does not compose"""
    d0, numel = int(shape[0]), 1
    for s in shape:
        numel *= int(s)
    rank = int(down.shape[0]) if down.dim() >= 2 else 0
    if not 1 <= rank <= MAX_RANK:
        raise PeaError(f"LoRA {key}: rank {rank} outside 1..{MAX_RANK} (down {tuple(down.shape)})")
    if len(shape) < 2:
        raise PeaError(f"LoRA {key}: the target is a vector of shape {tuple(shape)}")
    if up.dim() < 2 or up.shape[0] != d0 or up.numel() != d0 * rank or down.numel() * d0 != rank * numel:
        raise PeaError(f"LoRA {key}: up {tuple(up.shape)} . down {tuple(down.shape)} does not give {tuple(shape)}")
    return rank


def resolve_lora(lora_sd: Dict[str, torch.Tensor], weight_table) -> Tuple[Dict[str, tuple], List[str]]:
    """-> ({UNet weight key: (down fp32 [rank][Kf], up fp32 [d0][rank], alpha)}, skipped text-encoder keys).
    weight_table: {diffusers key: torch shape} (`HipUNet.weight_table()`, or the shapes of a state dict).  A UNet key that
    resolves to no weight of the table, a half pair, or factors of the wrong size raise."""
    kohya = kohya_names(weight_table)
    parts: Dict[str, dict] = {}
    skipped, unknown = [], []
    for key, val in lora_sd.items():
        if key.startswith(_TEXT_PREFIXES):
            skipped.append(key)
            continue
        p = _parse(key, kohya)
        if p is None or p[0] is None or p[0] + ".weight" not in weight_table:
            unknown.append(key)
            continue
        parts.setdefault(p[0] + ".weight", {})[p[1]] = val
    if unknown:
        raise PeaError(f"resolve_lora: {len(unknown)} keys name no weight of this UNet, first: {unknown[:5]}")
    out = {}
    for wkey, d in parts.items():
        if "down" not in d or "up" not in d:
            raise PeaError(f"resolve_lora: {wkey} has {sorted(d)} but needs both down and up")
        rank = check_factors(wkey, weight_table[wkey], d["down"], d["up"])
        alpha = float(d["alpha"]) if "alpha" in d else float(rank)
        out[wkey] = (d["down"].detach().to(torch.float32).reshape(rank, -1).contiguous(),
                     d["up"].detach().to(torch.float32).reshape(-1, rank).contiguous(), alpha)
    return out, skipped


def lcm_lora_target_keys(weight_table) -> List[str]:
    """the weight keys of a table that an LCM-LoRA touches"""
    return [k for k in weight_table if any(k.endswith("." + t + ".weight") for t in LCM_LORA_TARGETS)]


def merged_weight(base: torch.Tensor, adapters) -> torch.Tensor:
    """float64 host statement of the fusion, W + sum_i scale_i * up_i @ down_i in `base`'s shape and dtype (for checks and
    for exporting a fused checkpoint; the device path is HipUNet.fuse_lora).  adapters: [(down, up, scale)]"""
    w = base.detach().double().reshape(base.shape[0], -1).clone()
    for down, up, scale in adapters:
        w += float(scale) * (up.double().reshape(w.shape[0], -1) @ down.double().reshape(-1, w.shape[1]))
    return w.reshape(base.shape).to(base.dtype)
