"""Test infrastructure: cross-attention heat maps restated in plain torch.

Nothing here is pinned against another implementation (the `daam` package is not a dependency): it restates the definition the
package documents -- per layer the softmax probabilities of the text cross-attention averaged over heads, laid out [B, key, query],
summed per latent grid over layers and steps, every grid's sum upsampled bicubically to one size, clamped at 0, summed and divided
by the number of layer-forwards.

  maps_ref          kernel level: the head-mean probabilities in fp32
  MapAttention      `Attention` that also records them
  attach_maps / reset_maps / level_sums
  combine_ref       written with explicit loops over levels and tokens, no call into the package
"""
import torch
import torch.nn.functional as F

from ip_adapter_ref import ip_layers
from ip_multi_ref import grid_of
from oracle.unet_ref import Attention, _st


def maps_ref(q, k, H, kv_len=None):
    """q [B, Sq, H * 64], k [B, Skv, H * 64] (any float dtype), scale 1 / 8 -> fp32 [B, Skv, Sq]; kv_len: keys >= kv_len[b] are cut"""
    B, Sq, _ = q.shape
    qh = q.float().view(B, Sq, H, 64).transpose(1, 2)
    kh = k.float().view(B, -1, H, 64).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * 0.125                            # [B, H, Sq, Skv]
    if kv_len is not None:
        cut = torch.arange(k.shape[1])[None, :] >= torch.as_tensor(kv_len)[:, None]
        s = s.masked_fill(cut[:, None, None, :], float("-inf"))
    return torch.softmax(s, -1).mean(1).transpose(1, 2).contiguous()


class MapAttention(Attention):
    """the oracle's cross-attention, which also keeps the head mean of its probabilities: `record` is None (off) or a list that
    gets one fp32 [B, L, S] per forward"""

    def __init__(self, query_dim, heads, cross_dim):
        super().__init__(query_dim, heads, cross_dim)
        self.record = None

    def forward(self, x, ctx=None):
        if self.record is not None:
            B, S, C = x.shape
            H = self.heads
            q = _st(self.to_q(x)).view(B, S, H, C // H).transpose(1, 2)
            k = _st(self.to_k(ctx)).view(B, -1, H, C // H).transpose(1, 2)
            a = torch.softmax(q @ k.transpose(-1, -2) * (C // H) ** -0.5, dim=-1)       # fp32: the maps are not a bf16 operand
            self.record.append(a.mean(1).transpose(1, 2).float().clone())
        return super().forward(x, ctx)


def attach_maps(unet):
    """every attn2 of `unet` becomes a MapAttention with the same weights -> [(name, module)] in the adapter files' layer order"""
    out = []
    for name, old in ip_layers(unet):
        C, cross = old.to_q.weight.shape[0], old.to_k.weight.shape[1]
        new = MapAttention(C, old.heads, cross)
        new.load_state_dict(old.state_dict())
        for p in new.parameters():
            p.requires_grad_(False)
        setattr(unet.get_submodule(name.rsplit(".", 1)[0]), "attn2", new)
        out.append((name, new))
    return out


def reset_maps(unet, select=None):
    """start recording in every attn2 (select: name -> bool, which layers), forgetting what was recorded"""
    for name, m in ip_layers(unet):
        m.record = [] if select is None or select(name) else None


def level_sums(unet, latent_hw):
    """-> {(h_l, w_l): (fp32 [B, L, h_l, w_l], n)}: what was recorded since reset_maps, summed per latent grid in layer order"""
    out = {}
    for _, m in ip_layers(unet):
        for a in m.record or []:
            B, L, S = a.shape
            hw = grid_of(S, *latent_hw)
            tot, n = out.get(hw, (torch.zeros(B, L, *hw), 0))
            out[hw] = (tot + a.view(B, L, *hw), n + 1)
    return out


def combine_ref(levels, size=None, clamp=True):
    """levels {(h, w): (tensor [B, L, h, w], n)} -> fp32 [B, L, H, W]; token by token, one interpolate call per (level, token)"""
    keys = list(levels)
    if size is None:
        size = keys[0]
        for hw in keys[1:]:
            if hw[0] * hw[1] > size[0] * size[1]:
                size = hw
    B, L = levels[keys[0]][0].shape[:2]
    out = torch.zeros(B, L, size[0], size[1])
    n_total = 0
    for hw in keys:
        t, n = levels[hw]
        n_total += n
        for l in range(L):
            plane = t[:, l:l + 1].float()
            if tuple(hw) != tuple(size):
                plane = F.interpolate(plane, size=tuple(size), mode="bicubic", align_corners=False)
            if clamp:
                plane = torch.where(plane < 0, torch.zeros_like(plane), plane)
            out[:, l] += plane[:, 0]
    return out / n_total
