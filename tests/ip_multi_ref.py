"""Test infrastructure: several IP-Adapters at once, with region masks and per-layer scales, restated in plain torch.

Like tests/ip_adapter_ref.py nothing here is pinned against diffusers (not installed): it restates what
`IPAdapterAttnProcessor2_0` does with a list of adapters -- one more decoupled softmax per adapter over the same q, each output
multiplied by that adapter's scale and, where a mask is given, by the mask reduced to the layer's grid with bicubic
interpolation (`IPAdapterMaskProcessor.downsample`), all added to the text output.

  sdpa / multi_ip_terms     kernel level: the text term and every image term on their own, in fp32
  combine                   ... summed with weights and masks, plus the magnitude the tolerance rule needs
  rect_mask                 a binary rectangle whose bicubic reduction leaves [0, 1]
  grid_of                   the (h, w) grid of a layer with S queries under a latent of (H, W)
  MultiIPAttention          `Attention` with J pairs `to_k_ip[j]` / `to_v_ip[j]`, tokens, scales and masks per adapter
  attach_multi_ip / set_multi_ip / file_state_dict_of
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ip_adapter_ref import ip_layers
from oracle.unet_ref import Attention, _st


def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def sdpa(q, k, v, H, kv_len=None):
    """fp32 attention per head (head_dim 64, scale 1/8) -> (o [B,Sq,C], lse [B,H,Sq]); keys >= kv_len[b] of sample b are cut"""
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * 0.125
    if kv_len is not None:
        cut = torch.arange(k.shape[1])[None, :] >= torch.as_tensor(kv_len)[:, None]
        s = s.masked_fill(cut[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ _heads(v, H)).transpose(1, 2).reshape(q.shape)
    return o, torch.logsumexp(s, -1)


def multi_ip_terms(q, k, v, k2, v2, H, n_keys, kv_len=None):
    """-> o_text, lse, [o_j]: set j is rows sum(n_keys[:j]) .. + n_keys[j] of k2 / v2, with a softmax of its own"""
    o1, lse = sdpa(q, k, v, H, kv_len)
    terms, off = [], 0
    for n in n_keys:
        terms.append(sdpa(q, k2[:, off:off + n], v2[:, off:off + n], H)[0])
        off += n
    assert off == k2.shape[1]
    return o1, lse, terms


def combine(o1, terms, scales, masks=None):
    """-> (O, magnitude): O = o1 + sum_j w_j m_j o_j and |o1| + sum_j |w_j m_j| |o_j|; masks[j] None or [1|B, Sq]"""
    ref, mag = o1.clone(), o1.abs()
    for j, (o, w) in enumerate(zip(terms, scales)):
        f = torch.full((1, 1, 1), float(w))
        if masks is not None and masks[j] is not None:
            f = f * masks[j].float()[:, :, None]
        ref = ref + f * o
        mag = mag + f.abs() * o.abs()
    return ref, mag


def rect_mask(h_l, w_l, variant=0, up=8):
    """binary [up h_l, up w_l] rectangle whose edges fall where the 4 bicubic taps of a grid cell straddle them: rows from
    up a + 3 (taps 0 1 1 1: above 1), columns from up c + 5 (taps 0 0 0 1: below 0); `variant` moves it"""
    m = torch.zeros(up * h_l, up * w_l)
    r0, c0 = up * (variant % max(h_l // 2, 1)) + 3, up * (variant % max(w_l // 2, 1)) + 5
    r1, c1 = min(r0 + up * max(h_l // 2, 1) + 2, up * h_l), min(c0 + up * max(w_l // 2, 1) - 2, up * w_l)
    m[r0:r1, c0:c1] = 1.0
    return m


def grid_of(S, H, W):
    """(h, w) with h w == S after k stride-2 convolutions (padding 1: n -> ceil(n / 2)) of an (H, W) latent"""
    h, w = H, W
    while h * w > S and (h > 1 or w > 1):
        h, w = (h + 1) // 2, (w + 1) // 2
    assert h * w == S, (S, H, W)
    return h, w


def downsample_ref(mask, h_l, w_l):
    """IPAdapterMaskProcessor.downsample, restated: bicubic, align_corners False, no antialiasing -> [1|B, h_l w_l]"""
    m = mask if mask.dim() == 3 else mask[None]
    return F.interpolate(m[:, None].float(), size=(h_l, w_l), mode="bicubic", align_corners=False).reshape(m.shape[0], h_l * w_l)


class MultiIPAttention(Attention):
    def __init__(self, query_dim, heads, cross_dim, n_tokens, latent_hw):
        super().__init__(query_dim, heads, cross_dim)
        self.n_tokens, self.latent_hw = list(n_tokens), latent_hw
        self.to_k_ip = nn.ModuleList([nn.Linear(cross_dim, query_dim, bias=False) for _ in n_tokens])
        self.to_v_ip = nn.ModuleList([nn.Linear(cross_dim, query_dim, bias=False) for _ in n_tokens])
        self.tokens = [None] * len(n_tokens)     # per adapter [B, N_j, cross_dim] or None (adapter off)
        self.scales = [1.0] * len(n_tokens)      # per adapter, THIS layer's scale
        self.masks = [None] * len(n_tokens)      # per adapter None or [1|B, h, w] at any resolution

    def forward(self, x, ctx=None):
        if all(t is None for t in self.tokens):
            return super().forward(x, ctx)
        B, S, C = x.shape
        H = self.heads
        heads = lambda t: t.view(B, -1, H, C // H).transpose(1, 2)
        q = heads(_st(self.to_q(x)))
        k, v = heads(_st(self.to_k(ctx))), heads(_st(self.to_v(ctx)))
        s = (C // H) ** -0.5
        o = _st(torch.softmax(q @ k.transpose(-1, -2) * s, dim=-1)) @ v
        for j, tok in enumerate(self.tokens):
            if tok is None or self.scales[j] == 0.0:
                continue
            k2, v2 = heads(_st(self.to_k_ip[j](tok))), heads(_st(self.to_v_ip[j](tok)))
            oj = torch.softmax(q @ k2.transpose(-1, -2) * s, dim=-1) @ v2
            f = torch.full((1, 1, 1, 1), float(self.scales[j]))
            if self.masks[j] is not None:
                f = f * downsample_ref(self.masks[j], *grid_of(S, *self.latent_hw))[:, None, :, None]
            o = o + f * oj                       # (the kernel folds the factor into P; the SUM is stored once)
        return self.to_out[0](_st(o.transpose(1, 2).reshape(B, S, C)))


def attach_multi_ip(unet, n_tokens, seeds, latent_hw, gain=1.0):
    """every attn2 of `unet` becomes a MultiIPAttention with the layer's own weights and, per adapter j, to_k_ip / to_v_ip drawn
    exactly as ip_adapter_ref.attach_ip(unet, n_tokens[j], seeds[j], gain) draws them.  -> [(name, module)] in file order"""
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    out = []
    for name, old in ip_layers(unet):
        C, cross = old.to_q.weight.shape[0], old.to_k.weight.shape[1]
        new = MultiIPAttention(C, old.heads, cross, n_tokens, latent_hw)
        new.load_state_dict(old.state_dict(), strict=False)
        with torch.no_grad():
            for j, g in enumerate(gens):
                for lin in (new.to_k_ip[j], new.to_v_ip[j]):
                    bound = gain * cross ** -0.5
                    lin.weight.copy_(((torch.rand(C, cross, generator=g) * 2 - 1) * bound).to(torch.bfloat16).float())
        for p in new.parameters():
            p.requires_grad_(False)
        setattr(unet.get_submodule(name.rsplit(".", 1)[0]), "attn2", new)
        out.append((name, new))
    return out


def set_multi_ip(unet, tokens, layer_scales, masks=None):
    """tokens[j] [B, N_j, cross_dim] or None; layer_scales[j] a number or a per-layer list in file order; masks[j] None or a mask"""
    layers = ip_layers(unet)
    for l, (_, m) in enumerate(layers):
        m.tokens = list(tokens)
        m.scales = [float(s[l]) if isinstance(s, (list, tuple)) else float(s) for s in layer_scales]
        m.masks = [None] * len(tokens) if masks is None else list(masks)


def file_state_dict_of(unet, j, proj):
    """adapter j as its published file holds it (ip_adapter_ref.file_state_dict for one member of the list)"""
    ip = {}
    for n, (_, m) in enumerate(ip_layers(unet)):
        ip[f"{2 * n + 1}.to_k_ip.weight"] = m.to_k_ip[j].weight.detach().clone()
        ip[f"{2 * n + 1}.to_v_ip.weight"] = m.to_v_ip[j].weight.detach().clone()
    return {"image_proj": {k: v.detach().clone() for k, v in proj.items()}, "ip_adapter": ip}
