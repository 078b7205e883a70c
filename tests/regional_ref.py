"""Test infrastructure: regional text prompts restated in plain torch.

Nothing here is pinned against another implementation: it restates the definition the package documents -- R prompts back to
back in one context, every cross-attention layer R softmaxes over the same q, their outputs mixed per query position with
weights that come from the regions' masks reduced to the layer's grid by area means.

  regions_terms             kernel level: every region's attention output on its own, in fp32
  combine                   ... mixed with the weights, plus the magnitude the tolerance rule needs
  region_weights_ref        pea_diffusion_amd.regional.region_weights restated with explicit window means (no call into the package)
  half_masks / quadrant_masks
  RegionalAttention         `Attention` with R runs of context rows, masks and weights
  attach_regions / set_regions
"""
import math

import torch

from ip_adapter_ref import ip_layers
from ip_multi_ref import grid_of, sdpa
from oracle.unet_ref import Attention, _st


def regions_terms(q, k, v, H, R):
    """-> [o_r]: region r is rows r Lr .. (r + 1) Lr of k / v (Lr = rows / R), with a softmax of its own; fp32, head_dim 64"""
    assert k.shape[1] % R == 0
    Lr = k.shape[1] // R
    return [sdpa(q, k[:, r * Lr:(r + 1) * Lr], v[:, r * Lr:(r + 1) * Lr], H)[0] for r in range(R)]


def combine(terms, w):
    """w [1|B, R, Sq] -> (O, magnitude): O = sum_r w_r o_r and sum_r |w_r| |o_r|"""
    ref, mag = torch.zeros_like(terms[0]), torch.zeros_like(terms[0])
    for r, o in enumerate(terms):
        f = w[:, r, :, None].float()
        ref = ref + f * o
        mag = mag + f.abs() * o.abs()
    return ref, mag


def _window_mean(m, h_l, w_l):
    """[B, h, w] -> [B, h_l, w_l]: cell (i, j) is the mean over rows floor(i h / h_l) .. ceil((i + 1) h / h_l) and the same in w"""
    B, h, w = m.shape
    out = torch.empty(B, h_l, w_l, dtype=torch.float64)
    for i in range(h_l):
        r0, r1 = (i * h) // h_l, -((-(i + 1) * h) // h_l)
        for j in range(w_l):
            c0, c1 = (j * w) // w_l, -((-(j + 1) * w) // w_l)
            out[:, i, j] = m[:, r0:r1, c0:c1].double().sum((1, 2)) / ((r1 - r0) * (c1 - c0))
    return out


def region_weights_ref(masks, weights, h_l, w_l):
    """-> fp32 [Bm, R, h_l w_l]: a_r = weights[r] x (window mean of masks[r], None = 1), a_r / sum_r a_r where the sum exceeds
    1e-6, elsewhere region 0 alone"""
    R = len(masks)
    weights = [1.0] * R if weights is None else list(weights)
    red = []
    for m in masks:
        if m is None:
            red.append(torch.ones(1, h_l, w_l, dtype=torch.float64))
        else:
            m = torch.as_tensor(m).float()
            red.append(_window_mean(m[None] if m.dim() == 2 else m, h_l, w_l))
    Bm = max(m.shape[0] for m in red)
    out = torch.zeros(Bm, R, h_l, w_l, dtype=torch.float64)
    for b in range(Bm):
        for i in range(h_l):
            for j in range(w_l):
                a = [float(weights[r]) * float(red[r][b if red[r].shape[0] > 1 else 0, i, j]) for r in range(R)]
                tot = math.fsum(a)
                if tot > 1e-6:
                    for r in range(R):
                        out[b, r, i, j] = a[r] / tot
                else:
                    out[b, 0, i, j] = 1.0
    return out.float().reshape(Bm, R, h_l * w_l)


def half_masks(h, w):
    """left / right halves of an h x w picture: a partition"""
    left = torch.zeros(h, w)
    left[:, : w // 2] = 1.0
    return [left, 1.0 - left]


def quadrant_masks(h, w):
    """the four quadrants of an h x w picture (cut at h // 2, w // 2): a partition"""
    out = []
    for top in (True, False):
        for lft in (True, False):
            m = torch.zeros(h, w)
            m[(slice(0, h // 2) if top else slice(h // 2, h)), (slice(0, w // 2) if lft else slice(w // 2, w))] = 1.0
            out.append(m)
    return out


class RegionalAttention(Attention):
    def __init__(self, query_dim, heads, cross_dim, latent_hw):
        super().__init__(query_dim, heads, cross_dim)
        self.latent_hw = latent_hw
        self.masks = None            # None: one softmax over the whole context; else R masks (None or [h, w] / [1|B, h, w])
        self.weights = None
        self.do_cfg = False          # the first half of the batch attends to region 0 alone

    def forward(self, x, ctx=None):
        if self.masks is None:
            return super().forward(x, ctx)
        B, S, C = x.shape
        H, R = self.heads, len(self.masks)
        heads = lambda t: t.view(B, -1, H, C // H).transpose(1, 2)
        q, k, v = heads(_st(self.to_q(x))), heads(_st(self.to_k(ctx))), heads(_st(self.to_v(ctx)))
        assert k.shape[2] % R == 0
        Lr = k.shape[2] // R
        w = region_weights_ref(self.masks, self.weights, *grid_of(S, *self.latent_hw)).expand(B, R, S).clone()
        if self.do_cfg:
            w[: B // 2] = 0.0
            w[: B // 2, 0] = 1.0
        o = 0.0
        for r in range(R):
            kr, vr = k[:, :, r * Lr:(r + 1) * Lr], v[:, :, r * Lr:(r + 1) * Lr]
            a = torch.softmax(q @ kr.transpose(-1, -2) * (C // H) ** -0.5, dim=-1)
            o = o + w[:, r, None, :, None] * (_st(a) @ vr)          # (P is a bf16 MFMA operand; the SUM is stored once)
        return self.to_out[0](_st(o.transpose(1, 2).reshape(B, S, C)))


def attach_regions(unet, latent_hw):
    """every attn2 of `unet` becomes a RegionalAttention with the layer's own weights -> [(name, module)]"""
    out = []
    for name, old in ip_layers(unet):
        C, cross = old.to_q.weight.shape[0], old.to_k.weight.shape[1]
        new = RegionalAttention(C, old.heads, cross, latent_hw)
        new.load_state_dict(old.state_dict())
        for p in new.parameters():
            p.requires_grad_(False)
        setattr(unet.get_submodule(name.rsplit(".", 1)[0]), "attn2", new)
        out.append((name, new))
    return out


def set_regions(unet, masks, weights=None, do_cfg=False):
    """masks: a list of R masks, or None for the plain attention"""
    for _, m in ip_layers(unet):
        m.masks = None if masks is None else list(masks)
        m.weights, m.do_cfg = weights, do_cfg
