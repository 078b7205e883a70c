"""Test infrastructure: IP-Adapter restated in plain torch, independent of pea_diffusion_amd.

Neither diffusers nor the IP-Adapter package is installed here, so nothing in this file is pinned against them: it restates
the published algorithm (IPAttnProcessor2_0, ImageProjModel and the pipeline's CFG rule of tencent-ailab/IP-Adapter) on top of
the oracle UNet of oracle/unet_ref.py.

  IPAttention       `Attention` with `to_k_ip` / `to_v_ip` and the decoupled forward: the text states go through the layer's own
                    softmax, the N image tokens (held by the module: set_ip) through a second one over the same q, and the two
                    outputs are added with `scale`.  `_st` marks what the HIP path stores in bf16: the image K and V, and the
                    SUMMED output once (the fused kernel never stores either term).
  attach_ip         swaps it into every `attn2` of an oracle instance, keeping that layer's weights
  image_proj_ref    ImageProjModel: LayerNorm(proj(embeds).view(B, N, cross_dim))
  ip_tokens_ref     ... with the CFG rule: the tokens of an all-zero embedding first
  file_state_dict   the adapter as its published `.bin` holds it, numbered by position in `unet.attn_processors`
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.unet_ref import Attention, _st


class IPAttention(Attention):
    def __init__(self, query_dim, heads, cross_dim, n_tokens):
        super().__init__(query_dim, heads, cross_dim)
        self.n_tokens = n_tokens
        self.scale = 1.0
        self.tokens = None                       # [B, N, cross_dim], set by set_ip; None: the plain layer
        self.to_k_ip = nn.Linear(cross_dim, query_dim, bias=False)
        self.to_v_ip = nn.Linear(cross_dim, query_dim, bias=False)

    def forward(self, x, ctx=None):
        if self.tokens is None:
            return super().forward(x, ctx)
        B, S, C = x.shape
        H = self.heads
        heads = lambda t: t.view(B, -1, H, C // H).transpose(1, 2)
        q = heads(_st(self.to_q(x)))
        k, v = heads(_st(self.to_k(ctx))), heads(_st(self.to_v(ctx)))
        k2, v2 = heads(_st(self.to_k_ip(self.tokens))), heads(_st(self.to_v_ip(self.tokens)))
        s = (C // H) ** -0.5
        a = torch.softmax(q @ k.transpose(-1, -2) * s, dim=-1)
        a2 = torch.softmax(q @ k2.transpose(-1, -2) * s, dim=-1)
        o = _st(a) @ v + self.scale * (_st(a2) @ v2)                # (P and P2 are bf16 MFMA operands; the sum is stored once)
        return self.to_out[0](_st(o.transpose(1, 2).reshape(B, S, C)))


def ip_layers(unet):
    """[(diffusers module name, module)] of every attn2 in the order of `unet.attn_processors`: down, up, then mid"""
    named = [(n, m) for n, m in unet.named_modules() if n.endswith(".attn2")]
    rank = lambda n: 0 if n.startswith("down_blocks") else 1 if n.startswith("up_blocks") else 2
    return sorted(named, key=lambda nm: rank(nm[0]))               # stable: module order inside each group


def attach_ip(unet, n_tokens, seed, gain=1.0):
    """every attn2 of `unet` becomes an IPAttention with the same to_q / to_k / to_v / to_out and seeded to_k_ip / to_v_ip
    (torch's Linear init times `gain`, rounded to bf16 as the HIP path stores them).  Returns the swapped modules, in file order."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for name, old in ip_layers(unet):
        C, cross = old.to_q.weight.shape[0], old.to_k.weight.shape[1]
        new = IPAttention(C, old.heads, cross, n_tokens)
        new.load_state_dict(old.state_dict(), strict=False)
        with torch.no_grad():
            for lin in (new.to_k_ip, new.to_v_ip):
                bound = gain * cross ** -0.5
                lin.weight.copy_(((torch.rand(C, cross, generator=g) * 2 - 1) * bound).to(torch.bfloat16).float())
        for p in new.parameters():
            p.requires_grad_(False)
        parent = unet.get_submodule(name.rsplit(".", 1)[0])
        setattr(parent, "attn2", new)
        out.append((name, new))
    return out


def set_ip(unet, tokens, scale=1.0):
    """tokens [B, N, cross_dim] (None: plain layers) and the scale, for every IPAttention of `unet`"""
    for m in unet.modules():
        if isinstance(m, IPAttention):
            m.tokens, m.scale = tokens, scale


def file_state_dict(unet, proj):
    """{"image_proj": ..., "ip_adapter": {"<i>.to_k_ip.weight": ...}}: processor i = 2 * (position among the attn2 layers) + 1,
    attn1 / attn2 alternating"""
    ip = {}
    for n, (_, m) in enumerate(ip_layers(unet)):
        ip[f"{2 * n + 1}.to_k_ip.weight"] = m.to_k_ip.weight.detach().clone()
        ip[f"{2 * n + 1}.to_v_ip.weight"] = m.to_v_ip.weight.detach().clone()
    return {"image_proj": {k: v.detach().clone() for k, v in proj.items()}, "ip_adapter": ip}


def make_image_proj(embed_dim, cross_dim, n_tokens, seed):
    """seeded ImageProjModel weights; proj.weight bf16-representable (the HIP path holds it in bf16)"""
    g = torch.Generator().manual_seed(seed)
    return {"proj.weight": (torch.randn(n_tokens * cross_dim, embed_dim, generator=g) * embed_dim ** -0.5).to(torch.bfloat16).float(),
            "proj.bias": torch.randn(n_tokens * cross_dim, generator=g) * 0.1,
            "norm.weight": 1.0 + 0.1 * torch.randn(cross_dim, generator=g),
            "norm.bias": 0.1 * torch.randn(cross_dim, generator=g)}


def image_proj_ref(proj, image_embeds, dtype=torch.float64):
    """ImageProjModel.forward; the embeddings enter as the HIP GEMM reads them, rounded to bf16"""
    cross = proj["norm.weight"].shape[0]
    e = image_embeds.to(torch.bfloat16).to(dtype)
    y = F.linear(e, proj["proj.weight"].to(dtype), proj["proj.bias"].to(dtype)).view(e.shape[0], -1, cross)
    return F.layer_norm(y, (cross,), proj["norm.weight"].to(dtype), proj["norm.bias"].to(dtype), 1e-5)


def ip_tokens_ref(proj, image_embeds, do_cfg=False, dtype=torch.float64):
    """pipeline rule: with CFG the unconditional half is the projection of an all-zero embedding, and it comes first"""
    t = image_proj_ref(proj, image_embeds, dtype)
    return torch.cat([image_proj_ref(proj, torch.zeros_like(image_embeds), dtype), t]) if do_cfg else t
