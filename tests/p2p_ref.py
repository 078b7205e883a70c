"""Test infrastructure: prompt-to-prompt editing restated in plain torch.

Nothing here is pinned against another implementation (diffusers' community pipeline is not available): it restates the
definition the package documents, once as the paper's controllers applied one after another and once on the oracle's `Attention`.

  chain_replace / chain_refine / chain_reweight / chain_blend      the controllers, one at a time, float64
  edit_reference            kernel level: O and the magnitude the tolerance rule needs, fp32 on the CPU
  EditState, EditedAttention, attach_edit                           the oracle's attn1 / attn2 with the edit
"""
import torch

from oracle.unet_ref import Attention, _st


# ---------------------------------------------------------------------------------------------- the controllers, one by one
def chain_replace(p0, M):
    """word swap: new[q, n] = sum_w base[q, w] M[w, n]   (M: row = source key, column = target key)"""
    return p0 @ M


def chain_refine(p0, p1, gather, alphas):
    """refinement: the source's probabilities gathered to the target's positions where the token has a source, its own elsewhere"""
    g = gather.clamp(min=0)
    return p0[..., g] * alphas + p1 * (1.0 - alphas)


def chain_reweight(replaced, eq):
    return replaced * eq


def chain_blend(replaced, p1, w):
    """the cross-replace window of this step: w = 1 takes the controller's result, w = 0 the sample's own probabilities"""
    return replaced * w + p1 * (1.0 - w)


# ---------------------------------------------------------------------------------------------- kernel level
def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def edit_reference(q, k, v, H, src, Mt, c, d):
    """fp32: q [B,Sq,H*64], k / v [B,L,H*64], src B ints, Mt [B,L,L] (row = target key, column = source key), c / d [B,L]
    -> (O [B,Sq,H*64], mag): mag = sum_j (|c_j| (P0 |Mt|^T)_j + |d_j| P1_j) |V_j| (P1 |V| for an unedited sample)."""
    q, k, v = q.float(), k.float(), v.float()
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * 0.125       # [B, H, Sq, L]
    p = torch.softmax(s, -1)
    vh = _heads(v, H)
    O, mag = torch.empty_like(q), torch.empty_like(q)
    for b, sb in enumerate(src):
        if sb < 0 or sb == b:                                        # (its own source: not edited)
            a, am = p[b], p[b]
        else:
            p0 = p[sb]
            m = Mt[b].float()
            a = c[b].float() * (p0 @ m.t()) + d[b].float() * p[b]
            am = c[b].float().abs() * (p0 @ m.abs().t()) + d[b].float().abs() * p[b]
        O[b] = (a @ vh[b]).transpose(0, 1).reshape(q.shape[1], -1)
        mag[b] = (am @ vh[b].abs()).transpose(0, 1).reshape(q.shape[1], -1)
    return O, mag


# ---------------------------------------------------------------------------------------------- the oracle's attention layers
class EditState:
    """what HipUNet.set_prompt_edit holds: shared by every EditedAttention of a UNet.  Mt as the bf16 values the library gets"""

    def __init__(self):
        self.edit = None            # a pea_diffusion_amd.prompt2prompt.PromptEdit, laid out for the batch; None: plain attention
        self.step = 0

    def set(self, edit, step=0):
        self.edit, self.step = edit, step


class EditedAttention(Attention):
    def __init__(self, query_dim, heads, cross_dim, state):
        super().__init__(query_dim, heads, cross_dim)
        self.state = state

    def forward(self, x, ctx=None):
        ed = self.state.edit
        if ed is None:
            return super().forward(x, ctx)
        cross = ctx is not None
        ctx = x if ctx is None else ctx
        B, S, C = x.shape
        H = self.heads
        q = _st(self.to_q(x)).view(B, S, H, C // H).transpose(1, 2)
        k = _st(self.to_k(ctx)).view(B, -1, H, C // H).transpose(1, 2)
        v = _st(self.to_v(ctx)).view(B, -1, H, C // H).transpose(1, 2)
        a = torch.softmax(q @ k.transpose(-1, -2) * (C // H) ** -0.5, dim=-1)
        out = a.clone()
        step = self.state.step
        for b, sb in enumerate(ed.src.tolist()):
            if sb < 0 or sb == b:
                continue
            if cross:
                m = ed.Mt[b].to(torch.bfloat16).to(a.dtype)
                c, d = ed.cd[step, 0, b].to(a.dtype), ed.cd[step, 1, b].to(a.dtype)
                out[b] = c * (a[sb] @ m.t()) + d * a[b]
            elif S <= ed.self_max_tokens and step < ed.self_until:
                out[b] = a[sb]
        o = _st((_st(out) @ v).transpose(1, 2).reshape(B, S, C))       # (the mixture is a bf16 MFMA operand, rounded once)
        return self.to_out[0](o)


def attach_edit(unet):
    """every attn1 / attn2 of `unet` becomes an EditedAttention with the layer's own weights -> the shared EditState"""
    state = EditState()
    named = [(n, m) for n, m in unet.named_modules() if n.endswith(".attn1") or n.endswith(".attn2")]
    for name, old in named:
        C = old.to_q.weight.shape[0]
        cross = old.to_k.weight.shape[1] if name.endswith(".attn2") else None
        new = EditedAttention(C, old.heads, cross, state)
        new.load_state_dict(old.state_dict())
        for p in new.parameters():
            p.requires_grad_(False)
        parent, leaf = name.rsplit(".", 1)
        setattr(unet.get_submodule(parent), leaf, new)
    return state
