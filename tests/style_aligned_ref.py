"""Test infrastructure: StyleAligned shared self-attention restated in plain torch.

Nothing here is pinned against another implementation (the authors' code is not available): it restates the definition the
package documents, in the EXPLICIT form -- AdaIN'd copies of Q and K, concatenated K and V, one softmax over 2 S keys.

  adain_coef                coefficients (a_q, s_q, a_k, s_k) per target sample
  shared_reference          kernel level: O and the magnitude the tolerance rule needs
  shared_folded             the form the kernel computes: (q' o a_k) . k + q' . s_k, two segments, one softmax
  StyleState, SharedAttention, attach_style      the oracle's attn1 with the sharing
"""
import torch

from oracle.unet_ref import Attention, _st

EPS = 1e-5


def _stats(x, eps):
    """x [S, C] -> mean, sqrt(unbiased variance + eps) over the tokens"""
    return x.mean(0), (x.var(0, unbiased=True) + eps).sqrt()


def adain_coef(q, k, ref, eps_q=EPS, eps_k=EPS, adain_queries=True, adain_keys=True):
    """q, k [B, S, C] -> coef [B, 4, C] = (a_q, s_q, a_k, s_k); rows of plain samples are (1, 0, 1, 0)"""
    B, _, C = q.shape
    coef = torch.zeros(B, 4, C, dtype=q.dtype)
    coef[:, 0] = coef[:, 2] = 1
    for b, r in enumerate(ref):
        if r < 0 or r == b:
            continue
        for i, (x, eps, on) in enumerate(((q, eps_q, adain_queries), (k, eps_k, adain_keys))):
            if not on:
                continue
            mb, sb = _stats(x[b], eps)
            mr, sr = _stats(x[r], eps)
            a = sr / sb
            coef[b, 2 * i], coef[b, 2 * i + 1] = a, mr - a * mb
    return coef


def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def shared_reference(q, k, v, H, ref, scale=0.125, adain_queries=True, adain_keys=True, share_scale=1.0, share_shift=0.0,
                     q_factor=1.0):
    """q, k, v [B, S, H*64] (any float dtype; computed in it), ref B ints.  q_factor: q holds (unscaled q) * q_factor (a prescaled
    Q: scale * log2 e), and the scores are scale / q_factor times q . k; the variance epsilon of Q follows (q_factor^2 1e-5).
    -> (O [B, S, H*64], mag, coef): mag = P |[V[b]; V[r]]|, the softmax's own magnitude."""
    B, S, C = q.shape
    coef = adain_coef(q, k, ref, EPS * q_factor * q_factor, EPS, adain_queries, adain_keys)
    sc = scale / q_factor
    O, mag = torch.empty_like(q), torch.empty_like(q)
    for b, r in enumerate(ref):
        if r < 0 or r == b:
            qq, kk, vv = q[b:b + 1], k[b:b + 1], v[b:b + 1]
            s = _heads(qq, H) @ _heads(kk, H).transpose(-1, -2) * sc
        else:
            qq = (coef[b, 0] * q[b] + coef[b, 1])[None]                          # AdaIN'd queries
            ko = (coef[b, 2] * k[b] + coef[b, 3])[None]                          # AdaIN'd keys
            s_own = _heads(qq, H) @ _heads(ko, H).transpose(-1, -2) * sc
            s_ref = _heads(qq, H) @ _heads(k[r:r + 1], H).transpose(-1, -2) * (sc * share_scale) + share_shift
            s = torch.cat([s_own, s_ref], -1)
            vv = torch.cat([v[b:b + 1], v[r:r + 1]], 1)
        p = torch.softmax(s, -1)
        vh = _heads(vv, H)
        O[b] = (p @ vh)[0].transpose(0, 1).reshape(S, C)
        mag[b] = (p @ vh.abs())[0].transpose(0, 1).reshape(S, C)
    return O, mag, coef


def shared_folded(q, k, v, H, ref, coef, scale=0.125, share_scale=1.0, share_shift=0.0):
    """the same from the coefficients the way the kernel forms it: K untouched, a second query set q' o a_k and one constant
    q' . s_k per query for the own segment; the reference segment from share_scale q' and share_shift"""
    B, S, C = q.shape
    O = torch.empty_like(q)
    for b, r in enumerate(ref):
        if r < 0 or r == b:
            s = _heads(q[b:b + 1], H) @ _heads(k[b:b + 1], H).transpose(-1, -2) * scale
            vv = v[b:b + 1]
        else:
            qp = (coef[b, 0] * q[b] + coef[b, 1])[None]
            qo = qp * coef[b, 2]
            kc = (_heads(qp, H) * coef[b, 3].view(1, H, 1, 64)).sum(-1, keepdim=True)       # [1, H, S, 1]
            s_own = (_heads(qo, H) @ _heads(k[b:b + 1], H).transpose(-1, -2) + kc) * scale
            s_ref = _heads(qp * share_scale, H) @ _heads(k[r:r + 1], H).transpose(-1, -2) * scale + share_shift
            s = torch.cat([s_own, s_ref], -1)
            vv = torch.cat([v[b:b + 1], v[r:r + 1]], 1)
        O[b] = (torch.softmax(s, -1) @ _heads(vv, H))[0].transpose(0, 1).reshape(S, C)
    return O


# ---------------------------------------------------------------------------------------------- the oracle's attention layers
class StyleState:
    """what HipUNet.set_style_aligned holds: shared by every SharedAttention of a UNet"""

    def __init__(self):
        self.ref = None             # B ints; None: plain attention
        self.on = {}                # layer name -> bool (missing: on)
        self.adain_queries = self.adain_keys = True
        self.share_scale, self.share_shift = 1.0, 0.0

    def set(self, ref, on=None, adain_queries=True, adain_keys=True, share_scale=1.0, share_shift=0.0):
        self.ref, self.on = ref, dict(on or {})
        self.adain_queries, self.adain_keys = adain_queries, adain_keys
        self.share_scale, self.share_shift = share_scale, share_shift


class SharedAttention(Attention):
    def __init__(self, query_dim, heads, state, name):
        super().__init__(query_dim, heads, None)
        self.state, self.name = state, name

    def forward(self, x, ctx=None):
        st = self.state
        if ctx is not None or st.ref is None or not st.on.get(self.name, True):
            return super().forward(x, ctx)
        B, S, C = x.shape
        H = self.heads
        q, k, v = _st(self.to_q(x)), _st(self.to_k(x)), _st(self.to_v(x))
        coef = adain_coef(q, k, st.ref, EPS, EPS, st.adain_queries, st.adain_keys)
        sc = (C // H) ** -0.5
        o = torch.empty_like(q)
        for b, r in enumerate(st.ref):
            if r < 0 or r == b:
                s = _heads(q[b:b + 1], H) @ _heads(k[b:b + 1], H).transpose(-1, -2) * sc
                vv = v[b:b + 1]
            else:
                qq = _st(coef[b, 0] * q[b] + coef[b, 1])[None]                   # (q' is a bf16 MFMA operand)
                ko = (coef[b, 2] * k[b] + coef[b, 3])[None]
                s = torch.cat([_heads(qq, H) @ _heads(ko, H).transpose(-1, -2) * sc,
                               _heads(qq, H) @ _heads(k[r:r + 1], H).transpose(-1, -2) * (sc * st.share_scale) + st.share_shift], -1)
                vv = torch.cat([v[b:b + 1], v[r:r + 1]], 1)
            a = torch.softmax(s, -1)
            o[b] = (_st(a) @ _heads(vv, H))[0].transpose(0, 1).reshape(S, C)     # (P is a bf16 MFMA operand of the P.V product)
        return self.to_out[0](_st(o))


def attach_style(unet):
    """every attn1 of `unet` becomes a SharedAttention with the layer's own weights and its module name (the key of
    StyleState.on) -> the shared StyleState"""
    state = StyleState()
    named = [(n, m) for n, m in unet.named_modules() if n.endswith(".attn1")]
    for name, old in named:
        C = old.to_q.weight.shape[0]
        new = SharedAttention(C, old.heads, state, name)
        new.load_state_dict(old.state_dict())
        for p in new.parameters():
            p.requires_grad_(False)
        parent, leaf = name.rsplit(".", 1)
        setattr(unet.get_submodule(parent), leaf, new)
    return state
