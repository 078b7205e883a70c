"""Test infrastructure: masked attention in plain torch, independent of pea_diffusion_amd, and the cases the mask tests share.

  attn_mask_ref     attention per head in the dtype of its inputs (fp32 in the GPU tests, float64 against SDPA) with ONE additive
                    mask built from `causal` (key index <= query index), `kv_len` (keys >= kv_len[b] of sample b are cut) and a
                    natural-log score bias [H][Sq][Skv] shared by the batch -> (O [B,Sq,H*64], lse [B,H,Sq]).  Gradients come
                    from autograd: a cut key has P = 0, so its dK / dV rows are exact zeros.
  additive_mask     that mask alone, [B|1, H|1, Sq, Skv], as F.scaled_dot_product_attention(attn_mask=...) takes it
  FWD_CASES / BWD_CASES   the parametrised cases of tests/test_attn_mask_gpu.py; tests/test_attn_mask_cpu.py checks on each the
                    conditions the GPU tests rely on (counts in 1..Skv, the dispatch conditions of the kernel form a case is
                    meant to reach, the share of ill-conditioned query rows)
  fwd_inputs / bwd_inputs   the bf16 inputs of a case (torch.Generator seeds: the same tensors on every machine)
"""
import math

import torch

BF = torch.bfloat16
LOG2E = math.log2(math.e)
HARD_P = 0.9          # a query row whose largest softmax weight exceeds this is ill-conditioned in bf16 (see hard_rows)
HARD_SHARE = 0.30     # at most this share of a case's query rows may be such rows


def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def additive_mask(Sq, Skv, causal=False, kv_len=None, bias=None, dtype=torch.float32):
    """0 / -inf (plus the bias) per (sample, head, query, key); None when nothing is masked or added"""
    m = None
    if causal:
        m = torch.full((Sq, Skv), float("-inf"), dtype=dtype).triu(1)[None, None]
    if kv_len is not None:
        cut = torch.arange(Skv)[None, :] >= torch.as_tensor(kv_len)[:, None]                    # [B, Skv]
        pad = torch.zeros(cut.shape, dtype=dtype).masked_fill(cut, float("-inf"))[:, None, None, :]
        m = pad if m is None else m + pad
    if bias is not None:
        m = bias.to(dtype)[None] if m is None else m + bias.to(dtype)[None]
    return m


def attn_mask_ref(q, k, v, H, scale, causal=False, kv_len=None, bias=None):
    """q [B,Sq,H*64], k / v [B,Skv,H*64] (any float dtype; leaf tensors for autograd) -> (O [B,Sq,H*64], lse [B,H,Sq])"""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * scale
    m = additive_mask(Sq, Skv, causal, kv_len, bias, dtype=s.dtype)
    if m is not None:
        s = s + m
    o = (torch.softmax(s, -1) @ _heads(v, H)).transpose(1, 2).reshape(B, Sq, C)
    return o, torch.logsumexp(s, -1)


def softmax_peak(q, k, H, scale, kv_len=None):
    """(largest softmax weight, its key) per (sample, head, query) of the kv_len-masked attention"""
    with torch.no_grad():
        s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * scale
        m = additive_mask(q.shape[1], k.shape[1], False, kv_len, None, dtype=s.dtype)
        p = torch.softmax(s if m is None else s + m, -1)
        return p.max(-1)


# ---------------------------------------------------------------------------------------------- forward cases
# kernel: which forward launch_attention_fwd picks (attention.hip, attn_decide_fwd): the resident-key kernel xattn_fwd_kernel needs no
# causal mask, no bias, Sq >= 128 and Skv <= 128; everything else that is masked or biased runs attn_q_kernel<0, true, 1, true>
FWD_CASES = [
    dict(id="xattn-3blocks", kernel="xattn", B=4, H=2, Sq=200, Skv=77, kv_len=[77, 33, 32, 1]),
    dict(id="xattn-4blocks", kernel="xattn", B=4, H=1, Sq=128, Skv=128, kv_len=[128, 97, 96, 65]),
    dict(id="xattn-2blocks", kernel="xattn", B=3, H=2, Sq=132, Skv=40, kv_len=[40, 31, 5]),
    dict(id="text-trailing-tiles", kernel="text", B=4, H=2, Sq=52, Skv=200, kv_len=[200, 129, 64, 5]),
    dict(id="text-200keys", kernel="text", B=3, H=1, Sq=200, Skv=200, kv_len=[65, 64, 63]),
    dict(id="text-causal-padded", kernel="text", B=3, H=2, Sq=200, Skv=200, kv_len=[200, 130, 7], causal=True),
    dict(id="text-causal", kernel="text", B=1, H=2, Sq=130, Skv=130, causal=True),
    dict(id="bias-pitch128", kernel="text", B=3, H=3, Sq=77, Skv=77, kv_len=[77, 68, 1], bias=True),
    dict(id="bias-nopad", kernel="text", B=2, H=2, Sq=64, Skv=64, kv_len=[64, 40], bias=True),
    dict(id="bias-pitch192", kernel="text", B=2, H=2, Sq=130, Skv=130, bias=True),
    dict(id="bias-causal", kernel="text", B=1, H=2, Sq=77, Skv=77, bias=True, causal=True),
]
BIAS_PAD = 1e30       # what the columns Skv .. pitch of the bias hold: finite, and fatal to the softmax if one leaked


def bias_pitch(Skv):
    return (Skv + 63) // 64 * 64


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def case_scale(case):
    """softmax scale: head_dim^-0.5, or 1 with a bias (T5 does not scale its scores)"""
    return 1.0 if case.get("bias") else 0.125


def fwd_inputs(case, prescaled):
    """-> q, k, v (bf16), q_ref (fp32, what q stands for: q' / (scale log2 e) when prescaled), bias_nat ([H,Sq,Skv] fp32 or None).
    Unit-scale inputs; with a bias Q is drawn at 0.125 so that scale 1 leaves the logits the size the tolerances were set for."""
    B, H, Sq, Skv = case["B"], case["H"], case["Sq"], case["Skv"]
    scale = case_scale(case)
    q = _rand(B, Sq, H * 64, seed=1, scale=0.125 if case.get("bias") else 1.0)
    k, v = _rand(B, Skv, H * 64, seed=2), _rand(B, Skv, H * 64, seed=3)
    alpha = scale * LOG2E
    if prescaled:
        q = (q.float() * alpha).to(BF)                 # any bf16 tensor is a valid Q'
    q_ref = q.float() / alpha if prescaled else q.float()
    bias_nat = None
    if case.get("bias"):
        g = torch.Generator().manual_seed(7)
        bias_nat = torch.randn(H, Sq, Skv, generator=g) * 1.5
    return q, k, v, q_ref, bias_nat


def padded_log2_bias(bias_nat):
    """the bias as the kernel reads it: x log2(e), rows padded to whole 64-key tiles with BIAS_PAD"""
    H, Sq, Skv = bias_nat.shape
    out = torch.full((H, Sq, bias_pitch(Skv)), BIAS_PAD, dtype=torch.float32)
    out[..., :Skv] = bias_nat * LOG2E
    return out


# ---------------------------------------------------------------------------------------------- backward cases
# A form is (one-pass kernel selector for pea_debug_set_xattn_bwd_v2 or None, fused single launch, scratch passed, gradients,
# transpose reads or pea_debug_set_attn_tr(0)).
# kernel: what launch_attention_bwd picks for it (attention.hip, attn_decide_bwd / attention_bwd_nsplit):
#   <= 128 keys and all three gradients -> one-pass: selector 3 = xattn_bwd3_kernel for 33..80 keys, xattn_bwd2_kernel for 81..96,
#   xattn_bwd_kernel otherwise; 2 = xattn_bwd2_kernel for 33..96; 0 = xattn_bwd_kernel.  With the scratch and Sq >= 512 they write
#   fp32 partials per query split and attn_dkv_reduce_kernel sums them.
#   > 128 keys -> attn_bwd_fused_kernel (attn_q_body + attn_dkv_body in one grid), or attn_q_kernel<1> then attn_dkv_kernel.
#   dK/dV only -> attn_delta_kernel + attn_dkv_kernel (+ reduce with the scratch); dQ only -> attn_q_kernel<1>.
def _form(id, kernel, ver=None, fused=1, scratch=False, grads="all", tr=1):
    return dict(id=id, kernel=kernel, ver=ver, fused=fused, scratch=scratch, grads=grads, tr=tr)


_ONE_PASS_77 = [("v3", "xattn_bwd3", 3), ("v2", "xattn_bwd2", 2), ("v1", "xattn_bwd", 0)]
BWD_CASES = [
    dict(id="x77", B=4, H=2, Sq=260, Skv=77, kv_len=[77, 64, 33, 1],
         forms=[_form(n, kn, ver=ver) for n, kn, ver in _ONE_PASS_77]),
    dict(id="x77-split", B=4, H=2, Sq=520, Skv=77, kv_len=[77, 64, 33, 1],
         forms=[_form(n + ("-scratch" if sc else "-null"), kn, ver=ver, scratch=sc) for n, kn, ver in _ONE_PASS_77
                for sc in (True, False)]),
    dict(id="x96", B=3, H=2, Sq=260, Skv=96, kv_len=[96, 65, 64],
         forms=[_form("v2", "xattn_bwd2", ver=3), _form("v1", "xattn_bwd", ver=0)]),
    dict(id="x128", B=4, H=2, Sq=260, Skv=128, kv_len=[128, 97, 96, 32], forms=[_form("v1", "xattn_bwd", ver=3)]),
    dict(id="x20", B=2, H=2, Sq=260, Skv=20, kv_len=[20, 3], forms=[_form("v1", "xattn_bwd", ver=3)]),
    dict(id="g200", B=4, H=2, Sq=260, Skv=200, kv_len=[200, 129, 128, 65],
         forms=[_form("fused", "general-fused", fused=1), _form("two-launch", "general-split", fused=0),
                _form("two-launch-gather", "general-split", fused=0, tr=0)]),      # (tr=0: pea_debug_set_attn_tr, the gathering instances)
    dict(id="first-layer", B=4, H=2, Sq=520, Skv=77, kv_len=[77, 64, 33, 1],
         forms=[_form("dkv-scratch", "dkv", scratch=True, grads="dkv"), _form("dkv-null", "dkv", grads="dkv"),
                _form("dq", "dq", grads="dq")]),
]
BWD_PARAMS = [(c, f) for c in BWD_CASES for f in c["forms"]]


def one_pass_kernel(ver, Skv):
    """the one-pass kernel pea_debug_set_xattn_bwd_v2(ver) selects at Skv <= 128 keys (attn_decide_bwd)"""
    if ver not in (0, 2) and 32 < Skv <= 80:
        return "xattn_bwd3"
    if ver != 0 and 32 < Skv <= 96:
        return "xattn_bwd2"
    return "xattn_bwd"


def bwd_inputs(case, prescaled):
    """-> q, k, v, do (bf16) and q_ref (fp32), as tests/test_ops_gpu.py::test_attention_fwd_bwd draws them"""
    B, H, Sq, Skv = case["B"], case["H"], case["Sq"], case["Skv"]
    q, k, v = _rand(B, Sq, H * 64, seed=1), _rand(B, Skv, H * 64, seed=2), _rand(B, Skv, H * 64, seed=3)
    do = _rand(B, Sq, H * 64, seed=4)
    alpha = 0.125 * LOG2E
    if prescaled:
        q = (q.float() * alpha).to(BF)
    q_ref = q.float() / alpha if prescaled else q.float()
    return q, k, v, do, q_ref


def hard_rows(case, prescaled):
    """-> (hard [B,H,Sq] bool, captured [B,H,Skv] bool).  A query whose softmax sits on one key (P > HARD_P there) has
    dS = P (dP - delta) cancelling to rounding level, so its dQ row is ill-conditioned in ANY bf16 implementation, and so is the
    dK row of the key that captures it (tests/test_ops_gpu.py::test_attention_softmax_spike)."""
    q, k, v, do, q_ref = bwd_inputs(case, prescaled)
    pmax, arg = softmax_peak(q_ref, k.float(), case["H"], 0.125, case["kv_len"])
    hard = pmax > HARD_P
    count = torch.zeros(case["B"], case["H"], case["Skv"], dtype=torch.int64)
    count.scatter_add_(2, arg, hard.to(torch.int64))   # a key is captured if ANY of the queries that peak on it is hard
    return hard, count > 0
