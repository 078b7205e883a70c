"""SHA-256 digests of the raw output bytes (and lse, where there is one) of every attention op on seeded inputs, at the
smallest shapes that reach every path of csrc/attention.hip's resident-key and streamed-key kernels: one JSON line.  Two builds of the library
that print the same line compute the same bits:  python scripts/lib_ab.py 1 scripts/attn_digest.py
(profiles/attn_digest.json is the line of the committed sources on an MI355X.)"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib

BF = torch.bfloat16
B, H, SQ = 2, 3, 130                                     # two 128-query units, the second one ragged
out = {}


def rnd(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def put(name, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    assert name not in out, name
    out[name] = h.hexdigest()


def kvl(on, Skv, n=B):
    return torch.tensor([Skv, max(1, Skv - 7)][:n], dtype=torch.int32).cuda() if on else None


q = rnd(B, SQ, H * 64, seed=1, scale=0.5)
for Skv in (20, 33, 77, 128):                            # KB = 1 .. 4
    k, v = rnd(B, Skv, H * 64, seed=2), rnd(B, Skv, H * 64, seed=3)
    for pre in (False, True):
        put(f"fwd/{Skv}/pre{int(pre)}", *ops.attention_fwd(q, k, v, H, q_prescaled=pre))
        put(f"fwd/{Skv}/pre{int(pre)}/kv_len", *ops.attention_fwd_text(q, k, v, H, q_prescaled=pre, kv_len=kvl(True, Skv)))
        for n2 in (4, 20):
            k2, v2 = rnd(B, n2, H * 64, seed=4), rnd(B, n2, H * 64, seed=5)
            m = [rnd(B, SQ, seed=6, dtype=torch.float32).abs(), rnd(1, SQ, seed=7, dtype=torch.float32), rnd(B, SQ, seed=8, dtype=torch.float32)]
            for kl in (False, True):
                tag = f"{Skv}/{n2}/pre{int(pre)}/kv{int(kl)}"
                put(f"ip/{tag}", *ops.attention_fwd_ip(q, k, v, k2, v2, H, 0.6, q_prescaled=pre, kv_len=kvl(kl, Skv), want_lse=True))
                put(f"ipn1/{tag}", *ops.attention_fwd_ipn(q, k, v, k2, v2, H, [n2], [0.7], [m[0]], q_prescaled=pre, kv_len=kvl(kl, Skv),
                                                         want_lse=True))
                sets = [1, 1, n2 - 2] if n2 == 4 else [4, 4, n2 - 8]
                put(f"ipn3/{tag}", *ops.attention_fwd_ipn(q, k, v, k2, v2, H, sets, [0.7, 0.5, 1.1], m, q_prescaled=pre, kv_len=kvl(kl, Skv),
                                                         want_lse=True))

for R, Lr in ((2, 77), (4, 33), (4, 96)):
    k, v = rnd(B, R * Lr, H * 64, seed=12), rnd(B, R * Lr, H * 64, seed=13)
    w = rnd(B, R, SQ, seed=14, dtype=torch.float32).abs()
    w[:, 0, :64] = 0.0                                   # a wave that skips region 0, and one (rows 96..127 of sample 1) with nothing left
    w[1, :, 96:128] = 0.0
    for pre in (False, True):
        put(f"regions/{R}x{Lr}/pre{int(pre)}", ops.attention_fwd_regions(q, k, v, H, R, w, q_prescaled=pre))

H9 = 9                                                   # nine heads over eight waves: wave 0 runs two
q9 = rnd(B, SQ, H9 * 64, seed=21, scale=0.5)
for Skv in (20, 33, 77, 128):
    k9 = rnd(B, Skv, H9 * 64, seed=22)
    for pre in (False, True):
        for kl in (False, True):
            tag = f"maps/{Skv}/pre{int(pre)}/kv{int(kl)}"
            mp = ops.attention_maps(q9, k9, H9, q_prescaled=pre, kv_len=kvl(kl, Skv))
            put(tag, mp)
            buf = rnd(B * Skv * SQ, seed=23, dtype=torch.float32)
            put(tag + "/accumulate", ops.attention_maps(q9, k9, H9, q_prescaled=pre, kv_len=kvl(kl, Skv), out=buf, accumulate=True))

for Skv in (20, 40, 77):
    k, v = rnd(B, Skv, H * 64, seed=31), rnd(B, Skv, H * 64, seed=32)
    ldm = (Skv + 7) // 8 * 8
    Mt = rnd(B, Skv, ldm, seed=33, scale=0.3)
    c, d = rnd(B, Skv, seed=34, dtype=torch.float32), rnd(B, Skv, seed=35, dtype=torch.float32)
    for pre in (False, True):
        put(f"edit/{Skv}/pre{int(pre)}", ops.attention_fwd_edit(q, k, v, H, (-1, 0), Mt, c, d, q_prescaled=pre))

ks, vs = rnd(B, SQ, H * 64, seed=41), rnd(B, SQ, H * 64, seed=42)
for pre in (False, True):
    coef = ops.attn_adain_coef(q, ks, H, (-1, 0), q_prescaled=pre)
    put(f"shared/pre{int(pre)}", ops.attention_fwd_shared(q, ks, vs, H, (-1, 0), coef, q_prescaled=pre, shared_score_scale=0.9,
                                                         shared_score_shift=-0.25))

qb = rnd(B, 256, H * 64, seed=51, scale=0.5)
for Skv in (20, 77, 96, 128):                            # the three one-pass backward kernels: v1 (KB 1, 4), v3, v2
    k, v = rnd(B, Skv, H * 64, seed=52), rnd(B, Skv, H * 64, seed=53)
    for pre in (False, True):
        o, lse = ops.attention_fwd(qb, k, v, H, q_prescaled=pre)
        do = rnd(B, 256, H * 64, seed=54)
        put(f"bwd/{Skv}/pre{int(pre)}", *ops.attention_bwd(qb, k, v, o, do, lse, H, q_prescaled=pre))

# ---- the streamed-key kernels (K / V or Q / dO through the 2-deep LDS-DMA ring): attn_q_kernel, attn_dkv_kernel, attn_bwd_fused_kernel,
# attn_shared_kernel, attn_colsum_kernel.  tr 0: the gathering instances; fused 0: dQ and dK / dV as two launches.
def switches(tr=1, fused=1):
    lib().pea_debug_set_attn_tr(tr)
    lib().pea_debug_set_attn_fused_bwd(fused)


try:
    for Skv in (130, 200):                               # 130: three key tiles, the last one holding 2 keys
        for nd in (1, 2, 3):
            D = 64 * nd
            qs, k, v = rnd(B, SQ, H * D, seed=61, scale=0.5), rnd(B, Skv, H * D, seed=62), rnd(B, Skv, H * D, seed=63)
            for pre, tr in ((0, 1), (0, 0), (1, 1)):
                switches(tr)
                put(f"self_fwd/{Skv}/nd{nd}/pre{pre}/tr{tr}", *ops.attention_fwd(qs, k, v, H, q_prescaled=bool(pre)))
    switches()

    S = SQ                                               # the text instance: causal, per-sample key counts (60: a whole tile masked), bias
    qs, k, v = rnd(B, S, H * 64, seed=64, scale=0.5), rnd(B, S, H * 64, seed=65), rnd(B, S, H * 64, seed=66)
    kl = torch.tensor([130, 60], dtype=torch.int32).cuda()
    bias = rnd(H, S, ops.attention_bias_pitch(S), seed=67, dtype=torch.float32)
    for pre in (False, True):
        for tag, kw in (("causal", dict(causal=True)), ("kv_len", dict(kv_len=kl)), ("bias", dict(bias=bias)),
                        ("causal_kv_len", dict(causal=True, kv_len=kl))):
            put(f"text/{tag}/pre{int(pre)}", *ops.attention_fwd_text(qs, k, v, H, q_prescaled=pre, **kw))

    SB = 132                                             # not 130: the backward launcher's shape check wants Sq % 4 == 0
    # (csrc/attention.hip, "attention bwd: Sq=%d must be a multiple of 4").  The masked backward runs at nd 1 / tr 1 only: the key-count
    # mask is the same text in every instantiation, and nd / tr are covered by the unmasked cases beside it.
    for Skv in (SB, 200):
        for nd in (1, 2, 3):
            D = 64 * nd
            qs, k, v = rnd(B, SB, H * D, seed=71, scale=0.5), rnd(B, Skv, H * D, seed=72), rnd(B, Skv, H * D, seed=73)
            do = rnd(B, SB, H * D, seed=74)
            for pre, tr in ((0, 1), (0, 0), (1, 1)):
                for fused in (1, 0):
                    switches(tr, fused)
                    o, lse = ops.attention_fwd(qs, k, v, H, q_prescaled=bool(pre))
                    put(f"self_bwd/{Skv}/nd{nd}/pre{pre}/tr{tr}/fused{fused}", *ops.attention_bwd(qs, k, v, o, do, lse, H, q_prescaled=bool(pre)))
                    if nd == 1 and tr == 1:
                        klb = torch.tensor([Skv, 60], dtype=torch.int32).cuda()
                        o, lse = ops.attention_fwd_text(qs, k, v, H, q_prescaled=bool(pre), kv_len=klb)
                        for scr in (True, False):
                            put(f"self_bwd_masked/{Skv}/pre{pre}/fused{fused}/scratch{int(scr)}",
                                *ops.attention_bwd_masked(qs, k, v, o, do, lse, H, q_prescaled=bool(pre), kv_len=klb, use_scratch=scr))
    switches()

    # split dK / dV: head width 128 is never resident-key, so the query-range splits reach the fp32 partials and the reduce
    assert lib().pea_op_attention_bwd_scratch_bytes(B, H, 640, 77, 2) > 0
    qs, k, v, do = rnd(B, 640, H * 128, seed=75, scale=0.5), rnd(B, 77, H * 128, seed=76), rnd(B, 77, H * 128, seed=77), rnd(B, 640, H * 128, seed=78)
    for pre in (False, True):
        o, lse = ops.attention_fwd(qs, k, v, H, q_prescaled=pre)
        for fused in (1, 0):
            switches(1, fused)
            put(f"split_bwd/pre{int(pre)}/fused{fused}", *ops.attention_bwd(qs, k, v, o, do, lse, H, q_prescaled=pre))
    switches()
finally:
    switches()

for pre in (False, True):
    coef = ops.attn_adain_coef(q, ks, H, (-1, 0), q_prescaled=pre, adain_queries=False, adain_keys=False)
    put(f"shared/noadain/pre{int(pre)}", ops.attention_fwd_shared(q, ks, vs, H, (-1, 0), coef, q_prescaled=pre, shared_score_scale=0.9,
                                                                 shared_score_shift=-0.25))
    put(f"shared/plain/pre{int(pre)}", ops.attention_fwd_shared(q, ks, vs, H, (-1, -1), None, q_prescaled=pre))
    q3, k3, v3 = rnd(3, 364, H * 64, seed=43, scale=0.5), rnd(3, 364, H * 64, seed=44), rnd(3, 364, H * 64, seed=45)
    coef = ops.attn_adain_coef(q3, k3, H, (-1, 0, 0), q_prescaled=pre)
    put(f"shared/364/pre{int(pre)}", ops.attention_fwd_shared(q3, k3, v3, H, (-1, 0, 0), coef, q_prescaled=pre, shared_score_scale=0.9,
                                                             shared_score_shift=-0.25))

# column sums behind attention_fwd's lse.  330 queries: two stages of four tiles, the last tile ragged.  At these sizes every head
# group holds one head (the launch cuts the heads until the chip is full); 4100 keys x 2 samples is the smallest problem whose
# groups hold two.
for Hc, Sq, Skv in ((H, SQ, SQ), (9, 330, 330), (9, 330, 4100)):
    qc, kc, vc = rnd(B, Sq, Hc * 64, seed=81, scale=0.5), rnd(B, Skv, Hc * 64, seed=82), rnd(B, Skv, Hc * 64, seed=83)
    for pre in ((False, True) if Hc == H else (False,)):
        lse = ops.attention_fwd(qc, kc, vc, Hc, q_prescaled=pre)[1]
        put(f"colsum/{Hc}/{Sq}/{Skv}/pre{int(pre)}", ops.attention_colsum(qc, kc, lse, Hc, q_prescaled=pre))

print(json.dumps(out, sort_keys=True))
