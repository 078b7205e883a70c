"""SHA-256 digests of the raw output bytes (and lse, where there is one) of every cross-attention op on seeded inputs, at the
smallest shapes that reach every path of csrc/attention.hip's resident-key kernels: one JSON line.  Two builds of the library
that print the same line compute the same bits:  python scripts/lib_ab.py 1 scripts/attn_digest.py
(profiles/attn_digest.json is the line of the committed sources on an MI355X.)"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import ops

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

print(json.dumps(out, sort_keys=True))
