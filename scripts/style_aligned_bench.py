"""StyleAligned shared self-attention on the SDXL UNet at 1024 x 1024, N = 2 prompts, CFG batch 4 with one reference per half
(ref = [-1, 0, -1, 2]).  One JSON line, also written to profiles/style_aligned_bench.json (--out).
  kernels: the two self-attention shapes of that UNet (10 heads x 4096 tokens, 20 heads x 1024 tokens), three forms alternating
           inside every round:
             shared   (a) `ops.attn_adain_coef` + `ops.attention_fwd_shared`: the coefficient launches and the one shared launch
             unfused  (b) the composition from existing pieces: AdaIN of Q and K as torch ops, `torch.cat` of K and V to 2 S rows per
                      target, `ops.attention_fwd` over 2 S keys for the targets and over S keys for the references
             plain    (c) one `ops.attention_fwd` on the same batch: what the layer costs without sharing
           and the coefficient launches alone (coef).  Microseconds per call from device events around the replay of a captured
           graph of --iters back-to-back calls, the median over --rounds; per form the spread (max - min) / median.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents, batch 4) without and with sharing in all 70
           self-attention layers, alternating.
Q arrives prescaled, as the UNet's to_q hands it over.  Run it twice: the spread between two runs is the margin a claimed
difference has to exceed."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "style_aligned_bench.json"))
a = ap.parse_args()
dev, BF, L, B = torch.device("cuda"), torch.bfloat16, 77, 4
REF = [-1, 0, -1, 2]
ALPHA = 0.125 * 1.4426950408889634
out = {"bench": "style_aligned", "batch": B, "ref": REF, "iters": a.iters, "rounds": a.rounds}
tf, mhz = ctypes.c_double(), ctypes.c_double()
if lib().pea_probe_mfma_peak(0.5, 0, ctypes.byref(tf), ctypes.byref(mhz), stream_ptr()) == 0:
    out["clock_mhz"] = round(mhz.value)           # in-kernel clock under sustained MFMA load


def event_us(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def captured(f, iters):
    """`iters` calls of f as one graph (a single chain of kernels); its replay is what gets timed"""
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(iters):
            f()
    return gr.replay


def adain(x, xr, eps):
    """x onto xr's per-channel statistics over the tokens, as torch ops on bf16 rows (fp32 inside)"""
    x, xr = x.float(), xr.float()
    mu, mur = x.mean(1, keepdim=True), xr.mean(1, keepdim=True)
    sg, sgr = (x.var(1, keepdim=True) + eps).sqrt(), (xr.var(1, keepdim=True) + eps).sqrt()
    return ((x - mu) / sg * sgr + mur).to(BF)


out["kernels"] = {}
g = torch.Generator().manual_seed(1)
tg, rf = [b for b in range(B) if REF[b] >= 0], [b for b in range(B) if REF[b] < 0]
tr = [REF[b] for b in tg]
assert tg == [1, 3] and tr == rf == [0, 2]            # below: targets are the odd samples, their references the even ones (views)
for H, S in ((10, 4096), (20, 1024)):
    C = H * 64
    q = (torch.randn(B, S, C, generator=g) * ALPHA).to(dev, BF)
    k, v = (torch.randn(B, S, C, generator=g).to(dev, BF) for _ in range(2))
    coef_buf = torch.zeros(B, 4, C, device=dev)
    plain = lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]
    coef = lambda: ops.attn_adain_coef(q, k, H, REF, q_prescaled=True, out=coef_buf)
    shared = lambda: ops.attention_fwd_shared(q, k, v, H, REF, coef(), q_prescaled=True)

    def unfused():
        qt = adain(q[1::2], q[0::2], 1e-5 * ALPHA * ALPHA)
        kt = adain(k[1::2], k[0::2], 1e-5)
        k2, v2 = torch.cat([kt, k[0::2]], 1), torch.cat([v[1::2], v[0::2]], 1)
        o_t = ops.attention_fwd(qt, k2, v2, H, q_prescaled=True)[0]
        o_r = ops.attention_fwd(q[0::2].contiguous(), k[0::2].contiguous(), v[0::2].contiguous(), H, q_prescaled=True)[0]
        return o_t, o_r
    o_s, (o_t, o_r) = shared(), unfused()
    agree = float(((o_s[tg].float() - o_t.float()).pow(2).sum().sqrt() / o_t.float().pow(2).sum().sqrt()).item())
    variants = {"shared": shared, "unfused": unfused, "plain": plain, "coef": coef}
    for f in variants.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    replays = {n: captured(f, a.iters) for n, f in variants.items()}
    for r in replays.values():
        r()
    t = {n: [] for n in variants}
    for _ in range(a.rounds):
        for n, r in replays.items():
            t[n].append(event_us(r, 3) / a.iters)
    med = {n: statistics.median(x) for n, x in t.items()}
    out["kernels"][f"H{H}_S{S}"] = {**{f"{n}_us": round(m, 2) for n, m in med.items()},
                                   "shared_over_unfused": round(med["shared"] / med["unfused"], 3),
                                   "shared_over_plain": round(med["shared"] / med["plain"], 3),
                                   "shared_vs_unfused_rel_l2": round(agree, 5),
                                   "references_keep_bits": bool(torch.equal(o_s[rf], o_r)),
                                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                                   "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}

if not a.no_unet:
    cfg, hw = pc.sdxl_config(), a.latent
    unet = HipUNet(cfg, B, hw, hw, L)
    unet.init_random(1)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(B, 4, hw, hw, generator=gc).to(dev)
    tt = torch.full((B,), 500.0).to(dev)
    ehs = torch.randn(B, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(B, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * B).to(dev)}
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]

    def form(name):
        if name == "plain":
            unet.clear_style_aligned()
        else:
            unet.set_style_aligned(do_cfg=True)
    names = ("plain", "shared")
    t = {n: [] for n in names}
    eps = {}
    for n in names + names:                               # warm-up of every form: arenas, weight-prefetch sequence, code objects
        form(n)
        eps[n] = fwd().clone()
    for _ in range(a.unet_rounds):
        for n in names:
            form(n)                                       # (the buffers are allocated outside the timed calls)
            torch.cuda.synchronize()
            t[n].append(event_us(fwd, 3))
    unet.clear_style_aligned()
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "shared_over_plain": round(med["shared"] / med["plain"], 4),
                   "finite": bool(all(torch.isfinite(e).all() for e in eps.values())),
                   "references_keep_bits": bool(torch.equal(eps["shared"][0::2], eps["plain"][0::2])),
                   "targets_move": bool(not torch.equal(eps["shared"][1], eps["plain"][1]) and not torch.equal(eps["shared"][3], eps["plain"][3])),
                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
