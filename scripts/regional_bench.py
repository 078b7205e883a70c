"""Regional text prompts on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line, also written to profiles/regional_bench.json
(--out).
  kernels: the two cross-attention shapes of that UNet (10 heads x 4096 queries, 20 heads x 1024 queries), regions of 77 keys:
             R2_halves     two regions, left / right halves of the picture (a wave's 32 queries lie in one of them)
             R4_quadrants  four regions, the quadrants
             R2_soft       two regions that overlap everywhere (weights 0.5 / 0.5): nothing is skipped
           and per case three forms, alternating inside every round:
             fused    `ops.attention_fwd_regions`, one launch
             unfused  the composition it replaces: R `attention_fwd` launches on the regions' rows and R weighted elementwise passes
             plain    one `attention_fwd` over 77 keys: what a cross-attention layer costs without regions
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the median
           over --rounds; per form the spread (max - min) / median.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents): the plain 77-row context, the 154-row context with two
           regions (left / right, do_cfg) and the same 154-row context as one softmax, alternating.
Q arrives prescaled, as the UNet's to_q hands it over.  Run it twice: the spread between two runs is the margin a claimed
difference has to exceed."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.regional import region_weights
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regional_bench.json"))
a = ap.parse_args()
dev, BF, LR = torch.device("cuda"), torch.bfloat16, 77
out = {"bench": "regional", "batch": 2, "keys_per_region": LR, "iters": a.iters, "rounds": a.rounds}
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


def halves(h, w):
    m = torch.zeros(h, w)
    m[:, : w // 2] = 1.0
    return [m, 1.0 - m]


def quadrants(h, w):
    ms = []
    for rows in (slice(0, h // 2), slice(h // 2, h)):
        for cols in (slice(0, w // 2), slice(w // 2, w)):
            m = torch.zeros(h, w)
            m[rows, cols] = 1.0
            ms.append(m)
    return ms


out["kernels"] = {}
g = torch.Generator().manual_seed(1)
for H, Sq in ((10, 4096), (20, 1024)):
    B, C, side = 2, H * 64, int(Sq ** 0.5)
    q = (torch.randn(B, Sq, C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
    cases = {"R2_halves": (2, region_weights(halves(8 * side, 8 * side), None, side, side)),
             "R4_quadrants": (4, region_weights(quadrants(8 * side, 8 * side), None, side, side)),
             "R2_soft": (2, region_weights([None, None], None, side, side))}
    k1, v1 = (torch.randn(B, LR, C, generator=g).to(dev, BF) for _ in range(2))
    plain = lambda: ops.attention_fwd(q, k1, v1, H, q_prescaled=True)[0]
    res = {}
    for name, (R, w) in cases.items():
        k, v = (torch.randn(B, R * LR, C, generator=g).to(dev, BF) for _ in range(2))
        w = w.to(dev)
        parts = [(k[:, r * LR:(r + 1) * LR].contiguous(), v[:, r * LR:(r + 1) * LR].contiguous(), w[:, r, :, None].to(BF)) for r in range(R)]
        fused = lambda k=k, v=v, R=R, w=w: ops.attention_fwd_regions(q, k, v, H, R, w, q_prescaled=True)

        def unfused(parts=parts):
            o = None
            for kr, vr, f in parts:                   # bf16 elementwise passes: each reads one or two O-sized tensors and writes one
                t = ops.attention_fwd(q, kr, vr, H, q_prescaled=True)[0]
                o = t * f if o is None else torch.addcmul(o, t, f)
            return o
        variants = {"fused": fused, "unfused": unfused, "plain": plain}
        for f in variants.values():
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        replays = {n: captured(f, a.iters) for n, f in variants.items()}
        for r in replays.values():
            r()
        t = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, r in replays.items():
                t[n].append(event_us(r, 5) / a.iters)
        med = {n: statistics.median(x) for n, x in t.items()}
        res[name] = {**{f"{n}_us": round(m, 2) for n, m in med.items()},
                     "fused_over_unfused": round(med["fused"] / med["unfused"], 3), "fused_over_plain": round(med["fused"] / med["plain"], 3),
                     "skipped_fraction": round(float((w == 0).float().mean()), 3),
                     "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                     "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}
    out["kernels"][f"H{H}_Sq{Sq}"] = res

if not a.no_unet:
    cfg, hw = pc.sdxl_config(), a.latent
    unet = HipUNet(cfg, 2, hw, hw, LR)
    unet.init_random(1)
    reg = HipUNet(cfg, 2, hw, hw, 2 * LR, share_weights_from=unet)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    tt = torch.tensor([500.0, 500.0]).to(dev)
    ehs2 = torch.randn(2, 2 * LR, 2048, generator=gc).to(dev, BF)
    ehs1 = ehs2[:, :LR].contiguous()
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    masks = halves(8 * hw, 8 * hw)

    def run(name):
        if name == "plain":
            return unet(x, tt, ehs1, added_cond_kwargs=added)[0]
        if name == "two_regions":
            reg.set_prompt_regions(masks, do_cfg=True)
        else:
            reg.clear_prompt_regions()
        return reg(x, tt, ehs2, added_cond_kwargs=added)[0]
    names = ("plain", "two_regions", "one_softmax_154")
    t = {n: [] for n in names}
    for n in names + names:                               # warm-up of every form: arenas, weight-prefetch sequence, code objects
        run(n)
    for _ in range(a.unet_rounds):
        for n in names:
            run(n)                                        # sets the form (the weight tables are copied outside the timed calls)
            torch.cuda.synchronize()
            f = (lambda: unet(x, tt, ehs1, added_cond_kwargs=added)[0]) if n == "plain" else (lambda: reg(x, tt, ehs2, added_cond_kwargs=added)[0])
            t[n].append(event_us(f, 3))
    eps = run("two_regions")
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, "query_counts": reg.ip_query_counts(), **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "two_regions_over_plain": round(med["two_regions"] / med["plain"], 4),
                   "two_regions_over_one_softmax_154": round(med["two_regions"] / med["one_softmax_154"], 4),
                   "finite": bool(torch.isfinite(eps).all()),
                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
