"""Semantic guidance (SEGA) at SDXL 1024 x 1024: latents of C = 4 channels x 128 x 128 = groups of hw = 16384 positions, n = 1 and 2
images, K = 1, 2 and 4 edit concepts.  One JSON line, also written to profiles/sega_bench.json (--out).  Nothing here is a gate.
  kernels: per (n, K), forms alternating inside every round:
             select         `ops.abs_diff_quantile`: one workgroup per (concept, sample, channel) group, K n 4 of them
             combine        `ops.cfg_sega_combine`: the select and the elementwise pass, two launches; every concept live and warm
             cfg            `ops.cfg_combine` on [uncond | cond]: the launch plain classifier-free guidance pays
             torch_select   `torch.quantile(|d|.flatten(2), q, dim=2)` per concept, on the device
             torch_combine  the whole step's composition on the device: torch.quantile, torch.where, the weighted sum, the momentum
           select, combine, cfg: microseconds per call from device events around the replay of a captured graph of --iters
           back-to-back calls; torch_*: events around --torch-iters eager calls.  The median over --rounds; the whole measurement
           runs --repeats times and `repeat_spread` is (max - min) / min of the medians.
  forward: the full UNet (random weights, 128 x 128 latents, 77 text tokens), alternating inside every round: a batch-4 call
           ([uncond | cond | edit_1 | edit_2] of one image), the batch-2 call plain CFG pays (a context sharing the weights), and
           `sega.denoise_semantic` at K = 2 over --steps steps (DPM-Solver, warm-up 1), per step, against its UNet call alone."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops, sega
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.sampler import DPMSolverMultistep
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--torch-iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sega_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
out = {"bench": "sega", "iters": a.iters, "rounds": a.rounds, "repeats": a.repeats}
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
    return lambda: gr.replay()


def spread(vals):
    return round((max(vals) - min(vals)) / min(vals), 4)


def measure(variants, eager=()):
    """variants: name -> callable.  Those named in `eager` are timed as they are, the others from a captured graph."""
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    timed = {n: ((lambda f=f: event_us(f, a.torch_iters)) if n in eager
                 else (lambda r=captured(f, a.iters): event_us(r, 5) / a.iters)) for n, f in variants.items()}
    for t in timed.values():
        t()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, fn in timed.items():
                t[n].append(fn())
        reps.append({n: statistics.median(x) for n, x in t.items()})
    med = {n: statistics.median(r[n] for r in reps) for n in variants}
    return med, {"repeat_spread": {n: spread([r[n] for r in reps]) for n in variants},
                 "per_repeat_us": {n: [round(r[n], 2) for r in reps] for n in variants}}


g = torch.Generator().manual_seed(1)
G, MU, BETA, Q, S = 7.5, 0.1, 0.4, 0.9, 5.0
C, hw = 4, a.latent
out["kernels"] = {}
for n in (1, 2):
    for K in (1, 2, 4):
        eps = torch.randn((2 + K) * n, C, hw, hw, generator=g).to(BF).float().to(dev)       # what the UNet delivers
        eps2 = eps[:2 * n].contiguous()
        mom, tmom = torch.zeros(n, C, hw, hw, device=dev), torch.zeros(n, C, hw, hw, device=dev)
        ws = ops.sega_workspace(n, C, K, dev)
        scale, quant, weight, warm = [S] * K, [Q] * K, [1.0] * K, [1] * K
        res = torch.empty(n, C, hw, hw, device=dev)

        def diffs():
            u = eps[:n]
            return u, [S * (eps[(2 + c) * n:(3 + c) * n] - u) for c in range(K)]

        def torch_select():
            return [torch.quantile(d.abs().flatten(2), Q, dim=2) for d in diffs()[1]]

        def torch_combine():
            u, ds = diffs()
            e = torch.zeros_like(u)
            for d in ds:
                thr = torch.quantile(d.abs().flatten(2), Q, dim=2)
                e = e + 1.0 * torch.where(d.abs() >= thr[:, :, None, None], d, torch.zeros_like(d))
            used = e + MU * tmom
            tmom.mul_(BETA).add_(used, alpha=1.0 - BETA)
            return u + G * (eps[n:2 * n] - u) + used

        med, extra = measure({"select": lambda: ops.abs_diff_quantile(eps, scale, quant, weight),
                              "combine": lambda: ops.cfg_sega_combine(eps, mom, G, scale, quant, weight, warm, MU, BETA, workspace=ws, out=res),
                              "cfg": lambda: ops.cfg_combine(eps2, G),
                              "torch_select": torch_select, "torch_combine": torch_combine}, eager=("torch_select", "torch_combine"))
        thr = ops.abs_diff_quantile(eps, scale, quant, weight)
        agree = bool(torch.allclose(thr, torch.stack(torch_select()), rtol=1e-6, atol=0.0))
        out["kernels"][f"n{n}_K{K}"] = {**{f"{m}_us": round(t, 2) for m, t in med.items()}, "groups": K * n * C, "hw": hw * hw,
                                        "torch_select_over_select": round(med["torch_select"] / med["select"], 1),
                                        "torch_combine_over_combine": round(med["torch_combine"] / med["combine"], 1),
                                        "select_over_cfg": round(med["select"] / med["cfg"], 2),
                                        "combine_over_cfg": round(med["combine"] / med["cfg"], 2),
                                        "cut_agrees_with_torch": agree, "finite": bool(torch.isfinite(res).all() and torch.isfinite(mom).all()),
                                        **extra}

if not a.no_unet:
    cfg, L, K, steps = pc.sdxl_config(), 77, 2, a.steps
    unet = HipUNet(cfg, 2 + K, hw, hw, L)
    unet.init_random(1)
    unet2 = HipUNet(cfg, 2, hw, hw, L, share_weights_from=unet)
    gc = torch.Generator().manual_seed(3)
    B = 2 + K
    x = torch.randn(B, 4, hw, hw, generator=gc).to(dev)
    ehs = torch.randn(B, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(B, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * B).to(dev)}
    tt = torch.tensor([500.0] * B).to(dev)
    cut = lambda lo, hi: dict(added_cond_kwargs={k_: v_[lo:hi] for k_, v_ in added.items()})
    b4 = lambda: unet(x, tt, ehs, **cut(0, B))[0]
    b2 = lambda: unet2(x[:2], tt[:2], ehs[:2], **cut(0, 2))[0]
    lat = x[:1].clone()
    final = []

    def guided_steps():
        final[:] = [sega.denoise_semantic(unet, DPMSolverMultistep(), lat, ehs[:2], cut(0, 2)["added_cond_kwargs"], ehs[2:],
                                          cut(2, B)["added_cond_kwargs"], edit_warmup_steps=1, num_inference_steps=steps, guidance_scale=G)]

    def unet_steps():
        for _ in range(steps):
            b4()
    forms = {"b4": (b4, 1), "b2": (b2, 1), "guided_step": (guided_steps, steps), "unet_step": (unet_steps, steps)}
    for f, _ in list(forms.values()) * 2:             # warm-up: arenas, weight-prefetch sequence, code objects
        f()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.repeats):
        t = {m: [] for m in forms}
        for _ in range(a.rounds):
            for m, (f, per) in forms.items():
                f()
                torch.cuda.synchronize()
                t[m].append(event_us(f, 2) / per)
        reps.append({m: statistics.median(x_) for m, x_ in t.items()})
    med = {m: statistics.median(r[m] for r in reps) for m in forms}
    out["forward"] = {"latent": hw, "K": K, "steps": steps, **{f"{m}_ms": round(t * 1e-3, 3) for m, t in med.items()},
                      "b4_over_b2": round(med["b4"] / med["b2"], 4), "guided_step_over_unet_step": round(med["guided_step"] / med["unet_step"], 4),
                      "guided_step_minus_unet_step_us": round(med["guided_step"] - med["unet_step"], 1),
                      "repeat_spread": {m: spread([r[m] for r in reps]) for m in forms},
                      "per_repeat_ms": {m: [round(r[m] * 1e-3, 3) for r in reps] for m in forms},
                      "finite": bool(torch.isfinite(final[0]).all())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
