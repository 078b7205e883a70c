"""Self-attention guidance on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line, also written to
profiles/sag_bench.json (--out).  Nothing here is a gate.
  kernels: the mid block's self-attention shape (B = 2, 20 heads, 1024 tokens), three forms alternating inside every round:
             colsum  `ops.attention_colsum`, as the UNet runs it behind the layer's ordinary launch
             plain   `ops.attention_fwd` of the same shape: the yardstick (two products, V and O; the colsum evaluates one)
             torch   the composition that materialises the probabilities: softmax(q k^T) in fp32 [B, 20, 1024, 1024], head mean,
                     column sum (from the same prescaled bf16 operands)
           colsum and plain: microseconds per call from device events around the replay of a captured graph of --iters
           back-to-back calls; torch: events around --torch-iters eager calls.  The median over --rounds; the whole measurement
           runs --repeats times and `repeat_spread` is (max - min) / min of the medians.
  degrade: `ops.sag_degrade` on 2 x 4 x 128 x 128 latents from a 32 x 32 map against its torch composition (sum of the partials,
           compare, nearest interpolate, reflect pad, two grouped convolutions, where, the two affine forms), the same way.
  step:    the full UNet (random weights, 128 x 128 latents, one image under CFG): `sag.denoise_sag` per step against
           `sampler.denoise` per step plus one batch-1 forward, --steps DPM-Solver steps each, alternating, --repeats times.
Q arrives prescaled, as the UNet's to_q hands it over."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.sag import denoise_sag, nearest_tables
from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--torch-iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sag_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
out = {"bench": "sag", "batch": 2, "iters": a.iters, "rounds": a.rounds, "repeats": a.repeats}
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
B, H, S = 2, 20, 1024
C = H * 64
q = (torch.randn(B, S, C, generator=g) * 2.0 * 0.125 * 1.4426950408889634).to(dev, BF)      # q x 2: a mask, not a coin flip
k, v = (torch.randn(B, S, C, generator=g).to(dev, BF) for _ in range(2))
_, lse = ops.attention_fwd(q, k, v, H, q_prescaled=True)
G = ops.attention_colsum_groups(B, H, S, S)
part = torch.empty(B, G, S, device=dev)


def torch_colsum():
    qh = q.float().view(B, S, H, 64).transpose(1, 2)
    kh = k.float().view(B, S, H, 64).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 0.6931471805599453, dim=-1)
    return p.mean(1).sum(1)


med, extra = measure({"colsum": lambda: ops.attention_colsum(q, k, lse, H, q_prescaled=True, out=part),
                      "plain": lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0],
                      "torch": torch_colsum}, eager=("torch",))
dev_A, ref_A = part.sum(1), torch_colsum()
out["kernels"] = {f"H{H}_S{S}": {**{f"{n}_us": round(m, 2) for n, m in med.items()}, "groups": G,
                                 "colsum_over_plain": round(med["colsum"] / med["plain"], 3),
                                 "torch_over_colsum": round(med["torch"] / med["colsum"], 1),
                                 "max_abs_vs_torch": float((dev_A - ref_A).abs().max()),
                                 "share_above_1": round(float((dev_A > 1).float().mean()), 3), **extra}}

hw = a.latent
lat, eps = 3.0 * torch.randn(B, 4, hw, hw, generator=g).to(dev), torch.randn(B, 4, hw, hw, generator=g).to(dev)
iy, ix = (t.to(dev) for t in nearest_tables(32, 32, hw, hw))
coef = (5.9905, -5.9064, 0.16693, 0.98597)
taps = torch.exp(-0.5 * torch.arange(-4, 5, dtype=torch.float64) ** 2)
taps = (taps / taps.sum()).float().to(dev)


def torch_degrade():
    c_x, c_e, o_b, o_e = coef
    A = part[:, 0]
    for j in range(1, G):
        A = A + part[:, j]
    m = F.interpolate((A > 1.0).view(B, 1, 32, 32).float(), size=(hw, hw), mode="nearest") > 0.5
    x0 = c_x * lat + c_e * eps
    p = F.pad(x0, (4, 4, 4, 4), mode="reflect")
    p = F.conv2d(p, taps.view(1, 1, 1, 9).expand(4, 1, 1, 9), groups=4)
    blur = F.conv2d(p, taps.view(1, 1, 9, 1).expand(4, 1, 9, 1), groups=4)
    return o_b * torch.where(m, blur, x0) + o_e * eps


med, extra = measure({"degrade": lambda: ops.sag_degrade(lat, eps, part, (32, 32), iy, ix, *coef), "torch": torch_degrade},
                     eager=("torch",))
out["degrade"] = {"latent": hw, **{f"{n}_us": round(m, 2) for n, m in med.items()},
                  "torch_over_degrade": round(med["torch"] / med["degrade"], 1),
                  "max_abs_vs_torch": float((ops.sag_degrade(lat, eps, part, (32, 32), iy, ix, *coef) - torch_degrade()).abs().max()), **extra}

if not a.no_unet:
    cfg, L = pc.sdxl_config(), 77
    unet = HipUNet(cfg, 2, hw, hw, L)
    unet.init_random(1)
    unet1 = HipUNet(cfg, 1, hw, hw, L, share_weights_from=unet)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, hw, hw, generator=gc).to(dev)
    ehs = torch.randn(2, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    added1 = {k_: v_[:1] for k_, v_ in added.items()}
    tt = torch.tensor([500.0]).to(dev)
    forms = {"denoise_sag": lambda: denoise_sag(unet, unet1, DPMSolverMultistep(), x, ehs, added, sag_scale=0.75,
                                                num_inference_steps=a.steps, guidance_scale=7.5),
             "denoise": lambda: denoise(unet, DPMSolverMultistep(), x, ehs, added, num_inference_steps=a.steps, guidance_scale=7.5),
             "forward_b1": lambda: unet1(x, tt, ehs[:1], added_cond_kwargs=added1)[0]}
    for f in list(forms.values()) * 2:                    # warm-up: arenas, weight-prefetch sequence, code objects
        f()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in forms}
        for _ in range(a.rounds):
            for n, f in forms.items():
                t[n].append(event_us(f, 1))
        reps.append({n: statistics.median(x_) for n, x_ in t.items()})
    med = {n: statistics.median(r[n] for r in reps) for n in forms}
    sag_step, plain_step, fwd1 = med["denoise_sag"] / a.steps, med["denoise"] / a.steps, med["forward_b1"]
    final = forms["denoise_sag"]()
    out["step"] = {"latent": hw, "steps": a.steps, "sag_step_ms": round(sag_step * 1e-3, 3), "plain_step_ms": round(plain_step * 1e-3, 3),
                   "forward_b1_ms": round(fwd1 * 1e-3, 3), "sag_over_plain_plus_forward": round(sag_step / (plain_step + fwd1), 4),
                   "sag_minus_plain_minus_forward_us": round(sag_step - plain_step - fwd1, 1),
                   "repeat_spread": {n: spread([r[n] for r in reps]) for n in forms},
                   "per_repeat_ms": {n: [round(r[n] * 1e-3, 3) for r in reps] for n in forms},
                   "finite": bool(torch.isfinite(final).all())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
