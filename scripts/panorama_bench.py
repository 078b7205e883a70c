"""MultiDiffusion panoramas at the SDXL window: 128 x 128 latents, a 128 x 384 canvas, stride 64 (5 views), guidance batch 2 x vb.
One JSON line, also written to profiles/panorama_bench.json (--out).  Nothing here is a gate.
  kernels: per weight kind (uniform, gaussian), alternating inside every round:
             gather  `ops.views_gather` over the chunks of one step
             merge   `ops.views_merge_` over the chunks of one step (guided form, first / last flags as the loop sets them)
             torch_gather / torch_merge  the compositions doing the same work: V slices, a stack, a cat and a scale; V guidance
                     combines, V weighted adds into a value canvas and V adds into a weight canvas, a divide
           fused forms: microseconds per step's worth of launches from device events around the replay of a captured graph of
           --iters repetitions; torch forms: events around --torch-iters eager repetitions.  The median over --rounds; the whole
           measurement runs --repeats times and `repeat_spread` is (max - min) / min of the medians.  bytes: what the launches have
           to move, from the shapes (gather: crops read once, dup copies written; merge: eps read, canvas read by all chunks but
           the first and written by every chunk over its views -- by the first and the last over everything -- and T read once);
           `hbm_share` is bytes / time over the 6.3 TB/s a float4 copy reaches on this chip (8 TB/s spec).
  step:    the full UNet (random weights) at batch 2 x vb: `panorama.denoise_panorama` per step against the sum of its UNet
           calls alone, --steps DPM-Solver steps, alternating, --repeats times.
  decode:  `panorama.decode_tiled` of the canvas through a batch --tiles SDXL VAE decoder against its decoder calls alone."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops, panorama
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.sampler import DPMSolverMultistep
from pea_diffusion_amd.unet import HipUNet
from pea_diffusion_amd.vae import HipVAEDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--torch-iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--window", type=int, default=128)
ap.add_argument("--canvas-width", type=int, default=384)
ap.add_argument("--stride", type=int, default=64)
ap.add_argument("--vb", type=int, default=5)
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--tiles", type=int, default=1)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--no-vae", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
HBM_TBS = 6.3
h = w = a.window
N, C, Hc, Wc, vb, dup, G = 1, 4, a.window, a.canvas_width, a.vb, 2, 7.5
out = {"bench": "panorama", "window": a.window, "canvas": [Hc, Wc], "stride": a.stride, "vb": vb, "iters": a.iters, "rounds": a.rounds,
       "repeats": a.repeats}
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
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(iters):
            f()
    return lambda: gr.replay()


def spread(vals):
    return round((max(vals) - min(vals)) / min(vals), 4)


def measure(variants, eager=()):
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
triples = [(0, y0, x0) for y0, x0 in panorama.views(Hc, Wc, h, w, a.stride)]
chunks = [triples[k:k + vb] for k in range(0, len(triples), vb)]
x = torch.randn(N, C, Hc, Wc, generator=g).to(dev)
eps = [torch.randn(dup * vb, C, h, w, generator=g).to(dev) for _ in chunks]
model_in = torch.empty(dup * vb, C, h, w, device=dev)
canvas = torch.empty_like(x)
k_s = 0.3713
per = C * h * w * 4
out["views"], out["chunks"] = len(triples), len(chunks)
out["kernels"] = {}
for kind in ("uniform", "gaussian"):
    wy = wx = panorama.view_weights(h, kind)
    T = panorama.weight_total(triples, N, Hc, Wc, wy, wx).to(dev)
    wy = wx = wy.to(dev)
    plane = (wy[:, None] * wx[None, :]).contiguous()

    def gather():
        for ch in chunks:
            ops.views_gather(x, ch, vb, (h, w), k_s, dup, out=model_in)

    def merge():
        for ci, ch in enumerate(chunks):
            ops.views_merge_(canvas, eps[ci], ch, wy, wx, T, dup, G, first=ci == 0, last=ci == len(chunks) - 1)

    def torch_gather():
        got = []
        for ch in chunks:
            slots = list(ch) + [ch[-1]] * (vb - len(ch))
            one = torch.stack([x[n, :, y0:y0 + h, x0:x0 + w] for n, y0, x0 in slots])
            got.append(torch.cat([one] * dup) * k_s)
        return got

    def torch_merge():
        value, weight = torch.zeros_like(x), torch.zeros(N, 1, Hc, Wc, device=dev)
        for ci, ch in enumerate(chunks):
            for s, (n, y0, x0) in enumerate(ch):
                e = eps[ci][s] + G * (eps[ci][vb + s] - eps[ci][s])
                value[n, :, y0:y0 + h, x0:x0 + w] += plane * e
                weight[n, :, y0:y0 + h, x0:x0 + w] += plane
        return value / weight

    med, extra = measure({"gather": gather, "merge": merge, "torch_gather": torch_gather, "torch_merge": torch_merge},
                         eager=("torch_gather", "torch_merge"))
    gather_bytes = sum((len(ch) + dup * vb) * per for ch in chunks)
    plane_bytes = N * C * Hc * Wc * 4
    merge_bytes = sum(dup * len(ch) * per + len(ch) * per for ch in chunks)              # eps read, the views' canvas elements written
    merge_bytes += sum(len(ch) * per for ch in chunks[1:])                               # ... and read back by the later chunks
    merge_bytes += (plane_bytes if len(chunks) > 1 else 0) + N * Hc * Wc * 4             # the last chunk sweeps the canvas; T
    merge()
    out["kernels"][kind] = {**{f"{n}_us": round(m, 2) for n, m in med.items()},
                            "torch_over_gather": round(med["torch_gather"] / med["gather"], 1),
                            "torch_over_merge": round(med["torch_merge"] / med["merge"], 1),
                            "gather_bytes": gather_bytes, "merge_bytes": merge_bytes,
                            "gather_hbm_share": round(gather_bytes / (med["gather"] * 1e-6) / (HBM_TBS * 1e12), 3),
                            "merge_hbm_share": round(merge_bytes / (med["merge"] * 1e-6) / (HBM_TBS * 1e12), 3),
                            "merge_max_abs_vs_torch": float((canvas - torch_merge()).abs().max()), **extra}


def alternate(forms):
    for f in list(forms.values()) * 2:                    # warm-up: arenas, weight-prefetch sequence, code objects
        f()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in forms}
        for _ in range(a.rounds):
            for n, f in forms.items():
                t[n].append(event_us(f, 1))
        reps.append({n: statistics.median(v) for n, v in t.items()})
    return {n: statistics.median(r[n] for r in reps) for n in forms}, reps


if not a.no_unet:
    cfg, L = pc.sdxl_config(), 77
    unet = HipUNet(cfg, dup * vb, h, w, L)
    unet.init_random(1)
    gc = torch.Generator().manual_seed(3)
    ehs = torch.randn(dup * N, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(dup * N, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[h * 8, w * 8, 0, 0, h * 8, w * 8]] * (dup * N)).to(dev)}
    ehs_b = ehs.repeat_interleave(vb, 0)
    added_b = {k_: v_.repeat_interleave(vb, 0) for k_, v_ in added.items()}
    tt = torch.tensor([500.0]).to(dev)
    xin = torch.randn(dup * vb, C, h, w, generator=gc).to(dev)

    def unet_calls():
        for _ in range(a.steps * len(chunks)):
            unet(xin, tt, ehs_b, added_cond_kwargs=added_b)[0]
    forms = {"denoise_panorama": lambda: panorama.denoise_panorama(unet, DPMSolverMultistep(), x, ehs, added, num_inference_steps=a.steps,
                                                                   guidance_scale=G, stride=a.stride, weights="gaussian"),
             "unet_calls": unet_calls}
    med, reps = alternate(forms)
    pano, calls = med["denoise_panorama"] / a.steps, med["unet_calls"] / a.steps
    out["step"] = {"steps": a.steps, "unet_batch": dup * vb, "unet_calls_per_step": len(chunks), "panorama_step_ms": round(pano * 1e-3, 3),
                   "unet_calls_ms": round(calls * 1e-3, 3), "panorama_over_unet_calls": round(pano / calls, 4),
                   "panorama_minus_unet_calls_us": round(pano - calls, 1),
                   "repeat_spread": {n: spread([r[n] for r in reps]) for n in forms},
                   "per_repeat_ms": {n: [round(r[n] * 1e-3, 3) for r in reps] for n in forms},
                   "finite": bool(torch.isfinite(forms["denoise_panorama"]()).all())}
    del unet

if not a.no_vae:
    dec = HipVAEDecoder(pc.sdxl_vae_config(), a.tiles, h, w)
    dec.init_random(5)
    z = torch.randn(N, C, Hc, Wc, generator=g).to(dev)
    tile = torch.randn(a.tiles, C, h, w, generator=g).to(dev)
    n_calls = -(-len(triples) // a.tiles)

    def decoder_calls():
        for _ in range(n_calls):
            dec.decode(tile)[0]
    forms = {"decode_tiled": lambda: panorama.decode_tiled(dec, z, stride=a.stride), "decoder_calls": decoder_calls}
    med, reps = alternate(forms)
    out["decode"] = {"tiles_per_call": a.tiles, "decoder_calls": n_calls, "decode_tiled_ms": round(med["decode_tiled"] * 1e-3, 3),
                     "decoder_calls_ms": round(med["decoder_calls"] * 1e-3, 3),
                     "tiled_over_calls": round(med["decode_tiled"] / med["decoder_calls"], 4),
                     "tiled_minus_calls_us": round(med["decode_tiled"] - med["decoder_calls"], 1),
                     "repeat_spread": {n: spread([r[n] for r in reps]) for n in forms},
                     "finite": bool(torch.isfinite(forms["decode_tiled"]()).all())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
