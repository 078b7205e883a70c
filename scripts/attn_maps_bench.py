"""Cross-attention heat maps on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line, also written to
profiles/attn_maps_bench.json (--out).
  kernels: the two cross-attention shapes of that UNet (10 heads x 4096 queries, 20 heads x 1024 queries), 77 keys, two forms
           alternating inside every round:
             maps    `ops.attention_maps` with accumulate=True, as the UNet runs it
             plain   `ops.attention_fwd` over the same 77 keys: the unfused yardstick (it also reads V and writes O)
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the median
           over --rounds; the whole measurement runs --repeats times and `repeat_spread` is (max - min) / min of the medians.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents) with capture off and on, alternating, --repeats times;
           and `heat_maps` (readout of both accumulators, bicubic upsampling, clamp, mean), once per image.
Q arrives prescaled, as the UNet's to_q hands it over."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.attention_maps import heat_maps
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_maps_bench.json"))
a = ap.parse_args()
dev, BF, L = torch.device("cuda"), torch.bfloat16, 77
out = {"bench": "attn_maps", "batch": 2, "keys": L, "iters": a.iters, "rounds": a.rounds, "repeats": a.repeats}
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


def spread(vals):
    return round((max(vals) - min(vals)) / min(vals), 4)


out["kernels"] = {}
g = torch.Generator().manual_seed(1)
for H, Sq in ((10, 4096), (20, 1024)):
    B, C = 2, H * 64
    q = (torch.randn(B, Sq, C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
    k, v = (torch.randn(B, L, C, generator=g).to(dev, BF) for _ in range(2))
    acc = torch.zeros(B, L, Sq, device=dev)
    variants = {"maps": lambda: ops.attention_maps(q, k, H, q_prescaled=True, out=acc, accumulate=True),
                "plain": lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]}
    for f in variants.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    replays = {n: captured(f, a.iters) for n, f in variants.items()}
    for r in replays.values():
        r()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, r in replays.items():
                t[n].append(event_us(r, 5) / a.iters)
        reps.append({n: statistics.median(x) for n, x in t.items()})
    med = {n: statistics.median(r[n] for r in reps) for n in variants}
    out["kernels"][f"H{H}_Sq{Sq}"] = {**{f"{n}_us": round(m, 2) for n, m in med.items()},
                                      "maps_over_plain": round(med["maps"] / med["plain"], 3),
                                      "repeat_spread": {n: spread([r[n] for r in reps]) for n in variants},
                                      "per_repeat_us": {n: [round(r[n], 2) for r in reps] for n in variants}}

if not a.no_unet:
    cfg, hw = pc.sdxl_config(), a.latent
    unet = HipUNet(cfg, 2, hw, hw, L)
    unet.init_random(1)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    tt = torch.tensor([500.0, 500.0]).to(dev)
    ehs = torch.randn(2, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]

    def set_form(name):
        if name == "capture_on":
            unet.enable_attention_maps()
        else:
            unet.disable_attention_maps()
    names = ("capture_off", "capture_on")
    for n in names + names:                               # warm-up of both forms: arenas, weight-prefetch sequence, code objects
        set_form(n)
        fwd()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in names}
        for _ in range(a.unet_rounds):
            for n in names:
                set_form(n)
                fwd()
                torch.cuda.synchronize()
                t[n].append(event_us(fwd, 3))
        reps.append({n: statistics.median(x) for n, x in t.items()})
    med = {n: statistics.median(r[n] for r in reps) for n in names}
    set_form("capture_on")
    eps = fwd()
    torch.cuda.synchronize()
    read = [event_us(lambda: heat_maps(unet, do_cfg=True), 1) for _ in range(5)]
    layers = sum(n for _, n in unet.attention_maps().values())
    out["unet"] = {"latent": hw, "query_counts": unet.ip_query_counts(), "captured_layers": layers,
                   **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "on_over_off": round(med["capture_on"] / med["capture_off"], 4),
                   "us_per_captured_layer": round((med["capture_on"] - med["capture_off"]) / max(layers, 1), 2),
                   "repeat_spread": {n: spread([r[n] for r in reps]) for n in names},
                   "per_repeat_ms": {n: [round(r[n] * 1e-3, 3) for r in reps] for n in names},
                   "heat_maps_readout_ms": round(statistics.median(read) * 1e-3, 3), "finite": bool(torch.isfinite(eps).all())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
