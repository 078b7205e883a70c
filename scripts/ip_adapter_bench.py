"""Image prompts (IP-Adapter) on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line.
  kernels: the two cross-attention shapes of that UNet (10 heads x 4096 queries, 20 heads x 1024 queries; 77 text keys) with
           N = 4 and 16 image keys -- the fused decoupled attention (`ops.attention_fwd_ip`), the plain `ops.attention_fwd` on the
           text keys alone, and the unfused composition of the same result (two `attention_fwd` launches and torch.add);
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls (a call
           takes the device 5-15 us, less than its enqueue from Python: uncaptured, the figure would be the host's), the median
           over --rounds, the three variants alternating inside every round.  ratios: fused / unfused (the yardstick), fused / plain (the price of the
           image branch), and the Q/O-sized tensors each form moves.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents) without and with a live image prompt, alternating,
           and the one-off `set_ip_tokens` (once per image, not per step).
Q arrives prescaled, as the UNet's to_q hands it over."""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[4, 16])
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
out = {"bench": "ip_adapter", "batch": 2, "text_keys": 77, "iters": a.iters, "rounds": a.rounds}
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


out["kernels"] = {}
g = torch.Generator().manual_seed(1)
for H, Sq in ((10, 4096), (20, 1024)):
    B, C, s = 2, H * 64, 0.6
    q = (torch.randn(B, Sq, C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
    k, v = (torch.randn(B, 77, C, generator=g).to(dev, BF) for _ in range(2))
    for N in a.tokens:
        k2, v2 = (torch.randn(B, N, C, generator=g).to(dev, BF) for _ in range(2))
        fused = lambda: ops.attention_fwd_ip(q, k, v, k2, v2, H, s, q_prescaled=True)
        plain = lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]

        def unfused():
            o1 = ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]
            o2 = ops.attention_fwd(q, k2, v2, H, q_prescaled=True)[0]
            return torch.add(o1, o2, alpha=s)      # torch's bf16 elementwise kernel: reads both, writes a third
        variants = {"fused": fused, "plain": plain, "unfused": unfused}
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
        qo = B * Sq * C * 2
        out["kernels"][f"H{H}_Sq{Sq}_N{N}"] = {
            "fused_us": round(med["fused"], 2), "plain_us": round(med["plain"], 2), "unfused_us": round(med["unfused"], 2),
            "fused_over_unfused": round(med["fused"] / med["unfused"], 3), "fused_over_plain": round(med["fused"] / med["plain"], 3),
            "fused_gbps": round(2 * qo / med["fused"] * 1e-3, 1), "qo_tensors_moved": {"fused": 2, "plain": 2, "unfused": 7},
            "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}

if not a.no_unet:
    cfg, hw, N = pc.sdxl_config(), a.latent, a.tokens[0]
    unet = HipUNet(cfg, 2, hw, hw, 77)
    unet.init_random(1)
    gd = torch.Generator(device="cuda").manual_seed(2)
    sd = {"image_proj": {"proj.weight": torch.randn(N * 2048, 1024, generator=gd, device=dev) / 32, "proj.bias": torch.zeros(N * 2048),
                         "norm.weight": torch.ones(2048), "norm.bias": torch.zeros(2048)}, "ip_adapter": {}}
    for (idx, _), (_, C) in zip(ipa.layer_keys(cfg), ipa._cross_layers(cfg)):
        for nm in ("to_k_ip", "to_v_ip"):
            sd["ip_adapter"][f"{idx}.{nm}.weight"] = torch.randn(C, 2048, generator=gd, device=dev) * 2048 ** -0.5
    ad = unet.load_ip_adapter(sd)
    del sd
    tok = ad.tokens(torch.randn(1, 1024, generator=gd, device=dev), do_cfg=True)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    tt = torch.tensor([500.0, 500.0]).to(dev)
    ehs = torch.randn(2, 77, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]
    t = {"plain": [], "image_prompt": [], "set_ip_tokens": []}
    for live in (False, True, False, True):          # warm-up of both forms: arenas, weight-prefetch sequence, code objects
        unet.set_ip_tokens(tok) if live else unet.clear_ip_tokens()
        fwd()
    for _ in range(a.unet_rounds):
        unet.clear_ip_tokens()
        t["plain"].append(event_us(fwd, 3))
        t["set_ip_tokens"].append(event_us(lambda: unet.set_ip_tokens(tok), 1))
        t["image_prompt"].append(event_us(fwd, 3))
    eps = fwd()
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, "image_tokens": N, "forward_ms": round(med["plain"] * 1e-3, 3),
                   "forward_image_prompt_ms": round(med["image_prompt"] * 1e-3, 3),
                   "image_prompt_over_plain": round(med["image_prompt"] / med["plain"], 4),
                   "set_ip_tokens_ms": round(med["set_ip_tokens"] * 1e-3, 3), "finite": bool(torch.isfinite(eps).all()),
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
print(json.dumps(out))
