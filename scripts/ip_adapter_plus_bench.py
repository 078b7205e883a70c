"""The IP-Adapter "plus" projection at the SDXL-plus shape: CFG batch 2, 20 heads, 16 latent queries, 257 image rows + the 16
latents themselves as keys.  One JSON line.
  kernels: the Resampler's attention on the operand layouts of its tape (K1 | V1 column blocks of the image rows' to_kv output
           [2, 257, 2 x 1280], Q | K2 | V2 column blocks of the latent rows' to_q | to_kv output [2, 16, 3 x 1280]; Q prescaled):
             fewq     `ops.attention_fwd_fewq`, both key sets read in place
             general  `ops.attention_fwd` over a pre-concatenated [2, 273, 2 x 1280] K | V buffer
             concat   the copy that builds that buffer (torch.cat into a preallocated output)
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the
           median over --rounds, the three alternating inside every round.  The yardstick: fewq against general + concat.
  tokens:  one `IPAdapterPlus.tokens(hidden, uncond_hidden)` call (batch 1 + its unconditional half), host enqueue included.
  unet:    one forward of the full SDXL UNet (random weights, 128 x 128 latents, batch 2) without and with 16 live image keys."""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
B, H, NQ, S = 2, 20, 16, 257
C = H * 64
out = {"bench": "ip_adapter_plus", "batch": B, "heads": H, "queries": NQ, "keys": [S, NQ], "iters": a.iters, "rounds": a.rounds}
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


# ---- the attention, on the tape's layouts
g = torch.Generator().manual_seed(1)
kv1 = torch.randn(B, S, 2 * C, generator=g).to(dev, BF)                    # to_kv(norm1(x)):        K1 | V1
qkv = torch.randn(B, NQ, 3 * C, generator=g)                               # to_q | to_kv(norm2(l)): Q | K2 | V2
qkv[..., :C] *= 0.125 * 1.4426950408889634
qkv = qkv.to(dev, BF)
q, k1, v1, k2, v2 = qkv[..., :C], kv1[..., :C], kv1[..., C:], qkv[..., C:2 * C], qkv[..., 2 * C:]
kvcat = torch.empty(B, S + NQ, 2 * C, device=dev, dtype=BF)
concat = lambda: torch.cat([kv1, qkv[..., C:]], 1, out=kvcat)
concat()
fewq = lambda: ops.attention_fwd_fewq(q, k1, v1, k2, v2, H, q_prescaled=True)
general = lambda: ops.attention_fwd(q, kvcat[..., :C], kvcat[..., C:], H, q_prescaled=True)[0]
variants = {"fewq": fewq, "general": general, "concat": concat}
diff = (fewq().float() - general().float()).abs().max().item()             # the two must agree before they are compared
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
out["kernels"] = {"fewq_us": round(med["fewq"], 2), "general_us": round(med["general"], 2), "concat_us": round(med["concat"], 2),
                  "fewq_over_general_plus_concat": round(med["fewq"] / (med["general"] + med["concat"]), 3),
                  "fewq_over_general": round(med["fewq"] / med["general"], 3), "max_abs_fewq_minus_general": round(diff, 5),
                  "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}

# ---- a whole tokens() call, then the UNet with the 16 tokens live
cfg = pc.sdxl_config()
rc = pc.sdxl_plus_resampler_config()
gd = torch.Generator(device="cuda").manual_seed(2)
sd = {"image_proj": {}, "ip_adapter": {}}
for key, shape in ipa.resampler_keys(rc).items():
    if len(shape) >= 2:
        sd["image_proj"][key] = torch.randn(shape, generator=gd, device=dev) * shape[-1] ** -0.5
    else:
        sd["image_proj"][key] = torch.ones(shape, device=dev) if key.endswith(".weight") else torch.zeros(shape, device=dev)
for (idx, _), (_, Cl) in zip(ipa.layer_keys(cfg), ipa._cross_layers(cfg)):
    for nm in ("to_k_ip", "to_v_ip"):
        sd["ip_adapter"][f"{idx}.{nm}.weight"] = torch.randn(Cl, 2048, generator=gd, device=dev) * 2048 ** -0.5
ad = ipa.IPAdapterPlus(sd, cfg)
del sd
hid, un = (torch.randn(1, S, rc.embed_dim, generator=gd, device=dev) for _ in range(2))
tokens = lambda: ad.tokens(hid, un)
for _ in range(3):
    tok = tokens()
tt = [event_us(tokens, 10) for _ in range(a.rounds)]
out["tokens"] = {"tokens_ms": round(statistics.median(tt) * 1e-3, 3), "shape": list(tok.shape), "finite": bool(torch.isfinite(tok).all()),
                 "n_params": ipa.resampler_plan(rc, 2, S)["n_params"], "all_rounds_ms": [round(x * 1e-3, 3) for x in tt]}

if not a.no_unet:
    hw = a.latent
    unet = HipUNet(cfg, 2, hw, hw, 77)
    unet.init_random(1)
    unet.load_ip_adapter(ad)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    ts = torch.tensor([500.0, 500.0]).to(dev)
    ehs = torch.randn(2, 77, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    fwd = lambda: unet(x, ts, ehs, added_cond_kwargs=added)[0]
    t = {"plain": [], "image_prompt": []}
    for live in (False, True, False, True):          # warm-up of both forms: arenas, weight-prefetch sequence, code objects
        unet.set_ip_tokens(tok) if live else unet.clear_ip_tokens()
        fwd()
    for _ in range(a.unet_rounds):
        unet.clear_ip_tokens()
        t["plain"].append(event_us(fwd, 3))
        unet.set_ip_tokens(tok)
        t["image_prompt"].append(event_us(fwd, 3))
    eps = fwd()
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, "image_tokens": NQ, "forward_ms": round(med["plain"] * 1e-3, 3),
                   "forward_image_prompt_ms": round(med["image_prompt"] * 1e-3, 3),
                   "image_prompt_over_plain": round(med["image_prompt"] / med["plain"], 4), "finite": bool(torch.isfinite(eps).all()),
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
print(json.dumps(out))
