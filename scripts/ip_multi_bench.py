"""Several image prompts (two IP-Adapters, 4 + 16 tokens) on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line, also
written to profiles/ip_multi_bench.json (--out).
  kernels: the two cross-attention shapes of that UNet (10 heads x 4096 queries, 20 heads x 1024 queries; 77 text keys), sets (4, 16):
             a  multi         `ops.attention_fwd_ipn` without masks
             b  multi_masked  ... with one mask shared by the batch (set 0) and one per sample (set 1)
             c  one_set       the one-set `ops.attention_fwd_ip` with 16 image keys: the yardstick for a and b (what does the packed
                              block cost beyond one set's softmax?)
             d  unfused       the composition the fused launch replaces: three `attention_fwd` launches (text, set 0, set 1) and the
                              weighted, masked adds in torch -- the yardstick for usefulness
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the median
           over --rounds with the four variants alternating inside every round; per variant the spread (max - min) / median.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents) with no, one (16 tokens, no mask: the one-set launch) and two
           (4 + 16 tokens, the first masked) live prompts, alternating.
Q arrives prescaled, as the UNet's to_q hands it over."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_multi_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
SETS, W = (4, 16), (0.6, 0.8)
out = {"bench": "ip_multi", "batch": 2, "text_keys": 77, "sets": list(SETS), "iters": a.iters, "rounds": a.rounds}
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


def region(h, w, b):
    m = torch.zeros(8 * h, 8 * w)
    m[8 * (h // 4) + 3:8 * (3 * h // 4) + 5, 8 * (b * w // 4) + 5:8 * ((b + 2) * w // 4) + 3] = 1.0
    return m


out["kernels"] = {}
g = torch.Generator().manual_seed(1)
for H, Sq in ((10, 4096), (20, 1024)):
    B, C, side = 2, H * 64, int(Sq ** 0.5)
    q = (torch.randn(B, Sq, C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
    k, v = (torch.randn(B, 77, C, generator=g).to(dev, BF) for _ in range(2))
    k2, v2 = (torch.randn(B, sum(SETS), C, generator=g).to(dev, BF) for _ in range(2))
    ka, va, kb, vb = (t[:, r].contiguous() for r in (slice(0, 4), slice(4, 20)) for t in (k2, v2))
    shared = ipa.downsample_mask(region(side, side, 0), side, side).to(dev)                                   # [1, Sq]
    per = torch.cat([ipa.downsample_mask(region(side, side, b), side, side) for b in range(B)]).to(dev)      # [B, Sq]
    fa, fb = (W[0] * shared)[:, :, None].to(BF), (W[1] * per)[:, :, None].to(BF)       # w_j m_j per query, for the unfused adds
    multi = lambda: ops.attention_fwd_ipn(q, k, v, k2, v2, H, SETS, W, q_prescaled=True)
    multi_masked = lambda: ops.attention_fwd_ipn(q, k, v, k2, v2, H, SETS, W, [shared, per], q_prescaled=True)
    one_set = lambda: ops.attention_fwd_ip(q, k, v, kb, vb, H, W[1], q_prescaled=True)

    def unfused():
        o = ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]
        oa = ops.attention_fwd(q, ka, va, H, q_prescaled=True)[0]
        ob = ops.attention_fwd(q, kb, vb, H, q_prescaled=True)[0]
        o = torch.addcmul(o, oa, fa)               # bf16 elementwise: reads two O-sized tensors, writes one
        return torch.addcmul(o, ob, fb)
    variants = {"multi": multi, "multi_masked": multi_masked, "one_set": one_set, "unfused": unfused}
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
    out["kernels"][f"H{H}_Sq{Sq}"] = {
        **{f"{n}_us": round(m, 2) for n, m in med.items()},
        "multi_over_one_set": round(med["multi"] / med["one_set"], 3), "multi_masked_over_one_set": round(med["multi_masked"] / med["one_set"], 3),
        "multi_over_unfused": round(med["multi"] / med["unfused"], 3), "multi_masked_over_unfused": round(med["multi_masked"] / med["unfused"], 3),
        "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
        "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}

if not a.no_unet:
    cfg, hw = pc.sdxl_config(), a.latent
    unet = HipUNet(cfg, 2, hw, hw, 77)
    unet.init_random(1)
    gd = torch.Generator(device="cuda").manual_seed(2)

    def adapter(N):
        sd = {"image_proj": {"proj.weight": torch.randn(N * 2048, 1024, generator=gd, device=dev) / 32, "proj.bias": torch.zeros(N * 2048),
                             "norm.weight": torch.ones(2048), "norm.bias": torch.zeros(2048)}, "ip_adapter": {}}
        for (idx, _), (_, C) in zip(ipa.layer_keys(cfg), ipa._cross_layers(cfg)):
            for nm in ("to_k_ip", "to_v_ip"):
                sd["ip_adapter"][f"{idx}.{nm}.weight"] = torch.randn(C, 2048, generator=gd, device=dev) * 2048 ** -0.5
        return ipa.IPAdapter(sd, cfg)
    ads = unet.load_ip_adapter([adapter(n) for n in SETS])
    toks = [ad.tokens(torch.randn(1, 1024, generator=gd, device=dev), do_cfg=True) for ad in ads]
    unet.set_ip_adapter_scale(list(W))
    unet.set_ip_adapter_masks([region(hw, hw, 1)[None], None])
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    tt = torch.tensor([500.0, 500.0]).to(dev)
    ehs = torch.randn(2, 77, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]

    def state(n_live):
        unet.clear_ip_tokens()
        if n_live == 1:
            unet.set_ip_tokens([None, toks[1]])
        elif n_live == 2:
            unet.set_ip_tokens(toks)
    names = {0: "plain", 1: "one_prompt", 2: "two_prompts"}
    t = {n: [] for n in names.values()}
    for n_live in (0, 1, 2, 0, 1, 2):                 # warm-up of every form: arenas, weight-prefetch sequence, code objects
        state(n_live)
        fwd()
    for _ in range(a.unet_rounds):
        for n_live, name in names.items():
            state(n_live)
            t[name].append(event_us(fwd, 3))
    eps = fwd()
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, "query_counts": unet.ip_query_counts(), **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "two_over_plain": round(med["two_prompts"] / med["plain"], 4), "two_over_one": round(med["two_prompts"] / med["one_prompt"], 4),
                   "finite": bool(torch.isfinite(eps).all()),
                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
