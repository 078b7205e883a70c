"""On-device CLIPScore of decoded samples (README "Beyond the step": CLIP image towers): synthetic weights, --batch images of
--size x --size in [-1, 1] (what `HipVAEDecoder` returns), for ViT-L/14 and ViT-H/14 (head_dim 80) at 224 x 224.  One JSON
line; per tower the milliseconds per stage
  preprocess: `vision.preprocess` (8-bit grid, antialiased bicubic resample, centre crop, normalise);
  tower:      `HipImageEncoder.encode` (patchify, patch GEMM, embedding + pre-LayerNorm, the blocks, pooled projection) and
              its TFLOP/s on the analytic FLOPs (2 x MACs of the linears and of the attention products);
  score:      `ops.clip_score` against random text embeddings.
Medians over --rounds, wall clock around a device synchronisation (each stage runs --inner times per measurement)."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc, ops, vision
from pea_diffusion_amd._lib import lib, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--inner", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda")
out = {"bench": "clip_score", "batch": a.batch, "size": a.size}
tf, mhz = ctypes.c_double(), ctypes.c_double()
if lib().pea_probe_mfma_peak(0.5, 0, ctypes.byref(tf), ctypes.byref(mhz), stream_ptr()) == 0:
    out["clock_mhz"] = round(mhz.value)           # in-kernel clock under sustained MFMA load


def tower_flops(c):
    L, W, Np = c.num_tokens, c.hidden_size, c.num_tokens - 1
    per_layer = 2.0 * L * (4 * W * W + 2 * W * c.intermediate_size) + 4.0 * L * L * W
    return 2.0 * Np * 3 * c.patch_size ** 2 * W + c.num_hidden_layers * per_layer + 2.0 * W * c.projection_dim


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.inner):
        r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.inner, r


images = (torch.rand(a.batch, 3, a.size, a.size, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
out["towers"] = {}
for cfg in (pc.clip_vit_l14_config(), pc.clip_vit_h14_config()):
    enc = vision.HipImageEncoder(cfg, a.batch)
    enc.init_random(1)
    text = torch.randn(a.batch, cfg.projection_dim, generator=torch.Generator().manual_seed(2)).to(dev)
    pre = lambda: vision.preprocess(images, cfg.image_size, cfg.image_mean, cfg.image_std)
    px = pre()
    emb = enc.encode(px)[2]                        # warm-up: arenas, tap tables
    t = {"preprocess": [], "tower": [], "score": [], "end_to_end": []}
    for _ in range(a.rounds):
        t["preprocess"].append(timed(pre)[0])
        t["tower"].append(timed(lambda: enc.encode(px))[0])
        dt, s = timed(lambda: ops.clip_score(emb, text))
        t["score"].append(dt)
        t["end_to_end"].append(timed(lambda: vision.clip_score_images(enc, images, text))[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    out["towers"][cfg.name] = {
        "preprocess_ms": round(med["preprocess"] * 1e3, 4), "tower_ms": round(med["tower"] * 1e3, 4),
        "score_ms": round(med["score"] * 1e3, 4), "end_to_end_ms": round(med["end_to_end"] * 1e3, 4),
        "tower_tflops": round(a.batch * tower_flops(cfg) / med["tower"] / 1e12, 2),
        "preprocess_read_gbs": round(images.numel() * 4 / med["preprocess"] / 1e9, 1),
        "finite": bool(torch.isfinite(s).all()) and bool(torch.isfinite(emb).all()),
        "tower_all_rounds_ms": [round(x * 1e3, 4) for x in t["tower"]]}
    del enc
    torch.cuda.empty_cache()
print(json.dumps(out))
