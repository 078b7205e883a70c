"""Per-token cross-attention heat maps of a short denoising run, written as .npy files.

The UNet has seeded random weights (no checkpoint is needed), so the maps show the mechanics, not a picture: enable capture,
run `sampler.denoise`, read `attention_maps.heat_maps`.  There is no tokenizer in this package: --tokens are indices of context
rows, and a caller with a real prompt passes the rows its words landed in.
  python scripts/attn_maps_demo.py --config tiny --steps 4 --tokens 1 2 3 --out /tmp/maps
writes maps_token<k>.npy (fp32 [H, W], the conditional half of the CFG batch) and maps_all.npy ([tokens, H, W])."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd.attention_maps import heat_maps
from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=("tiny", "sdxl"), default="tiny")
ap.add_argument("--latent", type=int, default=0, help="latent side (default: 16 for tiny, 128 for sdxl)")
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--layers", default="", help='e.g. "up" or "down_blocks.2,mid": capture these blocks only')
ap.add_argument("--tokens", type=int, nargs="*", default=[1, 2, 3])
ap.add_argument("--size", type=int, default=0, help="side of the written maps (default: the largest attention grid)")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="attn_maps_out")
a = ap.parse_args()
cfg = pc.tiny_config() if a.config == "tiny" else pc.sdxl_config()
hw, L, dev = a.latent or (16 if a.config == "tiny" else 128), 77, torch.device("cuda")
unet = HipUNet(cfg, 2, hw, hw, L)                         # CFG batch: [unconditional | conditional]
unet.init_random(a.seed)
g = torch.Generator().manual_seed(a.seed)
latents = torch.randn(1, cfg.in_channels, hw, hw, generator=g).to(dev)
ehs = torch.randn(2, L, cfg.cross_attention_dim, generator=g).to(dev, torch.bfloat16)
added = None
if cfg.addition_embed_type == "text_time":
    added = {"text_embeds": torch.randn(2, cfg.pooled_dim, generator=g).to(dev, torch.bfloat16),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
unet.enable_attention_maps({k: 1.0 for k in a.layers.split(",")} if a.layers else None)
denoise(unet, DPMSolverMultistep(), latents, ehs, added, num_inference_steps=a.steps, guidance_scale=a.guidance)
maps = heat_maps(unet, size=(a.size, a.size) if a.size else None, do_cfg=True, tokens=a.tokens)[0].cpu().numpy()
os.makedirs(a.out, exist_ok=True)
np.save(os.path.join(a.out, "maps_all.npy"), maps)
for i, k in enumerate(a.tokens):
    np.save(os.path.join(a.out, f"maps_token{k}.npy"), maps[i])
    print(f"token {k}: {maps[i].shape}, mean {maps[i].mean():.5f}, max {maps[i].max():.5f}")
counts = {hwl: n for hwl, (_, n) in unet.attention_maps().items()}
print(f"layer-forwards per grid: {counts}; wrote {len(a.tokens) + 1} files to {a.out}")
