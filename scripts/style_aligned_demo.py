"""n prompts in one style (StyleAligned, Hertz et al. 2023): the first prompt is the style reference, the others share its
self-attention.  Writes the final latents of a run with sharing and of the same run without, as .npy files.

  python scripts/style_aligned_demo.py --config tiny --n 3 --steps 4 --out /tmp/style
  python scripts/style_aligned_demo.py --config sdxl --unet unet.safetensors --embeds prompts.pt --n 4 --steps 30

--unet: a diffusers UNet2DConditionModel state dict (.safetensors / .bin); without it the UNet has seeded random weights and the
run shows the mechanics, not a picture.  There is no tokenizer or text encoder call here: --embeds is a torch file with
`prompt_embeds` [n, L, D], `negative_prompt_embeds` [n, L, D] and, for SDXL, `pooled` / `negative_pooled` [n, P]; without it the
embeddings are random.  The loop is `sampler.denoise` over the CFG batch [uncond x n | cond x n]; `set_style_aligned(do_cfg=True)`
gives each half its own reference (samples 0 and n).  --layers: a fraction 0..1 of the self-attention layers, or names / prefixes
("up", "up_blocks.0,mid") as `style_aligned.resolve_layers` reads them."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import style_aligned as sa
from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=("tiny", "sdxl"), default="tiny")
ap.add_argument("--unet", default="", help="UNet state dict (.safetensors / .bin); default: seeded random weights")
ap.add_argument("--embeds", default="", help="torch file with prompt_embeds / negative_prompt_embeds (/ pooled / negative_pooled)")
ap.add_argument("--n", type=int, default=3, help="prompts, the first is the style reference")
ap.add_argument("--latent", type=int, default=0, help="latent side (default: 16 for tiny, 128 for sdxl)")
ap.add_argument("--steps", type=int, default=4)
ap.add_argument("--guidance", type=float, default=5.0)
ap.add_argument("--layers", default="", help='a fraction ("0.5") or names ("up,mid"); default: every self-attention layer')
ap.add_argument("--no-adain-queries", action="store_true")
ap.add_argument("--no-adain-keys", action="store_true")
ap.add_argument("--score-scale", type=float, default=1.0)
ap.add_argument("--score-shift", type=float, default=0.0)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default="style_aligned_out")
a = ap.parse_args()
cfg = pc.tiny_config() if a.config == "tiny" else pc.sdxl_config()
hw, L, dev, n = a.latent or (16 if a.config == "tiny" else 128), 77, torch.device("cuda"), a.n
g = torch.Generator().manual_seed(a.seed)
if a.embeds:
    e = torch.load(a.embeds, map_location="cpu")
    ehs = torch.cat([e["negative_prompt_embeds"][:n], e["prompt_embeds"][:n]])
    pooled = torch.cat([e["negative_pooled"][:n], e["pooled"][:n]]) if "pooled" in e else None
    L = ehs.shape[1]
else:
    ehs = torch.randn(2 * n, L, cfg.cross_attention_dim, generator=g)
    pooled = torch.randn(2 * n, cfg.pooled_dim, generator=g) if cfg.addition_embed_type == "text_time" else None
unet = HipUNet(cfg, 2 * n, hw, hw, L)                     # CFG batch: [unconditional x n | conditional x n]
if a.unet:
    from pea_diffusion_amd.lora import load_lora_state_dict
    unet.load_state_dict(load_lora_state_dict(a.unet))
else:
    unet.init_random(a.seed)
latents = torch.randn(n, cfg.in_channels, hw, hw, generator=g).to(dev)
ehs = ehs.to(dev, torch.bfloat16)
added = None
if cfg.addition_embed_type == "text_time":
    added = {"text_embeds": pooled.to(dev, torch.bfloat16),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * (2 * n)).to(dev)}
layers = None
if a.layers:
    try:
        layers = float(a.layers)
    except ValueError:
        layers = a.layers.split(",")
run = lambda: denoise(unet, DPMSolverMultistep(), latents, ehs, added, num_inference_steps=a.steps, guidance_scale=a.guidance)
plain = run()
unet.set_style_aligned(layers=layers, adain_queries=not a.no_adain_queries, adain_keys=not a.no_adain_keys,
                       shared_score_scale=a.score_scale, shared_score_shift=a.score_shift, do_cfg=True)
styled = run()
unet.clear_style_aligned()
os.makedirs(a.out, exist_ok=True)
np.save(os.path.join(a.out, "latents_plain.npy"), plain.cpu().numpy())
np.save(os.path.join(a.out, "latents_style_aligned.npy"), styled.cpu().numpy())
on = sa.resolve_layers(unet, layers)
print(f"{n} prompts, reference_index {sa.reference_index(n, True)}, {int(sum(on))} of {len(on)} self-attention layers shared")
for b in range(n):
    d = (styled[b] - plain[b]).float().norm() / plain[b].float().norm()
    print(f"prompt {b}{' (reference)' if b == 0 else ''}: latents moved by {d.item():.4f} (relative L2)")
print(f"wrote latents_plain.npy and latents_style_aligned.npy to {a.out}")
