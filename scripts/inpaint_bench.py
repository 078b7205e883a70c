"""SDXL inpainting 1024x1024 (tests/test_sdxl_zh_inpaint.py denoise loop), N images per call with classifier-free guidance
(UNet batch 2N), DPM-Solver++ steps, random-init weights and synthetic inputs.  In one process, alternating, it times:
  gather: the 9-channel UNet with its inpainting condition set once (conv_in gathers latents, mask, masked latents),
  cat:    the same UNet fed the reference's per-step `torch.cat([cat([latents] * 2), mask, masked_latents], dim=1)`,
  t2i:    the plain text-to-image loop (`sampler.denoise`) on the 4-channel SDXL UNet,
and prints seconds per generation for each (median over the rounds) as one JSON line."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=4)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
N, hw, gs = a.images, a.latent, 5.0
dev = torch.device("cuda")
u9 = HipUNet(pc.sdxl_inpaint_config(), 2 * N, hw, hw, 77, inpaint_inputs=True)
u9.init_random(1)
u4 = HipUNet(pc.sdxl_config(), 2 * N, hw, hw, 77)
u4.init_random(1)
g = torch.Generator(device="cpu").manual_seed(0)
lat = torch.randn(N, 4, hw, hw, generator=g).to(dev)
ehs = torch.randn(2 * N, 77, 2048, generator=g).to(dev, torch.bfloat16)
added = {"text_embeds": torch.randn(2 * N, 1280, generator=g).to(dev, torch.bfloat16),
         "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * (2 * N)).to(dev)}
mask = (torch.rand(N, 1, hw, hw, generator=g) > 0.5).float().to(dev)
masked = torch.randn(N, 4, hw, hw, generator=g).to(dev)
mask2, masked2 = torch.cat([mask] * 2), torch.cat([masked] * 2)


def loop(steps, gather):
    s = DPMSolverMultistep()
    ts = s.set_timesteps(steps)
    s.set_begin_index(0)
    x = lat.clone()
    if gather:
        u9.set_inpaint_cond(mask, masked, latent_batch=N)
    for t in ts:
        if gather:
            inp = x
        else:
            inp = torch.cat([torch.cat([x] * 2), mask2, masked2], dim=1)
        n = u9(inp, t, encoder_hidden_states=ehs, added_cond_kwargs=added)[0]
        x = s.step(ops.cfg_combine(n.float(), gs), t, x)[0]
    if gather:
        u9.clear_inpaint_cond()
    return x


def t2i(steps):
    return denoise(u4, DPMSolverMultistep(), lat.clone(), ehs, added, num_inference_steps=steps, guidance_scale=gs)


runs = {"gather": lambda k: loop(k, True), "cat": lambda k: loop(k, False), "t2i": t2i}
for f in runs.values():
    f(2)
torch.cuda.synchronize()
times = {k: [] for k in runs}
finite = {}
for r in range(a.rounds):
    for k, f in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f(a.steps)
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
        finite[k] = bool(torch.isfinite(out).all())
med = {k: statistics.median(v) for k, v in times.items()}
print(json.dumps({"bench": "sdxl_inpaint", "images": N, "unet_batch": 2 * N, "steps": a.steps, "size": hw * 8,
                  "s_per_generation": {k: round(v, 4) for k, v in med.items()},
                  "all_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
                  "gather_vs_t2i": round(med["gather"] / med["t2i"] - 1, 4), "cat_vs_gather": round(med["cat"] / med["gather"] - 1, 4),
                  "finite": finite}))
