"""The few-step regime on the full SDXL UNet at 512 x 512 (README "Sampling Acceleration: SDXL-Turbo"): random weights, N
images, guidance 0 (UNet batch N).  One JSON line; per configuration and N the seconds per generation split into
  denoise: `sampler.denoise` -- the UNet evaluations plus the sampler's own launches (EulerAncestralDiscrete: one
           euler_update per step and the entry call, noise drawn on the device);
  decode:  `HipVAEDecoder.decode` of the final latents (64 x 64 -> 512 x 512);
for SDXL-Turbo (EulerAncestralDiscrete, "trailing") at 1 and 4 steps and for LCM-SDXL with the guidance embedding
(`lcm_sdxl_config()`, LCMScheduler, `timestep_cond` of guidance scale 8) at 4 steps.  Medians over --rounds, wall clock
around a device synchronisation."""
import argparse, ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.sampler import EulerAncestralDiscrete, LCMScheduler, denoise, guidance_scale_embedding
from pea_diffusion_amd.unet import HipUNet
from pea_diffusion_amd.vae import HipVAEDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--latent", type=int, default=64)
ap.add_argument("--turbo-steps", type=int, nargs="+", default=[1, 4])
ap.add_argument("--lcm-steps", type=int, default=4)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev, hw = torch.device("cuda"), a.latent
out = {"bench": "sdxl_turbo", "size": hw * 8}
tf, mhz = ctypes.c_double(), ctypes.c_double()
if lib().pea_probe_mfma_peak(0.5, 0, ctypes.byref(tf), ctypes.byref(mhz), stream_ptr()) == 0:
    out["clock_mhz"] = round(mhz.value)           # in-kernel clock under sustained MFMA load
vcfg = pc.sdxl_vae_config()


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


out["generate"] = {}
for N in a.images:
    turbo = HipUNet(pc.sdxl_config(), N, hw, hw, 77)
    turbo.init_random(1)
    lcm = HipUNet(pc.lcm_sdxl_config(), N, hw, hw, 77)
    lcm.init_random(1)
    vae = HipVAEDecoder(vcfg, N, hw, hw)
    vae.init_random(2)
    gc = torch.Generator().manual_seed(2)
    lat = torch.randn(N, 4, hw, hw, generator=gc).to(dev)
    ehs = torch.randn(N, 77, 2048, generator=gc).to(dev, torch.bfloat16)
    added = {"text_embeds": torch.randn(N, 1280, generator=gc).to(dev, torch.bfloat16),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * N).to(dev)}
    cond = guidance_scale_embedding(torch.full((N,), 7.0), 256).to(dev, torch.float32)      # w = guidance_scale - 1
    gn = torch.Generator(device="cuda").manual_seed(3)
    runs = {f"turbo_{k}": (lambda k=k: denoise(turbo, EulerAncestralDiscrete(), lat.clone(), ehs, added, num_inference_steps=k,
                                               guidance_scale=0.0, generator=gn)) for k in a.turbo_steps}
    runs[f"lcm_sdxl_{a.lcm_steps}"] = lambda: denoise(lcm, LCMScheduler(), lat.clone(), ehs, added, num_inference_steps=a.lcm_steps,
                                                      guidance_scale=0.0, generator=gn, timestep_cond=cond)
    decode = lambda z: vae.decode(z, inv_scaling=1.0 / vcfg.scaling_factor)[0]
    times = {k: {"denoise": [], "decode": []} for k in runs}
    finite = {}
    for k, f in runs.items():
        decode(f())                                # warm-up: arenas, weight-prefetch sequence
    for _ in range(a.rounds):
        for k, f in runs.items():
            td, z = timed(f)
            tv, img = timed(lambda: decode(z))
            times[k]["denoise"].append(td)
            times[k]["decode"].append(tv)
            finite[k] = bool(torch.isfinite(img).all()) and tuple(img.shape) == (N, 3, hw * 8, hw * 8)
    row = {}
    for k, v in times.items():
        d, c = statistics.median(v["denoise"]), statistics.median(v["decode"])
        row[k] = {"denoise_s": round(d, 5), "decode_s": round(c, 5), "generation_s": round(d + c, 5),
                  "decode_share": round(c / (d + c), 3), "finite": finite[k],
                  "denoise_all_rounds": [round(x, 5) for x in v["denoise"]]}
    out["generate"][f"images_{N}"] = row
    del turbo, lcm, vae
    torch.cuda.empty_cache()
print(json.dumps(out))
