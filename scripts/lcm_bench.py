"""LCM-LoRA on the full SDXL UNet (tests/test_sdxl_zh_lcm.py): random base weights, a rank-64 random LoRA on the LCM-LoRA
target set (pea_diffusion_amd.lora.LCM_LORA_TARGETS).  One JSON line with
  fuse:     device time of the composition kernels (pea_op_lora_compose timed per distinct weight shape with HIP events, summed
            over the target set), the TB/s that is on 4 (2 M Kf + r (M + Kf)) bytes, and the wall time of `HipUNet.fuse_lora`
            (base weights already on the device as fp32, LoRA factors uploaded from the host, every packer included);
  generate: seconds per generation at 1024 x 1024 for N images: the 4-step LCM loop at guidance 0 (UNet batch N) beside the
            30-step DPM-Solver++ loop with classifier-free guidance (UNet batch 2N) of the same tree."""
import argparse, collections, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd.lora import lcm_lora_target_keys
from pea_diffusion_amd.sampler import DPMSolverMultistep, LCMScheduler, denoise
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, nargs="+", default=[1, 4])
ap.add_argument("--rank", type=int, default=64)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--lcm-steps", type=int, default=4)
ap.add_argument("--cfg-steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
dev, hw, r = torch.device("cuda"), a.latent, a.rank
out = {"bench": "sdxl_lcm_lora", "rank": r, "size": hw * 8}
import ctypes
from pea_diffusion_amd._lib import lib, stream_ptr
tf, mhz = ctypes.c_double(), ctypes.c_double()
if lib().pea_probe_mfma_peak(0.5, 0, ctypes.byref(tf), ctypes.byref(mhz), stream_ptr()) == 0:
    out["clock_mhz"] = round(mhz.value)           # in-kernel clock under sustained MFMA load

# ---- fuse
probe = HipUNet(pc.sdxl_config(), 1, 16, 16, 77)
table = probe.weight_table()
keys = lcm_lora_target_keys(table)
gd = torch.Generator(device="cuda").manual_seed(0)
base = {k: torch.randn(table[k], generator=gd, device=dev) * (1.0 / table[k][1] ** 0.5) for k in keys}
g = torch.Generator().manual_seed(1)
lora = {}
for k in keys:
    M, kf = table[k][0], base[k][0].numel()
    mod = "lora_unet_" + k[:-len(".weight")].replace(".", "_")
    lora[mod + ".lora_down.weight"] = torch.randn(r, kf, generator=g) / kf ** 0.5
    lora[mod + ".lora_up.weight"] = torch.randn(M, r, generator=g) * (0.1 / r ** 0.5)
shapes = collections.Counter((table[k][0], base[k][0].numel()) for k in keys)
dev_ms, nbytes = 0.0, 0.0
for (M, kf), count in shapes.items():
    W, d, u = torch.randn(M, kf, device=dev), torch.randn(r, kf, device=dev), torch.randn(M, r, device=dev)
    o = torch.empty_like(W)
    ops.lora_compose(W, d, u, 0.1, out=o)
    reps = 20
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.lora_compose(W, d, u, 0.1, out=o)
    e1.record()
    torch.cuda.synchronize()
    dev_ms += count * e0.elapsed_time(e1) / reps
    nbytes += count * 4.0 * (2.0 * M * kf + r * (M + kf))
walls = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fused = probe.fuse_lora(base, lora)
    walls.append(time.perf_counter() - t0)
    probe.unfuse_lora(base)
out["fuse"] = {"keys": len(fused), "distinct_shapes": len(shapes), "bytes": nbytes, "compose_device_ms": round(dev_ms, 3),
               "compose_TBps": round(nbytes / (dev_ms * 1e-3) / 1e12, 3), "fuse_lora_wall_s": [round(w, 3) for w in walls]}
del probe, base, lora
torch.cuda.empty_cache()

# ---- generate
out["generate"] = {}
for N in a.images:
    u = HipUNet(pc.sdxl_config(), 2 * N, hw, hw, 77)
    u.init_random(1)
    u1 = HipUNet(pc.sdxl_config(), N, hw, hw, 77, share_weights_from=u)
    gc = torch.Generator().manual_seed(2)
    lat = torch.randn(N, 4, hw, hw, generator=gc).to(dev)
    ehs = torch.randn(2 * N, 77, 2048, generator=gc).to(dev, torch.bfloat16)
    added = {"text_embeds": torch.randn(2 * N, 1280, generator=gc).to(dev, torch.bfloat16),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * (2 * N)).to(dev)}
    half = {k: v[:N].contiguous() for k, v in added.items()}
    gn = torch.Generator(device="cuda").manual_seed(3)
    runs = {"lcm": lambda: denoise(u1, LCMScheduler(), lat.clone(), ehs[:N].contiguous(), half, num_inference_steps=a.lcm_steps,
                                   guidance_scale=0.0, generator=gn),
            "cfg": lambda: denoise(u, DPMSolverMultistep(), lat.clone(), ehs, added, num_inference_steps=a.cfg_steps,
                                   guidance_scale=5.0)}
    times = {k: [] for k in runs}
    finite = {}
    for k, f in runs.items():
        f()
    for _ in range(a.rounds):
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
            finite[k] = bool(torch.isfinite(x).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    out["generate"][f"images_{N}"] = {"lcm_steps": a.lcm_steps, "cfg_steps": a.cfg_steps,
                                      "s_per_generation": {k: round(v, 4) for k, v in med.items()},
                                      "all_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()},
                                      "cfg_over_lcm": round(med["cfg"] / med["lcm"], 2), "finite": finite}
    del u1, u
    torch.cuda.empty_cache()
print(json.dumps(out))
