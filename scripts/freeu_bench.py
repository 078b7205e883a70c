"""FreeU on the SDXL UNet at 1024 x 1024, CFG batch 2.  One JSON line, also written to profiles/freeu_bench.json (--out).
  sites: the six concats FreeU acts on -- up block 0 at 32 x 32 with C1 | C2 = 1280|1280, 1280|1280, 1280|640, up block 1 at 64 x 64
         with 1280|640 (the first operand depth-to-space: the upsampler's output), 640|640, 640|320:
             a  concat2   `ops.concat2`, the launch FreeU replaces (unchanged by it)
             b  freeu     `ops.freeu_concat`: the coefficient kernel (with its finalize launch where the reduction is split) plus
                          the fused concat
         microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the median
         over --rounds with the two alternating inside every round; per variant the spread (max - min) / median.  Beside them the
         byte model: the pair moves 2 * 2 rows C2 (the skip, read twice) + 2 * 2 rows C1 + 2 rows C2 bytes, concat2 4 rows (C1 + C2).
  unet:  one forward of the full UNet (random weights) with the switch off and on, alternating."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeu_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
S1, S2, B1, B2 = 0.9, 0.2, 1.3, 1.4                       # the SDXL values of the FreeU authors
out = {"bench": "freeu", "batch": 2, "factors": [S1, S2, B1, B2], "iters": a.iters, "rounds": a.rounds}
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


SITES = [("up0.0", 32, 1280, 1280, False, S1, B1), ("up0.1", 32, 1280, 1280, False, S1, B1), ("up0.2", 32, 1280, 640, False, S1, B1),
         ("up1.0", 64, 1280, 640, True, S2, B2), ("up1.1", 64, 640, 640, False, S2, B2), ("up1.2", 64, 640, 320, False, S2, B2)]
out["sites"] = {}
g = torch.Generator().manual_seed(1)
B = 2
for name, side, C1, C2, d2s, s, bs in SITES:
    rows = B * side * side
    av = torch.randn(B, side, side, C1, generator=g).to(dev, BF)
    bv = torch.randn(B, side, side, C2, generator=g).to(dev, BF)
    av = ops.nhwc_to_d2s(av) if d2s else av
    y = torch.empty(rows, C1 + C2, device=dev, dtype=BF)
    coef = torch.empty(B, 7, C2, device=dev, dtype=torch.float32)
    nbytes = ops.freeu_scratch_bytes(B, side, side, C2)
    scratch = torch.empty(max(nbytes // 4, 1), device=dev, dtype=torch.float32)

    def plain():
        lib().pea_op_concat2(av.data_ptr(), C1, bv.data_ptr(), C2, y.data_ptr(), rows, side if d2s else 0, side if d2s else 0, stream_ptr())
    freeu = lambda: ops.freeu_concat(av, bv, s, bs, d2s=d2s, y=y, coef=coef, scratch=scratch)
    variants = {"concat2": plain, "freeu": freeu}
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
    bytes_plain = 4 * rows * (C1 + C2)
    bytes_freeu = 2 * 2 * rows * C2 + 2 * 2 * rows * C1 + 2 * rows * C2
    out["sites"][name] = {
        "map": side, "C1": C1, "C2": C2, "depth_to_space": d2s, "slabs": nbytes // (4 * 7 * B * C2) if nbytes else 1,
        "launches": 3 if nbytes else 2, **{f"{n}_us": round(m, 2) for n, m in med.items()},
        "freeu_over_concat2": round(med["freeu"] / med["concat2"], 3), "extra_us": round(med["freeu"] - med["concat2"], 2),
        "bytes_concat2": bytes_plain, "bytes_freeu": bytes_freeu, "byte_ratio": round(bytes_freeu / bytes_plain, 3),
        "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
        "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}
out["sites_extra_us_total"] = round(sum(v["extra_us"] for v in out["sites"].values()), 2)

if not a.no_unet:
    cfg, hw = pc.sdxl_config(), a.latent
    unet = HipUNet(cfg, 2, hw, hw, 77)
    unet.init_random(1)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, hw, hw, generator=gc).to(dev)
    tt = torch.tensor([500.0, 500.0]).to(dev)
    ehs = torch.randn(2, 77, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(2, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 2).to(dev)}
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]

    def state(on):
        if on:
            unet.enable_freeu(S1, S2, B1, B2)
        else:
            unet.disable_freeu()
    names = {False: "plain", True: "freeu"}
    t = {n: [] for n in names.values()}
    for on in (False, True, False, True):             # warm-up of both forms: arenas, weight-prefetch sequence, code objects
        state(on)
        fwd()
    for _ in range(a.unet_rounds):
        for on, name in names.items():
            state(on)
            t[name].append(event_us(fwd, 3))
    eps = fwd()
    med = {n: statistics.median(x) for n, x in t.items()}
    out["unet"] = {"latent": hw, **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "freeu_minus_plain_us": round(med["freeu"] - med["plain"], 1), "freeu_over_plain": round(med["freeu"] / med["plain"], 4),
                   "finite": bool(torch.isfinite(eps).all()),
                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
