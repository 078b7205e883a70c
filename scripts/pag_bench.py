"""Perturbed-attention (PAG) and smoothed-energy (SEG) guidance on the SDXL UNet at 1024 x 1024, n = 1 and 2 perturbed samples.
One JSON line, also written to profiles/pag_bench.json (--out).  Nothing here is a gate.
  kernels: per self-attention shape -- 32 x 32 tokens x 1280 channels (the mid block, 20 heads) and 64 x 64 x 640 (10 heads) -- and
           per n, forms alternating inside every round:
             blur      `ops.query_blur_` in place on the Q columns of an [n, S, 3C] projection, as the UNet runs it in front of the
                       layer's ordinary launch (dense per-axis tables: the time does not depend on sigma)
             identity  `ops.attn_identity`, V columns of that projection -> O: what PAG runs instead of the launch
             plain     `ops.attention_fwd` of n samples of that layer: the launch the blur precedes and the copy replaces
             torch     the blur's composition at sigma 2 (13 taps): permute to [n, C, h, w], `F.pad(reflect)`, two grouped `F.conv2d`,
                       permute back, copy into the Q columns
           blur, identity, plain: microseconds per call from device events around the replay of a captured graph of --iters
           back-to-back calls; torch: events around --torch-iters eager calls.  The median over --rounds; the whole measurement
           runs --repeats times and `repeat_spread` is (max - min) / min of the medians.
  forward: the full UNet (random weights, 128 x 128 latents, 77 text tokens), one call each, alternating inside every round:
           batch 3 plain, batch 3 with mid-block PAG, batch 3 with mid-block SEG, and a batch-2 call plus a batch-1 call (contexts
           sharing the weights): the two-call form self-attention guidance pays.
Q arrives prescaled, as the UNet's to_q hands it over."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.pag import blur_matrix
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--torch-iters", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pag_bench.json"))
a = ap.parse_args()
dev, BF = torch.device("cuda"), torch.bfloat16
out = {"bench": "pag", "iters": a.iters, "rounds": a.rounds, "repeats": a.repeats}
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
    return lambda: gr.replay()


def spread(vals):
    return round((max(vals) - min(vals)) / min(vals), 4)


def measure(variants, eager=()):
    """variants: name -> callable.  Those named in `eager` are timed as they are, the others from a captured graph."""
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    timed = {n: ((lambda f=f: event_us(f, a.torch_iters)) if n in eager
                 else (lambda r=captured(f, a.iters): event_us(r, 5) / a.iters)) for n, f in variants.items()}
    for t in timed.values():
        t()
    reps = []
    for _ in range(a.repeats):
        t = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, fn in timed.items():
                t[n].append(fn())
        reps.append({n: statistics.median(x) for n, x in t.items()})
    med = {n: statistics.median(r[n] for r in reps) for n in variants}
    return med, {"repeat_spread": {n: spread([r[n] for r in reps]) for n in variants},
                 "per_repeat_us": {n: [round(r[n], 2) for r in reps] for n in variants}}


g = torch.Generator().manual_seed(1)
out["kernels"] = {}
for h, w, C in ((32, 32, 1280), (64, 64, 640)):
    H, S = C // 64, h * w
    Mh, Mw = (torch.from_numpy(blur_matrix(m, float("inf"))).to(dev) for m in (h, w))
    taps = torch.exp(-0.5 * (torch.linspace(-6.0, 6.0, 13, dtype=torch.float64) / 2.0) ** 2)
    taps = (taps / taps.sum()).float().to(dev)
    for n in (1, 2):
        qkv = (torch.randn(n, S, 3 * C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
        q, k, v = (qkv[..., i * C:(i + 1) * C].contiguous() for i in range(3))
        o = torch.empty(n, S, C, device=dev, dtype=BF)

        def torch_blur():
            x = qkv[..., :C].float().reshape(n, h, w, C).permute(0, 3, 1, 2)      # (fp32 between the passes, as the kernel)
            p = F.pad(x, (6, 6, 6, 6), mode="reflect")
            p = F.conv2d(p, taps.view(1, 1, 1, 13).expand(C, 1, 1, 13), groups=C)
            p = F.conv2d(p, taps.view(1, 1, 13, 1).expand(C, 1, 13, 1), groups=C)
            qkv[..., :C] = p.permute(0, 2, 3, 1).reshape(n, S, C)

        med, extra = measure({"blur": lambda: ops.query_blur_(qkv, (h, w), Mh, Mw, cols=C),
                              "identity": lambda: ops.attn_identity(qkv, o, C, col0=2 * C),
                              "plain": lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0],
                              "torch": torch_blur}, eager=("torch",))
        out["kernels"][f"{h}x{w}x{C}_n{n}"] = {**{f"{m}_us": round(t, 2) for m, t in med.items()},
                                               "blur_lds_bytes": int(lib().pea_op_query_blur_lds_bytes(h, w)), "workgroups": n * C // 8,
                                               "blur_over_plain": round(med["blur"] / med["plain"], 3),
                                               "identity_over_plain": round(med["identity"] / med["plain"], 3),
                                               "torch_over_blur": round(med["torch"] / med["blur"], 1),
                                               "finite": bool(torch.isfinite(qkv.float()).all()), **extra}

if not a.no_unet:
    cfg, L, hw = pc.sdxl_config(), 77, a.latent
    unet = HipUNet(cfg, 3, hw, hw, L)
    unet.init_random(1)
    unet2 = HipUNet(cfg, 2, hw, hw, L, share_weights_from=unet)
    unet1 = HipUNet(cfg, 1, hw, hw, L, share_weights_from=unet)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(3, 4, hw, hw, generator=gc).to(dev)
    ehs = torch.randn(3, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(3, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * 3).to(dev)}
    tt = torch.tensor([500.0] * 3).to(dev)
    cut = lambda lo, hi: dict(added_cond_kwargs={k_: v_[lo:hi] for k_, v_ in added.items()})
    b3 = lambda: unet(x, tt, ehs, **cut(0, 3))[0]

    def two_calls():
        unet2(x[:2], tt[:2], ehs[:2], **cut(0, 2))
        return unet1(x[2:], tt[2:], ehs[2:], **cut(2, 3))[0]
    # (setter, form): the setter runs outside the timed region
    forms = {"plain_b3": (unet.clear_attention_perturbation, b3), "pag_b3": (lambda: unet.set_attention_perturbation("pag"), b3),
             "seg_b3": (lambda: unet.set_attention_perturbation("seg"), b3), "b2_plus_b1": (unet.clear_attention_perturbation, two_calls)}
    for setter, f in list(forms.values()) * 2:            # warm-up: arenas, weight-prefetch sequence, code objects
        setter()
        f()
    torch.cuda.synchronize()
    reps = []
    for _ in range(a.repeats):
        t = {m: [] for m in forms}
        for _ in range(a.rounds):
            for m, (setter, f) in forms.items():
                setter()
                f()
                torch.cuda.synchronize()
                t[m].append(event_us(f, 2))
        reps.append({m: statistics.median(x_) for m, x_ in t.items()})
    med = {m: statistics.median(r[m] for r in reps) for m in forms}
    unet.set_attention_perturbation("seg")
    final = b3().float()
    unet.clear_attention_perturbation()
    out["forward"] = {"latent": hw, **{f"{m}_ms": round(t * 1e-3, 3) for m, t in med.items()},
                      "pag_over_plain_b3": round(med["pag_b3"] / med["plain_b3"], 4), "seg_over_plain_b3": round(med["seg_b3"] / med["plain_b3"], 4),
                      "pag_over_two_calls": round(med["pag_b3"] / med["b2_plus_b1"], 4), "seg_over_two_calls": round(med["seg_b3"] / med["b2_plus_b1"], 4),
                      "repeat_spread": {m: spread([r[m] for r in reps]) for m in forms},
                      "per_repeat_ms": {m: [round(r[m] * 1e-3, 3) for r in reps] for m in forms},
                      "finite": bool(torch.isfinite(final).all())}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
