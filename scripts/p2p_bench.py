"""Prompt-to-prompt editing on the SDXL UNet at 1024 x 1024, N = 2 prompts, CFG batch 4, 77 keys.  One JSON line, also written to
profiles/p2p_bench.json (--out).
  kernels: the two cross-attention shapes of that UNet (10 heads x 4096 queries, 20 heads x 1024 queries), src = [-1, -1, -1, 2]
           (one edited sample of four, the CFG layout) and [-1, 0, -1, 2] (two of four), a soft mapper, three forms alternating
           inside every round:
             edit     `ops.attention_fwd_edit`, one launch over the batch
             plain    one `attention_fwd` on the same batch: what the layer costs without editing
             two      two `attention_fwd` launches on that batch: evaluating both softmaxes separately before any mixing -- the
                      yardstick no unfused form could beat
           microseconds per call from device events around the replay of a captured graph of --iters back-to-back calls, the median
           over --rounds; per form the spread (max - min) / median.
  unet:    one forward of the full UNet (random weights, 128 x 128 latents, batch 4): without an edit, with the cross-attention
           edit live (the self-attention rule off), and with both live (self_max_tokens 1024: the 32 x 32 level), alternating;
           SDXL has 60 self-attention layers at 32 x 32: 60 extra B = 1 launches per forward and edited sample.
Q arrives prescaled, as the UNet's to_q hands it over.  Run it twice: the spread between two runs is the margin a claimed
difference has to exceed."""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ops
from pea_diffusion_amd._lib import lib, stream_ptr
from pea_diffusion_amd.prompt2prompt import PromptEdit, equalizer, replace_mapper
from pea_diffusion_amd.unet import HipUNet

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--latent", type=int, default=128)
ap.add_argument("--unet-rounds", type=int, default=7)
ap.add_argument("--no-unet", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p2p_bench.json"))
a = ap.parse_args()
dev, BF, L, B = torch.device("cuda"), torch.bfloat16, 77, 4
out = {"bench": "p2p", "batch": B, "keys": L, "iters": a.iters, "rounds": a.rounds}
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


M = replace_mapper(L, [((5, 6), (5, 7)), ((9, 11), (10, 12))])
out["kernels"] = {}
g = torch.Generator().manual_seed(1)
for H, Sq in ((10, 4096), (20, 1024)):
    C = H * 64
    q = (torch.randn(B, Sq, C, generator=g) * 0.125 * 1.4426950408889634).to(dev, BF)
    k, v = (torch.randn(B, L, C, generator=g).to(dev, BF) for _ in range(2))
    Mt = torch.zeros(B, L, 80)
    Mt[:, :, :L] = M.t().float()
    Mt = Mt.to(dev, BF)
    c, d = torch.full((B, L), 0.75, device=dev), torch.full((B, L), 0.25, device=dev)
    plain = lambda: ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]

    def two():
        ops.attention_fwd(q, k, v, H, q_prescaled=True)
        return ops.attention_fwd(q, k, v, H, q_prescaled=True)[0]
    res = {}
    for name, src in (("one_of_four", [-1, -1, -1, 2]), ("two_of_four", [-1, 0, -1, 2])):
        edit = lambda src=src: ops.attention_fwd_edit(q, k, v, H, src, Mt, c, d, q_prescaled=True)
        variants = {"edit": edit, "plain": plain, "two": two}
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
        res[name] = {**{f"{n}_us": round(m, 2) for n, m in med.items()},
                     "edit_over_plain": round(med["edit"] / med["plain"], 3), "edit_over_two_plain": round(med["edit"] / med["two"], 3),
                     "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                     "all_rounds_us": {n: [round(x, 2) for x in xs] for n, xs in t.items()}}
    out["kernels"][f"H{H}_Sq{Sq}"] = res

if not a.no_unet:
    cfg, hw, T = pc.sdxl_config(), a.latent, 4
    unet = HipUNet(cfg, B, hw, hw, L)
    unet.init_random(1)
    gc = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, hw, hw, generator=gc).expand(B, -1, -1, -1).contiguous().to(dev)
    tt = torch.full((B,), 500.0).to(dev)
    ehs = torch.randn(B, L, 2048, generator=gc).to(dev, BF)
    added = {"text_embeds": torch.randn(B, 1280, generator=gc).to(dev, BF),
             "time_ids": torch.tensor([[hw * 8, hw * 8, 0, 0, hw * 8, hw * 8]] * B).to(dev)}
    ed = dict(source=0, mapper=M, equalizer=equalizer(L, {5: 2.0}))
    cross = PromptEdit.compose(L, T, [None, ed], cross_replace_steps=1.0, self_replace_steps=0.0, do_cfg=True)
    both = PromptEdit.compose(L, T, [None, ed], cross_replace_steps=1.0, self_replace_steps=1.0, self_max_tokens=1024, do_cfg=True)
    fwd = lambda: unet(x, tt, ehs, added_cond_kwargs=added)[0]

    def form(name):
        unet.clear_prompt_edit()
        if name != "plain":
            unet.set_prompt_edit(cross if name == "cross_edit" else both)
            unet.set_prompt_edit_step(0)
    names = ("plain", "cross_edit", "cross_and_self_edit")
    t = {n: [] for n in names}
    eps = {}
    for n in names + names:                               # warm-up of every form: arenas, weight-prefetch sequence, code objects
        form(n)
        eps[n] = fwd().clone()
    for _ in range(a.unet_rounds):
        for n in names:
            form(n)                                       # (the tables are copied outside the timed calls)
            torch.cuda.synchronize()
            t[n].append(event_us(fwd, 3))
    unet.clear_prompt_edit()
    med = {n: statistics.median(x) for n, x in t.items()}
    counts = unet.ip_query_counts()
    out["unet"] = {"latent": hw, "query_counts": counts, **{f"forward_{n}_ms": round(m * 1e-3, 3) for n, m in med.items()},
                   "cross_edit_over_plain": round(med["cross_edit"] / med["plain"], 4),
                   "cross_and_self_edit_over_plain": round(med["cross_and_self_edit"] / med["plain"], 4),
                   "finite": bool(all(torch.isfinite(e).all() for e in eps.values())),
                   "source_and_uncond_keep_bits": bool(torch.equal(eps["cross_and_self_edit"][:3], eps["plain"][:3])),
                   "edited_sample_moves": bool(not torch.equal(eps["cross_and_self_edit"][3], eps["plain"][3])),
                   "spread": {n: round((max(x) - min(x)) / med[n], 3) for n, x in t.items()},
                   "all_rounds_ms": {n: [round(x * 1e-3, 3) for x in xs] for n, xs in t.items()}}
line = json.dumps(out)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
