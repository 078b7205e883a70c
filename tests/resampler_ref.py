"""Test infrastructure: the Perceiver Resampler of the IP-Adapter "plus" files restated in plain torch, independent of
pea_diffusion_amd.

Neither the IP-Adapter package nor a diffusers that carries the Resampler is installed here, so nothing in this file is pinned
against them: it restates the published algorithm (tencent-ailab/IP-Adapter, ip_adapter/resampler.py: Resampler,
PerceiverAttention, FeedForward) under the key names of the published files' `image_proj` group.

  dims / SDXL_PLUS / SD15_PLUS / TINY   the dimensions of a Resampler as a plain dict
  state_shapes      {key: shape} in the FILE's layout (`latents` [1, Nq, dim], `layers.L.0.*` attention, `layers.L.1.*` FF)
  random_state_dict seeded weights in that layout; matrices and `latents` bf16-representable (the HIP path holds them in bf16)
  resampler_ref     tokens = norm_out(proj_out(latents)) after `depth` layers of
                        latents += to_out(softmax(q k^T / 8) v),  q = to_q(norm2(latents)), k, v = to_kv([norm1(x) ; norm2(latents)])
                        latents += ff(latents)
                    in `dtype` (float64 / float32).  store=True rounds to bf16 every tensor the HIP tape stores between two
                    kernels -- the storage floor -- and keeps fp32 wherever it fuses (bias, GELU and residual epilogues run on
                    the fp32 accumulator; Q is stored multiplied by 1/8 log2 e; P is a bf16 MFMA operand).
  plus_file         the adapter as its published `.bin` holds it: ip_adapter_ref.file_state_dict with the Resampler as image_proj
"""
import functools
import math

import torch
import torch.nn.functional as F

HEAD = 64
ALPHA = 0.125 * math.log2(math.e)


def dims(embed_dim, dim, heads, depth, n_queries, ff_inner, out_dim):
    return dict(embed_dim=embed_dim, dim=dim, heads=heads, depth=depth, n_queries=n_queries, ff_inner=ff_inner, out_dim=out_dim)


SDXL_PLUS = dims(1280, 1280, 20, 4, 16, 5120, 2048)      # ip-adapter-plus_sdxl_vit-h: 82 961 664 parameters, S = 257
SD15_PLUS = dims(1280, 768, 12, 4, 16, 3072, 768)
TINY = dims(128, 128, 2, 2, 5, 512, 192)                 # S = 10, batch 3 in the GPU test


def state_shapes(d):
    inner = d["heads"] * HEAD
    out = {"latents": (1, d["n_queries"], d["dim"]), "proj_in.weight": (d["dim"], d["embed_dim"]), "proj_in.bias": (d["dim"],),
           "proj_out.weight": (d["out_dim"], d["dim"]), "proj_out.bias": (d["out_dim"],), "norm_out.weight": (d["out_dim"],),
           "norm_out.bias": (d["out_dim"],)}
    for l in range(d["depth"]):
        for n in ("norm1", "norm2"):
            out[f"layers.{l}.0.{n}.weight"] = out[f"layers.{l}.0.{n}.bias"] = (d["dim"],)
        out[f"layers.{l}.0.to_q.weight"] = (inner, d["dim"])
        out[f"layers.{l}.0.to_kv.weight"] = (2 * inner, d["dim"])
        out[f"layers.{l}.0.to_out.weight"] = (d["dim"], inner)
        out[f"layers.{l}.1.0.weight"] = out[f"layers.{l}.1.0.bias"] = (d["dim"],)
        out[f"layers.{l}.1.1.weight"] = (d["ff_inner"], d["dim"])
        out[f"layers.{l}.1.3.weight"] = (d["dim"], d["ff_inner"])
    return out


def n_params(d):
    return sum(math.prod(s) for s in state_shapes(d).values())


def random_state_dict(d, seed=0, gain=1.0):
    """Linear weights N(0, gain^2 / fan_in), `latents` N(0, 1 / dim) as the published initialisation, LayerNorm weights around
    1, biases around 0; matrices and latents rounded to bf16"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in state_shapes(d).items():
        if k == "latents":
            t = (torch.randn(shape, generator=g) * shape[-1] ** -0.5).to(torch.bfloat16).float()
        elif len(shape) == 2:
            t = (torch.randn(shape, generator=g) * gain * shape[1] ** -0.5).to(torch.bfloat16).float()
        elif k.endswith(".weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        sd[k] = t
    return sd


def _st(t, on):
    return t.to(torch.bfloat16).to(t.dtype) if on else t


def resampler_ref(sd, hidden, dtype=torch.float64, store=False):
    """hidden [B, S, embed_dim] -> tokens [B, Nq, out_dim] in `dtype`.  The states enter as the HIP tape reads them: rounded to bf16."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    st = lambda t: _st(t, store)
    depth = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("layers."))
    x = hidden.to(torch.bfloat16).to(dtype)
    B = x.shape[0]
    dim = w["latents"].shape[-1]
    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), w[p + ".weight"], w[p + ".bias"], 1e-5)
    latents = w["latents"].repeat(B, 1, 1)
    x = st(F.linear(x, w["proj_in.weight"], w["proj_in.bias"]))
    for l in range(depth):
        a, f = f"layers.{l}.0", f"layers.{l}.1"
        xn, lt = st(ln(x, a + ".norm1")), st(ln(latents, a + ".norm2"))
        q = F.linear(lt, w[a + ".to_q.weight"])
        k, v = st(F.linear(torch.cat([xn, lt], dim=1), w[a + ".to_kv.weight"])).chunk(2, dim=-1)
        if store:
            q = st(q * ALPHA) / ALPHA                               # Q leaves its projection prescaled, rounded once
        H = q.shape[-1] // HEAD
        heads = lambda t: t.view(B, t.shape[1], H, HEAD).transpose(1, 2)
        q, k, v = heads(q), heads(k), heads(v)
        s = (q * HEAD ** -0.25) @ (k * HEAD ** -0.25).transpose(-1, -2)
        p = torch.softmax(s, dim=-1)
        o = st((st(p) @ v).transpose(1, 2).reshape(B, -1, H * HEAD))
        latents = st(F.linear(o, w[a + ".to_out.weight"]) + latents)
        n = st(ln(latents, f + ".0"))
        h = st(F.gelu(F.linear(n, w[f + ".1.weight"])))
        latents = st(F.linear(h, w[f + ".3.weight"]) + latents)
    y = st(F.linear(latents, w["proj_out.weight"], w["proj_out.bias"]))
    assert dim == latents.shape[-1]
    return st(ln(y, "norm_out"))


def plus_file(unet_ref, sd):
    """{"image_proj": the Resampler, "ip_adapter": {"<i>.to_k_ip.weight": ...}} from an oracle UNet after ip_adapter_ref.attach_ip"""
    from ip_adapter_ref import file_state_dict
    return file_state_dict(unet_ref, sd)


# ---- the cases the CPU and the GPU tests share: inputs, the fp32 restatement and its bf16-storage floor, computed once
FULL_SEED, FULL_BATCH, FULL_S = 11, 2, 257
TINY_SEED, TINY_BATCH, TINY_S = 12, 3, 10


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (dims, state dict, hidden [B, S, embed_dim], fp32-path tokens, bf16-storage tokens).  "full": SDXL plus in float32
    (82 961 664 parameters: float64 would double a 330 MB table for nothing the bound can see), "tiny": float64."""
    d, seed, B, S, dt = (SDXL_PLUS, FULL_SEED, FULL_BATCH, FULL_S, torch.float32) if name == "full" else \
                        (TINY, TINY_SEED, TINY_BATCH, TINY_S, torch.float64)
    sd = random_state_dict(d, seed)
    hidden = torch.randn(B, S, d["embed_dim"], generator=torch.Generator().manual_seed(seed + 100))
    with torch.no_grad():
        want = resampler_ref(sd, hidden, dt).float()
        stored = resampler_ref(sd, hidden, dt, store=True).float()
    return d, sd, hidden, want, stored
