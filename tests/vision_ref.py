"""CPU restatement (pure torch, fp32) of the CLIP vision tower, of `vision.preprocess` and of the CLIPScore, and -- under
`__main__` -- the generator of tests/golden/vision_clip*.npz from the installed transformers'
`CLIPVisionModelWithProjection` (weights rounded to bf16 first, as the text goldens are).  The GPU tests read only the
.npz files and this restatement: the GPU machine may not have transformers.

    python tests/vision_ref.py            # rewrites the three goldens
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from pea_diffusion_amd import config as pc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FIELDS = ("image_size", "patch_size", "hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size",
           "projection_dim")


def golden_configs():
    return {
        "vision_clip": pc.tiny_vit_config(),                    # 17 tokens, K = 588 -> 640, quick-GELU
        "vision_clip_p32": pc.VisionConfig(image_size=64, patch_size=32, hidden_size=128, num_attention_heads=2,
                                           num_hidden_layers=2, intermediate_size=256, hidden_act="gelu", projection_dim=64,
                                           name="tiny_vit_p32"),    # 5 tokens, K = 3072 (unpadded), GELU
        "vision_clip_h80": pc.tiny_vit_h80_config(),            # head_dim 80
    }


# ---------------------------------------------------------------- the tower
def _act(x, name):
    return x * torch.sigmoid(1.702 * x) if name == "quick_gelu" else F.gelu(x)


def tower_ref(sd, cfg, pixels):
    """-> dict(hidden_states=[h_0 .. h_N], last_hidden_state, pooler_output, image_embeds); sd: HF keys, fp32 tensors"""
    sd = {k: v.float() for k, v in sd.items()}
    px = pixels.float()
    B, P, W, H = px.shape[0], cfg.patch_size, cfg.hidden_size, cfg.num_attention_heads
    G = cfg.image_size // P
    d = W // H
    e = "vision_model.embeddings."
    rows = px.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * P * P)      # column (c, py, px)
    x = rows @ sd[e + "patch_embedding.weight"].reshape(W, -1).t()
    x = torch.cat([sd[e + "class_embedding"].reshape(1, 1, W).expand(B, 1, W), x], 1) + sd[e + "position_embedding.weight"][None]
    ln = lambda t, p: F.layer_norm(t, (W,), sd[p + ".weight"], sd[p + ".bias"], cfg.layer_norm_eps)
    lin = lambda t, p: t @ sd[p + ".weight"].t() + sd[p + ".bias"]
    x = ln(x, "vision_model.pre_layrnorm")
    hs = [x]
    for i in range(cfg.num_hidden_layers):
        p = f"vision_model.encoder.layers.{i}"
        n = ln(x, p + ".layer_norm1")
        q, k, v = (lin(n, f"{p}.self_attn.{t}_proj").reshape(B, -1, H, d).transpose(1, 2) for t in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1) @ v
        x = x + lin(a.transpose(1, 2).reshape(B, -1, W), p + ".self_attn.out_proj")
        x = x + lin(_act(lin(ln(x, p + ".layer_norm2"), p + ".mlp.fc1"), cfg.hidden_act), p + ".mlp.fc2")
        hs.append(x)
    pooled = ln(x[:, 0], "vision_model.post_layernorm")
    return {"hidden_states": hs, "last_hidden_state": x, "pooler_output": pooled,
            "image_embeds": pooled @ sd["visual_projection.weight"].t()}


def random_state_dict(cfg, seed=0):
    """bf16-exact weights on a 1/64 grid (few distinct values: the goldens compress below the repository's file limit)"""
    g = torch.Generator().manual_seed(seed)
    W, I, P, L = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size, cfg.num_tokens
    grid = lambda shape, std: (torch.randn(shape, generator=g) * std * 64).round().clamp(-100, 100) / 64
    sd = {"vision_model.embeddings.class_embedding": grid((W,), 0.25),
          "vision_model.embeddings.patch_embedding.weight": grid((W, 3, P, P), 0.04),
          "vision_model.embeddings.position_embedding.weight": grid((L, W), 0.25),
          "visual_projection.weight": grid((cfg.projection_dim, W), 0.08)}
    norms = ["vision_model.pre_layrnorm", "vision_model.post_layernorm"]
    for i in range(cfg.num_hidden_layers):
        p = f"vision_model.encoder.layers.{i}"
        norms += [p + ".layer_norm1", p + ".layer_norm2"]
        for t, (n, k) in {"self_attn.q_proj": (W, W), "self_attn.k_proj": (W, W), "self_attn.v_proj": (W, W),
                          "self_attn.out_proj": (W, W), "mlp.fc1": (I, W), "mlp.fc2": (W, I)}.items():
            sd[f"{p}.{t}.weight"] = grid((n, k), 0.08)
            sd[f"{p}.{t}.bias"] = grid((n,), 0.1)
    for p in norms:
        sd[p + ".weight"] = 1.0 + grid((W,), 0.1)
        sd[p + ".bias"] = grid((W,), 0.1)
    for v in sd.values():
        assert torch.equal(v, v.to(torch.bfloat16).float())
    return sd


# ---------------------------------------------------------------- preprocessing and the score
def preprocess_ref(images, size, mean, std, value_range=(-1.0, 1.0), quantize=True):
    lo, hi = value_range
    x = ((images.float() - lo) / (hi - lo)).clamp(0.0, 1.0)
    if quantize:
        x = torch.round(x * 255.0) / 255.0
    H, W = x.shape[-2:]
    Hr, Wr = (size, int(size * W / H)) if H <= W else (int(size * H / W), size)
    x = F.interpolate(x, size=(Hr, Wr), mode="bicubic", antialias=True, align_corners=False)
    top, left = int(round((Hr - size) / 2.0)), int(round((Wr - size) / 2.0))
    x = x[:, :, top:top + size, left:left + size]
    m, s = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (mean, std))
    return (x - m) / s


def clip_score_ref(image_embeds, text_embeds, w=2.5, clamp=True):
    c = F.cosine_similarity(image_embeds.float(), text_embeds.float(), dim=-1)
    return w * (c.clamp(min=0.0) if clamp else c)


# ---------------------------------------------------------------- goldens
def _bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def load_golden(name):
    """-> (cfg, state dict fp32, {pixels, hidden_states [N+1,B,L,W], last_hidden_state, pooler_output, image_embeds})"""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    cfg = pc.VisionConfig(**{f: int(z["cfg:" + f]) for f in _FIELDS}, hidden_act=str(z["cfg:hidden_act"]),
                          layer_norm_eps=float(z["cfg:layer_norm_eps"]), name=name)
    sd = {k[2:]: torch.from_numpy(z[k].view(np.int16).copy()).view(torch.bfloat16).float() for k in z.files if k.startswith("w:")}
    out = {k: torch.from_numpy(z[k]) for k in ("pixels", "hidden_states", "last_hidden_state", "pooler_output", "image_embeds")}
    return cfg, sd, out


def hf_model(cfg, sd):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    hc = CLIPVisionConfig(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, projection_dim=cfg.projection_dim,
                          num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                          image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_act=cfg.hidden_act,
                          layer_norm_eps=cfg.layer_norm_eps)
    m = CLIPVisionModelWithProjection(hc).eval()
    if sd is not None:
        m.load_state_dict({k: v.reshape(m.state_dict()[k].shape) for k, v in sd.items()}, strict=True)
    return m


def hf_outputs(cfg, sd, pixels):
    with torch.no_grad():
        o = hf_model(cfg, sd)(pixel_values=pixels, output_hidden_states=True)
    return {"hidden_states": torch.stack(list(o.hidden_states)), "last_hidden_state": o.last_hidden_state,
            "pooler_output": o.pooler_output if getattr(o, "pooler_output", None) is not None else None,
            "image_embeds": o.image_embeds}


if __name__ == "__main__":
    for i, (name, cfg) in enumerate(golden_configs().items()):
        sd = random_state_dict(cfg, seed=100 + i)
        pixels = torch.randn(2, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(7 + i))
        out = hf_outputs(cfg, sd, pixels)
        if out["pooler_output"] is None:       # the projection model's output carries no pooler_output: take it from the inner model
            with torch.no_grad():
                out["pooler_output"] = hf_model(cfg, sd).vision_model(pixel_values=pixels).pooler_output
        arrays = {"w:" + k: _bf16_bits(v) for k, v in sd.items()}
        arrays.update({"cfg:" + f: np.array(getattr(cfg, f)) for f in _FIELDS})
        arrays["cfg:hidden_act"], arrays["cfg:layer_norm_eps"] = np.array(cfg.hidden_act), np.array(cfg.layer_norm_eps)
        arrays["pixels"] = pixels.numpy()
        arrays.update({k: v.numpy() for k, v in out.items()})
        path = os.path.join(GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {sum(v.numel() for v in sd.values())} parameters, {cfg.num_tokens} tokens, {os.path.getsize(path)} bytes")
