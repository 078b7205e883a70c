"""CPU (no device): the planning entry points of the C ABI give, for every graph the product builds, exactly what they gave when
tests/golden/tape_plans.json was recorded -- op, weight and parameter counts, the three arena sizes (weights, activations,
gradients), the scratch bytes, the attention census and a SHA-256 over the weight table.  The arena sizes follow the order in
which the graph builders create tensors, weight slots and fused matrices, so a builder that creates one more, one fewer or a
differently shaped one moves a number here.  Re-record only when a graph is meant to change:
`python tests/test_plan_golden_cpu.py --record`."""
import ctypes
import dataclasses
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import unet_ref  # noqa: E402
from pea_diffusion_amd import config as pc  # noqa: E402
from pea_diffusion_amd._lib import check, lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tape_plans.json")

# (config, latent size, context length, flags): the shapes of test_attn_census_cpu.py at inference / needs_grad / residual
# inputs, the inpainting inputs and the guidance-embedded LCM UNet
UNETS = [(name, hw, L, flags)
         for name, hw, L in [("sdxl_config", 128, 77), ("sdxl_config", 64, 52), ("sd15_config", 64, 77), ("ssd1b_config", 128, 77),
                             ("ssd1b_uniform_config", 64, 77), ("tiny_config", 16, 12), ("tiny15_config", 16, 12)]
         for flags in (0, 1, 2)] + [("sdxl_inpaint_config", 128, 77, 4), ("lcm_sdxl_config", 128, 77, 0)]
TEXTS = [("clip_l_config", 77), ("openclip_bigg_config", 77), ("cnclip_bert_large_config", 52), ("xlm_roberta_large_config", 77),
         ("mt5_xl_config", 77), ("tiny_clip_config", 12), ("tiny_bert_config", 12), ("tiny_xlmr_config", 12), ("tiny_t5_config", 12)]
VISIONS = ["clip_vit_b32_config", "clip_vit_l14_config", "clip_vit_h14_config"]


def _unet_keys(cfg):
    """state-dict keys of the UNet in the reference module's order (built on the meta device: names only)"""
    ref_cfg = unet_ref.UNetConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(unet_ref.UNetConfig)})
    with torch.device("meta"):
        keys = list(unet_ref.UNet2DConditionRef(ref_cfg).state_dict().keys())
    if cfg.time_cond_proj_dim and "time_embedding.cond_proj.weight" not in keys:
        keys.append("time_embedding.cond_proj.weight")
    return keys


def _unet_plan(name, hw, L, flags):
    cfg = getattr(pc, name)()
    c, tcd = pc.to_c(cfg), pc.time_cond_dim(cfg)
    n_ops, n_w, n_attn, n_pre = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n_par, wb, ab, gb, sb = (ctypes.c_longlong() for _ in range(5))
    check(lib().pea_unet_plan_cond(ctypes.byref(c), 2, hw, hw, L, flags, tcd, ctypes.byref(n_ops), ctypes.byref(n_w),
                                   ctypes.byref(n_par), ctypes.byref(wb), ctypes.byref(ab), ctypes.byref(gb), ctypes.byref(n_attn),
                                   ctypes.byref(n_pre)))
    out = {"n_ops": n_ops.value, "n_weights": n_w.value, "n_params": n_par.value, "weight_bytes": wb.value,
           "activation_bytes": ab.value, "grad_bytes": gb.value, "n_attn": n_attn.value, "n_prescaled": n_pre.value}
    if not tcd:        # (pea_unet_plan / pea_unet_plan_scratch carry no guidance-embedding width)
        check(lib().pea_unet_plan_scratch(ctypes.byref(c), 2, hw, hw, L, flags, 0, ctypes.byref(sb)))
        out["scratch_bytes"] = sb.value
        check(lib().pea_unet_plan(ctypes.byref(c), 2, hw, hw, L, flags, ctypes.byref(n_ops), ctypes.byref(n_w), ctypes.byref(n_par),
                                  ctypes.byref(wb), ctypes.byref(ab), ctypes.byref(gb)))
        assert (n_ops.value, n_w.value, n_par.value, wb.value, ab.value, gb.value) == tuple(
            out[k] for k in ("n_ops", "n_weights", "n_params", "weight_bytes", "activation_bytes", "grad_bytes"))
    return out


def _weights_sha(name):
    """SHA-256 over (key, numel, kind, d0, d1) of the config's weights in the reference module's key order.  The by-name planner
    rebuilds the graph for every lookup (about 2 ms at SDXL size, 1680 keys), so the full-size configs hash an evenly strided
    sample of at most 128 keys and the tiny ones, which go through every builder path, hash every key; the table does not depend
    on shape or flags.  n_weights, n_params and weight_bytes above pin the totals of the whole table."""
    cfg = getattr(pc, name)()
    c, tcd = pc.to_c(cfg), pc.time_cond_dim(cfg)
    keys = _unet_keys(cfg)
    n_w = ctypes.c_int()
    check(lib().pea_unet_plan_cond(ctypes.byref(c), 1, 16, 16, 12, 0, tcd, None, ctypes.byref(n_w), None, None, None, None, None, None))
    assert len(keys) == n_w.value, (name, len(keys), n_w.value)
    h = hashlib.sha256()
    numel, kind, d0, d1 = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for k in keys[::max(1, len(keys) // 128)]:
        check(lib().pea_unet_plan_weight(ctypes.byref(c), 1, 16, 16, 12, 0, tcd, k.encode(), ctypes.byref(numel),
                                         ctypes.byref(kind), ctypes.byref(d0), ctypes.byref(d1)))
        h.update(repr((k, numel.value, kind.value, d0.value, d1.value)).encode())
    return h.hexdigest()


def _census(fn, *args):
    n, pre = ctypes.c_int(), ctypes.c_int()
    check(fn(*args, ctypes.byref(n), ctypes.byref(pre)))
    return [n.value, pre.value]


def _collect():
    plans = {}
    for name, hw, L, flags in UNETS:
        plans[f"unet/{name}/{hw}/{L}/flags{flags}"] = _unet_plan(name, hw, L, flags)
    for name in sorted({u[0] for u in UNETS}):
        plans[f"unet_weights/{name}"] = _weights_sha(name)
    for name, L in TEXTS:
        plans[f"text/{name}/{L}"] = _census(lib().pea_text_plan_attention, ctypes.byref(pc.text_to_c(getattr(pc, name)())), 2, L)
    for name, hw in (("sdxl_config", 128), ("tiny_config", 16)):
        plans[f"controlnet/{name}/{hw}"] = _census(lib().pea_graph_plan_attention, 2, ctypes.byref(pc.to_c(getattr(pc, name)())), 2,
                                                   hw, hw, 77)
    vae = pc.sdxl_vae_config()
    plans["vae_encoder/sdxl"] = _census(lib().pea_graph_plan_attention, 1, ctypes.byref(pc.vae_to_c(vae)), 1, 128, 128, 0)
    plans["vae_decoder/sdxl"] = _census(lib().pea_graph_plan_attention, 3, ctypes.byref(pc.vae_decoder_to_c(vae)), 1, 16, 16, 0)
    for name in VISIONS:
        n, t, a = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
        check(lib().pea_vision_plan(ctypes.byref(pc.vision_to_c(getattr(pc, name)())), 2, ctypes.byref(n), ctypes.byref(t),
                                    ctypes.byref(a)))
        plans[f"vision/{name}"] = [n.value, t.value, a.value]
    return plans


@pytest.fixture(scope="module")
def plans():
    return _collect()


def test_every_graph_plans_as_recorded(plans):
    golden = json.load(open(GOLDEN))
    assert sorted(plans) == sorted(golden)
    for key in golden:
        assert plans[key] == golden[key], key


def test_the_recorded_plans_cover_every_graph_family():
    golden = json.load(open(GOLDEN))
    assert len(golden) == len(UNETS) + len({u[0] for u in UNETS}) + len(TEXTS) + 2 + 2 + len(VISIONS)
    assert golden["unet/sdxl_config/128/77/flags0"]["n_attn"] == 140          # 70 transformer blocks x (self + cross)
    assert golden["unet/sdxl_config/128/77/flags0"]["n_params"] == 2567463684


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    json.dump(_collect(), open(GOLDEN, "w"), indent=1, sort_keys=True)
    print("recorded", GOLDEN)
