"""CLIP vision tower, CPU side: the goldens against the installed transformers, the restatement against the goldens, the host
resampling tables against `F.interpolate(antialias=True)`, and the host-only planner."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vision_ref as vr  # noqa: E402

from pea_diffusion_amd import _lib, config as pc, vision  # noqa: E402

GOLDENS = ("vision_clip", "vision_clip_p32", "vision_clip_h80")


@pytest.fixture(scope="module")
def goldens():
    return {n: vr.load_golden(n) for n in GOLDENS}


def test_golden_shapes_and_size(goldens):
    assert [goldens[n][0].num_tokens for n in GOLDENS] == [17, 5, 17]
    assert goldens["vision_clip_h80"][0].hidden_size // goldens["vision_clip_h80"][0].num_attention_heads == 80
    assert 3 * goldens["vision_clip"][0].patch_size ** 2 == 588            # the padded K
    for n in GOLDENS:
        cfg, sd, out = goldens[n]
        assert os.path.getsize(os.path.join(vr.GOLDEN_DIR, n + ".npz")) < 1 << 20
        assert out["hidden_states"].shape == (cfg.num_hidden_layers + 1, 2, cfg.num_tokens, cfg.hidden_size)
        assert torch.equal(out["hidden_states"][-1], out["last_hidden_state"])
        assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values())


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_equal_installed_transformers(goldens, name):
    pytest.importorskip("transformers")
    cfg, sd, out = goldens[name]
    m = vr.hf_model(cfg, sd)
    assert set(m.state_dict()) == set(sd)
    with torch.no_grad():
        o = m(pixel_values=out["pixels"], output_hidden_states=True)
        pooled = m.vision_model(pixel_values=out["pixels"]).pooler_output
    assert len(o.hidden_states) == cfg.num_hidden_layers + 1
    for k, h in enumerate(o.hidden_states):
        torch.testing.assert_close(h, out["hidden_states"][k], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o.last_hidden_state, out["last_hidden_state"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pooled, out["pooler_output"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o.image_embeds, out["image_embeds"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_goldens(goldens, name):
    """fp32 round-off: two summation orders of O(1) values over at most 3072 terms"""
    cfg, sd, out = goldens[name]
    r = vr.tower_ref(sd, cfg, out["pixels"])
    for k, h in enumerate(r["hidden_states"]):
        torch.testing.assert_close(h, out["hidden_states"][k], rtol=1e-4, atol=5e-5)
    for key in ("last_hidden_state", "pooler_output", "image_embeds"):
        torch.testing.assert_close(r[key], out[key], rtol=1e-4, atol=5e-5)


CASES = [(96, 160, 42), (64, 64, 56), (40, 40, 56), (56, 56, 56)]


@pytest.mark.parametrize("H,W,size", CASES)
def test_host_tap_tables_reproduce_interpolate(H, W, size):
    ty, tx = vision.resample_taps(H, W, size)
    assert len(ty.first) == len(tx.first) == size
    np.testing.assert_allclose(ty.weights.sum(1), 1.0, atol=1e-12)
    np.testing.assert_allclose(tx.weights.sum(1), 1.0, atol=1e-12)
    assert (ty.first >= 0).all() and (ty.first + ty.count <= H).all() and (tx.first >= 0).all() and (tx.first + tx.count <= W).all()
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H + W))
    x[0, :, 0, :] = 4.0                       # a bright border row / column: a table shifted by one moves it
    x[0, :, :, -1] = -3.0
    ref = vr.preprocess_ref(x, size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), value_range=(-4.0, 4.0), quantize=False)
    ref01 = (x + 4.0) / 8.0                   # the same map applied by hand, then the tables on it
    got = torch.einsum("ih,bchw,jw->bcij", torch.from_numpy(ty.dense()), ref01.double(), torch.from_numpy(tx.dense())).float()
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=2e-5)        # interpolate accumulates its taps in fp32
    if H == W == size:                        # identity: a single tap of weight 1
        assert ty.weights.shape == (size, 1) and (ty.weights == 1.0).all() and (ty.first == np.arange(size)).all()
        assert tx.weights.shape == (size, 1) and (tx.weights == 1.0).all() and (tx.first == np.arange(size)).all()
    if H < size:                              # upscale: support stays 2
        assert ty.weights.shape[1] <= 5
    th, tw, wh, ww = vision.plan_tiles(ty, tx)
    assert tw % 4 == 0 and ww % 4 == 0 and 4 * (wh * ww + wh * tw + tw * tx.weights.shape[1] + th * ty.weights.shape[1]) <= 64 * 1024


def test_reduction_from_1024_keeps_about_19_taps():
    ty, tx = vision.resample_taps(1024, 1024, 224)
    assert 18 <= ty.weights.shape[1] <= 20 and ty.weights.shape == tx.weights.shape
    vision.plan_tiles(ty, tx)


@pytest.mark.parametrize("preset", ["clip_vit_l14_config", "clip_vit_h14_config"])
def test_vision_plan_without_a_device(preset):
    cfg = getattr(pc, preset)()
    p = vision.plan(cfg)
    assert p["n_tokens"] == 257 and p["n_attn"] == cfg.num_hidden_layers
    tr = pytest.importorskip("transformers")
    with torch.device("meta"):
        m = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(
            hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, projection_dim=cfg.projection_dim,
            num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads, image_size=cfg.image_size,
            patch_size=cfg.patch_size, hidden_act=cfg.hidden_act))
    assert p["n_params"] == sum(q.numel() for q in m.parameters())


def test_vit_h14_preset():
    c = pc.clip_vit_h14_config()
    assert (c.hidden_size, c.num_attention_heads, c.num_hidden_layers, c.intermediate_size, c.hidden_act, c.projection_dim) == \
        (1280, 16, 32, 5120, "gelu", 1024)
    assert pc.clip_vit_b32_config().num_tokens == 50


def test_head_dim_96_is_refused():
    L = _lib.lib()
    c = pc.vision_to_c(pc.VisionConfig(hidden_size=384, num_attention_heads=4))
    assert L.pea_vision_plan(ctypes.byref(c), 1, None, None, None) == -3          # PEA_E_SHAPE
    assert b"head width 96" in L.pea_last_error()
    assert L.pea_vision_plan(None, 1, None, None, None) == -1
