"""No GPU: the host half of the image prompt (IP-Adapter) -- layer numbering, the plan, the file forms and what they refuse --
and the restatement of tests/ip_adapter_ref.py against torch's own attention."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from ip_adapter_ref import (IPAttention, attach_ip, file_state_dict, image_proj_ref, ip_layers, ip_tokens_ref, make_image_proj,
                            set_ip)
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd._lib import PeaError, lib


def test_layer_keys_sdxl():
    keys = ipa.layer_keys(pc.sdxl_config())
    assert len(keys) == 70 and [i for i, _ in keys] == list(range(1, 140, 2))
    d = dict(keys)
    assert d[1] == "down_blocks.1.attentions.0.transformer_blocks.0.attn2"
    assert d[49] == "up_blocks.0.attentions.0.transformer_blocks.0.attn2"
    assert d[121] == "mid_block.attentions.0.transformer_blocks.0.attn2"
    assert d[139] == "mid_block.attentions.0.transformer_blocks.9.attn2"
    assert d[47] == "down_blocks.2.attentions.1.transformer_blocks.9.attn2"


def test_layer_keys_sd15_and_ssd1b():
    k15 = ipa.layer_keys(pc.sd15_config())
    assert len(k15) == 16 and k15[0] == (1, "down_blocks.0.attentions.0.transformer_blocks.0.attn2") and k15[-1][0] == 31
    assert k15[-1][1] == "mid_block.attentions.0.transformer_blocks.0.attn2"
    assert k15[6] == (13, "up_blocks.1.attentions.0.transformer_blocks.0.attn2")
    cfg = pc.ssd1b_config()
    down, up, mid = pc.depth_tables(cfg)
    n = sum(sum(down[i]) for i, t in enumerate(cfg.down_block_types) if t.startswith("CrossAttn"))
    n += sum(sum(up[i]) for i, t in enumerate(cfg.up_block_types) if t.startswith("CrossAttn"))
    ks = ipa.layer_keys(cfg)
    assert mid == -1 and len(ks) == n == 34 and not any(p.startswith("mid_block") for _, p in ks)
    assert ks[12] == (25, "up_blocks.0.attentions.0.transformer_blocks.0.attn2")        # 2 + 2 + 4 + 4 layers on the way down


def test_layer_keys_follow_the_oracle_modules():
    """the same order from the module tree of the oracle UNet (down, up, mid) as from the config"""
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    with torch.device("meta"):
        ref = UNet2DConditionRef(tiny_config())
    assert [n for n, _ in ip_layers(ref)] == [p for _, p in ipa.layer_keys(pc.tiny_config())]


def _plan(cfg, n):
    nl, cols, npar = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    rc = lib().pea_unet_ip_plan(ctypes.byref(pc.to_c(cfg)), n, ctypes.byref(nl), ctypes.byref(cols), ctypes.byref(npar))
    return rc, nl.value, cols.value, npar.value


def test_ip_plan():
    assert _plan(pc.sdxl_config(), 4) == (0, 70, 166400, 340787200)
    # the text K|V stack of the same graph is as wide: 2 x the channels of every cross-attention layer
    assert 166400 == 2 * sum(C for _, C in ipa._cross_layers(pc.sdxl_config()))
    rc, nl, cols, npar = _plan(pc.tiny_config(), 16)
    assert (rc, nl, npar) == (0, len(ipa.layer_keys(pc.tiny_config())), cols * 128)
    assert _plan(pc.sdxl_config(), 33)[0] != 0 and _plan(pc.sdxl_config(), 0)[0] != 0
    assert _plan(pc.sd15_config(), 4)[0] != 0 and b"head" in lib().pea_last_error()          # padded heads


def _tiny_file(n_tokens=4, embed=64):
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    torch.manual_seed(0)
    ref = UNet2DConditionRef(tiny_config())
    attach_ip(ref, n_tokens, seed=3)
    return ref, file_state_dict(ref, make_image_proj(embed, 128, n_tokens, seed=4))


def test_both_file_forms_load_alike(tmp_path):
    from safetensors.torch import save_file
    ref, sd = _tiny_file()
    torch.save(sd, str(tmp_path / "ip.bin"))
    flat = {f"{g}.{k}": v.contiguous() for g in sd for k, v in sd[g].items()}
    save_file(flat, str(tmp_path / "ip.safetensors"))
    a = ipa.load_ip_adapter_state_dict(str(tmp_path / "ip.bin"))
    b = ipa.load_ip_adapter_state_dict(str(tmp_path / "ip.safetensors"))
    for g in ("image_proj", "ip_adapter"):
        assert set(a[g]) == set(b[g]) == set(sd[g])
        assert all(torch.equal(a[g][k], b[g][k]) and torch.equal(a[g][k], sd[g][k]) for k in sd[g])
    ad = ipa.IPAdapter(str(tmp_path / "ip.safetensors"), pc.tiny_config())
    assert ad.n_tokens == 4 and ad.embed_dim == 64 and len(ad.layers) == 2 * len(ipa.layer_keys(pc.tiny_config()))
    for name, m in ip_layers(ref):
        assert torch.equal(ad.layers[name + ".to_k_ip.weight"], m.to_k_ip.weight)
        assert torch.equal(ad.layers[name + ".to_v_ip.weight"], m.to_v_ip.weight)


def test_refused_files():
    _, sd = _tiny_file()
    plus = {"image_proj": dict(sd["image_proj"], latents=torch.zeros(1, 16, 128)), "ip_adapter": sd["ip_adapter"]}
    plus["image_proj"]["layers.0.0.to_q.weight"] = torch.zeros(4, 4)
    with pytest.raises(PeaError, match="Resampler.*set_ip_tokens"):
        ipa.load_ip_adapter_state_dict(plus)
    less = {"image_proj": sd["image_proj"], "ip_adapter": {k: v for k, v in sd["ip_adapter"].items() if k != "3.to_v_ip.weight"}}
    with pytest.raises(PeaError, match="3.to_v_ip.weight"):
        ipa.IPAdapter(less, pc.tiny_config())
    more = {"image_proj": sd["image_proj"], "ip_adapter": dict(sd["ip_adapter"], **{"99.to_k_ip.weight": torch.zeros(64, 128)})}
    with pytest.raises(PeaError, match="99.to_k_ip"):
        ipa.IPAdapter(more, pc.tiny_config())
    with pytest.raises(PeaError):                                    # a file for cross_attention_dim 128 on a 2048-wide UNet
        ipa.IPAdapter(sd, pc.sdxl_config())
    _, sd96 = _tiny_file()
    sd96["image_proj"]["norm.weight"] = torch.ones(96)
    with pytest.raises(PeaError, match="cross_attention_dim"):
        ipa.IPAdapter(sd96, pc.tiny_config())
    _, sd33 = _tiny_file(n_tokens=33)
    with pytest.raises(PeaError, match="33 image tokens"):
        ipa.IPAdapter(sd33, pc.tiny_config())


@pytest.mark.parametrize("scale", [0.6, -1.0])
def test_restated_layer_is_two_sdpa(scale):
    torch.manual_seed(1)
    B, S, L, N, C, H, cross = 2, 24, 9, 4, 128, 2, 96
    m = IPAttention(C, H, cross, N).double()
    x, ctx, tok = torch.randn(B, S, C).double(), torch.randn(B, L, cross).double(), torch.randn(B, N, cross).double()
    m.tokens, m.scale = tok, scale
    heads = lambda t: t.view(B, -1, H, C // H).transpose(1, 2)
    q = heads(m.to_q(x))
    o = F.scaled_dot_product_attention(q, heads(m.to_k(ctx)), heads(m.to_v(ctx)))
    o = o + scale * F.scaled_dot_product_attention(q, heads(m.to_k_ip(tok)), heads(m.to_v_ip(tok)))
    want = m.to_out[0](o.transpose(1, 2).reshape(B, S, C))
    torch.testing.assert_close(m(x, ctx), want, rtol=1e-12, atol=1e-12)
    cat = torch.softmax(q @ torch.cat([heads(m.to_k(ctx)), heads(m.to_k_ip(tok))], 2).transpose(-1, -2) * (C // H) ** -0.5, -1)
    joint = m.to_out[0]((cat @ torch.cat([heads(m.to_v(ctx)), heads(m.to_v_ip(tok))], 2)).transpose(1, 2).reshape(B, S, C))
    assert (m(x, ctx) - joint).abs().max() > 1e-3                   # not one softmax over the concatenated keys


def test_oracle_with_ip_at_scale_zero_is_the_plain_oracle():
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    cfg = tiny_config()
    torch.manual_seed(0)
    ref = UNet2DConditionRef(cfg)
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 4, 16, 16, generator=g), torch.tensor([10, 500])
    ehs = torch.randn(2, 7, cfg.cross_attention_dim, generator=g)
    added = {"text_embeds": torch.randn(2, cfg.pooled_dim, generator=g), "time_ids": torch.tensor([[128, 128, 0, 0, 128, 128]] * 2)}
    tok = torch.randn(2, 4, cfg.cross_attention_dim, generator=g)
    with torch.no_grad():
        plain = ref(x, t, ehs, added_cond_kwargs=added)[0]
        attach_ip(ref, 4, seed=3)
        assert torch.equal(ref(x, t, ehs, added_cond_kwargs=added)[0], plain)       # attached, no tokens
        set_ip(ref, tok, 0.0)
        assert torch.equal(ref(x, t, ehs, added_cond_kwargs=added)[0], plain)       # through the decoupled forward, weight 0
        set_ip(ref, tok, 0.7)
        assert not torch.equal(ref(x, t, ehs, added_cond_kwargs=added)[0], plain)


def test_restated_projection_and_cfg_rule():
    proj = make_image_proj(64, 128, 4, seed=4)
    e = torch.randn(3, 64, generator=torch.Generator().manual_seed(2))
    t = image_proj_ref(proj, e)
    assert t.shape == (3, 4, 128)
    y = (e.to(torch.bfloat16).double() @ proj["proj.weight"].double().T + proj["proj.bias"].double()).view(3, 4, 128)
    yn = (y - y.mean(-1, keepdim=True)) / (y.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    torch.testing.assert_close(t, yn * proj["norm.weight"].double() + proj["norm.bias"].double(), rtol=1e-10, atol=1e-10)
    c = ip_tokens_ref(proj, e, do_cfg=True)
    assert c.shape == (6, 4, 128) and torch.equal(c[3:], t)
    assert torch.equal(c[:3], image_proj_ref(proj, torch.zeros(3, 64))) and torch.equal(c[0], c[1])
