"""No GPU: the host side of the IP-Adapter "plus" path -- the Resampler tape's planner and weight table against the restatement
of tests/resampler_ref.py, the plus file loader and its refusals, the shape refusals of pea_op_attention_fwd_fewq, and the
conditions the GPU tests (tests/test_ip_adapter_plus_gpu.py) rely on, checked on the fp32 references alone."""
import ctypes
import math

import pytest
import torch

import resampler_ref as rr
from ip_adapter_ref import attach_ip, file_state_dict, make_image_proj
from pea_diffusion_amd import _lib
from pea_diffusion_amd import config as pc
from pea_diffusion_amd import ip_adapter as ipa
from pea_diffusion_amd._lib import PeaError

from test_turbo_gpu import FLOOR_DEGENERATE  # noqa: E402


def _rc(d):
    return pc.ResamplerConfig(**d)


@pytest.mark.parametrize("name,d,total", [("sdxl", rr.SDXL_PLUS, 82_961_664), ("sd15", rr.SD15_PLUS, None)])
def test_plan_and_weight_table_without_a_device(name, d, total):
    sd_shapes = rr.state_shapes(d)
    want = sum(math.prod(s) for s in sd_shapes.values())
    assert total is None or want == total
    preset = pc.sdxl_plus_resampler_config() if name == "sdxl" else pc.sd15_plus_resampler_config()
    assert preset == _rc(d)
    p = ipa.resampler_plan(preset, batch=2, seq=257)
    assert p["n_params"] == want
    assert p["n_attn"] == d["depth"] == p["n_prescaled"]             # every latent Q leaves its projection prescaled
    assert ipa.resampler_weight_table(preset, 2, 257) == sd_shapes == ipa.resampler_keys(preset)


def test_plan_refusals():
    L = _lib.lib()
    for field, value in (("dim", 100), ("n_queries", 33), ("n_queries", 0), ("heads", 0), ("ff_inner", 100), ("depth", 0)):
        c = pc.resampler_to_c(pc.ResamplerConfig(**{field: value}))
        assert L.pea_resampler_plan(ctypes.byref(c), 1, 257, None, None, None) == -3, field      # PEA_E_SHAPE
        assert b"resampler" in L.pea_last_error()
    assert L.pea_resampler_plan(None, 1, 257, None, None, None) == -1


def _tiny_plus_file(d=None, seed=5):
    """(oracle UNet with IP layers, the plus file as its `.bin` holds it) for the tiny UNet (cross_attention_dim 128)"""
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    d = d or rr.dims(128, 128, 2, 2, 4, 512, 128)
    torch.manual_seed(0)
    ref = UNet2DConditionRef(tiny_config())
    attach_ip(ref, d["n_queries"], seed=3)
    return ref, rr.plus_file(ref, rr.random_state_dict(d, seed))


def test_plus_file_round_trips(tmp_path):
    _, sd = _tiny_plus_file()
    ad = ipa.IPAdapterPlus(sd, pc.tiny_config())
    assert ad.n_tokens == 4 and ad.embed_dim == 128
    assert ad.resampler == pc.ResamplerConfig(embed_dim=128, dim=128, heads=2, depth=2, n_queries=4, ff_inner=512, out_dim=128)
    assert len(ad.layers) == 2 * len(ipa.layer_keys(pc.tiny_config()))
    base = ipa.IPAdapter(file_state_dict(_tiny_plus_file()[0], make_image_proj(64, 128, 4, seed=4)), pc.tiny_config())
    assert set(ad.layers) == set(base.layers)                       # the same per-layer map as the base adapter's
    path = tmp_path / "ip-adapter-plus.bin"
    torch.save(sd, path)                                            # `.bin`: nested
    flat = {f"{g}.{k}": v for g, grp in sd.items() for k, v in grp.items()}          # `.safetensors`: flat, group prefix
    for src in (str(path), flat):
        again = ipa.load_ip_adapter_plus_state_dict(src)
        assert set(again) == {"image_proj", "ip_adapter"}
        for g in again:
            assert set(again[g]) == set(sd[g]) and all(torch.equal(again[g][k], sd[g][k]) for k in sd[g])
        assert ipa.IPAdapterPlus(src, pc.tiny_config()).resampler == ad.resampler


def test_refused_plus_files():
    cfg = pc.tiny_config()
    _, sd = _tiny_plus_file()
    ip = sd["image_proj"]
    edit = lambda **kw: {"image_proj": {k: v for k, v in dict(ip, **kw).items() if v is not None}, "ip_adapter": sd["ip_adapter"]}
    # head width: to_q of 2 x 32 rows against a to_kv of 2 x 128, and a width of 96 (not a multiple of 64)
    with pytest.raises(PeaError, match="64 wide"):
        ipa.IPAdapterPlus(edit(**{"layers.0.0.to_q.weight": torch.zeros(64, 128), "layers.1.0.to_q.weight": torch.zeros(64, 128)}), cfg)
    with pytest.raises(PeaError, match="64 wide"):
        ipa.IPAdapterPlus(edit(**{f"layers.{l}.0.{n}.weight": torch.zeros(r, 128) for l in (0, 1)
                                  for n, r in (("to_q", 96), ("to_kv", 192))}), cfg)
    _, sd33 = _tiny_plus_file(rr.dims(128, 128, 2, 2, 33, 512, 128))
    with pytest.raises(PeaError, match="33 image tokens"):
        ipa.IPAdapterPlus(sd33, cfg)
    _, sd192 = _tiny_plus_file(rr.dims(128, 128, 2, 2, 4, 512, 192))
    with pytest.raises(PeaError, match="cross_attention_dim"):
        ipa.IPAdapterPlus(sd192, cfg)
    with pytest.raises(PeaError, match="layers.1.1.3.weight"):      # a key missing ...
        ipa.IPAdapterPlus(edit(**{"layers.1.1.3.weight": None}), cfg)
    with pytest.raises(PeaError, match="layers.0.0.extra"):         # ... and one too many
        ipa.IPAdapterPlus(edit(**{"layers.0.0.extra.weight": torch.zeros(4)}), cfg)
    with pytest.raises(PeaError, match="expected"):                 # a shape the other tensors contradict
        ipa.IPAdapterPlus(edit(**{"layers.1.0.norm1.bias": torch.zeros(64)}), cfg)
    less = {"image_proj": ip, "ip_adapter": {k: v for k, v in sd["ip_adapter"].items() if k != "3.to_v_ip.weight"}}
    with pytest.raises(PeaError, match="3.to_v_ip.weight"):         # the shared layer map
        ipa.IPAdapterPlus(less, cfg)
    # each loader refuses the other kind of file
    base = file_state_dict(_tiny_plus_file()[0], make_image_proj(64, 128, 4, seed=4))
    with pytest.raises(PeaError, match="not a 'plus' file"):
        ipa.load_ip_adapter_plus_state_dict(base)
    with pytest.raises(PeaError, match="not a 'plus' file"):
        ipa.IPAdapterPlus(base, cfg)
    with pytest.raises(PeaError, match="Resampler.*set_ip_tokens"):
        ipa.load_ip_adapter_state_dict(sd)
    with pytest.raises(PeaError, match="IPAdapterPlus"):
        ipa.IPAdapter(sd, cfg)


def test_fewq_shape_errors_are_reported_without_gpu():
    """every refusal of the launcher comes back as PEA_E_SHAPE before anything touches a device (null operands would fault)"""
    L = _lib.lib()
    q = ctypes.c_void_p(4096)                                       # never dereferenced: an aligned non-null address
    base = dict(Q=q, ldq=128, K=q, ldk=128, V=q, ldv=128, K2=q, ldk2=128, V2=q, ldv2=128, O=q, ldo=128, lse=None, B=1, H=2, Sq=16,
                Skv=257, Skv2=16, scale=0.125, nd=1, pre=0, stream=None)                 # argument order of the prototype
    call = lambda **kw: L.pea_op_attention_fwd_fewq(*{**base, **kw}.values())
    for kw, msg in ((dict(Sq=33), b"at most 32 queries"), (dict(Skv2=33), b"0..32 keys"), (dict(nd=2), b"head_dim 64"),
                    (dict(V2=None), b"both K2 and V2"), (dict(K2=None), b"both K2 and V2"), (dict(Skv2=0), b"Skv2=0 with"),
                    (dict(K2=None, V2=None), b"Skv2=16 without"), (dict(ldk=132), b"multiples of 8"),
                    (dict(ldq=64), b"hold every head"), (dict(ldv2=120), b"ldk2 / ldv2"), (dict(ldo=130), b"ldo"),
                    (dict(Skv=0), b"empty problem"), (dict(Sq=0), b"empty problem")):
        assert call(**kw) == -3, kw
        assert msg in L.pea_last_error(), (kw, L.pea_last_error())


# ---------------------------------------------------------------------------------------------- what the GPU tests rely on
def test_gpu_test_conditions_hold_on_the_references():
    """the fp32 references alone: the spiked keys of tests/test_ip_adapter_plus_gpu.py dominate by more than 100 logits while
    every other logit stays small (so the reference output IS the spiked value row, exactly), the monotone case's block maxima
    rise strictly, and neither Resampler case has a degenerate storage floor"""
    import test_ip_adapter_plus_gpu as tg
    for where in ("set1", "set2"):
        q, k, v, k2, v2, j = tg.spiked_inputs(where)
        ks, vs = torch.cat([k, k2], 1).float(), torch.cat([v, v2], 1).float()
        o, _ = tg.sdpa_union(q.float(), ks, vs, tg.SPIKE_H)
        heads = lambda t: t.view(t.shape[0], t.shape[1], tg.SPIKE_H, 64).transpose(1, 2)
        s = heads(q.float()) @ heads(ks).transpose(-1, -2) * 0.125
        rest = torch.cat([s[..., :j], s[..., j + 1:]], -1)
        assert (s[..., j] - rest.max(-1).values).min() > 100 and rest.abs().max() < 30
        assert torch.equal(o, vs[:, j][:, None, :].expand_as(o))
        assert k.shape[1] % 32 == 1 and j == (k.shape[1] - 1 if where == "set1" else ks.shape[1] - 1)
    q, k, v, k2, v2 = tg.monotone_inputs()
    heads = lambda t: t.view(t.shape[0], t.shape[1], tg.SPIKE_H, 64).transpose(1, 2)
    s = heads(q.float()) @ heads(torch.cat([k, k2], 1).float()).transpose(-1, -2) * 0.125
    n = s.shape[-1] // 32 * 32
    block_max = s[..., :n].reshape(*s.shape[:-1], -1, 32).max(-1).values
    assert (block_max[..., 1:] - block_max[..., :-1]).min() > 0.5 and (s[..., n:].max(-1).values - block_max[..., -1]).min() > 0.5
    assert s.max() - s.min() < 60                                   # ... and no key underflows: every block still counts
    for name in ("tiny", "full"):
        d, sd, hidden, want, stored = rr.case(name)
        floor = ((stored - want).norm() / want.norm()).item()
        print(f"[resampler {name}] bf16-storage floor {floor:.3e}")
        assert floor >= FLOOR_DEGENERATE and torch.isfinite(want).all()
        assert set(sd) == set(rr.state_shapes(d)) and all(tuple(sd[k].shape) == s for k, s in rr.state_shapes(d).items())


def test_restatement_matches_a_direct_evaluation():
    """resampler_ref against the module structure written out once more with nn.Linear / nn.LayerNorm / nn.GELU and the
    reference's reshape_tensor, in float64: the restatement's own plumbing (key names, chunk order, head split)"""
    d, sd, hidden, _, _ = rr.case("tiny")
    w = {k: v.double() for k, v in sd.items()}
    x = hidden.to(torch.bfloat16).double()
    B, H = x.shape[0], d["heads"]
    ln = lambda t, p: torch.nn.functional.layer_norm(t, (t.shape[-1],), w[p + ".weight"], w[p + ".bias"])
    lat = w["latents"].repeat(B, 1, 1)
    x = x @ w["proj_in.weight"].T + w["proj_in.bias"]
    for l in range(d["depth"]):
        xn, lt = ln(x, f"layers.{l}.0.norm1"), ln(lat, f"layers.{l}.0.norm2")
        q = lt @ w[f"layers.{l}.0.to_q.weight"].T
        kv = torch.cat([xn, lt], 1) @ w[f"layers.{l}.0.to_kv.weight"].T
        k, v = kv[..., :H * 64], kv[..., H * 64:]
        o = torch.empty(B, lat.shape[1], H * 64, dtype=torch.float64)
        for h in range(H):
            c = slice(h * 64, h * 64 + 64)
            o[..., c] = torch.softmax(q[..., c] @ k[..., c].transpose(1, 2) / 8.0, -1) @ v[..., c]
        lat = o @ w[f"layers.{l}.0.to_out.weight"].T + lat
        n = ln(lat, f"layers.{l}.1.0")
        lat = torch.nn.functional.gelu(n @ w[f"layers.{l}.1.1.weight"].T) @ w[f"layers.{l}.1.3.weight"].T + lat
    want = ln(lat @ w["proj_out.weight"].T + w["proj_out.bias"], "norm_out")
    got = rr.resampler_ref(sd, hidden, torch.float64)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
