"""-m gpu: the CLIP vision tower on the HIP tape against the transformers goldens and tests/vision_ref.py, and the kernels
around it (antialiased resample + crop + normalise, patchify, CLIPScore) against their CPU restatements."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vision_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    return torch.device("cuda")


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).pow(2).sum().sqrt() / (b.pow(2).sum().sqrt() + 1e-30)).item()


def check_tower(enc, pixels, want, tag):
    """every hidden state, last_hidden_state, pooler_output, image_embeds at rel_l2 < 2e-2 (the bound of tests/test_text_gpu.py)"""
    n = len(want["hidden_states"])
    for k in range(n):
        hid, pooled, emb = enc.encode(pixels, hidden_index=k)
        e = rel_l2(hid, want["hidden_states"][k])
        print(f"[{tag}] hidden_states[{k}] rel_l2={e:.3e}")
        assert e < 2e-2 and torch.isfinite(hid).all(), k
    hid, pooled, emb = enc.encode(pixels)                       # -1: HF's last_hidden_state (before post_layernorm)
    errs = {"last_hidden_state": rel_l2(hid, want["last_hidden_state"]), "pooler_output": rel_l2(pooled, want["pooler_output"]),
            "image_embeds": rel_l2(emb, want["image_embeds"]), "hidden_states[-2]": rel_l2(enc.encode(pixels, -2)[0], want["hidden_states"][n - 2])}
    print(f"[{tag}] " + " ".join(f"{k} rel_l2={v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 2e-2, k


@pytest.mark.parametrize("name", ["vision_clip", "vision_clip_p32", "vision_clip_h80"])
def test_image_encoder_vs_transformers_golden(gpu, name):
    from pea_diffusion_amd.vision import HipImageEncoder
    cfg, sd, out = vr.load_golden(name)
    enc = HipImageEncoder(cfg, 2)
    assert set(enc.weight_table()) == set(sd)
    enc.load_state_dict(sd)
    px = out["pixels"].cuda()
    check_tower(enc, px, out, name)
    o = enc(pixel_values=px, output_hidden_states=True)          # the HF access pattern
    assert rel_l2(o.image_embeds, out["image_embeds"]) < 2e-2 and rel_l2(o.pooler_output, out["pooler_output"]) < 2e-2
    assert rel_l2(o.last_hidden_state, out["last_hidden_state"]) < 2e-2
    assert rel_l2(o.hidden_states[0], out["hidden_states"][0]) < 2e-2 and rel_l2(o.hidden_states[-2], out["hidden_states"][-2]) < 2e-2
    from pea_diffusion_amd._lib import PeaError
    with pytest.raises(PeaError):
        enc.load_state_dict(dict(sd, logit_scale=torch.zeros(())))          # strict by default
    enc.load_state_dict(dict(sd, logit_scale=torch.zeros(())), strict=False)


def test_image_encoder_257_tokens_vs_restatement(gpu):
    """image 224 / patch 14: the real token count, its ragged last attention tile and the full position table"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.vision import HipImageEncoder
    cfg = pc.VisionConfig(image_size=224, patch_size=14, hidden_size=128, num_attention_heads=2, num_hidden_layers=1,
                          intermediate_size=256, projection_dim=64, name="tiny_vit_224")
    assert cfg.num_tokens == 257
    sd = vr.random_state_dict(cfg, seed=3)
    px = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    want = vr.tower_ref(sd, cfg, px)
    enc = HipImageEncoder(cfg, 2)
    enc.load_state_dict(sd)
    check_tower(enc, px.cuda(), want, "257 tokens")


def _test_images(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    x = torch.rand(3, 3, H, W, generator=g) * 2.4 - 1.2                     # some values outside [-1, 1]: the clamp
    x[1] = torch.tensor([-0.6, 0.1, 0.7]).view(3, 1, 1)                     # channel-constant
    x[2] = -0.9
    x[2, :, 0, :] = x[2, :, -1, :] = x[2, :, :, 0] = x[2, :, :, -1] = 1.0   # one-pixel bright border
    return x


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("H,W,size", [(96, 160, 42), (64, 64, 56), (40, 40, 56), (56, 56, 56)])
def test_preprocess_vs_interpolate(gpu, H, W, size, quantize):
    """fp32-stored result: rtol 1e-3 / atol 1e-4 (README, per-kernel bound)"""
    from pea_diffusion_amd import vision
    x = _test_images(H, W)
    ref = vr.preprocess_ref(x, size, MEAN, STD, quantize=quantize)
    got = vision.preprocess(x.cuda(), size, MEAN, STD, quantize=quantize).cpu()
    assert got.shape == (3, 3, size, size)
    print(f"[preprocess {H}x{W}->{size} q{int(quantize)}] max |d| = {float((got - ref).abs().max()):.3e}")
    torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-4)
    m, s = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    const = ((x[1, :, 0, 0] + 1) / 2)
    const = (torch.round(const * 255) / 255 if quantize else const).view(3, 1, 1)
    torch.testing.assert_close(got[1], ((const - m[0]) / s[0]).expand(3, size, size), rtol=1e-3, atol=1e-4)   # weights sum to 1
    if H == W == size:                          # identity: the normalised input itself
        v = ((x + 1) / 2).clamp(0, 1)
        v = torch.round(v * 255) / 255 if quantize else v
        torch.testing.assert_close(got, (v - m) / s, rtol=1e-3, atol=1e-4)
    again = vision.preprocess(x.cuda(), size, MEAN, STD, quantize=quantize).cpu()
    assert torch.equal(got, again)


@pytest.mark.parametrize("S,P,kpad", [(56, 14, 640), (64, 32, 3072)])
def test_patchify_is_a_gather_and_one_rounding(gpu, S, P, kpad):
    from pea_diffusion_amd import vision
    B, G, K = 3, S // P, 3 * P * P
    px = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S))
    rows = vision.patchify(px.cuda(), P).cpu()
    assert rows.shape == (B * G * G, kpad) and rows.dtype == torch.bfloat16
    want = px.reshape(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, K).to(torch.bfloat16)
    assert torch.equal(rows[:, :K], want)
    assert (rows[:, K:] == 0).all()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [64, 67, 100, 1280])
def test_clip_score(gpu, B, D):
    from pea_diffusion_amd import ops
    g = torch.Generator().manual_seed(D * 10 + B)
    a = torch.randn(B, D, generator=g)
    t = a + 0.7 * torch.randn(B, D, generator=g)
    if B == 3:
        t[1] = -a[1] + 0.3 * torch.randn(D, generator=g)          # negative cosine
        a[2] = 0.0                                                # all-zero row: 0, not NaN
    ac, tc = a.cuda(), t.cuda()
    cos = torch.cosine_similarity(a, t, dim=-1)
    s = ops.clip_score(ac, tc)
    torch.testing.assert_close(s.cpu(), 2.5 * cos.clamp(min=0), rtol=1e-3, atol=1e-4)
    plain = ops.clip_score(ac, tc, w=1.0, clamp=False)
    torch.testing.assert_close(plain.cpu(), cos, rtol=1e-3, atol=1e-4)
    assert torch.equal(ops.clip_score(ac, tc), s) and torch.equal(ops.clip_score(ac, tc, w=1.0, clamp=False), plain)
    if B == 3:
        assert cos[1] < -0.5 and s[1].item() == 0.0 and plain[1].item() < -0.5
        assert s[2].item() == 0.0 and plain[2].item() == 0.0


def test_clip_score_images_end_to_end(gpu):
    """|d score| <= w * 2 * 2e-2: for unit vectors a cosine moves by at most the distance between the normalised embeddings,
    at most twice their relative L2 error, which the tower tests hold to 2e-2"""
    from pea_diffusion_amd import vision
    cfg, sd, _ = vr.load_golden("vision_clip")
    enc = vision.HipImageEncoder(cfg, 2)
    enc.load_state_dict(sd)
    g = torch.Generator().manual_seed(11)
    images = torch.rand(2, 3, 96, 160, generator=g) * 2 - 1
    w = 2.5
    px = vr.preprocess_ref(images, cfg.image_size, cfg.image_mean, cfg.image_std)
    emb = vr.tower_ref(sd, cfg, px)["image_embeds"]
    text = torch.stack([emb[0] + 0.5 * emb[0].norm() / 8 * torch.randn(64, generator=g), -emb[1] + 0.1 * torch.randn(64, generator=g)])
    want = vr.clip_score_ref(emb, text, w)
    img_d, text_d = images.cuda(), text.cuda()
    got = vision.clip_score_images(enc, img_d, text_d, w)          # first call: builds and uploads the tap tables
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                        # a synchronising torch call inside would raise
    try:
        again = vision.clip_score_images(enc, img_d, text_d, w)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert again.is_cuda and again.shape == (2,) and again.dtype == torch.float32
    print(f"[clip_score_images] hip {got.tolist()} ref {want.tolist()}")
    assert want[0] > 0.5 and want[1] == 0.0
    assert (got.cpu() - want).abs().max().item() <= w * 2 * 2e-2
    assert torch.equal(got, again)
