"""-m gpu: SDXL inpainting (tests/test_sdxl_zh_inpaint.py `StableDiffusionTest.__call__`) on the HIP path against the CPU
restatement in tests/inpaint_ref.py: the input-preparation kernel, the gathering conv_in, the 9-channel UNet with and
without its inpainting condition, the whole tiny chain, one full-size SDXL-inpainting UNet evaluation, and the errors."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
from test_model_gpu import cond_inputs, gpu, rel_l2, round_weights_bf16_  # noqa: E402,F401


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def test_inpaint_prepare_bitwise_vs_torch(gpu):
    from inpaint_ref import prepare_ref
    from pea_diffusion_amd.inpaint import prepare_mask_and_masked_image
    g = torch.Generator().manual_seed(0)
    for N, H, W in [(1, 64, 64), (3, 1024, 1024), (2, 136, 72)]:
        img = torch.rand(N, 3, H, W, generator=g)
        img[0, :, 0, :8] = torch.tensor([0.0, 1.0, 0.5, 0.25, 1e-8, 0.49999997, 0.50000006, 0.75])
        m = torch.rand(N, 1, H, W, generator=g)
        m[0, 0, 0, :8] = torch.tensor([0.5, 0.49999997, 0.50000006, 0.0, 1.0, 0.5, 0.4, 0.6])
        m[:, :, 8::16, ::8] = 0.5                       # exact 0.5 on sampled latent positions
        m[:, :, ::16, 8::8] = 0.49999997
        want = prepare_ref(img.cuda(), m.cuda())
        got = prepare_mask_and_masked_image(img, m)
        for a, b, name in zip(got, want, ("init_image", "masked_image", "latent_mask")):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (N, H, W, name)
        assert bool((got[1] == 0).any()) and bool(got[2].eq(1).any()) and bool(got[2].eq(0).any())


def _gather_case(B, lb, cb, H, W, Cout=320, seed=0):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(lb, 4, H, W, generator=g)
    mask = (torch.rand(cb, 1, H, W, generator=g) > 0.5).float()
    ml = torch.randn(cb, 4, H, W, generator=g)
    w = torch.randn(Cout, 9, 3, 3, generator=g) * 0.2
    bias = torch.randn(Cout, generator=g) * 0.1
    x9 = torch.cat([lat.repeat(B // lb, 1, 1, 1), mask.repeat(B // cb, 1, 1, 1), ml.repeat(B // cb, 1, 1, 1)], dim=1)
    return lat, mask, ml, w, bias, x9


@pytest.mark.parametrize("B,lb,cb,H,W", [(8, 4, 4, 128, 128), (4, 4, 4, 16, 24), (2, 1, 1, 32, 32), (4, 2, 4, 16, 16)])
def test_conv_in_gather_vs_plain_and_fp64(gpu, B, lb, cb, H, W):
    from pea_diffusion_amd import ops
    lat, mask, ml, w, bias, x9 = _gather_case(B, lb, cb, H, W)
    c = lambda t: t.cuda().contiguous()
    got = ops.conv_in_gather(c(lat), c(mask), c(ml), c(w), c(bias), B)
    plain = ops.conv_in(c(x9), c(w), c(bias))
    assert got.shape == (B, H, W, 320) and torch.equal(got.view(torch.int16), plain.view(torch.int16))
    assert bool((_ulp_err(got.cpu(), x9, w, bias) <= 1.0).all())


def _ulp_err(got, x9, w, bias):
    """|got - exact| in bf16 ulps of the larger of the two magnitudes, after taking off the worst-case rounding of an fp32
    sum of the 81 products (81 * 2^-24 * sum |x w|, which dominates only where the exact value is close to zero)"""
    ref = F.conv2d(x9.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(x9.double().abs(), w.double().abs(), bias.double().abs(), padding=1).permute(0, 2, 3, 1)
    got = got.double()
    ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(ref.abs(), got.abs()).clamp_min(1e-30))) - 7)
    return ((got - ref).abs() - 81 * 2.0 ** -24 * mag).clamp_min(0) / ulp


def test_conv_in_gather_refuses_unsupported_shapes(gpu):
    from pea_diffusion_amd import ops
    from pea_diffusion_amd._lib import PeaError
    lat, mask, ml, w, bias, _ = _gather_case(4, 2, 2, 16, 18)
    c = lambda t: t.cuda().contiguous()
    with pytest.raises(PeaError, match="multiple of 4"):
        ops.conv_in_gather(c(lat), c(mask), c(ml), c(w), c(bias), 4)
    lat, mask, ml, w, bias, _ = _gather_case(4, 2, 2, 16, 16)
    buf = torch.zeros(lat.numel() + 1, device="cuda")
    buf[1:] = lat.cuda().reshape(-1)
    with pytest.raises(PeaError, match="aligned"):
        ops.conv_in_gather(buf[1:].view(lat.shape), c(mask), c(ml), c(w), c(bias), 4)
    with pytest.raises(PeaError, match="multiple of latent_batch"):
        ops.conv_in_gather(c(lat), c(mask), c(ml), c(w), c(bias), 3)


def _tiny9_pair(B, L, seed=0, inpaint_inputs=True):
    from oracle import unet_ref as ou
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.unet import HipUNet
    ocfg = dataclasses.replace(ou.tiny_config(), in_channels=9)
    torch.manual_seed(seed)
    ref = ou.UNet2DConditionRef(ocfg)
    round_weights_bf16_(ref)
    for p in ref.parameters():
        p.requires_grad_(False)
    hip = HipUNet(dataclasses.replace(pc.tiny_config(), in_channels=9), B, 16, 16, L, inpaint_inputs=inpaint_inputs)
    missing, unexpected = hip.load_state_dict(ref.state_dict())
    assert not missing and not unexpected
    return ocfg, ref, hip


def test_tiny_9_channel_unet_plain_gathered_cleared(gpu):
    B, L = 4, 77
    cfg, ref, hip = _tiny9_pair(B, L)
    lat4, t, ehs, added = cond_inputs(cfg, B, L, 16)
    g = torch.Generator().manual_seed(5)
    lat = lat4[:B // 2]
    mask = (torch.rand(B // 2, 1, 16, 16, generator=g) > 0.5).float()
    ml = torch.randn(B // 2, 4, 16, 16, generator=g)
    x9 = torch.cat([torch.cat([lat] * 2), torch.cat([mask] * 2), torch.cat([ml] * 2)], dim=1)
    ehs = ehs.to(torch.bfloat16).float()
    cadd = {k: v.cuda() for k, v in added.items()}
    with torch.no_grad():
        want = ref(x9, t, ehs, added_cond_kwargs=added)[0]
    plain = hip(x9.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    e = rel_l2(plain, want)
    print(f"[tiny 9-channel unet B{B}] eps rel_l2={e:.3e}")
    assert e < 2e-2
    hip.set_inpaint_cond(mask.cuda(), ml.cuda())
    gathered = hip(lat.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    assert torch.equal(gathered, plain)
    # latent_batch = cond_batch = B (no CFG doubling) through the same context
    hip.set_inpaint_cond(torch.cat([mask] * 2).cuda(), torch.cat([ml] * 2).cuda())
    full = hip(torch.cat([lat] * 2).cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    assert torch.equal(full, plain)
    # the reference's own concatenated input still works while a condition is set, and after clearing it
    assert torch.equal(hip(x9.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0], plain)
    hip.clear_inpaint_cond()
    assert torch.equal(hip(x9.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0], plain)
    from pea_diffusion_amd._lib import PeaError
    with pytest.raises(PeaError):
        hip(lat.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)       # latents alone need a condition


def _vae_cfgs():
    """a 4-level tiny VAE: the 8x latent scale of the SDXL VAE (the inpainting mask is resized by 8)"""
    import oracle.vae_ref as ov
    from pea_diffusion_amd import config as pc
    return (dataclasses.replace(ov.tiny_vae_config(), block_out_channels=(64, 64, 128, 128)),
            dataclasses.replace(pc.tiny_vae_config(), block_out_channels=(64, 64, 128, 128)))


@pytest.mark.parametrize("strength", [0.9999, 0.6])
def test_inpaint_end_to_end_tiny_vs_oracle(gpu, strength):
    from inpaint_ref import inpaint_denoise_ref
    from oracle.sampler_ref import DPMSolverMultistepRef
    from oracle.step_ref import AdapterRef
    from oracle.text_ref import BertTextRef
    from oracle.vae_ref import VAEDecoderRef, VAEEncoderRef
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.adapter import PEAAdapter
    from pea_diffusion_amd.inpaint import inpaint_denoise
    from pea_diffusion_amd.sampler import DPMSolverMultistep
    from pea_diffusion_amd.text import HipTextEncoder
    from pea_diffusion_amd.vae import HipVAEDecoder, HipVAEEncoder
    N, L, hw = 2, 52, 16
    torch.manual_seed(0)
    tcfg = pc.tiny_bert_config()
    t_ref = BertTextRef(tcfg)
    with torch.no_grad():
        for p in t_ref.parameters():
            if p.dim() >= 2:
                p.mul_(3.0)
    round_weights_bf16_(t_ref)
    t_hip = HipTextEncoder(tcfg, 2 * N, L)
    t_hip.load_state_dict(t_ref.state_dict())
    cfg, u_ref, u_hip = _tiny9_pair(2 * N, L, seed=1)
    a_ref = AdapterRef(128, cfg.pooled_dim, 192, cfg.cross_attention_dim, False)
    a_hip = PEAAdapter(128, cfg.pooled_dim, 192, cfg.cross_attention_dim, False)
    a_hip.load_state_dict(a_ref.state_dict())
    a_hip = a_hip.cuda()
    round_weights_bf16_(a_ref)
    ovc, pvc = _vae_cfgs()
    e_ref, d_ref = VAEEncoderRef(ovc), VAEDecoderRef(ovc)
    round_weights_bf16_(e_ref)
    round_weights_bf16_(d_ref)
    e_hip = HipVAEEncoder(pvc, N, 8 * hw, 8 * hw)
    e_hip.load_state_dict(e_ref.state_dict())
    d_hip = HipVAEDecoder(pvc, N, hw, hw)
    d_hip.load_state_dict(d_ref.state_dict())
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 1000, (2 * N, L), generator=g)
    ids[:, 30:] = 0
    img = torch.rand(N, 3, 8 * hw, 8 * hw, generator=g)
    mask = torch.zeros(N, 1, 8 * hw, 8 * hw)
    mask[0, :, 32:96, 16:80] = 1.0
    mask[1, :, :, 64:] = 0.75
    noise = torch.randn(N, 4, hw, hw, generator=g)
    vn = (torch.randn(N, 4, hw, hw, generator=g), torch.randn(N, 4, hw, hw, generator=g))
    time_ids = torch.tensor([[128, 128, 0, 0, 128, 128]] * (2 * N))
    kw = dict(num_inference_steps=6, strength=strength, guidance_scale=5.0, guidance_rescale=0.7)
    with torch.no_grad():
        tok = t_ref(ids)["last_hidden_state"].to(torch.bfloat16).float()
        pooled, tokens = a_ref(tok)
        want_lat = inpaint_denoise_ref(lambda *a, **k: u_ref(*a, **k), DPMSolverMultistepRef(), e_ref, img, mask,
                                       tokens.to(torch.bfloat16).float(), {"text_embeds": pooled, "time_ids": time_ids},
                                       noise=noise, vae_noise=vn, **kw)
        want_img = d_ref.decode(want_lat / ovc.scaling_factor)[0]
    tok_h, _ = t_hip.encode_text(ids.cuda())
    pooled_h, tokens_h = a_hip(tok_h)
    add_h = {"text_embeds": pooled_h, "time_ids": time_ids.cuda()}
    run = lambda im, **o: inpaint_denoise(u_hip, DPMSolverMultistep(), e_hip, im, mask, tokens_h, add_h, noise=noise,
                                          vae_noise=o.get("vn", vn), **kw)
    got_lat = run(img)
    got_img = d_hip.decode(got_lat, inv_scaling=1.0 / pvc.scaling_factor)[0]
    e_lat, e_img = rel_l2(got_lat, want_lat), rel_l2(got_img, want_img)
    print(f"[inpaint end to end tiny, strength {strength}] latents rel_l2={e_lat:.3e} image rel_l2={e_img:.3e}")
    assert e_lat < 3e-2 and e_img < 4e-2 and torch.isfinite(got_img).all()
    assert torch.equal(run(img), got_lat)                     # bit-reproducible
    # the image outside the mask reaches the result (masked-image latents; and the start latents when strength < 1)
    img2 = img.clone()
    img2[:, :, :16, :16] = 1.0 - img2[:, :, :16, :16]
    assert float(mask[:, :, :16, :16].max()) == 0.0
    assert not torch.equal(run(img2), got_lat)
    # zeroing the masked latents changes the latents: wrap the encoder so its masked-image encode returns zeros
    class ZeroMasked:
        def __init__(self, enc):
            self.enc, self.calls = enc, 0

        def encode_latents(self, x, **k):
            self.calls += 1
            out = self.enc.encode_latents(x, **k)
            return torch.zeros_like(out) if self.calls == (1 if strength == 1.0 else 2) else out
    z = inpaint_denoise(u_hip, DPMSolverMultistep(), ZeroMasked(e_hip), img, mask, tokens_h, add_h, noise=noise, vae_noise=vn,
                        **kw)
    assert torch.isfinite(z).all() and not torch.equal(z, got_lat)


def test_sdxl_inpaint_full_size_step_vs_oracle_and_loop(gpu):
    """SDXL inpainting UNet (2.57 B + the 9-channel conv_in) at 1024x1024: one UNet evaluation of the loop body (latents
    alone, mask and masked latents from the context) against oracle/unet_ref.py in fp32 on the host cores on the
    concatenated input; then a 3-step loop at batch 2 (one image with CFG), finite and bit-reproducible."""
    import time
    from oracle import unet_ref as ou
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.sampler import DPMSolverMultistep
    from pea_diffusion_amd.unet import HipUNet
    from test_model_gpu import _fast_fill_
    torch.set_num_threads(min(64, len(__import__("os").sched_getaffinity(0))))
    cfg = dataclasses.replace(ou.sdxl_config(), in_channels=9)
    B, L, hw = 1, 77, 128
    orig = torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_
    torch.nn.init.kaiming_uniform_ = lambda t, *a, **k: t
    torch.nn.init.uniform_ = lambda t, *a, **k: t
    try:
        uref = ou.UNet2DConditionRef(cfg)
    finally:
        torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_ = orig
    _fast_fill_(uref, seed=7)
    round_weights_bf16_(uref)
    for p in uref.parameters():
        p.requires_grad_(False)
    unet = HipUNet(pc.sdxl_inpaint_config(), B, hw, hw, L, inpaint_inputs=True)
    missing, unexpected = unet.load_state_dict(uref.state_dict())
    assert not missing and not unexpected
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(B, 4, hw, hw, generator=g)
    mask = torch.zeros(B, 1, hw, hw)
    mask[:, :, 32:96, 40:100] = 1.0
    ml = torch.randn(B, 4, hw, hw, generator=g) * (1 - mask)
    t = torch.tensor([601])
    ehs = torch.randn(B, L, 2048, generator=g).to(torch.bfloat16).float()
    added = {"text_embeds": torch.randn(B, 1280, generator=g).to(torch.bfloat16).float(),
             "time_ids": torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * B)}
    x9 = torch.cat([lat, mask, ml], dim=1)
    t0 = time.time()
    with torch.no_grad():
        eps_ref = uref(x9, t, ehs, added_cond_kwargs=added)[0]
    t_or = time.time() - t0
    cadd = {k: v.cuda() for k, v in added.items()}
    unet.set_inpaint_cond(mask.cuda(), ml.cuda())
    eps = unet(lat.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    e = rel_l2(eps, eps_ref)
    eps_plain = unet(x9.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0]
    print(f"[sdxl inpaint 1024x1024 B=1 vs oracle] eps rel_l2={e:.3e}; oracle {t_or:.0f} s")
    assert e < 1.5e-2 and torch.equal(eps, eps_plain)
    del unet
    torch.cuda.empty_cache()
    # 3-step loop, one image with CFG (UNet batch 2), random-init weights
    u2 = HipUNet(pc.sdxl_inpaint_config(), 2, hw, hw, L, inpaint_inputs=True)
    u2.init_random(1)
    ehs2 = torch.randn(2, L, 2048, generator=g).cuda().to(torch.bfloat16)
    add2 = {"text_embeds": torch.randn(2, 1280, generator=g).cuda().to(torch.bfloat16),
            "time_ids": torch.tensor([[1024, 1024, 0, 0, 1024, 1024]] * 2).cuda()}

    def loop(masked):
        s = DPMSolverMultistep()
        s.set_timesteps(3)
        s.set_begin_index(0)
        u2.set_inpaint_cond(mask.cuda(), masked.cuda())
        x = lat.cuda().clone()
        from pea_diffusion_amd import ops
        for tt in s.timesteps:
            n = u2(x, tt, encoder_hidden_states=ehs2, added_cond_kwargs=add2)[0]
            x = s.step(ops.cfg_combine(n.float(), 5.0), tt, x)[0]
        return x
    a, b = loop(ml), loop(ml)
    assert a.shape == (1, 4, hw, hw) and torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, loop(torch.zeros_like(ml)))


def test_inpaint_errors(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.inpaint import inpaint_denoise
    from pea_diffusion_amd.sampler import DPMSolverMultistep
    from pea_diffusion_amd.unet import HipUNet
    tiny9 = dataclasses.replace(pc.tiny_config(), in_channels=9)
    u = HipUNet(tiny9, 4, 16, 16, 7, inpaint_inputs=True)
    u.init_random(0)
    m, ml = torch.zeros(3, 1, 16, 16).cuda(), torch.zeros(3, 4, 16, 16).cuda()
    with pytest.raises(PeaError, match="must each divide"):
        u.set_inpaint_cond(m, ml)                               # cond_batch 3 does not divide 4
    with pytest.raises(PeaError, match="must each divide"):
        u.set_inpaint_cond(m[:2], ml[:2], latent_batch=3)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        HipUNet(tiny9, 2, 16, 16, 7, needs_grad=True, inpaint_inputs=True)
    with pytest.raises(PeaError, match="in_channels"):
        HipUNet(pc.tiny_config(), 2, 16, 16, 7, inpaint_inputs=True)
    plain9 = HipUNet(tiny9, 2, 16, 16, 7)
    with pytest.raises(PeaError, match="inpaint_inputs"):
        plain9.set_inpaint_cond(m[:1], ml[:1])
    u4 = HipUNet(pc.tiny_config(), 4, 16, 16, 7)
    img, mk = torch.rand(2, 3, 128, 128), torch.zeros(2, 1, 128, 128)
    with pytest.raises(ValueError, match="img2img"):
        inpaint_denoise(u4, DPMSolverMultistep(), None, img, mk, None, None, num_inference_steps=4)
    with pytest.raises(ValueError, match="< 1"):
        inpaint_denoise(u, DPMSolverMultistep(), None, img, mk, None, None, num_inference_steps=4, strength=0.1)


def test_trainer_refuses_a_9_channel_unet(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.adapter import PEAAdapter
    from pea_diffusion_amd.train import PEATrainer
    from pea_diffusion_amd.unet import HipUNet
    tiny9 = dataclasses.replace(pc.tiny_config(), in_channels=9)
    cfg = pc.tiny_config()
    ad = PEAAdapter(128, cfg.pooled_dim, 192, cfg.cross_attention_dim, False).cuda()
    s9 = HipUNet(tiny9, 2, 16, 16, 12, needs_grad=True)
    t4 = HipUNet(cfg, 2, 16, 16, 77)
    t9 = HipUNet(tiny9, 2, 16, 16, 77)
    s4 = HipUNet(cfg, 2, 16, 16, 12, needs_grad=True)
    for st, te in ((s9, t4), (s4, t9), (s9, t9)):
        with pytest.raises(PeaError, match="in_channels must equal out_channels"):
            PEATrainer(ad, st, te)
