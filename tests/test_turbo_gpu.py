"""-m gpu: SDXL-Turbo sampling on the HIP path -- the fused Euler step kernel (pea_op_euler_update) against float64 torch,
the exactness properties of the Euler / Euler-ancestral schedulers on the device, the guidance-embedded UNet
(`time_cond_proj_dim`) on the tiny and the full SDXL config against the oracle subclass of tests/turbo_ref.py, and the few-step
loops (tiny, full size, inpainting with strength < 1, text tower -> adapter -> 1 step -> VAE decode) against the restated loop
around the fp32 oracle.  End-to-end limits follow check_against_storage_floor (tests/test_model_gpu.py): 1.5 x the distance of
the same oracle under bf16 storage from the fp32 oracle, measured in the run."""
import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
from test_model_gpu import STORAGE_FLOOR_FACTOR, _fast_fill_, cond_inputs, gpu, rel_l2, round_weights_bf16_  # noqa: E402,F401
from turbo_ref import CondUNetRef, EulerRef, euler_denoise_ref, euler_inpaint_ref  # noqa: E402

EPS_LIMIT = 2e-2                # eps of a whole UNet against the fp32 oracle, as tests/test_lcm_gpu.py / test_model_gpu.py
LOOP_FALLBACK = 3e-2            # the 6-step DPM loop's limit, used where the storage floor is degenerate
# A chain of bf16-stored tensors cannot be closer to fp32 than a fraction of one bf16 rounding (2^-9 relative per element,
# about 1e-3 in rel-L2 after a few of them): a measured floor below that says the storage mode did not act on the case.
FLOOR_DEGENERATE = 1e-3


# ---------------------------------------------------------------------------------------------- kernel
def _unaligned(t):
    """the same values behind a pointer offset by 4 bytes (the scalar path)"""
    pad = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = pad[1:]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("n", [1, 7, 8, 4 * 64 * 64 * 4, 4 * 64 * 64 * 4 + 3])
def test_euler_update_kernel(gpu, n):
    """every form of the op against float64 (rtol 1e-3 / atol 1e-4, the per-kernel rule for fp32 results); the 16-byte and the
    scalar path bit for bit on the same data; two runs bit-identical"""
    from pea_diffusion_amd import ops
    g = torch.Generator().manual_seed(n)
    x, e, z = (torch.randn(n, generator=g) for _ in range(3))
    x = x * 14.6
    k_e, k_n, k_s = -3.7, 2.1, 1.0 / math.sqrt(5.0 ** 2 + 1.0)
    xc, ec, zc = x.cuda(), e.cuda(), z.cuda()
    close = lambda got, want: torch.allclose(got.cpu().double(), want, rtol=1e-3, atol=1e-4)
    for noise in (zc, None):
        want = x.double() + k_e * e.double() + (k_n * z.double() if noise is not None else 0.0)
        for dup in (1, 2):
            for with_m in (True, False):
                s = xc.clone()
                m = torch.full((dup * n,), float("nan"), device="cuda") if with_m else None
                out = ops.euler_update_(s, ec, noise, m, k_e, k_n, k_s, dup)
                assert out.data_ptr() == s.data_ptr() and close(s, want), (noise is not None, dup, with_m)
                if with_m:
                    assert close(m, torch.cat([want * k_s] * dup))
                    assert torch.equal(m[:n], s * torch.tensor(k_s, device="cuda"))       # one rounding of the stored sample
                    assert dup == 1 or torch.equal(m[n:], m[:n])
                # the same data behind pointers offset by 4 bytes: the scalar path, bit for bit
                s2 = _unaligned(xc)
                m2 = _unaligned(torch.full((dup * n,), float("nan"), device="cuda")) if with_m else None
                ops.euler_update_(s2, _unaligned(ec), _unaligned(noise) if noise is not None else None, m2, k_e, k_n, k_s, dup)
                assert torch.equal(s2, s) and (not with_m or torch.equal(m2, m))
                # only the sample unaligned (mixed alignment falls back as a whole), and a second run
                s3 = _unaligned(xc)
                m3 = torch.empty(dup * n, device="cuda") if with_m else None
                ops.euler_update_(s3, ec, noise, m3, k_e, k_n, k_s, dup)
                assert torch.equal(s3, s) and (not with_m or torch.equal(m3, m))
                s4 = xc.clone()
                m4 = torch.empty(dup * n, device="cuda") if with_m else None
                ops.euler_update_(s4, ec, noise, m4, k_e, k_n, k_s, dup)
                assert torch.equal(s4, s) and (not with_m or torch.equal(m4, m))
    # the entry form (eps NULL): the sample is left alone, model_in = sample * k_s
    for dup in (1, 2):
        s = xc.clone()
        m = torch.empty(dup * n, device="cuda")
        ops.euler_update_(s, None, None, m, 0.0, 0.0, k_s, dup)
        assert torch.equal(s, xc) and close(m, torch.cat([x.double() * k_s] * dup))
        mu = _unaligned(torch.empty(dup * n, device="cuda"))
        ops.euler_update_(_unaligned(xc), None, None, mu, 0.0, 0.0, k_s, dup)
        assert torch.equal(mu, m)


def test_euler_update_refuses_bad_arguments(gpu):
    from pea_diffusion_amd import ops
    from pea_diffusion_amd._lib import PeaError
    s = torch.zeros(8, device="cuda")
    with pytest.raises(PeaError):
        ops.euler_update_(s, None, None, None, 0.0, 0.0, 1.0)                  # entry form without an output
    with pytest.raises(PeaError):
        ops.euler_update_(s, None, s.clone(), s.clone(), 0.0, 0.0, 1.0)        # entry form with noise
    with pytest.raises(PeaError):
        ops.euler_update_(s, s.clone(), None, torch.zeros(24, device="cuda"), 0.0, 0.0, 1.0, dup=3)


# ---------------------------------------------------------------------------------------------- exactness on the device
@pytest.mark.parametrize("ancestral,n", [(False, 1), (False, 4), (False, 30), (True, 1)])
def test_exact_eps_lands_on_x0(gpu, ancestral, n):
    """eps = (x - x0) / sigma for a fixed x0: the last step's sigma_to = 0 puts the sample on x0 whatever the earlier steps
    did (1e-5 relative); and on the way the fused model input equals the stand-alone scale_model_input bit for bit"""
    from pea_diffusion_amd.sampler import EulerAncestralDiscrete, EulerDiscrete
    cls = EulerAncestralDiscrete if ancestral else EulerDiscrete
    s = cls()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 4, 16, 16, generator=g)
    ts = s.set_timesteps(n)
    x = (torch.randn(x0.shape, generator=g) * s.init_noise_sigma).cuda()
    for i, t in enumerate(ts):
        sigma = s.sigmas[i]
        m = s.scale_model_input(x, t)              # i > 0: the buffer the previous step's kernel filled
        alone = cls()
        alone.set_timesteps(n)
        alone.set_begin_index(i)
        assert torch.equal(alone.scale_model_input(x.clone(), t), m)
        assert torch.allclose(m.cpu().double(), x.cpu().double() / math.sqrt(sigma ** 2 + 1), rtol=1e-6, atol=1e-6)
        eps = ((x.cpu().double() - x0.double()) / sigma).float().cuda()
        x = s.step(eps, t, x, generator=torch.Generator().manual_seed(i))[0]
    e = rel_l2(x, x0)
    print(f"[euler exactness ancestral={ancestral} n={n}] rel_l2 to x0 = {e:.2e}")
    assert e <= 1e-5


# ---------------------------------------------------------------------------------------------- guidance-embedded UNet, tiny
def _tiny_cond_pair(B, L, needs_grad=False, seed=0):
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.unet import HipUNet
    ocfg = tiny_config()
    torch.manual_seed(seed)
    ref = CondUNetRef(ocfg, 128)
    with torch.no_grad():
        # measured on the CPU, oracle alone: with torch's default init w = 8 against w = 1 moves eps by 0.086; at 4 x by 0.31
        ref.time_embedding.cond_proj.weight.mul_(4.0)
    round_weights_bf16_(ref)
    for p in ref.parameters():
        p.requires_grad_(False)
    pcfg = dataclasses.replace(pc.tiny_config(), time_cond_proj_dim=128)
    hip = HipUNet(pcfg, B, 16, 16, L, needs_grad=needs_grad)
    missing, unexpected = hip.load_state_dict(ref.state_dict())
    assert not missing and not unexpected
    return ocfg, pcfg, ref, hip


def _cond(ws, dim):
    """the guidance embedding as both sides receive it: bf16-representable, like the encoder states"""
    from pea_diffusion_amd.sampler import guidance_scale_embedding
    return guidance_scale_embedding(ws, dim).to(torch.bfloat16).float()


def test_tiny_guidance_embedded_unet(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    B, L = 2, 77
    cfg, pcfg, ref, hip = _tiny_cond_pair(B, L)
    assert hip.weight_table()["time_embedding.cond_proj.weight"] == (64, 128)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    ehs = ehs.to(torch.bfloat16).float()
    cadd = {k: v.cuda() for k, v in added.items()}
    c8, c1 = _cond([7.0, 7.0], 128), _cond([0.0, 0.0], 128)             # w = guidance_scale - 1 for guidance 8 and 1
    with torch.no_grad():
        r8 = ref(x, t, ehs, added_cond_kwargs=added, timestep_cond=c8)[0]
        r1 = ref(x, t, ehs, added_cond_kwargs=added, timestep_cond=c1)[0]
        r0 = ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda u, c: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd, timestep_cond=None if c is None else c.cuda())[0].clone()
    h8, h1, h0 = run(hip, c8), run(hip, c1), run(hip, None)
    e8, e1, e0 = rel_l2(h8, r8), rel_l2(h1, r1), rel_l2(h0, r0)
    shift_ref, shift_hip = rel_l2(r8, r1), rel_l2(h8, h1.cpu())
    print(f"[tiny guidance-embedded unet] eps rel_l2 w=8 {e8:.3e}, w=1 {e1:.3e}, no cond {e0:.3e}; "
          f"w=8 against w=1 moves eps by {shift_ref:.4f} (oracle) / {shift_hip:.4f} (hip)")
    assert max(e8, e1, e0) < EPS_LIMIT
    assert shift_ref > 10 * EPS_LIMIT, shift_ref               # the oracle alone: an ignored conditioning cannot pass
    assert abs(shift_hip - shift_ref) <= EPS_LIMIT             # both are rel-L2 figures in units of |eps|, as the limit is
    assert torch.equal(run(hip, c8), h8)                       # bit-reproducible
    # cond unset / cleared / weight zero: the plain tiny UNet with the same weights, bit for bit
    plain = HipUNet(pc.tiny_config(), B, 16, 16, L)
    sd = {k: v for k, v in ref.state_dict().items() if k != "time_embedding.cond_proj.weight"}
    plain.load_state_dict(sd)
    p0 = run(plain, None)
    assert torch.equal(h0, p0) and torch.equal(run(hip, None), p0)
    assert not torch.equal(h8, p0)
    with pytest.raises(PeaError):
        run(plain, c8)                                         # a plain UNet has no such input
    with pytest.raises(PeaError):
        hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd, timestep_cond=torch.zeros(B, 64))
    # a context sharing the weights follows, with and without the conditioning
    twin = HipUNet(pcfg, B, 16, 16, L, share_weights_from=hip)
    assert torch.equal(run(twin, c8), h8) and torch.equal(run(twin, None), p0)
    hip.release_activations()
    assert torch.equal(run(hip, None), p0) and torch.equal(run(hip, c8), h8)
    zero = dict(ref.state_dict())
    zero["time_embedding.cond_proj.weight"] = torch.zeros(64, 128)
    hip.load_state_dict(zero)
    assert torch.equal(run(hip, c8), p0) and torch.equal(run(twin, c8), p0)


def test_tiny_guidance_embedded_unet_training_context(gpu):
    """a PEA_UNET_GRAD context takes the conditioning too (the input itself needs no gradient) and still differentiates"""
    B, L = 2, 12
    cfg, pcfg, ref, hip = _tiny_cond_pair(B, L, needs_grad=True)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    ehs = ehs.to(torch.bfloat16).float()
    c8 = _cond([7.0, 3.0], 128)
    ehs_r = ehs.clone().requires_grad_(True)
    want = ref(x, t, ehs_r, added_cond_kwargs=added, timestep_cond=c8)[0]
    d = torch.randn(want.shape, generator=torch.Generator().manual_seed(4))
    want.backward(d)
    got = hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()}, timestep_cond=c8.cuda())[0]
    d_ehs, _ = hip.backward(d.cuda())
    e, eg = rel_l2(got, want), rel_l2(d_ehs, ehs_r.grad)
    print(f"[tiny guidance-embedded unet, training context] eps rel_l2={e:.3e} d_ehs rel_l2={eg:.3e}")
    assert e < EPS_LIMIT and eg < 4e-2                         # the forward / gradient limits of tests/test_model_gpu.py


# ---------------------------------------------------------------------------------------------- loops on the tiny UNet
def _floor_limit(tag, floor):
    degenerate = floor < FLOOR_DEGENERATE
    limit = LOOP_FALLBACK if degenerate else STORAGE_FLOOR_FACTOR * floor
    return limit, ("fixed 3e-2 (degenerate floor)" if degenerate else f"{STORAGE_FLOOR_FACTOR} x floor")


@pytest.mark.parametrize("ancestral,n,g", [(True, 1, 0.0), (True, 4, 0.0), (False, 6, 5.0)])
def test_turbo_loop_tiny_vs_oracle(gpu, ancestral, n, g):
    from oracle.bf16_store import bf16_storage
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd.sampler import EulerAncestralDiscrete, EulerDiscrete, denoise
    from test_model_gpu import make_pair
    B, L = 2, 77
    UB = 2 * B if g > 1.0 else B
    cfg, ref, hip = make_pair(tiny_config, UB, L, needs_grad=False)
    x, _, ehs, added = cond_inputs(cfg, UB, L, cfg.sample_size)
    x = x[:B]
    ehs = ehs.to(torch.bfloat16).float()
    loop = lambda: euler_denoise_ref(lambda *a, **k: ref(*a, **k), EulerRef(ancestral), x.clone(), ehs, added, n,
                                     guidance_scale=g, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        want = loop()
        with bf16_storage():
            stored = loop()
    floor = rel_l2(stored, want)
    limit, rule = _floor_limit("tiny", floor)
    sched = (EulerAncestralDiscrete if ancestral else EulerDiscrete)
    run = lambda: denoise(hip, sched(), x.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()}, num_inference_steps=n,
                          guidance_scale=g, generator=torch.Generator().manual_seed(4))
    got = run()
    e = rel_l2(got, want)
    print(f"[turbo loop tiny, {'ancestral' if ancestral else 'euler'} {n} steps, guidance {g}] latents rel_l2={e:.3e}, "
          f"bf16-storage floor {floor:.3e}, ratio {e / max(floor, 1e-30):.2f}, limit {limit:.3e} ({rule})")
    assert torch.isfinite(got).all() and e <= limit
    assert torch.equal(run(), got)                              # bit-reproducible


def test_inpaint_with_euler_and_strength(gpu):
    """`inpaint_denoise` with EulerDiscrete at strength 0.5: starts from image_latents + sigma noise at t_start and runs
    `timesteps[t_start:]`; latents against the restated program (3e-2, the limit of the DPM inpainting loop test)"""
    from oracle.vae_ref import VAEEncoderRef
    from pea_diffusion_amd.inpaint import inpaint_denoise
    from pea_diffusion_amd.sampler import EulerDiscrete
    from pea_diffusion_amd.vae import HipVAEEncoder
    from test_inpaint_gpu import _tiny9_pair, _vae_cfgs
    N, L, hw, n, strength, g = 2, 77, 16, 6, 0.5, 5.0
    cfg, u_ref, u_hip = _tiny9_pair(2 * N, L, seed=1)
    ovc, pvc = _vae_cfgs()
    torch.manual_seed(2)
    e_ref = VAEEncoderRef(ovc)
    round_weights_bf16_(e_ref)
    e_hip = HipVAEEncoder(pvc, N, 8 * hw, 8 * hw)
    e_hip.load_state_dict(e_ref.state_dict())
    _, _, ehs, added = cond_inputs(cfg, 2 * N, L, hw)
    ehs = ehs.to(torch.bfloat16).float()
    gen = torch.Generator().manual_seed(1)
    img = torch.rand(N, 3, 8 * hw, 8 * hw, generator=gen)
    mask = torch.zeros(N, 1, 8 * hw, 8 * hw)
    mask[0, :, 32:96, 16:80] = 1.0
    mask[1, :, :, 64:] = 0.75
    noise = torch.randn(N, 4, hw, hw, generator=gen)
    vn = (torch.randn(N, 4, hw, hw, generator=gen), torch.randn(N, 4, hw, hw, generator=gen))
    with torch.no_grad():
        want, ts_ref = euler_inpaint_ref(lambda *a, **k: u_ref(*a, **k), EulerRef(False), e_ref, img, mask, ehs, added, n,
                                         strength, g, noise, vn)
    seen = []
    got = inpaint_denoise(u_hip, EulerDiscrete(), e_hip, img, mask, ehs.cuda(), {k: v.cuda() for k, v in added.items()},
                          num_inference_steps=n, strength=strength, guidance_scale=g, noise=noise, vae_noise=vn,
                          callback=lambda i, t, lat: seen.append(int(t)))
    full = EulerDiscrete().set_timesteps(n).tolist()
    assert seen == full[3:] == ts_ref.tolist() and len(seen) == 3
    e = rel_l2(got, want)
    print(f"[inpaint, EulerDiscrete {n} steps, strength {strength}, guidance {g}] latents rel_l2={e:.3e}")
    assert torch.isfinite(got).all() and e < LOOP_FALLBACK


# ---------------------------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def full_oracle():
    """the 2.57 B-parameter SDXL oracle with a 256-wide cond_proj, filled once (tests/test_model_gpu.py:_fast_fill_), and its
    inputs at batch 1, 64 x 64 latents"""
    import os
    from oracle import unet_ref as ou
    torch.set_num_threads(min(64, len(os.sched_getaffinity(0))))
    cfg = ou.sdxl_config()
    orig = torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_
    torch.nn.init.kaiming_uniform_ = lambda t, *a, **k: t
    torch.nn.init.uniform_ = lambda t, *a, **k: t
    try:
        ref = CondUNetRef(cfg, 256)
    finally:
        torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_ = orig
    _fast_fill_(ref, seed=5)
    with torch.no_grad():
        # measured, oracle alone: with the fill's scale the conditioning moves eps by 0.058, ten times the bf16-storage floor
        # and no more; four times the weight puts an ignored conditioning well clear of the limit
        ref.time_embedding.cond_proj.weight.mul_(4.0)
    round_weights_bf16_(ref)
    for p in ref.parameters():
        p.requires_grad_(False)
    x, t, ehs, added = cond_inputs(cfg, 1, 77, 64)
    return cfg, ref, x, t, ehs.to(torch.bfloat16).float(), added


def test_lcm_sdxl_full_size_forward_vs_oracle(gpu, full_oracle):
    from oracle.bf16_store import bf16_storage
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.unet import HipUNet
    cfg, ref, x, t, ehs, added = full_oracle
    t = torch.tensor([499])
    c = _cond([7.0], 256)
    with torch.no_grad():
        want = ref(x, t, ehs, added_cond_kwargs=added, timestep_cond=c)[0]
        plain = ref(x, t, ehs, added_cond_kwargs=added)[0]
        with bf16_storage():
            stored = ref(x, t, ehs, added_cond_kwargs=added, timestep_cond=c)[0]
    hip = HipUNet(pc.lcm_sdxl_config(), 1, 64, 64, 77)
    missing, unexpected = hip.load_state_dict(ref.state_dict())
    assert not missing and not unexpected
    got = hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()}, timestep_cond=c.cuda())[0]
    e, floor, shift = rel_l2(got, want), rel_l2(stored, want), rel_l2(want, plain)
    print(f"[lcm-sdxl full size 512x512, cond set] eps rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio {e / floor:.2f} "
          f"(limit {STORAGE_FLOOR_FACTOR} x floor); the conditioning moves the oracle's eps by {shift:.3f}")
    assert shift > 10 * floor, (shift, floor)                  # the oracle alone: an ignored conditioning cannot pass
    assert e <= STORAGE_FLOOR_FACTOR * floor + 1e-3            # the rule of check_against_storage_floor


def test_turbo_one_step_full_size_vs_oracle(gpu, full_oracle):
    from oracle.bf16_store import bf16_storage
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.sampler import EulerAncestralDiscrete, denoise
    from pea_diffusion_amd.unet import HipUNet
    cfg, ref, x, _, ehs, added = full_oracle
    loop = lambda: euler_denoise_ref(lambda *a, **k: ref(*a, **k), EulerRef(True), x.clone(), ehs, added, 1)
    with torch.no_grad():
        want = loop()
        with bf16_storage():
            stored = loop()
    hip = HipUNet(pc.sdxl_config(), 1, 64, 64, 77)
    sd = {k: v for k, v in ref.state_dict().items() if k != "time_embedding.cond_proj.weight"}
    missing, unexpected = hip.load_state_dict(sd)
    assert not missing and not unexpected
    got = denoise(hip, EulerAncestralDiscrete(), x.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()},
                  num_inference_steps=1, guidance_scale=0.0, generator=torch.Generator().manual_seed(0))
    e, floor = rel_l2(got, want), rel_l2(stored, want)
    limit, rule = _floor_limit("full", floor)
    print(f"[turbo 1 step, full SDXL 512x512] latents rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, "
          f"ratio {e / max(floor, 1e-30):.2f}, limit {limit:.3e} ({rule})")
    assert torch.isfinite(got).all() and e <= limit


# ---------------------------------------------------------------------------------------------- end to end
def test_turbo_end_to_end_image(gpu):
    """text tower -> adapter -> 1-step Turbo on the full SDXL UNet -> HipVAEDecoder at 512 x 512, random weights"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.adapter import PEAAdapter
    from pea_diffusion_amd.sampler import EulerAncestralDiscrete, denoise
    from pea_diffusion_amd.text import HipTextEncoder
    from pea_diffusion_amd.unet import HipUNet
    from pea_diffusion_amd.vae import HipVAEDecoder
    N, L, hw = 2, 52, 64
    tcfg = pc.tiny_bert_config()
    text = HipTextEncoder(tcfg, N, L)
    text.init_random(1)
    torch.manual_seed(0)
    adapter = PEAAdapter(tcfg.hidden_size, 1280, 256, 2048, False).cuda()
    unet = HipUNet(pc.sdxl_config(), N, hw, hw, L)
    unet.init_random(2)
    vcfg = pc.sdxl_vae_config()
    vae = HipVAEDecoder(vcfg, N, hw, hw)
    vae.init_random(3)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 1000, (N, L), generator=g)
    ids[:, 30:] = 0
    with torch.no_grad():
        tok, _ = text.encode_text(ids.cuda())
        pooled, tokens = adapter(tok)
    added = {"text_embeds": pooled, "time_ids": torch.tensor([[512, 512, 0, 0, 512, 512]] * N).cuda()}
    lat = denoise(unet, EulerAncestralDiscrete(), torch.randn(N, 4, hw, hw, generator=g).cuda(), tokens, added,
                  num_inference_steps=1, guidance_scale=0.0, generator=torch.Generator().manual_seed(2))
    img = vae.decode(lat, inv_scaling=1.0 / vcfg.scaling_factor)[0]
    assert tuple(img.shape) == (N, 3, 512, 512) and torch.isfinite(img).all() and torch.isfinite(lat).all()
    assert float(img.float().std()) > 0.0
