"""-m gpu: the LCM few-step sampler on the HIP path -- the step kernel (pea_op_lcm_update behind `LCMScheduler.step`) against
the float64 restatement tests/lcm_ref.py on the same noise, and the LCM-LoRA program end to end on the tiny UNet: fused LoRA,
4 steps, guidance_scale 0, CPU generator, against the oracle UNet with merged weights under the restated loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu
from lcm_ref import LCMSchedulerRef, lcm_denoise_ref  # noqa: E402
from test_lora_gpu import merged_oracle, random_lora, spelled  # noqa: E402
from test_model_gpu import cond_inputs, gpu, make_pair, rel_l2  # noqa: E402,F401


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (1, 4, 128, 128), (3, 4, 5, 7)])
def test_lcm_update_vs_restatement(gpu, shape):
    """every step of a 4- and a 5-step schedule (middle steps with noise, the last without) with the same noise on both
    sides; rtol 1e-4 / atol 1e-4 as test_dpm_update_vs_oracle"""
    from pea_diffusion_amd.sampler import LCMScheduler
    for n in (4, 5, 1):
        ref, hip = LCMSchedulerRef(), LCMScheduler()
        ref.set_timesteps(n)
        ts = hip.set_timesteps(n)
        g = torch.Generator().manual_seed(n)
        x_ref = torch.randn(shape, generator=g, dtype=torch.float64)
        x_hip = x_ref.float().cuda()
        for t in ts:
            eps, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
            x_ref, d_ref = ref.step(eps.double(), t, x_ref, noise=noise)
            x_hip, d_hip = hip.step(eps.cuda(), t, x_hip, noise=noise.cuda())
            assert torch.allclose(x_hip.cpu().double(), x_ref, rtol=1e-4, atol=1e-4), (n, int(t))
            assert torch.allclose(d_hip.cpu().double(), d_ref, rtol=1e-4, atol=1e-4), (n, int(t))


def test_lcm_update_op_options(gpu):
    """the raw op: with and without the `denoised` output and the noise, an unaligned view (scalar path), in-place result"""
    from pea_diffusion_amd import ops
    g = torch.Generator().manual_seed(0)
    n = 4 * 33 * 17 + 3
    x, e, z = (torch.randn(n, generator=g) for _ in range(3))
    kx, ke, cp, cn = 1.7, -2.9, 0.8, 0.6
    den = kx * x.double() + ke * e.double()
    for noise in (z, None):
        want = cp * den + (cn * noise.double() if noise is not None else 0.0)
        for with_den in (True, False):
            s = x.cuda().clone()
            d = torch.empty_like(s) if with_den else None
            out = ops.lcm_update_(s, e.cuda(), noise.cuda() if noise is not None else None, kx, ke, cp, cn, d)
            assert out.data_ptr() == s.data_ptr()
            assert torch.allclose(s.cpu().double(), want, rtol=1e-4, atol=1e-4)
            if with_den:
                assert torch.allclose(d.cpu().double(), den, rtol=1e-4, atol=1e-4)
    pad = torch.empty(n + 1, device="cuda")
    s = pad[1:]
    s.copy_(x)
    ops.lcm_update_(s, e.cuda(), z.cuda(), kx, ke, cp, cn)
    s2 = x.cuda().clone()
    ops.lcm_update_(s2, e.cuda(), z.cuda(), kx, ke, cp, cn)
    assert torch.equal(s, s2)


def test_lcm_step_draws_from_a_cpu_generator_like_the_restatement(gpu):
    from pea_diffusion_amd.sampler import LCMScheduler
    ref, hip = LCMSchedulerRef(), LCMScheduler()
    ref.set_timesteps(4)
    g0 = torch.Generator().manual_seed(2)
    x = torch.randn(2, 4, 16, 16, generator=g0)
    gh, gr = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    xh, xr = x.cuda(), x.double()
    for t in hip.set_timesteps(4):
        eps = torch.randn(x.shape, generator=g0)
        xh = hip.step(eps.cuda(), t, xh, generator=gh)[0]
        xr = ref.step(eps, t, xr, generator=gr)[0]
        assert torch.allclose(xh.cpu().double(), xr, rtol=1e-4, atol=1e-4)
    assert torch.equal(gh.get_state(), gr.get_state())


# fused LoRA + LCMScheduler, 4 steps on the tiny UNet: latents rel_l2 against the fp32 oracle loop measured at 2.9e-3 (RHO_LOOP
# below; profiles/EXPERIMENTS.md section 9), the limit is twice that.  It is well under the 3e-2 of the
# 6-step DPM loop because the noise drawn between the steps is common to both sides and carries most of the final latents.
LCM_LOOP_LIMIT = 6e-3
# For the same reason the LoRA has to be large to move the oracle's own result: measured on the CPU, oracle alone, the latents
# shift by 0.25 / 0.30 / 0.35 at RHO 0.5 / 0.75 / 1.0; required: ten times the limit
RHO_LOOP = 1.0


def test_lcm_lora_loop_tiny_vs_oracle(gpu):
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd.lora import lcm_lora_target_keys
    from pea_diffusion_amd.sampler import LCMScheduler, denoise
    B, L, n = 2, 77, 4
    cfg, ref, hip = make_pair(tiny_config, B, L, needs_grad=False)
    base_sd = ref.state_dict()
    keys = lcm_lora_target_keys({k: tuple(v.shape) for k, v in base_sd.items()})
    lora = random_lora(base_sd, keys, 4, RHO_LOOP, seed=3)
    merged = merged_oracle(cfg, ref, lora)
    x, _, ehs, added = cond_inputs(cfg, B, L, cfg.sample_size)
    ehs = ehs.to(torch.bfloat16).float()
    calls = []
    with torch.no_grad():
        want = lcm_denoise_ref(lambda *a, **k: merged(*a, **k), LCMSchedulerRef(), x.clone(), ehs, added, n,
                               generator=torch.Generator().manual_seed(4), calls=calls)
        base = lcm_denoise_ref(lambda *a, **k: ref(*a, **k), LCMSchedulerRef(), x.clone(), ehs, added, n,
                               generator=torch.Generator().manual_seed(4))
    assert calls == [B] * n
    shift = rel_l2(base, want)
    hip.fuse_lora(base_sd, spelled(lora, "kohya"))
    cadd = {k: v.cuda() for k, v in added.items()}
    got = denoise(hip, LCMScheduler(), x.cuda(), ehs.cuda(), cadd, num_inference_steps=n, guidance_scale=0.0,
                  generator=torch.Generator().manual_seed(4))
    e = rel_l2(got, want)
    print(f"[lcm-lora loop tiny, {n} steps, guidance 0] latents rel_l2={e:.3e} (oracle shift by the LoRA {shift:.3f})")
    assert shift > 10 * LCM_LOOP_LIMIT, shift                 # the oracle alone: an ignored LoRA cannot pass
    assert torch.isfinite(got).all() and e < LCM_LOOP_LIMIT
    again = denoise(hip, LCMScheduler(), x.cuda(), ehs.cuda(), cadd, num_inference_steps=n, guidance_scale=0.0,
                    generator=torch.Generator().manual_seed(4))
    assert torch.equal(again, got)                            # bit-reproducible
