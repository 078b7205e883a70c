"""CPU checks of the LCM few-step sampler: the schedule and host scalars of `LCMScheduler` against the float64 restatement in
tests/lcm_ref.py, and the step / loop logic with the HIP update kernel replaced by a torch statement of its contract
(include/pea_hip.h: pea_op_lcm_update) -- the kernel itself is checked in tests/test_lcm_gpu.py."""
import math

import pytest
import torch

from lcm_ref import LCMSchedulerRef, lcm_denoise_ref
from pea_diffusion_amd import sampler
from pea_diffusion_amd.sampler import LCMScheduler, denoise


def lcm_update_cpu_(sample, eps, noise, kx, ke, c_prev, c_noise, denoised=None):
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    d = f(kx) * sample + f(ke) * eps
    y = f(c_prev) * d
    if noise is not None:
        y = y + f(c_noise) * noise
    sample.copy_(y)
    if denoised is not None:
        denoised.copy_(d)
    return sample


@pytest.fixture
def cpu_kernel(monkeypatch):
    monkeypatch.setattr(sampler.ops, "lcm_update_", lcm_update_cpu_)


def test_timesteps():
    s = LCMScheduler()
    assert s.set_timesteps(4).tolist() == [999, 759, 519, 279]
    assert s.set_timesteps(5).tolist() == [999, 799, 599, 399, 199]
    assert s.set_timesteps(1).tolist() == [999]
    assert s.set_timesteps(50).tolist() == list(range(999, 0, -20))
    assert s.timesteps.dtype == torch.int64 and s.init_noise_sigma == 1.0
    with pytest.raises(ValueError):
        s.set_timesteps(51)
    with pytest.raises(ValueError):
        s.set_timesteps(0)
    x = torch.ones(2)
    assert s.scale_model_input(x, 999) is x


def test_boundary_scalings():
    s = LCMScheduler()
    assert s.boundary_scalings(0) == (1.0, 0.0)                  # t = 0: the consistency function is the identity
    for t in (1, 19, 279, 999):
        c_skip, c_out = s.boundary_scalings(t)
        assert c_skip == pytest.approx(0.25 / (100.0 * t * t + 0.25), rel=1e-15)
        assert c_out == pytest.approx(10.0 * t / math.sqrt(100.0 * t * t + 0.25), rel=1e-15)
        assert c_out ** 2 + c_skip == pytest.approx(1.0, rel=1e-12)       # c_out^2 = 1 - c_skip for these two formulas
    c_skip, c_out = s.boundary_scalings(999)
    assert c_skip < 3e-9 and 1.0 - c_out < 2e-9


def test_host_scalars_equal_the_float64_restatement():
    for n in (1, 2, 4, 5, 8, 50):
        hip, ref = LCMScheduler(), LCMSchedulerRef()
        assert hip.set_timesteps(n).tolist() == ref.set_timesteps(n).tolist()
        for i in range(n):
            hip._i = i
            last, (sa, sb, c_skip, c_out, sp, sn) = hip.next_step_plan()
            a_t, a_prev, r_skip, r_out = ref.scalars(i)
            assert last == (i == n - 1)
            for got, want in ((sa, math.sqrt(a_t)), (sb, math.sqrt(1 - a_t)), (c_skip, r_skip), (c_out, r_out),
                              (sp, math.sqrt(a_prev)), (sn, math.sqrt(1 - a_prev))):
                assert abs(got - want) <= 1e-12, (n, i, got, want)
    assert abs(LCMScheduler().alphas_cumprod[0] - (1 - 0.00085)) < 1e-15


def test_constant_x0_steps(cpu_kernel):
    """eps consistent with a constant x0 = c (eps = (x - sqrt(a_t) c) / sqrt(1 - a_t)) and zero noise: every step returns
    sqrt(a_prev) (c_out c + c_skip x), the last returns denoised = c_out c + c_skip x"""
    c, n = 0.37, 5
    hip, ref = LCMScheduler(), LCMSchedulerRef()
    ref.set_timesteps(n)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, 8, generator=g)
    for i, t in enumerate(hip.set_timesteps(n)):
        a_t, a_prev, c_skip, c_out = ref.scalars(i)
        x64 = x.double()
        eps = ((x64 - math.sqrt(a_t) * c) / math.sqrt(1 - a_t)).float()
        den = c_out * c + c_skip * x64
        want = den if i == n - 1 else math.sqrt(a_prev) * den
        r_out, r_den = ref.step(eps, t, x, noise=torch.zeros_like(x))
        out, got_den = hip.step(eps, t, x.clone(), noise=torch.zeros_like(x))
        assert torch.allclose(r_out, want, rtol=0, atol=2e-5) and torch.allclose(r_den, den, rtol=0, atol=2e-5)
        assert torch.allclose(out.double(), want, rtol=0, atol=2e-5) and torch.allclose(got_den.double(), den, rtol=0, atol=2e-5)
        x = out
    with pytest.raises(ValueError):
        hip.step(eps, t, x)                          # past the end of the schedule


def test_step_draws_noise_like_the_restatement(cpu_kernel):
    """same CPU generator state on both sides -> the same noise, so the two agree to fp32 rounding; the last step draws none"""
    n = 4
    hip, ref = LCMScheduler(), LCMSchedulerRef()
    ref.set_timesteps(n)
    g0 = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 8, 8, generator=g0)
    gh, gr = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    xh, xr = x.clone(), x.double()
    for t in hip.set_timesteps(n):
        eps = torch.randn(x.shape, generator=g0)
        xh = hip.step(eps, t, xh, generator=gh)[0]
        xr = ref.step(eps, t, xr, generator=gr)[0]
        assert torch.allclose(xh.double(), xr, rtol=1e-5, atol=1e-5)
    assert torch.equal(gh.get_state(), gr.get_state())            # the same number of draws: none on the last step


def test_loop_makes_n_calls_at_batch_b(cpu_kernel):
    """guidance_scale 0: no CFG doubling, n UNet evaluations at batch B, and the loop equals the restated one"""
    B, n = 3, 4
    calls = []
    W = torch.linspace(-0.3, 0.4, 16).reshape(4, 4)

    def toy_unet(x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        calls.append((x.shape[0], int(t)))
        return (torch.einsum("oc,bchw->bohw", W.to(x.dtype), x) * (1.0 + 1e-4 * float(t)) + 0.1,)

    g = torch.Generator().manual_seed(5)
    lat = torch.randn(B, 4, 8, 8, generator=g)
    got = denoise(toy_unet, LCMScheduler(), lat.clone(), None, None, num_inference_steps=n, guidance_scale=0.0,
                  generator=torch.Generator().manual_seed(9))
    assert calls == [(B, t) for t in (999, 759, 519, 279)]
    rcalls = []
    want = lcm_denoise_ref(toy_unet, LCMSchedulerRef(), lat.clone(), None, None, n, generator=torch.Generator().manual_seed(9),
                           calls=rcalls)
    assert rcalls == [B] * n
    assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError, match="timestep_cond"):
        denoise(toy_unet, LCMScheduler(), lat, None, None, num_inference_steps=n, guidance_scale=0.0,
                timestep_cond=torch.zeros(B, 256))
