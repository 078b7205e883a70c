"""CPU checks of the SDXL-Turbo sampling path: the schedules and host scalars of `EulerDiscrete` / `EulerAncestralDiscrete`
against known answers and the float64 restatement tests/turbo_ref.py, `guidance_scale_embedding`, the planning pass of the
guidance-embedded UNet (`time_cond_proj_dim`), and the loop logic of `denoise` with the HIP step kernel replaced by a torch
statement of its contract (include/pea_hip.h: pea_op_euler_update) -- the kernel itself is checked in tests/test_turbo_gpu.py."""
import ctypes
import math

import pytest
import torch

from pea_diffusion_amd import config as pc
from pea_diffusion_amd import sampler
from pea_diffusion_amd._lib import check, lib
from pea_diffusion_amd.sampler import (DPMSolverMultistep, EulerAncestralDiscrete, EulerDiscrete, denoise,
                                       guidance_scale_embedding)
from turbo_ref import EulerRef, euler_denoise_ref, guidance_scale_embedding_ref

SIGMA_999 = 14.614642              # sqrt((1 - ac) / ac) at t = 999 of the scaled-linear 0.00085-0.012 schedule


def euler_update_cpu_(sample, eps, noise, model_in, k_e, k_n, k_s, dup=1):
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    x = sample
    if eps is not None:
        x = sample + f(k_e) * eps
        if noise is not None:
            x = x + f(k_n) * noise
        sample.copy_(x)
    else:
        assert noise is None and model_in is not None
    if model_in is not None:
        m = x * f(k_s)
        model_in.copy_(m.repeat((dup,) + (1,) * (m.dim() - 1)))
    return sample


@pytest.fixture
def counted(monkeypatch):
    """the `ops` functions the loop may call, counted; torch.cat counted too"""
    calls = {"euler": [], "cfg": 0, "cat": 0}

    def euler(sample, eps, noise, model_in, k_e, k_n, k_s, dup=1):
        calls["euler"].append(("entry" if eps is None else "step", noise is not None, model_in is not None, dup))
        return euler_update_cpu_(sample, eps, noise, model_in, k_e, k_n, k_s, dup)

    def cfg(eps2, g, rescale=0.0):
        calls["cfg"] += 1
        u, t = eps2.chunk(2)
        return u + g * (t - u)

    real_cat = torch.cat

    def cat(*a, **k):
        calls["cat"] += 1
        return real_cat(*a, **k)
    monkeypatch.setattr(sampler.ops, "euler_update_", euler)
    monkeypatch.setattr(sampler.ops, "cfg_combine", cfg)
    monkeypatch.setattr(sampler.torch, "cat", cat)
    return calls


def test_trailing_schedule_known_answers():
    s = EulerAncestralDiscrete()
    assert s.set_timesteps(1).tolist() == [999]
    assert len(s.sigmas) == 2 and s.sigmas[1] == 0.0
    assert s.sigmas[0] == pytest.approx(SIGMA_999, rel=1e-6) and s.init_noise_sigma == s.sigmas[0]
    draws, (sigma, sigma_to, down, up, k_s) = s.next_step_plan()
    assert not draws and up == 0.0 and down == 0.0 and sigma_to == 0.0 and k_s == 1.0 and sigma == s.sigmas[0]
    assert s.set_timesteps(4).tolist() == [999, 749, 499, 249]
    assert s.timesteps.dtype == torch.int64
    ac = s.alphas_cumprod
    for t, sg in zip((999, 749, 499, 249), s.sigmas):
        assert sg == pytest.approx(math.sqrt((1 - ac[t]) / ac[t]), rel=1e-15)


def test_leading_and_linspace_known_answers():
    s = EulerDiscrete()
    ts = s.set_timesteps(30).tolist()
    assert ts[0] == 958 and ts[-1] == 1 and len(ts) == 30 and ts == [33 * j + 1 for j in range(29, -1, -1)]
    assert s.init_noise_sigma == pytest.approx(math.sqrt(max(s.sigmas) ** 2 + 1), rel=1e-15)
    assert s.init_noise_sigma != 1.0
    lin = EulerDiscrete(timestep_spacing="linspace")
    ts = lin.set_timesteps(4).tolist()
    assert ts == pytest.approx([999.0, 666.0, 333.0, 0.0]) and lin.init_noise_sigma == max(lin.sigmas)
    assert lin.set_timesteps(3).tolist() == pytest.approx([999.0, 499.5, 0.0])
    ac = lin.alphas_cumprod
    sg = lambda t: math.sqrt((1 - ac[t]) / ac[t])
    assert lin.sigmas[1] == pytest.approx(0.5 * (sg(499) + sg(500)), rel=1e-14)      # linear interpolation
    with pytest.raises(ValueError):
        EulerDiscrete(timestep_spacing="karras")
    with pytest.raises(ValueError):
        s.set_timesteps(0)


@pytest.mark.parametrize("n", [1, 2, 4, 7, 30])
def test_ancestral_sigmas_split_the_target_variance(n):
    s = EulerAncestralDiscrete()
    s.set_timesteps(n)
    for i in range(n):
        s._i = i
        draws, (sigma, sigma_to, down, up, k_s) = s.next_step_plan()
        assert abs(up * up + down * down - sigma_to * sigma_to) <= 1e-12
        assert draws == (i != n - 1) and (up > 0) == draws
        assert k_s == pytest.approx(1.0 / math.sqrt(sigma_to ** 2 + 1.0), rel=1e-15)


@pytest.mark.parametrize("ancestral", [False, True])
@pytest.mark.parametrize("spacing,offset", [("leading", 1), ("leading", 0), ("linspace", 0), ("trailing", 0)])
def test_host_scalars_equal_the_float64_restatement(ancestral, spacing, offset):
    cls = EulerAncestralDiscrete if ancestral else EulerDiscrete
    for n in (1, 2, 3, 4, 6, 30, 50):
        hip = cls(timestep_spacing=spacing, steps_offset=offset)
        ref = EulerRef(ancestral, spacing, offset)
        got_ts, want_ts = hip.set_timesteps(n).tolist(), ref.set_timesteps(n).tolist()
        assert got_ts == pytest.approx(want_ts, abs=1e-9), (n, got_ts, want_ts)
        assert abs(hip.init_noise_sigma - ref.init_noise_sigma) <= 1e-12
        for i in range(n):
            hip._i = i
            _, got = hip.next_step_plan()
            for g, w in zip(got[:4], ref.scalars(i)):
                assert abs(g - w) <= 1e-12, (n, i, got, ref.scalars(i))
    with pytest.raises(ValueError):
        hip._i = n
        hip.next_step_plan()                                 # past the end of the schedule


def test_defaults_and_begin_index():
    e, a = EulerDiscrete(), EulerAncestralDiscrete()
    assert (e.timestep_spacing, e.steps_offset, e.ancestral) == ("leading", 1, False)
    assert (a.timestep_spacing, a.ancestral) == ("trailing", True)
    with pytest.raises(ValueError):
        e.set_begin_index(0)
    e.set_timesteps(6)
    e.set_begin_index(3)
    assert e.next_step_plan()[1][0] == e.sigmas[3]
    with pytest.raises(ValueError):
        e.set_begin_index(6)


def test_guidance_scale_embedding():
    w = torch.tensor([0.0, 1.0, 7.0, 0.5])
    got = guidance_scale_embedding(w)
    want = guidance_scale_embedding_ref(w.tolist())
    assert tuple(got.shape) == (4, 256) and got.dtype == torch.float64
    assert (got - want).abs().max() <= 1e-12
    assert torch.equal(got[0, :128], torch.zeros(128, dtype=torch.float64)) and torch.equal(got[0, 128:], torch.ones(128, dtype=torch.float64))
    # the first half is sines: column 0 has frequency 1, so it is sin(1000 w); the cosines of it sit in column 128
    assert got[1, 0] == pytest.approx(math.sin(1000.0), abs=1e-12) and got[1, 128] == pytest.approx(math.cos(1000.0), abs=1e-12)
    # divisor half - 1: the last frequency is exactly 1 / 10000
    assert got[1, 127] == pytest.approx(math.sin(0.1), abs=1e-12)
    assert tuple(guidance_scale_embedding(7.0, 128).shape) == (1, 128)
    assert (guidance_scale_embedding([1.5, 2.0], 128) - guidance_scale_embedding_ref([1.5, 2.0], 128)).abs().max() <= 1e-12


# ---------------------------------------------------------------------------------------------- planning (no device)
def _plan(cfg, hw=128, flags=0, B=2, L=77, dim=None):
    c = pc.to_c(cfg)
    n_ops, n_w, n_attn, n_pre = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    n_par = ctypes.c_longlong()
    rc = lib().pea_unet_plan_cond(ctypes.byref(c), B, hw, hw, L, flags, pc.time_cond_dim(cfg) if dim is None else dim,
                                  ctypes.byref(n_ops), ctypes.byref(n_w), ctypes.byref(n_par), None, None, None,
                                  ctypes.byref(n_attn), ctypes.byref(n_pre))
    return rc, dict(ops=n_ops.value, weights=n_w.value, params=n_par.value, attn=n_attn.value, pre=n_pre.value)


def test_lcm_sdxl_config_and_plan():
    cfg = pc.lcm_sdxl_config()
    assert cfg.time_cond_proj_dim == 256 and pc.sdxl_config().time_cond_proj_dim is None
    assert pc.time_cond_dim(cfg) == 256 and pc.time_cond_dim(pc.sdxl_config()) == 0
    d = dict(block_out_channels=[320, 640, 1280], down_block_types=list(cfg.down_block_types), up_block_types=list(cfg.up_block_types),
             attention_head_dim=[5, 10, 20], time_cond_proj_dim=256)
    assert pc.unet_config_from_diffusers(d).time_cond_proj_dim == 256
    d["time_cond_proj_dim"] = None
    assert pc.unet_config_from_diffusers(d).time_cond_proj_dim is None
    rc, plain = _plan(pc.sdxl_config())
    assert rc == 0 and plain["params"] == 2_567_463_684
    rc, lcm = _plan(cfg)
    assert rc == 0 and lcm["params"] == 2_567_545_604 == plain["params"] + 320 * 256
    assert lcm["weights"] == plain["weights"] + 1 and lcm["ops"] == plain["ops"] + 1
    # the attention census is unchanged and every attention is still fed a prescaled Q (tests/test_attn_census_cpu.py)
    assert (lcm["attn"], lcm["pre"]) == (plain["attn"], plain["pre"]) == (140, 140)
    for flags in (0, 1, 2):
        rc, p = _plan(cfg, flags=flags)
        assert rc == 0 and p["attn"] == p["pre"] == 140
    # the plain planning entry point is the cond one with width 0
    n_par = ctypes.c_longlong()
    c = pc.to_c(cfg)
    check(lib().pea_unet_plan(ctypes.byref(c), 2, 128, 128, 77, 0, None, None, ctypes.byref(n_par), None, None, None))
    assert n_par.value == plain["params"]


def _plan_weight(cfg, name, dim):
    c = pc.to_c(cfg)
    numel, kind, d0, d1 = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib().pea_unet_plan_weight(ctypes.byref(c), 1, 64, 64, 77, 0, dim, name.encode(), ctypes.byref(numel), ctypes.byref(kind),
                                    ctypes.byref(d0), ctypes.byref(d1))
    return rc, (numel.value, kind.value, d0.value, d1.value)


def test_plan_lists_the_cond_proj_weight():
    cfg = pc.lcm_sdxl_config()
    rc, info = _plan_weight(cfg, "time_embedding.cond_proj.weight", 256)
    assert rc == 0 and info == (320 * 256, 1, 320, 256)                     # kind 1: a Linear [N][K]
    assert _plan_weight(cfg, "time_embedding.cond_proj.bias", 256)[0] == -5      # bias-free
    assert _plan_weight(cfg, "time_embedding.cond_proj.weight", 0)[0] == -5      # PEA_E_NOTFOUND on a plain UNet
    assert _plan_weight(cfg, "time_embedding.linear_1.weight", 256) == (0, (1280 * 320, 1, 1280, 320))


def test_plan_refuses_a_width_the_gemm_cannot_take():
    rc, _ = _plan(pc.tiny_config(), hw=16, dim=100)
    assert rc == -3
    msg = lib().pea_last_error().decode()
    assert "time_cond_proj_dim=100" in msg and "multiple of 64" in msg
    assert _plan(pc.tiny_config(), hw=16, dim=-64)[0] == -1
    assert _plan(pc.tiny_config(), hw=16, dim=128)[0] == 0


def test_kernel_argument_errors_need_no_device():
    L = lib()
    one = ctypes.c_void_p(16)
    assert L.pea_op_euler_update(one, one, None, one, 0, 1, 1.0, 0.0, 1.0, None) == -3 and b"n=0" in L.pea_last_error()
    assert L.pea_op_euler_update(one, one, None, one, 8, 3, 1.0, 0.0, 1.0, None) == -3 and b"dup=3" in L.pea_last_error()
    assert L.pea_op_euler_update(None, one, None, one, 8, 1, 1.0, 0.0, 1.0, None) == -1
    assert L.pea_op_euler_update(one, None, None, None, 8, 1, 1.0, 0.0, 1.0, None) == -1      # entry form without an output
    assert L.pea_op_euler_update(one, None, one, one, 8, 1, 1.0, 0.0, 1.0, None) == -1        # entry form with noise
    assert L.pea_unet_set_timestep_cond(None, None, None) == -1


# ---------------------------------------------------------------------------------------------- the loop, without a device
W4 = torch.linspace(-0.3, 0.4, 16).reshape(4, 4)


def make_toy(calls):
    def toy_unet(x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False, timestep_cond=None):
        calls.append((x.shape[0], float(t)))
        y = torch.einsum("oc,bchw->bohw", W4.to(x.dtype), x) * (1.0 + 1e-4 * float(t)) + 0.1
        if timestep_cond is not None:
            y = y + timestep_cond.to(x.dtype).mean(dim=1)[:, None, None, None]
        if x.shape[0] % 2 == 0:
            y[x.shape[0] // 2:] *= 1.25                     # the "text" half of a CFG batch differs from the unconditional one
        return (y,)
    return toy_unet


def test_refusal_of_timestep_cond_on_a_plain_unet(counted):
    lat = torch.zeros(2, 4, 8, 8)
    for sched in (EulerAncestralDiscrete(), DPMSolverMultistep()):
        with pytest.raises(ValueError, match="timestep_cond"):
            denoise(make_toy([]), sched, lat, None, None, num_inference_steps=2, guidance_scale=0.0,
                    timestep_cond=torch.zeros(2, 256))


@pytest.mark.parametrize("ancestral,n,g", [(True, 1, 0.0), (True, 4, 0.0), (False, 6, 5.0), (False, 3, 0.0), (True, 3, 5.0)])
def test_loop_launches_and_result(counted, ancestral, n, g):
    """n + 1 euler_update launches (the entry call and one per step), scale_model_input / step interleaved, one CFG combine per
    step under guidance, the doubled batch from dup == 2 and never from torch.cat; the result equals the restated loop"""
    B = 3
    do_cfg = g > 1.0
    seq = []
    cls = EulerAncestralDiscrete if ancestral else EulerDiscrete

    class Logged(cls):
        def scale_model_input(self, *a, **k):
            seq.append("scale")
            return super().scale_model_input(*a, **k)

        def step(self, *a, **k):
            seq.append("step")
            return super().step(*a, **k)
    lat = torch.randn(B, 4, 8, 8, generator=torch.Generator().manual_seed(5))
    ucalls, rcalls = [], []
    got = denoise(make_toy(ucalls), Logged(), lat.clone(), None, None, num_inference_steps=n, guidance_scale=g,
                  generator=torch.Generator().manual_seed(9))
    dup = 2 if do_cfg else 1
    assert seq == ["scale", "step"] * n
    assert counted["euler"] == [("entry", False, True, dup)] + \
        [("step", ancestral and i != n - 1, i != n - 1, dup) for i in range(n)]
    assert len(counted["euler"]) == n + 1
    assert counted["cfg"] == (n if do_cfg else 0) and counted["cat"] == 0
    ref = EulerRef(ancestral)
    want = euler_denoise_ref(make_toy(rcalls), ref, lat.clone(), None, None, n, guidance_scale=g,
                             generator=torch.Generator().manual_seed(9))
    assert [c[0] for c in ucalls] == [dup * B] * n and [c[1] for c in ucalls] == [float(t) for t in ref.timesteps]
    assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))


def test_loop_passes_timestep_cond_to_a_guidance_embedded_unet(counted):
    B, n = 2, 2
    seen = []
    toy = make_toy([])

    class Embedded:
        time_cond_proj_dim = 256

        def __call__(self, x, t, timestep_cond=None, **k):
            seen.append(None if timestep_cond is None else tuple(timestep_cond.shape))
            return toy(x, t, timestep_cond=timestep_cond, **k)
    cond = guidance_scale_embedding(torch.full((B,), 7.0))
    lat = torch.randn(B, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    unet = Embedded()
    unet.B = B
    got = denoise(unet, EulerDiscrete(), lat.clone(), None, None, num_inference_steps=n, guidance_scale=0.0, timestep_cond=cond)
    assert seen == [(B, 256)] * n
    want = euler_denoise_ref(make_toy([]), EulerRef(False), lat.clone(), None, None, n, timestep_cond=cond)
    assert torch.allclose(got.double(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    base = denoise(unet, EulerDiscrete(), lat.clone(), None, None, num_inference_steps=n, guidance_scale=0.0)
    assert seen[-1] is None and not torch.equal(base, got)
    # under CFG the conditioning is doubled once, outside the loop, for a UNet built for 2B
    seen.clear()
    unet.B = 2 * B
    denoise(unet, EulerDiscrete(), lat.clone(), None, None, num_inference_steps=n, guidance_scale=5.0, timestep_cond=cond)
    assert seen == [(2 * B, 256)] * n


def test_scale_model_input_reuses_the_step_buffer_only_for_that_steps_result(counted):
    s = EulerDiscrete()
    s.set_timesteps(3)
    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(2)) * s.init_noise_sigma
    m0 = s.scale_model_input(x, s.timesteps[0])
    assert torch.allclose(m0, x / math.sqrt(s.sigmas[0] ** 2 + 1)) and len(counted["euler"]) == 1
    out = s.step(torch.ones_like(x), s.timesteps[0], x)[0]
    assert out is x and len(counted["euler"]) == 2
    m1 = s.scale_model_input(out, s.timesteps[1])
    assert len(counted["euler"]) == 2                          # handed out, not recomputed
    assert torch.equal(m1, out * torch.tensor(1.0 / math.sqrt(s.sigmas[1] ** 2 + 1), dtype=torch.float32))
    other = out.clone()
    m2 = s.scale_model_input(other, s.timesteps[1])              # any other tensor: the entry form
    assert len(counted["euler"]) == 3 and counted["euler"][-1][0] == "entry" and torch.equal(m2, m1)


def test_existing_schedulers_keep_the_cat_path(counted, monkeypatch):
    """DPM-Solver under CFG: the loop still doubles with torch.cat and calls scale_model_input(x, t) without `dup`"""
    monkeypatch.setattr(sampler.ops, "dpm_update_", lambda sample, eps, x0_prev, a, s, cs, c0, c1: sample)
    args = []

    class Logged(DPMSolverMultistep):
        def scale_model_input(self, *a, **k):
            args.append((len(a), dict(k)))
            return super().scale_model_input(*a, **k)
    denoise(make_toy([]), Logged(), torch.zeros(2, 4, 8, 8), None, None, num_inference_steps=3, guidance_scale=5.0)
    assert counted["cat"] == 3 and counted["euler"] == [] and args == [(2, {})] * 3
