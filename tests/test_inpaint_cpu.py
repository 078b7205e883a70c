"""CPU checks of the inpainting pieces that need no device: strength -> timesteps (tests/test_sdxl_zh_inpaint.py:383-417),
the scheduler's begin index against oracle/sampler_ref.py, the 9-channel configuration, the host-side plan of an inpainting
UNet context (PEA_UNET_INPAINT_INPUTS) and the CPU restatement of the input preparation."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.sampler_ref import DPMSolverMultistepRef
from pea_diffusion_amd import _lib
from pea_diffusion_amd import config as pc
from pea_diffusion_amd.inpaint import get_timesteps
from pea_diffusion_amd.sampler import DPMSolverMultistep

INPAINT = 4            # PEA_UNET_INPAINT_INPUTS


def _sched(n):
    s = DPMSolverMultistep()
    s.set_timesteps(n)
    return s


def test_get_timesteps_default_strength_skips_the_first_step():
    s = _sched(50)
    ts, left, t_start = get_timesteps(s, 50, 0.9999)
    assert left == 49 and t_start == 1 and len(ts) == 49 and torch.equal(ts, s.timesteps[1:])


def test_get_timesteps_strength_cases():
    s = _sched(30)
    ts, left, t_start = get_timesteps(s, 30, 0.3)
    assert left == 9 and t_start == 21 and torch.equal(ts, s.timesteps[21:])
    ts, left, t_start = get_timesteps(s, 30, 1.0)
    assert left == 30 and t_start == 0 and torch.equal(ts, s.timesteps)
    with pytest.raises(ValueError):
        get_timesteps(s, 30, 0.02)          # int(30 * 0.02) = 0 steps left


@pytest.mark.parametrize("n,start", [(50, 1), (30, 21), (6, 2), (10, 9), (20, 0)])
def test_set_begin_index_matches_oracle_at_the_offset(n, start):
    hip, ref = DPMSolverMultistep(), DPMSolverMultistepRef()
    hip.set_timesteps(n)
    ref.set_timesteps(n)
    hip.set_begin_index(start)
    ref.step_index, ref.lower_order_nums = start, 0
    for i in range(start, n):
        order, coef = hip.next_step_plan()
        want = ref.order_at(i)
        assert order == want, (i, order, want)
        np.testing.assert_allclose(coef, ref.coefficients(i, want), rtol=1e-12)
        if i == start:
            assert order == 1                     # no earlier data prediction exists
        hip._advance()
        ref.step_index += 1
        ref.lower_order_nums = min(ref.lower_order_nums + 1, ref.solver_order)


def test_set_begin_index_changes_nothing_for_existing_callers():
    a, b = _sched(30), _sched(30)
    b.set_begin_index(0)
    for _ in range(30):
        assert a.next_step_plan() == b.next_step_plan()
        a._advance()
        b._advance()
    with pytest.raises(ValueError):
        _sched(30).set_begin_index(30)


def test_sdxl_inpaint_config():
    c = pc.sdxl_inpaint_config()
    base = pc.sdxl_config()
    assert c.in_channels == 9 and c.out_channels == 4 and c.name == "sdxl_inpaint"
    assert {k: v for k, v in c.__dict__.items() if k not in ("in_channels", "name")} == \
           {k: v for k, v in base.__dict__.items() if k not in ("in_channels", "name")}
    d = pc.unet_config_from_diffusers(dict(in_channels=9, out_channels=4, block_out_channels=[320, 640, 1280],
                                           down_block_types=list(base.down_block_types), up_block_types=list(base.up_block_types),
                                           attention_head_dim=[5, 10, 20], transformer_layers_per_block=[1, 2, 10]))
    assert d.in_channels == 9


def _plan(cfg, flags, B=2):
    L = _lib.lib()
    c = pc.to_c(cfg)
    npar = C.c_longlong()
    rc = L.pea_unet_plan(C.byref(c), B, 128, 128, 77, flags, None, None, C.byref(npar), None, None, None)
    return rc, npar.value, L.pea_last_error()


def test_plan_accepts_the_inpainting_flag_on_a_9_channel_unet():
    rc, npar, _ = _plan(pc.sdxl_inpaint_config(), INPAINT)
    assert rc == 0
    rc0, base, _ = _plan(pc.sdxl_config(), 0)
    assert rc0 == 0 and npar == base + 5 * 320 * 9 == 2_567_463_684 + 14_400
    rc, npar_plain, _ = _plan(pc.sdxl_inpaint_config(), 0)      # the plain 9-channel context (reference's own input)
    assert rc == 0 and npar_plain == npar


def test_plan_refuses_inpainting_with_grad_or_on_4_channels():
    rc, _, msg = _plan(pc.sdxl_inpaint_config(), INPAINT | 1)
    assert rc == -3 and b"PEA_UNET_GRAD" in msg
    rc, _, msg = _plan(pc.sdxl_config(), INPAINT)
    assert rc == -3 and b"in_channels" in msg


def test_prepare_restatement_semantics():
    """the torch restatement the GPU kernel is checked against: binarise at 0.5 (0.5 itself is masked), keep factor 0/1,
    nearest resize = every 8th pixel"""
    from inpaint_ref import prepare_ref
    img = torch.rand(1, 3, 16, 16)
    m = torch.zeros(1, 1, 16, 16)
    m[..., 0, 0] = 0.5
    m[..., 8, 8] = 0.4999
    m[..., 3, 3] = 1.0
    init, masked, lm = prepare_ref(img, m)
    assert torch.equal(init, 2 * img - 1)
    assert masked[0, :, 0, 0].eq(0).all() and masked[0, :, 3, 3].eq(0).all() and torch.equal(masked[0, :, 8, 8], init[0, :, 8, 8])
    assert lm.shape == (1, 1, 2, 2) and lm.flatten().tolist() == [1.0, 0.0, 0.0, 0.0]
