"""Self-attention guidance without a GPU: the column-sum launcher's grid rule and refusals through
pea_debug_attn_colsum_dispatch, the null-operand refusals of the C ABI, `sag.nearest_tables` against `F.interpolate`,
`sag.sag_coefficients` against the closed forms of the four schedulers, and the restatement's own blur (tests/sag_ref.py)
against a direct double loop at the smallest reflect case."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from sag_ref import coefficients_ref, degrade_ref, gaussian_taps

# the shapes of tests/test_sag_gpu.py, (B, H, Sq, Skv)
SHAPES = [(1, 1, 1, 1), (2, 2, 16, 16), (1, 3, 33, 33), (1, 2, 64, 64), (1, 2, 91, 91), (2, 3, 129, 129), (1, 2, 260, 33),
          (1, 1, 64, 7), (2, 5, 256, 256), (2, 20, 1024, 1024)]


def _dispatch(B, H, Sq, Skv, nd=1, ldq=0, ldk=0, flags=0):
    from pea_diffusion_amd._lib import lib
    q = (ctypes.c_int * 8)(B, H, Sq, Skv, nd, ldq, ldk, flags)
    out = (ctypes.c_int * 6)()
    rc = lib().pea_debug_attn_colsum_dispatch(q, out)
    return rc, list(out)


@pytest.mark.parametrize("shape", SHAPES + [(64, 20, 1024, 1024), (4, 20, 1024, 1024), (1, 7, 300, 4096), (3, 7, 50, 50)])
def test_colsum_dispatch_covers_heads_and_keys(shape):
    from pea_diffusion_amd._lib import lib
    B, H, Sq, Skv = shape
    for flags in (0, 1):
        rc, (G, gx, gy, gz, lds, hpg) = _dispatch(B, H, Sq, Skv, flags=flags)
        assert rc == 0, lib().pea_last_error()
        assert 1 <= G <= H and hpg >= 1
        assert G * hpg >= H and (G - 1) * hpg < H                    # the groups cover the heads and none is empty
        assert gx * 128 >= Skv and (gx - 1) * 128 < Skv              # 128 keys per workgroup cover the keys
        assert (gy, gz) == (G, B)
        assert lds == 2 * 4 * (8192 + 256)                           # two stages of four 64 x 64 bf16 Q tiles and their row constants
        assert lib().pea_op_attention_colsum_groups(B, H, Sq, Skv) == G


def test_colsum_dispatch_fills_the_chip_at_the_sdxl_mid_block():
    """B = 2, H = 20, 1024 tokens: 16 (sample, key block) pairs; with all 20 heads in one workgroup that is 16 workgroups on
    256 CUs.  The rule cuts the heads until one round of 512 workgroup slots is there or every head stands alone."""
    rc, (G, gx, gy, gz, lds, hpg) = _dispatch(2, 20, 1024, 1024)
    assert rc == 0 and gx * gy * gz >= 256, (G, gx, gy, gz)
    assert (G, hpg) == (20, 1)
    rc, (G, gx, gy, gz, lds, hpg) = _dispatch(64, 20, 1024, 1024)    # the key blocks alone fill it: nothing to cut
    assert rc == 0 and (G, hpg) == (1, 20)
    rc, (G, gx, gy, gz, lds, hpg) = _dispatch(8, 20, 1024, 1024)     # 64 pairs: 8 groups would do, made even: 7 of 3 heads
    assert rc == 0 and (G, hpg) == (7, 3)


def test_colsum_dispatch_refusals():
    from pea_diffusion_amd._lib import lib
    L = lib()
    for kw, msg in ((dict(nd=2), b"head_dim 64"), (dict(B=0), b"empty problem"), (dict(Sq=0), b"empty problem"),
                    (dict(Skv=0), b"empty problem"), (dict(H=0), b"empty problem"), (dict(ldq=132), b"multiples of 8"),
                    (dict(ldk=140), b"multiples of 8"), (dict(ldq=64), b"hold every head"), (dict(flags=2), b"null lse"),
                    (dict(B=65536), b"empty problem")):
        args = dict(B=2, H=2, Sq=64, Skv=64)
        args.update(kw)
        rc, _ = _dispatch(**args)
        assert rc == -3 and msg in L.pea_last_error(), (kw, L.pea_last_error())
    assert L.pea_op_attention_colsum_groups(0, 2, 8, 8) == -3


def test_null_operands_are_refused_through_the_c_abi():
    from pea_diffusion_amd._lib import lib
    L = lib()
    page = (ctypes.c_float * 64)()
    p = ctypes.cast(page, ctypes.c_void_p)
    ok = dict(Q=p, K=p, lse=p, part=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        rc = L.pea_op_attention_colsum(a["Q"], 128, a["K"], 128, a["lse"], a["part"], 1, 2, 8, 8, 0.125, 0, None)
        assert rc == -3 and b"null" in L.pea_last_error(), (missing, L.pea_last_error())
    ok = dict(lat=p, eps=p, part=p, iy=p, ix=p, out=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        rc = L.pea_op_sag_degrade(a["lat"], a["eps"], a["part"], 1, 2, 2, a["iy"], a["ix"], a["out"], 1, 4, 8, 8, 1.0, -1.0, 1.0, 1.0, None)
        assert rc == -3 and b"null operand" in L.pea_last_error(), missing
    rc = L.pea_op_sag_degrade(p, p, p, 0, 2, 2, p, p, p, 1, 4, 8, 8, 1.0, -1.0, 1.0, 1.0, None)
    assert rc == -3 and b"G=0" in L.pea_last_error()
    for H, W in ((4, 8), (8, 4)):
        rc = L.pea_op_sag_degrade(p, p, p, 1, 2, 2, p, p, p, 1, 4, H, W, 1.0, -1.0, 1.0, 1.0, None)
        assert rc == -3 and b"reflect padding" in L.pea_last_error()
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.pea_op_cfg_sag_combine(a[0], a[1], a[2], 1, 64, 1, 5.0, 0.75, None) == -3
    assert L.pea_unet_enable_sag(None, 0, 0, 1) == -1 and L.pea_unet_disable_sag(None) == -1
    assert L.pea_unet_sag_colsum(None, None, None, None) == -1


@pytest.mark.parametrize("hw,HW", [((8, 8), (64, 64)), ((32, 32), (128, 128)), ((7, 13), (56, 104)), ((26, 26), (102, 102)),
                                   ((2, 2), (8, 8)), ((1, 1), (5, 5)), ((4, 4), (16, 16))])
def test_nearest_tables_are_interpolate_nearest(hw, HW):
    from pea_diffusion_amd.sag import nearest_tables
    (h, w), (H, W) = hw, HW
    iy, ix = nearest_tables(h, w, H, W)
    assert iy.dtype == torch.int32 and ix.dtype == torch.int32 and tuple(iy.shape) == (H,) and tuple(ix.shape) == (W,)
    src = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
    want = F.interpolate(src, size=(H, W), mode="nearest")[0, 0]
    got = src[0, 0][iy.long()][:, ix.long()]
    assert torch.equal(got, want)


def _schedulers():
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerAncestralDiscrete, EulerDiscrete, LCMScheduler
    return [(DPMSolverMultistep(), 5, "alpha"), (LCMScheduler(), 4, "alpha"), (EulerDiscrete(), 5, "sigma"),
            (EulerAncestralDiscrete(), 3, "sigma")]


def test_sag_coefficients_closed_forms_and_round_trip():
    """the closed forms, and with an all-false mask the degraded input is scale_model_input(x): alpha-space x itself, sigma-space
    x / sqrt(sigma^2 + 1)"""
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.sag import sag_coefficients
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(2, 4, 9, 11, generator=g, dtype=torch.float64), torch.randn(2, 4, 9, 11, generator=g, dtype=torch.float64)
    none = torch.zeros(2, 3, 3, dtype=torch.bool)
    for sch, n, kind in _schedulers():
        with pytest.raises(PeaError):
            sag_coefficients(sch, 0)                                 # no schedule yet
        sch.set_timesteps(n)
        for i in range(n):
            got = sag_coefficients(sch, i)
            if type(sch).__name__ == "LCMScheduler":
                a = float(sch.alphas_cumprod[int(sch.timesteps[i])])
                sigma = math.sqrt(1.0 - a) / math.sqrt(a)
                want = (1.0 / math.sqrt(a), -math.sqrt(1.0 - a) / math.sqrt(a), math.sqrt(a), math.sqrt(1.0 - a))
                assert got == pytest.approx(want, rel=1e-12)
            else:
                sigma = float(sch.sigmas[i])
            assert got == pytest.approx(coefficients_ref(kind, sigma), rel=1e-12)
            k = 1.0 / math.sqrt(sigma * sigma + 1.0)
            xs = x / k if kind == "sigma" else x                     # a sigma-space latent has that magnitude
            back = degrade_ref(xs, eps, none, *got)
            want_in = xs * k if kind == "sigma" else xs              # scale_model_input
            assert float((back - want_in).abs().max() / want_in.abs().max()) <= 1e-6
        with pytest.raises(PeaError):
            sag_coefficients(sch, n)

    class Other:
        timesteps = [1]
    with pytest.raises(PeaError, match="no rule"):
        sag_coefficients(Other(), 0)


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def test_degrade_ref_against_a_double_loop():
    """6 x 5: the smallest width reflect padding of 4 takes, and rows that reflect from both edges"""
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 3, 6, 5
    x, eps = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    mask = torch.tensor([[[True, False], [False, True]], [[False, False], [True, True]]])
    c = (1.25, -0.75, 0.8, 0.6)
    got = degrade_ref(x, eps, mask, *c)
    w = gaussian_taps().double()
    x0 = (c[0] * x + c[1] * eps).double()
    want = torch.empty(B, C, H, W, dtype=torch.float64)
    for b in range(B):
        for ch in range(C):
            for y in range(H):
                for xx in range(W):
                    my, mx = min(int(math.floor(y * 2 / H)), 1), min(int(math.floor(xx * 2 / W)), 1)
                    v = x0[b, ch, y, xx]
                    if mask[b, my, mx]:
                        v = sum(w[dy + 4] * w[dx + 4] * x0[b, ch, _reflect(y + dy, H), _reflect(xx + dx, W)]
                                for dy in range(-4, 5) for dx in range(-4, 5))
                    want[b, ch, y, xx] = c[2] * v + c[3] * eps[b, ch, y, xx].double()
    assert float((got.double() - want).abs().max()) <= 1e-5
    assert abs(float(gaussian_taps().sum()) - 1.0) <= 1e-6 and float(gaussian_taps()[4]) == pytest.approx(0.39894, abs=2e-4)


def test_denoise_sag_refuses_guidance_rescale():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.sag import denoise_sag
    with pytest.raises(PeaError, match="guidance_rescale"):
        denoise_sag(None, None, None, torch.zeros(1, 4, 8, 8), None, None, guidance_rescale=0.7)
