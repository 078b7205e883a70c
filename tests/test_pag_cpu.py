"""Perturbed-attention / smoothed-energy guidance without a GPU: `pag.blur_matrix` applied as Mh X Mw^T against
`F.pad(mode="reflect")` + `F.conv2d` (tests/pag_ref.py), `pag.perturbed_scale` against its closed forms, the restatement's own
combine against a double loop, the null-operand and shape refusals of the C ABI, and the argument refusals of
`pag.denoise_perturbed` that need no device.

Tolerance of the blur: the tables are fp32 roundings of a float64 construction, so a blurred value deviates by at most
2^-24 sum |M| |x| per pass; against float64 data of magnitude up to 5 that is below 1e-6 absolute, and rtol 1e-5 is the rule
for everything larger."""
import ctypes

import numpy as np
import pytest
import torch

from pag_ref import blur_ref, combine_ref

GRIDS = [(4, 4), (8, 8), (7, 13), (32, 32)]


def _grid_data(h, w, C=3):
    g = torch.Generator().manual_seed(100 * h + w)
    return torch.randn(2, h * w, C, generator=g, dtype=torch.float64)


def _apply(Mh, Mw, x, h, w):
    n, S, C = x.shape
    g = x.reshape(n, h, w, C)
    return torch.einsum("ij,njkc,lk->nilc", Mh, g, Mw).reshape(n, S, C)


@pytest.mark.parametrize("sigma", [0.5, 2.0, 10.0])
@pytest.mark.parametrize("hw", GRIDS)
def test_blur_matrix_is_reflect_pad_and_conv(hw, sigma):
    from pea_diffusion_amd.pag import blur_kernel_size, blur_matrix
    h, w = hw
    Mh, Mw = blur_matrix(h, sigma), blur_matrix(w, sigma)
    assert Mh.dtype == np.float32 and Mh.shape == (h, h) and Mw.shape == (w, w)
    for M in (Mh, Mw):
        assert np.abs(M.astype(np.float64).sum(1) - 1.0).max() <= 1e-6 and (M >= 0).all()
    assert blur_kernel_size(h, sigma) % 2 == 1 and blur_kernel_size(h, sigma) // 2 <= max(h - 1, 0)
    x = _grid_data(h, w)
    got = _apply(torch.from_numpy(Mh).double(), torch.from_numpy(Mw).double(), x, h, w)
    torch.testing.assert_close(got, blur_ref(x, h, w, sigma), rtol=1e-5, atol=1e-6)
    if sigma == 0.5 and h > 4:
        assert not torch.allclose(got, x, atol=1e-3)                 # three taps already move the data


@pytest.mark.parametrize("hw", GRIDS + [(1, 1)])
def test_blur_matrix_infinite_sigma_is_the_mean(hw):
    from pea_diffusion_amd.pag import blur_matrix
    h, w = hw
    for sigma in (float("inf"), 1.0e4):
        Mh, Mw = blur_matrix(h, sigma), blur_matrix(w, sigma)
        assert np.array_equal(Mh, np.full((h, h), np.float32(1.0 / h))) and np.array_equal(Mw, np.full((w, w), np.float32(1.0 / w)))
        x = _grid_data(h, w)
        got = _apply(torch.from_numpy(Mh).double(), torch.from_numpy(Mw).double(), x, h, w)
        want = x.mean(1, keepdim=True).expand_as(x)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(blur_ref(x, h, w, sigma), want, rtol=1e-12, atol=1e-12)


def test_blur_matrix_sizes_and_refusals():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.pag import blur_kernel_size, blur_matrix
    assert blur_kernel_size(64, 0.5) == 3 and blur_kernel_size(64, 2.0) == 13 and blur_kernel_size(64, 10.0) == 61
    assert blur_kernel_size(32, 10.0) == 33 and blur_kernel_size(7, 10.0) == 7 and blur_kernel_size(1, 2.0) == 1     # the clamp
    assert np.array_equal(blur_matrix(1, 2.0), np.ones((1, 1), np.float32))
    # an even axis takes m + 1 taps: position 0 sees the far edge once, through the reflection, and nothing twice over
    M = blur_matrix(4, 10.0).astype(np.float64)
    taps = np.exp(-0.5 * (np.arange(-2, 3) / 10.0) ** 2)
    taps /= taps.sum()
    assert np.allclose(M[0], [taps[2], taps[1] + taps[3], taps[0] + taps[4], 0.0], atol=1e-7)
    for m, sigma in ((0, 1.0), (4, 0.0), (4, -1.0), (4, float("nan"))):
        with pytest.raises(PeaError):
            blur_matrix(m, sigma)


def test_perturbed_scale_closed_forms():
    from pea_diffusion_amd.pag import perturbed_scale
    assert perturbed_scale(3.0, 0.0, 981) == 3.0 and perturbed_scale(3.0, 0.0, 1) == 3.0
    assert perturbed_scale(3.0, 0.005, 1000) == 3.0
    assert perturbed_scale(3.0, 0.005, 800) == pytest.approx(2.0, rel=1e-12)
    assert perturbed_scale(3.0, 0.005, torch.tensor(400)) == 0.0     # 3 - 3: the clip's edge
    assert perturbed_scale(3.0, 0.005, 1) == 0.0                      # clipped at 0, never negative
    assert perturbed_scale(0.0, 0.1, 500) == 0.0


def test_combine_ref_against_a_double_loop():
    g = torch.Generator().manual_seed(7)
    B, per = 2, 12
    e3 = torch.randn(3 * B, 3, 4, generator=g, dtype=torch.float64)
    gs, s, phi = 5.0, 3.0, 0.7
    for rescale in (0.0, phi):
        got = combine_ref(e3, gs, s, rescale)
        for b in range(B):
            u, t, p = e3[b].reshape(-1), e3[B + b].reshape(-1), e3[2 * B + b].reshape(-1)
            c = [float(u[i] + gs * (t[i] - u[i]) + s * (t[i] - p[i])) for i in range(per)]
            if rescale > 0.0:
                std = lambda v: (sum((a - sum(v) / per) ** 2 for a in v) / (per - 1)) ** 0.5
                f = phi * std([float(a) for a in t]) / std(c) + 1.0 - phi
                c = [a * f for a in c]
            assert torch.allclose(got[b].reshape(-1), torch.tensor(c, dtype=torch.float64), rtol=1e-12, atol=1e-12)
    e2 = e3[:2 * B]
    got = combine_ref(e2, 0.0, s, 0.0, do_cfg=False)
    assert torch.allclose(got, e2[:B] + s * (e2[:B] - e2[B:]), rtol=1e-12, atol=0)
    assert torch.equal(combine_ref(e3, gs, 0.0), e3[:B] + gs * (e3[B:2 * B] - e3[:B]))      # s = 0: plain CFG


def test_null_operands_and_shapes_are_refused_through_the_c_abi():
    from pea_diffusion_amd._lib import lib
    L = lib()
    page = (ctypes.c_float * 64)()
    p = ctypes.cast(page, ctypes.c_void_p)
    ok = dict(Q=p, Mh=p, Mw=p)
    for missing in ok:
        a = dict(ok, **{missing: None})
        rc = L.pea_op_query_blur(a["Q"], 192, 0, 1, 4, 4, 64, a["Mh"], a["Mw"], None)
        assert rc == -3 and b"null operand" in L.pea_last_error(), (missing, L.pea_last_error())
    for kw, msg in ((dict(C=72), b"whole heads"), (dict(C=32), b"whole heads"), (dict(h=65), b"LDS"), (dict(w=128), b"LDS"),
                    (dict(ld=100), b"pitch"), (dict(col0=4), b"offset"), (dict(col0=192), b"offset"), (dict(n=0), b"samples"),
                    (dict(n=65536), b"samples")):
        a = dict(ld=192, col0=0, n=1, h=4, w=4, C=64)
        a.update(kw)
        rc = L.pea_op_query_blur(p, a["ld"], a["col0"], a["n"], a["h"], a["w"], a["C"], p, p, None)
        assert rc == -3 and msg in L.pea_last_error(), (kw, L.pea_last_error())
    assert b"64 x 64" in (L.pea_op_query_blur(p, 192, 0, 1, 65, 64, 64, p, p, None), L.pea_last_error())[1]     # the limit is named
    assert L.pea_op_query_blur_lds_bytes(64, 64) == 64 * (64 * 8 + 8) * 4 <= 160 * 1024
    assert L.pea_op_query_blur_lds_bytes(32, 32) == 32 * (32 * 8 + 8) * 4
    assert L.pea_op_query_blur_lds_bytes(65, 4) == -3 and L.pea_op_query_blur_lds_bytes(0, 4) == -3
    for a in ((None, p), (p, None)):
        rc = L.pea_op_attn_identity(a[0], 64, 0, a[1], 64, 4, 64, None)
        assert rc == -3 and b"null operand" in L.pea_last_error()
    for args in ((p, 64, 0, p, 64, 0, 64), (p, 64, 0, p, 64, 4, 60), (p, 64, 8, p, 64, 4, 64), (p, 64, 0, p, 32, 4, 64)):
        assert L.pea_op_attn_identity(*args, None) == -3 and b"attn_identity" in L.pea_last_error()
    for a in ((None, p), (p, None)):
        rc = L.pea_op_cfg_pag_combine(a[0], a[1], 1, 64, 1, 5.0, 3.0, 0.0, None, None)
        assert rc == -3 and b"null operand" in L.pea_last_error()
    assert L.pea_op_cfg_pag_combine(p, p, 0, 64, 1, 5.0, 3.0, 0.0, None, None) == -3
    rc = L.pea_op_cfg_pag_combine(p, p, 1, 16, 1, 5.0, 3.0, 0.7, None, None)
    assert rc == -3 and b"workspace" in L.pea_last_error()           # a rescale without its workspace
    assert L.pea_unet_set_attn_perturb(None, 1, 1, None, 0, 0, None, None, None, None) == -1
    assert L.pea_unet_clear_attn_perturb(None) == -1


def test_denoise_perturbed_argument_refusals():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.pag import denoise_perturbed

    class Ctx:
        B = 4
    lat, emb = torch.zeros(1, 4, 8, 8), torch.zeros(2, 77, 64)
    with pytest.raises(PeaError, match="mode"):
        denoise_perturbed(Ctx(), None, lat, emb, None, mode="blur")
    with pytest.raises(PeaError, match="scale"):
        denoise_perturbed(Ctx(), None, lat, emb, None, scale=-1.0)
    with pytest.raises(PeaError, match="blur_sigma"):
        denoise_perturbed(Ctx(), None, lat, emb, None, mode="seg", blur_sigma=0.0)
    with pytest.raises(PeaError, match="UNet of batch 3"):
        denoise_perturbed(Ctx(), None, lat, emb, None)                # CFG: [uncond | cond | perturbed]
    with pytest.raises(PeaError, match="UNet of batch 2"):
        denoise_perturbed(Ctx(), None, lat, emb, None, guidance_scale=1.0)
    Ctx.B = 3
    with pytest.raises(PeaError, match="prompt_embeds of batch 3"):
        denoise_perturbed(Ctx(), None, lat, torch.zeros(3, 77, 64), None)
