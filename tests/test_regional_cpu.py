"""Regional text prompts, the host side (no GPU): the weights of a layer grid against their restatement, the composed context,
and what pea_op_attention_fwd_regions launches or refuses (pea_debug_attn_regions_dispatch), without a device."""
import ctypes

import pytest
import torch

from regional_ref import half_masks, quadrant_masks, region_weights_ref


def _levels(h, w, n=3):
    out = [(h, w)]
    for _ in range(n - 1):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def _soft_masks(h, w, R, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(h, w, generator=g) for _ in range(R)]


@pytest.mark.parametrize("latent", [(16, 16), (13, 20)])            # 16 -> 8 -> 4 divides the mask; 13 x 20 -> 7 x 10 -> 4 x 5 does not
def test_region_weights_equal_the_restatement(latent):
    from pea_diffusion_amd.regional import region_weights
    h, w = 8 * latent[0], 8 * latent[1]
    cases = [(half_masks(h, w), None), (quadrant_masks(h, w), [1.0, 0.5, 2.0, 1.0]), (_soft_masks(h, w, 3, 1), [1.0, 2.0, 0.25]),
             ([None, _soft_masks(h, w, 1, 2)[0]], None),
             ([torch.stack(_soft_masks(h, w, 2, 3)), half_masks(h, w)[0][None]], [0.7, 1.3]),           # [2, h, w] beside [1, h, w]
             (_soft_masks(37, 51, 2, 4), None)]                                                         # a mask at an odd resolution
    for masks, weights in cases:
        for h_l, w_l in _levels(*latent):
            got, want = region_weights(masks, weights, h_l, w_l), region_weights_ref(masks, weights, h_l, w_l)
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (want.shape[0], len(masks), h_l * w_l)
            # both are fp32 roundings of the same rational numbers in [0, 1]: a few ulps of 1
            assert torch.allclose(got, want, rtol=0, atol=4 * 2.0 ** -23), (h_l, w_l, (got - want).abs().max())
            assert (got >= 0).all() and (got <= 1).all()


@pytest.mark.parametrize("latent", [(16, 16), (13, 20)])
def test_partition_stays_a_partition_at_every_level(latent):
    from pea_diffusion_amd.regional import region_weights
    h, w = 8 * latent[0], 8 * latent[1]
    for masks in (half_masks(h, w), quadrant_masks(h, w)):
        assert torch.equal(sum(masks), torch.ones(h, w))
        for h_l, w_l in _levels(*latent):
            got = region_weights(masks, None, h_l, w_l)
            assert (got.sum(1) - 1.0).abs().max() <= 1e-6
            # no weights: the area means themselves, which already sum to 1
            assert torch.allclose(got, region_weights_ref(masks, None, h_l, w_l), rtol=0, atol=4 * 2.0 ** -23)
    # cells inside one half are one-hot at the top level (what lets a wave skip the other region)
    top = region_weights(half_masks(h, w), None, *latent).view(2, *latent)
    assert torch.equal(top[0, :, : latent[1] // 2], torch.ones(latent[0], latent[1] // 2)) and top[1, :, : latent[1] // 2].abs().max() == 0


def test_uncovered_positions_go_to_region_zero():
    from pea_diffusion_amd.regional import region_weights
    m0, m1 = torch.zeros(32, 32), torch.zeros(32, 32)
    m0[:8] = 1.0
    m1[8:16] = 1.0                                                   # rows 16.. belong to nobody
    got = region_weights([m0, m1], None, 4, 4).view(2, 4, 4)
    assert torch.equal(got[0], torch.tensor([1.0, 0.0, 1.0, 1.0])[:, None].expand(4, 4))
    assert torch.equal(got[1], torch.tensor([0.0, 1.0, 0.0, 0.0])[:, None].expand(4, 4))
    assert torch.equal(got, region_weights_ref([m0, m1], None, 4, 4).view(2, 4, 4))
    # a weight of 0 uncovers a region's cells as well
    got = region_weights([m0, m1], [1.0, 0.0], 4, 4).view(2, 4, 4)
    assert torch.equal(got[0], torch.ones(4, 4)) and got[1].abs().max() == 0


def test_region_weights_refusals():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.regional import region_weights
    neg = torch.ones(8, 8)
    neg[3, 3] = -0.1
    with pytest.raises(PeaError, match="negative"):
        region_weights([None, neg], None, 4, 4)
    with pytest.raises(PeaError):
        region_weights([None, torch.full((8, 8), float("nan"))], None, 4, 4)
    with pytest.raises(PeaError):
        region_weights([None, None], [1.0], 4, 4)
    with pytest.raises(PeaError):
        region_weights([None, None], [1.0, -1.0], 4, 4)
    with pytest.raises(PeaError):
        region_weights([], None, 4, 4)
    with pytest.raises(PeaError):
        region_weights([torch.ones(2, 8, 8), torch.ones(3, 8, 8)], None, 4, 4)


def test_compose_prompt_embeds():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.regional import compose_prompt_embeds
    g = torch.Generator().manual_seed(0)
    e = [torch.randn(2, 77, 32, generator=g) for _ in range(3)]
    neg = torch.randn(2, 77, 32, generator=g)
    cond = compose_prompt_embeds(e)
    assert tuple(cond.shape) == (2, 231, 32)
    for r in range(3):
        assert torch.equal(cond[:, 77 * r:77 * (r + 1)], e[r])
    both = compose_prompt_embeds(e, neg)
    assert tuple(both.shape) == (4, 231, 32) and torch.equal(both[2:], cond)
    for r in range(3):
        assert torch.equal(both[:2, 77 * r:77 * (r + 1)], neg)      # the unconditional half: the negative prompt tiled
    with pytest.raises(PeaError):
        compose_prompt_embeds([e[0], e[1][:, :76]])
    with pytest.raises(PeaError):
        compose_prompt_embeds(e, neg[:1])
    with pytest.raises(PeaError):
        compose_prompt_embeds([])


# ---------------------------------------------------------------------------------------------- the launcher, without a device
def _dispatch(B, H, Sq, R, Lr, nd=1, ldk=0, Bw=0):
    from pea_diffusion_amd._lib import lib
    q = (ctypes.c_int * 8)(B, H, Sq, R, Lr, nd, ldk, Bw)
    out = (ctypes.c_int * 6)()
    rc = lib().pea_debug_attn_regions_dispatch(q, out)
    return rc, list(out), lib().pea_last_error().decode()


def test_regions_dispatch_lds_and_grid():
    for R in (1, 2, 3, 4):
        for KB, Lr in ((1, 1), (1, 32), (2, 33), (2, 64), (3, 65), (3, 77), (3, 96)):
            for Sq in (1, 127, 128, 129, 1024, 4096):
                for BH in (2, 20, 80):
                    rc, (kb, gx, gy, gz, lds, upw), msg = _dispatch(2, BH // 2, Sq, R, Lr)
                    assert rc == 0, msg
                    assert kb == KB and (gy, gz) == (BH // 2, 2)
                    # the trimmed form: the O images are 4 096 bytes per wave (128-byte pitch, swizzled), not 4 608
                    assert lds == R * KB * 2 * 4096 + 4 * 4096 + 4 * 4096 and lds <= 163840
                    assert upw >= 1 and gx >= 1 and gx * upw * 128 >= Sq
                    assert (gx - 1) * upw * 128 < Sq                 # no workgroup without a unit
    # the two figures the header quotes
    assert _dispatch(2, 10, 4096, 2, 77)[1][4] == 81920 and _dispatch(2, 10, 4096, 4, 96)[1][4] == 131072
    # units per workgroup: one round of the workgroups the LDS lets the 256 CUs hold -- two each up to 80 KiB, one above
    assert _dispatch(2, 10, 4096, 2, 77)[1][5] == 2                  # 640 units over 512 workgroups (81 920 bytes: two per CU)
    assert _dispatch(2, 10, 4096, 3, 77)[1][5] == 3                  # ... over 256
    assert _dispatch(2, 20, 1024, 2, 77)[1][5] == 1 and _dispatch(2, 20, 1024, 4, 77)[1][5] == 2


def test_regions_dispatch_refusals():
    ok = dict(B=2, H=2, Sq=128, R=2, Lr=77)
    assert _dispatch(**ok)[0] == 0
    for what, kw in (("R = 0", dict(R=0)), ("R = 5", dict(R=5)), ("Lr = 97", dict(Lr=97)), ("Lr = 0", dict(Lr=0)), ("nd = 2", dict(nd=2)),
                     ("ldk = 132", dict(ldk=132)), ("ldk = 64", dict(ldk=64)), ("Bw = 3", dict(Bw=3)), ("Sq = 0", dict(Sq=0))):
        rc, _, msg = _dispatch(**{**ok, **kw})
        assert rc == -3 and "attention_regions" in msg, (what, rc, msg)          # PEA_E_SHAPE
    assert _dispatch(**{**ok, "Bw": 2})[0] == 0 and _dispatch(**{**ok, "ldk": 136})[0] == 0


def test_regions_entry_points_without_a_device():
    from pea_diffusion_amd import _lib
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("pea_op_attention_fwd_regions", "pea_unet_set_prompt_regions", "pea_unet_clear_prompt_regions",
                 "pea_debug_attn_regions_dispatch"):
        assert name in protos and hasattr(L, name)
    assert len(protos["pea_op_attention_fwd_regions"][1]) == 18
    fake = ctypes.c_void_p(4096)                                     # never followed: refused first
    assert L.pea_op_attention_fwd_regions(fake, 128, fake, 128, fake, 128, fake, 128, 1, 2, 128, 5, 77, fake, 1, 0.125, 0, None) == -3
    assert b"1..4 regions" in L.pea_last_error()
    assert L.pea_op_attention_fwd_regions(fake, 128, fake, 128, fake, 128, fake, 128, 1, 2, 128, 2, 77, None, 1, 0.125, 0, None) == -3
    assert L.pea_unet_set_prompt_regions(None, 2, 64, None, 1, None) == -1 and b"pea_unet_set_prompt_regions" in L.pea_last_error()
    assert L.pea_unet_clear_prompt_regions(None) == -1
