"""Cross-attention heat maps without a GPU: `attention_maps.combine` / `heat_maps` against the restatement of
tests/attn_maps_ref.py, the launcher's grid and LDS rule and its refusals through pea_debug_attn_maps_dispatch, and the entry
points of the C ABI.

Why the 1024-query SDXL level has fewer workgroups than the chip has CUs: the sum over heads has to stay inside one workgroup
(no atomics, a fixed order), and a workgroup's queries are one 32-wide MFMA column block, so a launch has B x ceil(Sq / 32)
workgroups whatever H is -- 256 at B = 2 x 4096 queries, 64 at B = 2 x 1024 queries, where each workgroup's eight waves run two
or three heads each.  Sharing the heads of one query block out over several workgroups would need a second pass (or atomics) to add
their partial sums; sharing out the keys would repeat every score product per workgroup.  The test below pins both figures."""
import ctypes

import pytest
import torch

from attn_maps_ref import combine_ref

SDXL_SHAPES = {(2, 10, 4096, 77): 256, (2, 20, 1024, 77): 64}        # (B, H, Sq, Skv) -> workgroups (see the module docstring)


def _levels(shapes, B=2, L=5, seed=0, signed=False):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for (h, w), n in shapes:
        t = torch.rand(B, L, h, w, generator=g) * n
        if signed:
            t = t - 0.3 * n                                          # negatives before and after the upsampling
        out[(h, w)] = (t, n)
    return out


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("shapes,size", [
    ((((8, 8), 3), ((4, 4), 5)), None),
    ((((8, 8), 3), ((4, 4), 5)), (16, 16)),
    ((((7, 10), 3), ((4, 5), 5)), None),
    ((((4, 4), 5), ((8, 8), 3)), None),                              # the largest grid is not the first level
])
def test_combine_against_the_restatement(shapes, size, clamp):
    from pea_diffusion_amd.attention_maps import combine
    for signed in (False, True):
        lv = _levels(shapes, signed=signed)
        got, want = combine(lv, size=size, clamp=clamp), combine_ref(lv, size=size, clamp=clamp)
        big = size or max((hw for hw, _ in shapes), key=lambda hw: hw[0] * hw[1])
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5, *big)
        torch.testing.assert_close(got, want, rtol=0, atol=1e-6)
        if clamp:
            assert float(got.min()) >= 0.0
    if not clamp:
        assert float(combine(_levels(shapes, signed=True), size=size, clamp=False).min()) < 0.0
    # a list of (tensor, n) pairs is the same as the dict
    lv = _levels(shapes)
    assert torch.equal(combine(list(lv.values()), size=size, clamp=clamp), combine(lv, size=size, clamp=clamp))


def test_combine_keeps_a_constant_map():
    """bicubic taps sum to 1: a probability that is the same everywhere stays that probability at any size, and the division by
    the number of layer-forwards undoes the sum"""
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.attention_maps import combine
    p = 1.0 / 77
    lv = {(8, 8): (torch.full((2, 5, 8, 8), 3 * p), 3), (4, 4): (torch.full((2, 5, 4, 4), 5 * p), 5)}
    for size in (None, (16, 16), (5, 9)):
        got = combine(lv, size=size)
        assert float((got - p).abs().max()) <= 1e-6
    with pytest.raises(PeaError):
        combine({})
    with pytest.raises(PeaError):
        combine({(4, 4): (torch.zeros(1, 2, 4, 4), 0)})              # nothing accumulated
    with pytest.raises(PeaError):
        combine({(4, 4): (torch.zeros(2, 16), 1)})


class _StubUNet:
    def __init__(self, levels):
        self.levels = levels

    def attention_maps(self):
        return self.levels


def test_heat_maps_tokens_and_cfg_half():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.attention_maps import combine, heat_maps
    lv = _levels((((8, 8), 3), ((4, 4), 5)), B=4, L=6, seed=2)
    full = combine(lv)
    stub = _StubUNet(lv)
    assert torch.equal(heat_maps(stub), full)
    assert torch.equal(heat_maps(stub, do_cfg=True), full[2:])
    assert torch.equal(heat_maps(stub, tokens=[4, 1]), full[:, [4, 1]])
    got = heat_maps(stub, size=(16, 16), do_cfg=True, tokens=(0, 5, 5))
    assert tuple(got.shape) == (2, 3, 16, 16) and torch.equal(got, combine(lv, size=(16, 16))[2:][:, [0, 5, 5]])
    with pytest.raises(PeaError):
        heat_maps(_StubUNet(_levels((((4, 4), 1),), B=3)), do_cfg=True)


# ---------------------------------------------------------------------------------------------- the launcher, without a device
def _dispatch(B, H, Sq, Skv, nd=1, ldq=0, ldk=0, flags=0):
    from pea_diffusion_amd._lib import lib
    q = (ctypes.c_int * 8)(B, H, Sq, Skv, nd, ldq, ldk, flags)
    out = (ctypes.c_int * 6)()
    rc = lib().pea_debug_attn_maps_dispatch(q, out)
    return rc, list(out), lib().pea_last_error().decode()


def test_maps_dispatch_lds_and_grid():
    for Skv in (1, 32, 33, 64, 65, 77, 96, 128):
        for Sq in (1, 31, 32, 33, 127, 128, 129, 1024, 4096):
            for H in (1, 2, 3, 10, 20):
                for B in (1, 2):
                    for flags in (0, 7):
                        rc, (kb, gx, gy, gz, lds, upw), msg = _dispatch(B, H, Sq, Skv, flags=flags)
                        assert rc == 0, msg
                        assert kb == (Skv + 31) // 32
                        assert upw >= 1 and gx >= 1 and (gy, gz) == (B, 1)
                        assert gx * upw * 32 >= Sq                   # the grid covers every query
                        assert (gx - 1) * upw * 32 < Sq              # no workgroup without a unit
                        assert lds == 8 * (kb + 1) * 4096 and lds <= 163840
    for (B, H, Sq, Skv), wgs in SDXL_SHAPES.items():
        rc, (kb, gx, gy, gz, lds, upw), msg = _dispatch(B, H, Sq, Skv)
        assert rc == 0 and kb == 3 and gx * gy * gz == wgs and lds == 131072, msg
    assert _dispatch(2, 10, 4096, 77)[1][1] * 2 >= 256               # the 4096-query level fills the 256 CUs; the other: see above


def test_maps_dispatch_refusals():
    ok = dict(B=2, H=2, Sq=128, Skv=77)
    assert _dispatch(**ok)[0] == 0
    for what, kw in (("Skv = 0", dict(Skv=0)), ("Skv = 129", dict(Skv=129)), ("nd = 2", dict(nd=2)), ("H = 0", dict(H=0)),
                     ("Sq = 0", dict(Sq=0)), ("ldq = 132", dict(ldq=132)), ("ldk = 132", dict(ldk=132)), ("ldq = 64", dict(ldq=64)),
                     ("B = 0", dict(B=0))):
        rc, _, msg = _dispatch(**{**ok, **kw})
        assert rc == -3 and "attention_maps" in msg, (what, rc, msg)             # PEA_E_SHAPE
    assert _dispatch(**{**ok, "ldq": 136})[0] == 0 and _dispatch(**{**ok, "ldk": 256})[0] == 0


def test_maps_entry_points_without_a_device():
    import subprocess
    from pea_diffusion_amd import _lib
    L = _lib.lib()
    protos = _lib.parse_header()
    names = ("pea_op_attention_maps", "pea_unet_enable_attention_maps", "pea_unet_reset_attention_maps",
             "pea_unet_disable_attention_maps", "pea_unet_attention_maps", "pea_debug_attn_maps_dispatch")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in names:
        assert name in protos and hasattr(L, name) and f" T {name}\n" in nm, name
    assert len(protos["pea_op_attention_maps"][1]) == 14
    fake = ctypes.c_void_p(4096)                                     # never followed: refused first
    assert L.pea_op_attention_maps(fake, 128, fake, 128, fake, 1, 2, 128, 129, 0.125, 0, None, 0, None) == -3
    assert b"attention_maps: 1..128 keys" in L.pea_last_error()
    assert L.pea_op_attention_maps(fake, 128, fake, 132, fake, 1, 2, 128, 77, 0.125, 0, None, 1, None) == -3
    assert b"multiples of 8" in L.pea_last_error()
    assert L.pea_op_attention_maps(fake, 128, fake, 128, None, 1, 2, 128, 77, 0.125, 0, None, 0, None) == -3
    assert L.pea_unet_enable_attention_maps(None, None, 0) == -1 and b"pea_unet_enable_attention_maps" in L.pea_last_error()
    assert L.pea_unet_reset_attention_maps(None, None) == -1
    assert L.pea_unet_disable_attention_maps(None) == -1
    assert L.pea_unet_attention_maps(None, 64, None, None) == -1 and b"pea_unet_attention_maps" in L.pea_last_error()


def test_python_surface():
    import inspect
    from pea_diffusion_amd import attention_maps, ops
    from pea_diffusion_amd.unet import HipUNet
    sig = inspect.signature(ops.attention_maps)
    assert list(sig.parameters) == ["q", "k", "heads", "scale", "q_prescaled", "kv_len", "out", "accumulate"]
    for name in ("enable_attention_maps", "disable_attention_maps", "reset_attention_maps", "attention_maps"):
        assert callable(getattr(HipUNet, name))
    assert list(inspect.signature(attention_maps.combine).parameters) == ["levels", "size", "clamp"]
    assert list(inspect.signature(attention_maps.heat_maps).parameters) == ["unet", "size", "do_cfg", "tokens"]
