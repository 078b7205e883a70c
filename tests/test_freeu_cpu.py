"""CPU (no device): FreeU's reference filter against literals that do not depend on FFT conventions, the closed form the HIP
kernels evaluate against that reference in float64, the new entry points' host-side refusals, and the tape plans, which the
switch must not move."""
import ctypes as C
import json
import math
import os

import pytest
import torch

from freeu_ref import fourier_filter, fourier_filter_closed, freeu_sums
from pea_diffusion_amd import _lib
from pea_diffusion_amd import config as pc

F64 = torch.float64


def _grid(H, W):
    y = torch.arange(H, dtype=F64)[:, None].expand(H, W)
    x = torch.arange(W, dtype=F64)[None, :].expand(H, W)
    return y, x


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (6, 10), (24, 40)])
@pytest.mark.parametrize("s", [0.2, 0.5, 1.0, 1.7])
def test_reference_filter_literals(H, W, s):
    """a constant map is DC only: s times itself.  cos(2 pi x / W) and sin(2 pi y / H) sit in the two conjugate bins +1 / -1 of
    which the window holds -1 alone, and the real part is taken: (1 + s) / 2 times themselves (at a side of 2 the bin -1 is the
    Nyquist bin, its own conjugate: s times).  A frequency-2 cosine lies outside the window."""
    y, x = _grid(H, W)
    const = torch.full((1, 1, H, W), 1.25, dtype=F64)
    torch.testing.assert_close(fourier_filter(const, 1, s), s * const, rtol=0, atol=1e-13)
    cx = torch.cos(2 * math.pi * x / W)[None, None]
    sy = torch.sin(2 * math.pi * y / H)[None, None]
    torch.testing.assert_close(fourier_filter(cx, 1, s), (s if W == 2 else (1 + s) / 2) * cx, rtol=0, atol=1e-13)
    torch.testing.assert_close(fourier_filter(sy, 1, s), (s if H == 2 else (1 + s) / 2) * sy, rtol=0, atol=1e-13)
    if W >= 5:
        c2 = torch.cos(2 * math.pi * 2 * x / W)[None, None]
        torch.testing.assert_close(fourier_filter(c2, 1, s), c2, rtol=0, atol=1e-13)


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (6, 10), (24, 40)])
def test_closed_form_is_the_reference_filter(H, W):
    """x + (s - 1) / (H W) * (the seven sums against their basis maps) == fftn, fftshift, scale the 2 x 2 block, back, .real; float64:
    both sides carry rounding of a few 1e-16 per term of sums over H W <= 960 values of magnitude <= 5"""
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=F64) * 0.7 + 1.5
    for s in (0.2, 0.5, 1.0, 1.9):
        torch.testing.assert_close(fourier_filter_closed(x, s), fourier_filter(x, 1, s), rtol=0, atol=1e-12)
    coef, _ = freeu_sums(x)
    assert coef.shape == (2, 7, 3)
    torch.testing.assert_close(coef[:, 0], x.sum((2, 3)), rtol=0, atol=1e-11)


def test_entry_points_are_declared():
    protos = _lib.parse_header()
    assert protos["pea_op_freeu_scratch_bytes"][0] is C.c_longlong and len(protos["pea_op_freeu_scratch_bytes"][1]) == 4
    assert protos["pea_op_freeu_coef"][0] is C.c_int and len(protos["pea_op_freeu_coef"][1]) == 8
    assert protos["pea_op_concat2_freeu"][0] is C.c_int and len(protos["pea_op_concat2_freeu"][1]) == 14
    assert protos["pea_unet_set_freeu"][1] == [C.c_void_p] + [C.c_float] * 4 + [C.c_void_p]
    assert protos["pea_unet_clear_freeu"][1] == [C.c_void_p]
    from pea_diffusion_amd import ops
    from pea_diffusion_amd.unet import HipUNet
    assert callable(ops.freeu_concat) and callable(HipUNet.enable_freeu) and callable(HipUNet.disable_freeu)


def test_null_handles_are_refused():
    L = _lib.lib()
    assert L.pea_unet_set_freeu(None, 0.9, 0.2, 1.3, 1.4, None) == -1 and b"pea_unet_set_freeu" in L.pea_last_error()
    assert L.pea_unet_clear_freeu(None) == -1 and b"pea_unet_clear_freeu" in L.pea_last_error()


def test_op_refusals_without_gpu():
    """every argument check of the two launchers answers PEA_E_SHAPE on the host, before any device work (null operands)"""
    L = _lib.lib()
    coef = C.cast((C.c_float * 8)(), C.c_void_p)                    # never read: each call is refused on the host
    cat = lambda C1, C2, H, W, s, b, aH=0, aW=0: L.pea_op_concat2_freeu(None, C1, None, C2, coef, None, 1, H, W, s, b, aH, aW, None)
    assert cat(24, 8, 4, 4, 0.5, 1.2) == -3 and b"C1=24" in L.pea_last_error()          # C1 / 2 = 12 is no multiple of 8
    assert cat(8, 8, 4, 4, 0.5, 1.2) == -3 and b"C1=8" in L.pea_last_error()
    assert cat(16, 12, 4, 4, 0.5, 1.2) == -3 and b"C2=12" in L.pea_last_error()
    assert cat(16, 8, 1, 4, 0.5, 1.2) == -3 and b"1 x 4" in L.pea_last_error()
    assert cat(16, 8, 4, 1, 0.5, 1.2) == -3 and b"4 x 1" in L.pea_last_error()
    for s, b in [(float("nan"), 1.2), (float("inf"), 1.2), (0.0, 1.2), (-0.5, 1.2), (0.5, float("nan")), (0.5, float("inf")),
                 (0.5, 0.0), (0.5, -1.0)]:
        assert cat(16, 8, 4, 4, s, b) == -3 and b"finite and positive" in L.pea_last_error(), (s, b)
    assert cat(16, 8, 4, 4, 0.5, 1.2, 4, 6) == -3 and b"depth-to-space" in L.pea_last_error()
    assert cat(16, 8, 5, 4, 0.5, 1.2, 5, 4) == -3 and b"depth-to-space" in L.pea_last_error()
    assert L.pea_op_concat2_freeu(None, 16, None, 8, None, None, 1, 4, 4, 0.5, 1.2, 0, 0, None) == -3
    assert b"no coefficients" in L.pea_last_error()
    assert L.pea_op_freeu_coef(None, 1, 1, 4, 8, coef, None, None) == -3 and b"1 x 4" in L.pea_last_error()
    assert L.pea_op_freeu_coef(None, 1, 4, 4, 12, coef, None, None) == -3 and b"C2=12" in L.pea_last_error()
    assert L.pea_op_freeu_coef(None, 1, 64, 64, 320, coef, None, None) == -3 and b"scratch" in L.pea_last_error()


def test_reduction_split_follows_the_shape():
    """one slab (no scratch) where a map has too few pixels to share out; the production maps split, into whole rows, and the
    partial buffer is [B][slabs][7][C2] fp32"""
    L = _lib.lib()
    for shape in [(1, 2, 2, 8), (2, 5, 7, 24), (3, 6, 10, 64)]:
        assert L.pea_op_freeu_scratch_bytes(*shape) == 0, shape
    for B, H, W, C2 in [(1, 64, 64, 320), (2, 32, 32, 640), (2, 32, 32, 1280), (2, 64, 64, 640)]:
        nbytes = L.pea_op_freeu_scratch_bytes(B, H, W, C2)
        slabs, rem = divmod(nbytes, 4 * 7 * B * C2)
        assert rem == 0 and 2 <= slabs <= H, (B, H, W, C2, nbytes)
    assert L.pea_op_freeu_scratch_bytes(1, 64, 64, 320) == 4 * 7 * 320 * 64          # one row per slab
    assert L.pea_op_freeu_scratch_bytes(1, 1, 64, 320) == 0                           # (a refused shape has no size)


@pytest.mark.parametrize("name,hw,L", [("tiny_config", 16, 12), ("sdxl_config", 128, 77)])
def test_plans_did_not_move(name, hw, L, golden_dir):
    """tagging the up-path concats uses a free field of their ops: tensors, ops, weights and arenas are what they were"""
    golden = json.load(open(os.path.join(golden_dir, "tape_plans.json")))
    lib = _lib.lib()
    c = pc.to_c(getattr(pc, name)())
    for flags in (0, 1, 2):
        want = golden[f"unet/{name}/{hw}/{L}/flags{flags}"]
        n_ops, n_w = C.c_int(), C.c_int()
        n_par, wb, ab, gb = (C.c_longlong() for _ in range(4))
        _lib.check(lib.pea_unet_plan(C.byref(c), 2, hw, hw, L, flags, C.byref(n_ops), C.byref(n_w), C.byref(n_par), C.byref(wb),
                                     C.byref(ab), C.byref(gb)))
        got = (n_ops.value, n_w.value, n_par.value, wb.value, ab.value, gb.value)
        assert got == tuple(want[k] for k in ("n_ops", "n_weights", "n_params", "weight_bytes", "activation_bytes", "grad_bytes"))
