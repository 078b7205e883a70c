"""StyleAligned generation, the host side (no GPU): the folded arithmetic the kernel computes against the explicit restatement,
the reference / layer bookkeeping, and what pea_op_attention_fwd_shared launches or refuses (pea_debug_attn_shared_dispatch)."""
import ctypes

import pytest
import torch

from style_aligned_ref import adain_coef, shared_folded, shared_reference

F64 = torch.float64


# ---------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("B,H,S,ref", [(2, 2, 16, (-1, 0)), (3, 1, 70, (-1, 0, 0)), (4, 2, 33, (-1, 0, -1, 2)), (2, 1, 2, (-1, 0))])
@pytest.mark.parametrize("aq,ak", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("ss,sh", [(1.0, 0.0), (0.5, 1.5)])
def test_folded_form_equals_the_restatement(B, H, S, ref, aq, ak, ss, sh):
    """float64: AdaIN'd Q and K with concatenated K and V  ==  (q' o a_k) . k + q' . s_k, two segments, one softmax"""
    g = torch.Generator().manual_seed(B * 100 + S)
    C = 64 * H
    q, k, v = (torch.randn(B, S, C, generator=g, dtype=F64) * (0.5 + 1.5 * torch.rand(B, 1, C, generator=g, dtype=F64))
               + 0.6 * (torch.rand(B, 1, C, generator=g, dtype=F64) - 0.5) for _ in range(3))
    O, mag, coef = shared_reference(q, k, v, H, ref, adain_queries=aq, adain_keys=ak, share_scale=ss, share_shift=sh)
    F = shared_folded(q, k, v, H, ref, coef, share_scale=ss, share_shift=sh)
    assert (O - F).abs().max().item() < 1e-12
    assert (mag >= O.abs() - 1e-12).all()
    for b, r in enumerate(ref):
        if r < 0:                                                    # a plain sample is plain attention
            s = (q[b].view(S, H, 64).transpose(0, 1) @ k[b].view(S, H, 64).transpose(0, 1).transpose(-1, -2)) * 0.125
            o = (torch.softmax(s, -1) @ v[b].view(S, H, 64).transpose(0, 1)).transpose(0, 1).reshape(S, C)
            assert (O[b] - o).abs().max().item() < 1e-12
            assert coef[b].tolist() == adain_coef(q, k, [-1] * B)[b].tolist()
        else:                                                        # AdaIN: the target's statistics become the reference's
            for i, on in ((0, aq), (2, ak)):
                x = q if i == 0 else k
                if on:
                    y = coef[b, i] * x[b] + coef[b, i + 1]
                    assert (y.mean(0) - x[r].mean(0)).abs().max().item() < 1e-10
                    assert ((y.var(0) + 1e-5 * coef[b, i] ** 2).sqrt() - (x[r].var(0) + 1e-5).sqrt()).abs().max().item() < 1e-10
                else:
                    assert coef[b, i].eq(1).all() and coef[b, i + 1].eq(0).all()


def test_prescaled_q_needs_the_scaled_epsilon():
    """the statistics of q * c are those of q scaled by c: with eps c^2 the coefficients give the same q' * c, with eps alone not"""
    g = torch.Generator().manual_seed(3)
    c = 0.125 * 1.4426950408889634
    q, k = 0.02 * torch.randn(2, 40, 64, generator=g, dtype=F64), torch.randn(2, 40, 64, generator=g, dtype=F64)
    q[1] *= 3.0
    plain = adain_coef(q, k, (-1, 0))
    pre = adain_coef(q * c, k, (-1, 0), eps_q=1e-5 * c * c)
    wrong = adain_coef(q * c, k, (-1, 0))
    assert (pre[1, 0] - plain[1, 0]).abs().max().item() < 1e-12 and (pre[1, 1] - c * plain[1, 1]).abs().max().item() < 1e-12
    assert (wrong[1, 0] - plain[1, 0]).abs().max().item() > 1e-3


# ---------------------------------------------------------------------------------------------- bookkeeping
def test_reference_index():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.style_aligned import reference_index
    assert reference_index(1) == [-1] and reference_index(3) == [-1, 0, 0]
    assert reference_index(2, do_cfg=True) == [-1, 0, -1, 2] and reference_index(3, True) == [-1, 0, 0, -1, 3, 3]
    with pytest.raises(PeaError):
        reference_index(0)


def test_level_switches():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.style_aligned import level_switches
    assert level_switches(6, 0.0) == [False] * 6 and level_switches(6, 1.0) == [True] * 6
    assert level_switches(6, 0.5) == [True, False] * 3                          # int(0.5 * 6) = 3 -> every 2nd
    assert level_switches(8, 0.25) == [True, False, False, False] * 2
    assert level_switches(8, 0.75) == [False, True, True, True] * 2             # the complement of 0.25
    assert level_switches(70, 0.75) == [not v for v in level_switches(70, 0.25)]
    assert level_switches(4, 0.1) == [False] * 4 and level_switches(4, 0.9) == [True] * 4
    for bad in (-0.1, 1.5):
        with pytest.raises(PeaError):
            level_switches(4, bad)


def test_layer_names_and_selection():
    """the SDXL layout: 70 self-attention layers in the order a forward runs them; names, prefixes and fractions select"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import style_aligned as sa
    from pea_diffusion_amd._lib import PeaError
    names = sa.layer_names_of(pc.sdxl_config())
    assert len(names) == 70 and len(set(names)) == 70 and all(n.endswith(".attn1") for n in names)
    assert names[0] == "down_blocks.1.attentions.0.transformer_blocks.0.attn1"
    assert names[4] == "down_blocks.2.attentions.0.transformer_blocks.0.attn1"
    assert names[24] == "mid_block.attentions.0.transformer_blocks.0.attn1"     # down (4 + 20), then mid (10), then up (30 + 6)
    assert names[34] == "up_blocks.0.attentions.0.transformer_blocks.0.attn1" and names[-1].startswith("up_blocks.1.attentions.2.")
    tiny = sa.layer_names_of(pc.tiny_config())

    class U:                                                         # resolve_layers asks the context for its count only
        cfg, _h = pc.tiny_config(), None
    real = sa.layer_names
    sa.layer_names = lambda u: sa.layer_names_of(u.cfg)
    try:
        assert sa.resolve_layers(U, None) == [1.0] * len(tiny) and sa.resolve_layers(U, 1.0) == [1.0] * len(tiny)
        assert sa.resolve_layers(U, 0.0) == [0.0] * len(tiny)
        assert sa.resolve_layers(U, [tiny[0]]) == [1.0] + [0.0] * (len(tiny) - 1)
        up = sa.resolve_layers(U, ["up"])
        assert up == [1.0 if n.startswith("up_blocks.") else 0.0 for n in tiny] and 0 < sum(up) < len(tiny)
        both = sa.resolve_layers(U, {"up": True, tiny[-1]: False})
        assert both[-1] == 0.0 and sum(both) == sum(up) - 1
        with pytest.raises(PeaError, match="names no self-attention layer"):
            sa.resolve_layers(U, ["up_blocks.7"])
    finally:
        sa.layer_names = real


# ---------------------------------------------------------------------------------------------- the launcher, without a device
def _dispatch(B=2, H=2, Sq=128, Skv=None, nd=1, ldk=0, null_coef=False, ref=None):
    from pea_diffusion_amd._lib import lib
    ref = ([-1] + [0] * (B - 1) if ref is None else list(ref))[:32]
    q = (ctypes.c_int * 40)(B, H, Sq, Sq if Skv is None else Skv, nd, ldk, int(null_coef), *(ref + [-1] * (32 - len(ref))))
    out = (ctypes.c_int * 8)()
    rc = lib().pea_debug_attn_shared_dispatch(q, out)
    return rc, list(out), lib().pea_last_error().decode()


def test_shared_dispatch_lds_and_grid():
    for (B, H, S), ref in (((2, 2, 16), (-1, 0)), ((4, 2, 260), (-1, 0, -1, 2)), ((4, 10, 4096), (-1, 0, -1, 2)),
                           ((4, 20, 1024), (-1, 0, -1, 2)), ((3, 2, 364), (-1, 0, 0)), ((4, 2, 130), (-1, -1, -1, 2))):
        rc, (gx, gy, gz, lds, n_tw, n_pw, plain_first, n_t), msg = _dispatch(B, H, S, ref=ref)
        assert rc == 0, msg
        nu, nt = (S + 127) // 128, sum(r >= 0 for r in ref)
        assert (gy, gz) == (1, 1) and lds == 2 * 2 * 8192 == 32768   # the forward's ring: 2 stages x (K tile + V tile)
        assert n_t == nt and n_tw == nt * H * nu and n_pw == (B - nt) * H * nu and gx == n_tw + n_pw and plain_first == 0
    assert _dispatch(4, 10, 4096, ref=(-1, 0, -1, 2))[1][0] == 4 * 10 * 32 and _dispatch(4, 20, 1024, ref=(-1, 0, -1, 2))[1][0] == 4 * 20 * 8
    # 128 tokens: pea_op_attention_fwd is the resident-key kernel there; it runs first and the grid holds the targets only
    rc, out, msg = _dispatch(2, 2, 128)
    assert rc == 0 and out[6] == 1 and out[0] == out[4] == 2 and out[5] == 0, msg
    # nobody is a target: the plain launch is all there is (no target workgroups), coef may be absent
    rc, out, msg = _dispatch(2, 2, 200, ref=(-1, -1), null_coef=True)
    assert rc == 0 and out[4] == 0 and out[7] == 0, msg


def test_shared_dispatch_refusals():
    assert _dispatch()[0] == 0
    cases = (("S >= 2", dict(Sq=1)), ("Sq == Skv", dict(Sq=128, Skv=77)), ("head_dim 64", dict(nd=2)), ("at most 32 samples", dict(B=33)),
             ("out of range", dict(ref=[-1, 2])), ("itself a target", dict(B=3, ref=[-1, 0, 1])), ("leading dimension", dict(ldk=132)),
             ("null coef", dict(null_coef=True)), ("empty problem", dict(Sq=0)), ("empty problem", dict(B=0)), ("empty problem", dict(H=0)))
    for cause, kw in cases:
        rc, _, msg = _dispatch(**kw)
        assert rc == -3 and "attention_shared" in msg and cause in msg, (cause, kw, rc, msg)      # PEA_E_SHAPE, the cause named
    # a sample that names itself is its own reference, that is, plain: [-1, -1, 2, 2] needs no coefficients for sample 2 ...
    rc, out, _ = _dispatch(B=4, ref=[-1, -1, 2, 2])
    assert rc == 0 and out[7] == 1
    assert _dispatch(ref=[-1, 1], null_coef=True)[0] == 0
    # ... S = 1 is fine while nobody is a target, and so is a wider K
    assert _dispatch(Sq=1, ref=[-1, -1], null_coef=True)[0] == 0 and _dispatch(ldk=136)[0] == 0


def test_style_entry_points_without_a_device():
    from pea_diffusion_amd import _lib
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("pea_op_attn_adain_coef", "pea_op_attn_adain_scratch_bytes", "pea_op_attention_fwd_shared", "pea_unet_set_style_aligned",
                 "pea_unet_clear_style_aligned", "pea_unet_num_self_attention_layers", "pea_debug_attn_shared_dispatch"):
        assert name in protos and hasattr(L, name)
    assert len(protos["pea_op_attention_fwd_shared"][1]) == 20 and len(protos["pea_unet_set_style_aligned"][1]) == 9
    assert len(protos["pea_op_attn_adain_coef"][1]) == 15
    fake = ctypes.c_void_p(4096)                                     # never followed: refused first
    ref = (ctypes.c_int * 2)(-1, 0)
    call = lambda B=2, S=128, Skv=128, r=ref, coef=fake, ldk=128: L.pea_op_attention_fwd_shared(
        fake, 128, fake, ldk, fake, 128, fake, 128, B, 2, S, Skv, r, coef, 0.125, 0, 1.0, 0.0, 1, None)
    assert call(Skv=77) == -3 and b"Sq == Skv" in L.pea_last_error()
    assert call(coef=None) == -3 and b"null coef" in L.pea_last_error()
    assert call(r=(ctypes.c_int * 2)(-1, 5)) == -3 and b"out of range" in L.pea_last_error()
    assert call(S=1, Skv=1) == -3 and b"S >= 2" in L.pea_last_error()
    assert call(ldk=132) == -3 and call(r=None) == -1 and b"null ref" in L.pea_last_error()
    coef = lambda B=2, S=128, r=ref, ldq=128, scratch=fake: L.pea_op_attn_adain_coef(fake, ldq, fake, 128, B, 2, S, r, 0.125, 0, 1, 1, fake,
                                                                                    scratch, None)
    assert coef(r=None) == -1 and b"null ref" in L.pea_last_error()
    assert coef(S=1) == -3 and b"two tokens" in L.pea_last_error()
    assert coef(B=33) == -3 and b"at most 32 samples" in L.pea_last_error()
    assert coef(ldq=132) == -3 and b"leading dimension" in L.pea_last_error()
    assert coef(r=(ctypes.c_int * 2)(1, 0)) == -3 and b"itself a target" in L.pea_last_error()
    assert coef(scratch=None) == -3 and b"null operand" in L.pea_last_error()
    assert coef(r=(ctypes.c_int * 2)(-1, -1), scratch=None) == 0     # no target: nothing to do, nothing launched
    # the partials of the split reduction: [B][2][slabs][2][64 H] floats, slabs of at least 64 rows
    assert L.pea_op_attn_adain_scratch_bytes(2, 2, 16) == 4 * 2 * 2 * 1 * 2 * 128
    assert L.pea_op_attn_adain_scratch_bytes(4, 10, 4096) % (4 * 4 * 2 * 2 * 640) == 0 and L.pea_op_attn_adain_scratch_bytes(33, 2, 16) == 0
    assert L.pea_unet_set_style_aligned(None, ref, None, 0, 1, 1, 1.0, 0.0, None) == -1 and b"pea_unet_set_style_aligned" in L.pea_last_error()
    assert L.pea_unet_clear_style_aligned(None) == -1 and b"pea_unet_clear_style_aligned" in L.pea_last_error()
    assert L.pea_unet_num_self_attention_layers(None) == -1
