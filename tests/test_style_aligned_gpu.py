"""-m gpu: StyleAligned generation -- the AdaIN coefficient launch (pea_op_attn_adain_coef) and the shared self-attention
(pea_op_attention_fwd_shared) against the fp32 restatement of tests/style_aligned_ref.py, the exactness properties, and the UNet
runtime (HipUNet.set_style_aligned) against `attach_style` on the oracle.

Tolerance of the coefficients: the project's fp32 rule, rtol 1e-3 / atol 1e-4.
Tolerance of the kernel's O: the rule of tests/test_ip_multi_gpu.py (close_terms) with the softmax's own magnitude -- an element may
be off by 2 x 2^-7 x (mag + rms(O)), mag = P |[V[b]; V[r]]|, rel-L2 below 6e-3, no element outside.  The kernel rounds to bf16: q'
(reference segment), q' o a_k (own segment), P and O; the own segment's constant q' . s_k stays fp32.  A CPU simulation of those
roundings stayed at or below 1.13 of the 1 x bound (0.57 of the rule) at S >= 16; at S = 2 the variance over two tokens is
ill-conditioned (9.3 x the 1 x bound), so S = 2 is only checked to run and be finite.
Measured on an MI355X: worst err / tol of this file's cases 0.506, rel-L2 1.9e-3 - 3.7e-3 (profiles/EXPERIMENTS.md section 9, f12)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from style_aligned_ref import adain_coef, attach_style, shared_reference  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE  # noqa: E402

F64 = torch.float64


def _default_ref(B):
    return tuple(-1 if b % 2 == 0 else b - 1 for b in range(B))      # (-1, 0) and (-1, 0, -1, 2)


@functools.lru_cache(maxsize=None)
def _case(B, H, S, prescaled, kind="spread"):
    """q, k with per-sample, per-channel scales 0.5 .. 2 and shifts +-0.3 (so that AdaIN has something to do), v plain.
    kind "offset": every fourth channel of q and k has mean 8 and standard deviation 0.25.  -> (device bf16, host fp32)"""
    g = torch.Generator().manual_seed(1000 * B + S)
    C = 64 * H

    def make():
        x = torch.randn(B, S, C, generator=g) * (0.5 + 1.5 * torch.rand(B, 1, C, generator=g)) + 0.6 * (torch.rand(B, 1, C, generator=g) - 0.5)
        if kind == "offset":
            x[:, :, ::4] = 8.0 + 0.25 * torch.randn(B, S, C // 4, generator=g)
        return x
    q, k, v = make(), make(), bfr(B, S, C, seed=3)
    if prescaled:
        q = q * ALPHA
    q, k = q.to(BF), k.to(BF)
    return tuple(t.cuda() for t in (q, k, v)), (q.float(), k.float(), v.float())


@functools.lru_cache(maxsize=None)
def _reference(B, H, S, ref, prescaled, aq, ak, ss, sh):
    """the fp32 restatement, once per case; a prescaled q enters as the kernel gets it, with its factor named"""
    _, (q, k, v) = _case(B, H, S, prescaled)
    return shared_reference(q, k, v, H, ref, adain_queries=aq, adain_keys=ak, share_scale=ss, share_shift=sh,
                            q_factor=ALPHA if prescaled else 1.0)


WORST = {"ratio": 0.0}


def _close(name, got, ref, mag, rows=None):
    """close_terms of tests/test_ip_multi_gpu.py with the shared softmax's magnitude; rows: the samples to judge"""
    got = got.detach().float().cpu()
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    if rows is not None:
        got, ref, mag = got[rows], ref[rows], mag[rows]
    err = (got - ref).abs()
    tol = 2.0 * 2.0 ** -7 * (mag + rms)
    bad = (err > tol).float().mean().item()
    e = rel_l2(got, ref)
    WORST["ratio"] = max(WORST["ratio"], (err / tol).max().item())
    print(f"[{name}] max_abs={err.max().item():.3e} worst err/tol={(err / tol).max().item():.3f} (so far {WORST['ratio']:.3f}) "
          f"rel_l2={e:.3e} rms={rms:.3e} frac_bad={bad:.2e}")
    assert torch.isfinite(got).all(), name
    assert bad == 0.0 and e < 6e-3, f"{name}: frac_bad={bad} rel_l2={e}"


# ---------------------------------------------------------------------------------------------- the coefficients
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,S,kind", [(2, 2, 16, "spread"), (2, 2, 200, "spread"), (3, 2, 364, "spread"), (4, 2, 1024, "spread"),
                                        (2, 2, 1024, "offset"), (2, 3, 364, "offset")])
def test_adain_coef_vs_restatement(ops, B, H, S, kind, prescaled):
    ref = (-1, 0, 0) if B == 3 else _default_ref(B)
    (q, k, _), (qf, kf, _) = _case(B, H, S, prescaled, kind)
    c = ALPHA if prescaled else 1.0
    want = adain_coef(qf.to(F64), kf.to(F64), ref, eps_q=1e-5 * c * c).float()
    got = ops.attn_adain_coef(q, k, H, ref, q_prescaled=prescaled)
    tg = [b for b in range(B) if ref[b] >= 0]
    close_f32(f"adain-coef {kind} pre{int(prescaled)} B{B} H{H} S{S}", got[tg], want[tg])
    pl = [b for b in range(B) if ref[b] < 0]
    assert got[pl].eq(0).all()                                       # rows of plain samples are not written
    assert torch.equal(ops.attn_adain_coef(q, k, H, ref, q_prescaled=prescaled), got)          # two runs, the same bits
    for aq, ak in ((False, True), (True, False)):
        half = ops.attn_adain_coef(q, k, H, ref, q_prescaled=prescaled, adain_queries=aq, adain_keys=ak)
        off, on = (0, 2) if not aq else (2, 0)
        assert half[tg, off].eq(1).all() and half[tg, off + 1].eq(0).all() and torch.equal(half[tg, on:on + 2], got[tg, on:on + 2])


def test_adain_coef_reads_projection_columns_in_place(ops):
    """Q and K as column ranges of one Q | K | V buffer, the layout the runtime hands over"""
    B, H, S = 2, 2, 200
    (q, k, v), _ = _case(B, H, S, False)
    qkv = torch.cat([q, k, v], -1)
    C = 64 * H
    assert torch.equal(ops.attn_adain_coef(qkv[..., :C], qkv[..., C:2 * C], H, (-1, 0)), ops.attn_adain_coef(q, k, H, (-1, 0)))


# ---------------------------------------------------------------------------------------------- the shared forward
SHAPES = [(2, 2, 16, None), (2, 2, 200, None), (3, 2, 364, (-1, 0, 0)), (4, 2, 260, (-1, 0, -1, 2)), (2, 2, 130, None)]


@pytest.mark.parametrize("ss", [1.0, 0.5])
@pytest.mark.parametrize("sh", [0.0, 1.5])
@pytest.mark.parametrize("aq,ak", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,S,ref", SHAPES)
def test_attention_fwd_shared_vs_fp32(ops, B, H, S, ref, prescaled, aq, ak, sh, ss):
    """S = 364: a masked last tile in both segments; S = 130: three tiles per segment, the last with 2 keys"""
    ref = _default_ref(B) if ref is None else ref
    (q, k, v), _ = _case(B, H, S, prescaled)
    coef = ops.attn_adain_coef(q, k, H, ref, q_prescaled=prescaled, adain_queries=aq, adain_keys=ak)
    o = ops.attention_fwd_shared(q, k, v, H, ref, coef, q_prescaled=prescaled, shared_score_scale=ss, shared_score_shift=sh)
    want, mag, _ = _reference(B, H, S, ref, prescaled, aq, ak, ss, sh)
    _close(f"attn-shared pre{int(prescaled)} B{B} H{H} S{S} ref{list(ref)} adain q{int(aq)} k{int(ak)} shift {sh} scale {ss}", o, want, mag)


def test_attention_fwd_shared_two_tokens_runs(ops):
    """S = 2: the variance over two tokens is ill-conditioned, so no tolerance is claimed; it runs and is finite"""
    (q, k, v), _ = _case(2, 2, 2, False)
    coef = ops.attn_adain_coef(q, k, 2, (-1, 0))
    o = ops.attention_fwd_shared(q, k, v, 2, (-1, 0), coef)
    assert torch.isfinite(o.float()).all() and torch.isfinite(coef).all()
    assert torch.equal(o[0], ops.attention_fwd(q, k, v, 2)[0][0])


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,S,ref", [(2, 2, 16, (-1, 0)), (3, 2, 364, (-1, 0, 0)), (4, 2, 260, (-1, 0, -1, 2)), (4, 3, 1024, (-1, -1, 1, 3)),
                                       (2, 2, 128, (-1, 0))])
def test_attention_fwd_shared_exactness(ops, B, H, S, ref, prescaled):
    """S = 128: pea_op_attention_fwd is the resident-key kernel there, which then writes the plain samples itself"""
    (q, k, v), _ = _case(B, H, S, prescaled)
    plain, _ = ops.attention_fwd(q, k, v, H, q_prescaled=prescaled)
    # nobody is a target: the plain launch's bits, the coefficients may be absent
    assert torch.equal(ops.attention_fwd_shared(q, k, v, H, [-1] * B, None, q_prescaled=prescaled), plain)
    coef = ops.attn_adain_coef(q, k, H, ref, q_prescaled=prescaled)
    run = lambda c=coef: ops.attention_fwd_shared(q, k, v, H, ref, c, q_prescaled=prescaled)
    pl = [b for b in range(B) if ref[b] < 0 or ref[b] == b]
    tg = [b for b in range(B) if b not in pl]
    a = run()
    # plain samples: the plain launch's bits whatever their coefficient rows hold -- NaN there is never read
    cn = coef.clone()
    cn[pl] = float("nan")
    an = run(cn)
    assert torch.equal(a[pl], plain[pl]) and torch.equal(an, a) and torch.isfinite(an.float()).all()
    for b in tg:
        assert not torch.equal(a[b], plain[b])
    assert torch.equal(run(), a)                                     # two runs, the same bits


def test_attention_fwd_shared_reads_projection_columns_in_place(ops):
    B, H, S = 2, 2, 200
    (q, k, v), _ = _case(B, H, S, True)
    qkv = torch.cat([q, k, v], -1)
    C = 64 * H
    coef = ops.attn_adain_coef(q, k, H, (-1, 0), q_prescaled=True)
    o = ops.attention_fwd_shared(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], H, (-1, 0), coef, q_prescaled=True)
    assert torch.equal(o, ops.attention_fwd_shared(q, k, v, H, (-1, 0), coef, q_prescaled=True))


@pytest.mark.parametrize("spike_on", ["reference", "own"])
def test_attention_fwd_shared_spiked_key(ops, spike_on):
    """a key that leads its row by 60 and more, in the SECOND tile of its segment (key 70 of 260): the rescale branch runs there --
    for the reference segment that is after the segment change, with the other constant in the accumulator operand"""
    B, H, S, j = 2, 2, 260, 70
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)                                     # unit vector
    q = (8.0 * u + 0.5 * torch.randn(B, S, H, 64, generator=g)).reshape(B, S, H * 64).to(BF)
    k, v = bfr(B, S, H * 64, seed=2), bfr(B, S, H * 64, seed=3)
    k[0 if spike_on == "reference" else 1, j] = ((160.0 if spike_on == "reference" else 512.0) * u).repeat(H).to(BF)
    ref = (-1, 0)
    want, mag, coef = shared_reference(q.float(), k.float(), v.float(), H, ref)
    heads = lambda t: t.view(t.shape[0], H, 64).transpose(0, 1)
    qp = coef[1, 0] * q[1].float() + coef[1, 1]
    kk = k[0].float() if spike_on == "reference" else coef[1, 2] * k[1].float() + coef[1, 3]
    other = coef[1, 2] * k[1].float() + coef[1, 3] if spike_on == "reference" else k[0].float()
    ls = heads(qp) @ heads(kk).transpose(-1, -2) * 0.125
    rest = torch.cat([ls[..., :j], ls[..., j + 1:], heads(qp) @ heads(other).transpose(-1, -2) * 0.125], -1)
    lead = (ls[..., j] - rest.max(-1).values).min().item()
    print(f"[attn-shared spike on the {spike_on} segment] the spiked key leads by {lead:.1f} and more")
    assert lead > 60
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    o = ops.attention_fwd_shared(qd, kd, vd, H, ref, ops.attn_adain_coef(qd, kd, H, ref))
    _close(f"attn-shared spike on the {spike_on} segment", o, want, mag)


def test_attention_fwd_shared_refusals(ops):
    """the list of tests/test_style_aligned_cpu.py on the device: an O filled with 7.0 stays as it is"""
    import ctypes
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    n = 0

    def refused(what, B=2, S=128, Skv=None, ldk=128, ref=(-1, 0), coef=True, nd=1):
        nonlocal n
        Skv = S if Skv is None else Skv
        q = bfr(max(B, 1), max(S, 1), 128).cuda()
        k = bfr(max(B, 1), max(Skv, 1), max(ldk, 128), seed=2).cuda()
        o = torch.full((max(B, 1), max(S, 1), 128), 7.0, dtype=BF).cuda()
        cf = torch.ones(max(B, 1), 4, 128).cuda()
        hr = (ctypes.c_int * 40)(*(list(ref) + [-1] * (40 - len(ref))))
        rc = lib().pea_op_attention_fwd_shared(ptr(q), 128, ptr(k), ldk, ptr(k), ldk, ptr(o), 128, B, 2, S, Skv, hr, ptr(cf) if coef else None,
                                               0.125, 0, 1.0, 0.0, nd, stream_ptr())
        torch.cuda.synchronize()
        msg = lib().pea_last_error().decode()
        print(f"[attn-shared refused] {what}: rc={rc} {msg}")
        assert rc == -3 and what in msg and bool((o == 7.0).all()), what          # PEA_E_SHAPE
        n += 1

    refused("S >= 2", S=1)
    refused("Sq == Skv", Skv=77)
    refused("head_dim 64", nd=2)
    refused("at most 32 samples", B=33)
    refused("out of range", ref=(-1, 2))
    refused("itself a target", B=3, ref=(-1, 0, 1))
    refused("leading dimension", ldk=132)
    refused("null coef", coef=False)
    refused("empty problem", S=0)
    assert n == 9
    wide = bfr(2, 128, 256).cuda()
    with pytest.raises(PeaError, match="head_dim"):
        ops.attn_adain_coef(wide, wide, 2, (-1, 0))
    # ref[b] == b: its own reference, that is, a plain sample
    (q, k, v), _ = _case(2, 2, 200, False)
    assert torch.equal(ops.attention_fwd_shared(q, k, v, 2, (0, 1), None), ops.attention_fwd(q, k, v, 2)[0])


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
CTX_GAIN = 5.0                                                       # as tests/test_p2p_gpu.py: unscaled, the storage floor is degenerate


def _setup(B, L=77, hw=16):
    """the tiny UNet pair of tests/test_p2p_gpu.py; B different latents and prompts at ONE timestep"""
    from test_ip_adapter_gpu import _tiny_ip_pair
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    t = t[1:2].expand(B).contiguous()
    ehs = (CTX_GAIN * ehs).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
    return cfg, ref, hip, run_ref, run, plain_ref


def _oracle(state, run_ref, *args, **kw):
    from oracle.bf16_store import bf16_storage
    with torch.no_grad():
        state.set(*args, **kw)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
        state.set(None)
    return want, stored


def _check_eps(tag, got, want, stored, plain_ref):
    """the limits of tests/test_p2p_gpu.py"""
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[{tag}] eps rel_l2={e:.3e} (against the oracle WITHOUT sharing {e_plain:.3e}), bf16-storage floor {floor:.3e}, "
          f"ratio {e / floor:.2f}; sharing moves the oracle's eps by {shift:.3f}")
    assert e < EPS_LIMIT and e < e_plain
    assert floor >= FLOOR_DEGENERATE, floor
    assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)


def test_tiny_unet_style_aligned(gpu):
    """B = 2: the reference and one target; every layer, one layer, the switches; back to the first bits"""
    from pea_diffusion_amd import style_aligned as sa
    B = 2
    cfg, ref, hip, run_ref, run, plain_ref = _setup(B)
    before = run()
    assert rel_l2(before, plain_ref) < EPS_LIMIT
    state = attach_style(ref)
    names = sa.layer_names(hip)
    assert sorted(names) == sorted(n for n, _ in ref.named_modules() if n.endswith(".attn1")) and len(names) >= 3
    r = sa.reference_index(B)
    want, stored = _oracle(state, run_ref, r)
    assert torch.equal(want[0], plain_ref[0])                        # the oracle's reference does not move
    # ... and sharing that is ignored cannot pass: a forward within EPS_LIMIT of the PLAIN oracle is then at least 2 x EPS_LIMIT
    # away from this one (the oracle alone: nothing of the code under test enters)
    assert rel_l2(want[1], plain_ref[1]) >= 3 * EPS_LIMIT
    hip.set_style_aligned()
    got = run()
    _check_eps("tiny unet + StyleAligned, every layer", got[1:], want[1:], stored[1:], plain_ref[1:])
    assert torch.equal(got[0], before[0])                            # the reference keeps the bits of a forward without sharing
    assert not torch.equal(got[1], before[1])
    assert torch.equal(run(), got)                                   # bit-reproducible
    # one layer: fewer launches change, and the result follows the oracle with the same selection
    one = names[len(names) // 2]
    want1, stored1 = _oracle(state, run_ref, r, on={n: n == one for n in names})
    hip.set_style_aligned(layers=[one])
    got1 = run()
    _check_eps(f"tiny unet + StyleAligned, {one} only", got1[1:], want1[1:], stored1[1:], plain_ref[1:])
    assert torch.equal(got1[0], before[0]) and not torch.equal(got1[1], got[1]) and not torch.equal(got1[1], before[1])
    assert rel_l2(got1[1], want1[1]) < rel_l2(got1[1], want[1]) and rel_l2(got[1], want[1]) < rel_l2(got[1], want1[1])
    hip.set_style_aligned(layers=0.0)                                # no layer: the plain launches
    assert torch.equal(run(), before)
    # the switches and the score knobs
    want2, stored2 = _oracle(state, run_ref, r, adain_queries=False, share_scale=0.5, share_shift=1.5)
    hip.set_style_aligned(adain_queries=False, shared_score_scale=0.5, shared_score_shift=1.5)
    got2 = run()
    _check_eps("tiny unet + StyleAligned, no query AdaIN, scale 0.5, shift 1.5", got2[1:], want2[1:], stored2[1:], plain_ref[1:])
    assert not torch.equal(got2[1], got[1])
    hip.set_style_aligned(ref=[-1, -1])                              # nobody refers to anybody
    assert torch.equal(run(), before)
    hip.set_style_aligned()
    hip.release_activations()                                        # the coefficient buffers are not part of the activation arena
    assert torch.equal(run(), got)
    hip.clear_style_aligned()
    assert torch.equal(run(), before)                                # the bits from before `set` come back


def test_tiny_unet_style_aligned_cfg_layout(gpu):
    from pea_diffusion_amd import style_aligned as sa
    B = 4
    cfg, ref, hip, run_ref, run, plain_ref = _setup(B)
    before = run()
    state = attach_style(ref)
    r = sa.reference_index(2, do_cfg=True)
    assert r == [-1, 0, -1, 2]
    want, stored = _oracle(state, run_ref, r)
    hip.set_style_aligned(do_cfg=True)
    got = run()
    assert torch.equal(got[0], before[0]) and torch.equal(got[2], before[2])             # each half's reference
    assert not torch.equal(got[1], before[1]) and not torch.equal(got[3], before[3])
    _check_eps("tiny unet + StyleAligned, CFG layout", got[1::2], want[1::2], stored[1::2], plain_ref[1::2])
    hip.clear_style_aligned()
    assert torch.equal(run(), before)


def test_tiny_unet_style_aligned_refusals(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import PromptEdit
    from pea_diffusion_amd.unet import HipUNet
    grad = HipUNet(pc.tiny_config(), 2, 16, 16, 77, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.set_style_aligned()
    B, L = 2, 77
    cfg, ref, hip, run_ref, run, plain_ref = _setup(B, L)
    before = run()
    with pytest.raises(PeaError, match="out of range"):
        hip.set_style_aligned(ref=[-1, 2])
    with pytest.raises(PeaError, match="itself a target"):
        hip.set_style_aligned(ref=[1, 0])
    with pytest.raises(PeaError, match="references for a batch"):
        hip.set_style_aligned(ref=[-1, 0, 0])
    with pytest.raises(PeaError, match="names no self-attention layer"):
        hip.set_style_aligned(layers=["up_blocks.9"])
    assert torch.equal(run(), before)
    edit = PromptEdit.compose(L, 2, [None, dict(source=0)])
    hip.set_prompt_edit(edit)
    with pytest.raises(PeaError, match="prompt editing"):
        hip.set_style_aligned()                                      # set while a prompt edit is live
    hip.clear_prompt_edit()
    hip.set_style_aligned()
    shared = run()
    hip.set_prompt_edit(edit)                                        # ... and an edit that arrives afterwards: the forward refuses
    with pytest.raises(PeaError, match="prompt editing"):
        run()
    hip.clear_prompt_edit()
    assert torch.equal(run(), shared)
    hip.clear_style_aligned()
    assert torch.equal(run(), before)


def test_tiny_unet_style_aligned_with_image_prompt(gpu):
    """a live IP-Adapter works in the cross-attention, the sharing in the self-attention: both attached to the oracle"""
    from ip_adapter_ref import attach_ip, file_state_dict, make_image_proj, set_ip
    from test_ip_adapter_gpu import GAIN, N_TOK
    B, scale = 2, 0.7
    cfg, ref, hip, run_ref, run, plain_ref = _setup(B)
    tok = torch.randn(B, N_TOK, 128, generator=torch.Generator().manual_seed(7)).to(BF).float()
    with torch.no_grad():
        attach_ip(ref, N_TOK, seed=3, gain=GAIN)
        set_ip(ref, tok, scale)
        ip_only = run_ref()
    state = attach_style(ref)
    want, stored = _oracle(state, run_ref, [-1, 0])
    assert rel_l2(want[1], ip_only[1]) >= 3 * EPS_LIMIT and torch.equal(want[0], ip_only[0])
    hip.load_ip_adapter(file_state_dict(ref, make_image_proj(64, 128, N_TOK, seed=4)))
    hip.set_ip_tokens(tok.cuda())
    hip.set_ip_adapter_scale(scale)
    with_ip = run()
    hip.set_style_aligned()
    got = run()
    _check_eps("tiny unet + image prompt + StyleAligned", got[1:], want[1:], stored[1:], ip_only[1:])
    assert torch.equal(got[0], with_ip[0]) and not torch.equal(got[1], with_ip[1])
    hip.clear_style_aligned()
    assert torch.equal(run(), with_ip)
