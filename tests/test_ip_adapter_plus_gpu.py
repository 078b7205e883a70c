"""-m gpu: the IP-Adapter "plus" path on the HIP side -- the few-query attention over the union of two key sets
(pea_op_attention_fwd_fewq) against fp32 attention over the concatenated keys, the properties a key-split kernel can break, its
refusals; the Resampler tape against the restatement of tests/resampler_ref.py; and tower -> tokens -> tiny UNet against the
oracle with the restated tokens.

Tolerances are the project's: the kernel's O follows the attention-output rule of tests/test_ops_gpu.py (close_bf16 at 2 ulps,
rel_l2 < 6e-3), lse rtol 1e-3 / atol 2e-3; the Resampler is held to STORAGE_FLOOR_FACTOR x the bf16-storage floor of the
restatement computed in the same run (FLOOR_DEGENERATE as the fallback switch); the UNet to the rule of
test_tiny_unet_with_image_prompt.  tests/test_ip_adapter_plus_cpu.py checks on the CPU that the references alone meet what the
spiked / monotone cases and the floors assume."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
import resampler_ref as rr  # noqa: E402
from ip_adapter_ref import attach_ip, set_ip  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, make_pair, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, close_bf16, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE  # noqa: E402


# ---------------------------------------------------------------------------------------------- kernel
def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def sdpa_union(q, k, v, H):
    """fp32 attention per head over the given (concatenated) keys, scale 1/8 -> (o [B,Sq,C], lse [B,H,Sq])"""
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * 0.125
    o = (torch.softmax(s, -1) @ _heads(v, H)).transpose(1, 2).reshape(q.shape)
    return o, torch.logsumexp(s, -1)


def _inputs(B, H, Sq, S1, S2, prescaled):
    q, k, v = bfr(B, Sq, H * 64, seed=1), bfr(B, S1, H * 64, seed=2), bfr(B, S1, H * 64, seed=3)
    k2, v2 = (bfr(B, S2, H * 64, seed=5), bfr(B, S2, H * 64, seed=6)) if S2 else (None, None)
    if prescaled:
        q = (q.float() * ALPHA).to(BF)
    return q, k, v, k2, v2


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, S1, S2, prescaled):
    q, k, v, k2, v2 = _inputs(B, H, Sq, S1, S2, prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    ks = torch.cat([k, k2], 1) if S2 else k
    vs = torch.cat([v, v2], 1) if S2 else v
    o, lse = sdpa_union(qr, ks.float(), vs.float(), H)
    return tuple(None if t is None else t.cuda() for t in (q, k, v, k2, v2)), o, lse


SHAPES = [(1, 1, 1, 1, 0),            # one key: three waves without a block; the merge must not make NaN of -inf - -inf
          (1, 2, 16, 3, 1),           # fewer keys than waves
          (2, 2, 16, 31, 16), (1, 2, 17, 32, 32), (1, 3, 32, 33, 1),      # block edges on both sets, ragged query counts
          (1, 2, 5, 50, 5),           # ragged everything
          (2, 20, 16, 257, 16),       # SDXL plus
          (1, 12, 16, 577, 16),       # ViT-L/14 at 336
          (1, 2, 8, 1025, 0)]         # many blocks per wave, no second set


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,S1,S2", SHAPES)
def test_attention_fwd_fewq_vs_fp32(ops, B, H, Sq, S1, S2, prescaled):
    (q, k, v, k2, v2), oref, lref = _case(B, H, Sq, S1, S2, prescaled)
    o, lse = ops.attention_fwd_fewq(q, k, v, k2, v2, H, q_prescaled=prescaled, want_lse=True)
    tag = f"attn-fewq pre{int(prescaled)} B{B} H{H} Sq{Sq} S1 {S1} S2 {S2}"
    close_bf16(tag + " O", o, oref, ulps=2.0)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)
    o_again, lse_again = ops.attention_fwd_fewq(q, k, v, k2, v2, H, q_prescaled=prescaled, want_lse=True)
    assert torch.equal(o, o_again) and torch.equal(lse, lse_again)           # fixed merge order: the same bits


@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_fwd_fewq_set_boundary(ops, prescaled):
    """the same 273 keys split 257 + 16 and 241 + 32: both pass the rule against ONE reference"""
    B, H, Sq = 2, 3, 16
    q, k, v, _, _ = _inputs(B, H, Sq, 273, 0, prescaled)
    oref, lref = sdpa_union(q.float() / ALPHA if prescaled else q.float(), k.float(), v.float(), H)
    for s1 in (257, 241):
        parts = [t.contiguous().cuda() for t in (k[:, :s1], v[:, :s1], k[:, s1:], v[:, s1:])]
        o, lse = ops.attention_fwd_fewq(q.cuda(), *parts, H, q_prescaled=prescaled, want_lse=True)
        close_bf16(f"attn-fewq boundary {s1}+{273 - s1} pre{int(prescaled)} O", o, oref, ulps=2.0)
        close_f32(f"attn-fewq boundary {s1}+{273 - s1} lse", lse, lref, rtol=1e-3, atol=2e-3)


SPIKE_H = 2


def spiked_inputs(where):
    """S1 = 65 (S1 % 32 == 1: the spiked last key of set 1 is alone in its block, on another wave than most), S2 = 16.  One key
    -- the last of set 1, or the last of set 2 -- is aligned with every query and scaled until it leads by > 100 logits; its
    value row is distinctive.  -> q, k, v, k2, v2, index of that key in the union"""
    B, H, Sq, S1, S2 = 1, SPIKE_H, 16, 65, 16
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)
    q = (4.0 * u + 0.5 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    k, v, k2, v2 = bfr(B, S1, H * 64, seed=2), bfr(B, S1, H * 64, seed=3), bfr(B, S2, H * 64, seed=5), bfr(B, S2, H * 64, seed=6)
    (k if where == "set1" else k2)[:, -1] = (512.0 * u).repeat(H).to(BF)
    (v if where == "set1" else v2)[:, -1] = torch.linspace(-3.0, 3.0, H * 64).to(BF)
    return q, k, v, k2, v2, (S1 - 1 if where == "set1" else S1 + S2 - 1)


@pytest.mark.parametrize("where", ["set1", "set2"])
def test_attention_fwd_fewq_spiked_key(ops, where):
    q, k, v, k2, v2, j = spiked_inputs(where)
    want = torch.cat([v, v2], 1)[:, j]                               # the reference is exactly this row (checked on the CPU)
    o = ops.attention_fwd_fewq(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), SPIKE_H)
    assert torch.equal(o.cpu(), want[:, None, :].expand_as(o)), (o.cpu().float() - want.float()[:, None]).abs().max()


def monotone_inputs():
    """scores that rise along the keys of the union (200 + 20 keys, about 0.13 per key): every 32-key block's maximum exceeds
    the last one's, so every wave ends on another running maximum and the merge has to rescale all four partials"""
    B, H, Sq, S1, S2 = 1, SPIKE_H, 16, 200, 20
    g = torch.Generator().manual_seed(13)
    u = torch.full((64,), 0.125)
    q = (4.0 * u + 0.05 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    ramp = torch.arange(S1 + S2, dtype=torch.float32) * 0.25        # q . k / 8 = 4 x 0.25 i / 8 ... per unit of u
    ks = (ramp[None, :, None, None] * u + 0.05 * torch.randn(B, S1 + S2, H, 64, generator=g)).reshape(B, S1 + S2, H * 64).to(BF)
    vs = bfr(B, S1 + S2, H * 64, seed=3)
    return q, ks[:, :S1].contiguous(), vs[:, :S1].contiguous(), ks[:, S1:].contiguous(), vs[:, S1:].contiguous()


def test_attention_fwd_fewq_rising_scores(ops):
    q, k, v, k2, v2 = monotone_inputs()
    oref, lref = sdpa_union(q.float(), torch.cat([k, k2], 1).float(), torch.cat([v, v2], 1).float(), SPIKE_H)
    o, lse = ops.attention_fwd_fewq(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), SPIKE_H, want_lse=True)
    close_bf16("attn-fewq rising scores O", o, oref, ulps=2.0)
    close_f32("attn-fewq rising scores lse", lse, lref, rtol=1e-3, atol=2e-3)


def test_attention_fwd_fewq_never_reads_behind_a_set(ops):
    """K / V with NaN rows behind Skv1 / Skv2, inside the allocation: finite, and bit for bit the output of tight buffers"""
    B, H, Sq, S1, S2 = 1, 2, 16, 45, 7
    q, k, v, k2, v2 = _inputs(B, H, Sq, S1, S2, False)
    tight = ops.attention_fwd_fewq(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), H)
    pad = lambda t, n: torch.cat([t, torch.full((B, n, t.shape[2]), float("nan"), dtype=BF)], 1).cuda()
    o = ops.attention_fwd_fewq(q.cuda(), pad(k, 40), pad(v, 40), pad(k2, 30), pad(v2, 30), H, kv_rows=S1, kv2_rows=S2)
    assert torch.isfinite(o).all() and torch.equal(o, tight)


def test_attention_fwd_fewq_refusals(ops):
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    B, H = 1, 2
    mk = lambda n, seed=1, c=128: bfr(B, n, c, seed=seed).cuda()
    q, k, v, k2, v2 = mk(16), mk(50, 2), mk(50, 3), mk(8, 5), mk(8, 6)
    for what, call in (("Sq = 33", lambda: ops.attention_fwd_fewq(mk(33), k, v, k2, v2, H)),
                       ("Skv2 = 33", lambda: ops.attention_fwd_fewq(q, k, v, mk(33, 5), mk(33, 6), H)),
                       ("K2 without V2", lambda: ops.attention_fwd_fewq(q, k, v, k2, None, H)),
                       ("head_dim 128", lambda: ops.attention_fwd_fewq(q, k, v, k2, v2, 1))):
        with pytest.raises(PeaError):
            call()
        print(f"[attn-fewq refused] {what}: {lib().pea_last_error().decode()}")
    k_bad = bfr(B, 50, 132, seed=2).cuda()                           # rows 132 elements apart: not a multiple of 8
    o = torch.full((B, 16, 128), 7.0, dtype=BF).cuda()
    rc = lib().pea_op_attention_fwd_fewq(ptr(q), 128, ptr(k_bad), 132, ptr(v), 128, ptr(k2), 128, ptr(v2), 128, ptr(o), 128, None, B, H,
                                         16, 50, 8, 0.125, 1, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc == -3 and b"multiples of 8" in lib().pea_last_error() and bool((o == 7.0).all())       # refused before any launch


# ---------------------------------------------------------------------------------------------- the Resampler tape
def _tape(name, batch=None):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    d, sd, hidden, want, stored = rr.case(name)
    t = ipa.HipResampler(pc.ResamplerConfig(**d), batch or hidden.shape[0], hidden.shape[1])
    assert t.weight_table() == rr.state_shapes(d)
    missing, unexpected = t.load_state_dict(sd)
    assert not missing and not unexpected
    return t, hidden, want, stored


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_resampler_vs_restatement(gpu, name):
    from pea_diffusion_amd._lib import lib
    t, hidden, want, stored = _tape(name)
    na, npre = ctypes.c_int(), ctypes.c_int()
    assert lib().pea_tape_attention_census(t._h, ctypes.byref(na), ctypes.byref(npre)) == 0
    assert na.value == npre.value == t.cfg.depth
    got = t(hidden.cuda())
    e, floor = rel_l2(got, want), rel_l2(stored, want)
    print(f"[resampler {name}] tokens rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio {e / floor:.2f}")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all()
    assert floor >= FLOOR_DEGENERATE, floor                          # (the CPU test pins this for the same seeds)
    assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)
    assert torch.equal(t(hidden.cuda()), got)
    if name == "tiny":                                               # the latents broadcast and every batch stride
        one, _, _, _ = _tape(name, batch=1)
        first = one(hidden[:1].cuda())[0]
        print(f"[resampler tiny] batch 1 against row 0 of batch 3: max_abs={(first - got[0]).abs().max().item():.3e}")
        assert torch.equal(first, got[0])


def test_resampler_init_random_and_refusals(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd._lib import PeaError
    t = ipa.HipResampler(pc.ResamplerConfig(**rr.TINY), 2, 10)
    h = torch.randn(2, 10, 128, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(PeaError, match="never loaded"):
        t(h)
    t.init_random(3)
    out = t(h)
    assert torch.isfinite(out).all() and out.std() > 0.5             # a LayerNorm output with unit gammas
    with pytest.raises(PeaError):
        t(h[:, :9])


# ---------------------------------------------------------------------------------------------- tower -> tokens -> tiny UNet
def test_tower_to_plus_tokens_to_tiny_unet(gpu):
    import vision_ref as vr
    from oracle.bf16_store import bf16_storage
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd.vision import HipImageEncoder
    B, L, scale, NQ, GAIN = 1, 77, 0.7, 4, 4.0
    vcfg = pc.tiny_vit_config()
    vsd = vr.random_state_dict(vcfg, seed=3)
    enc = HipImageEncoder(vcfg, B)
    enc.load_state_dict(vsd)
    px = torch.randn(B, 3, vcfg.image_size, vcfg.image_size, generator=torch.Generator().manual_seed(5))
    d = rr.dims(vcfg.hidden_size, 128, 2, 2, NQ, 512, 128)
    rsd = rr.random_state_dict(d, seed=21)
    cfg, ref, hip = make_pair(tiny_config, 2 * B, L, False)
    for p in ref.parameters():
        p.requires_grad_(False)
    x, t, ehs, added = cond_inputs(cfg, 2 * B, L, 16)
    ehs = ehs.to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
        attach_ip(ref, NQ, seed=3, gain=GAIN)
    ad = hip.load_ip_adapter(ipa.IPAdapterPlus(rr.plus_file(ref, rsd), pc.tiny_config()))
    assert isinstance(ad, ipa.IPAdapterPlus)
    # tokens: the restatement fed the reference tower's hidden_states[-2]; the unconditional half is the ZERO-PIXEL path
    tok = ad.encode(enc, px.cuda(), do_cfg=True)
    with torch.no_grad():
        hs = lambda p: vr.tower_ref(vsd, vcfg, p)["hidden_states"][-2]
        hid = torch.cat([hs(torch.zeros_like(px)), hs(px)])
        tok_ref = rr.resampler_ref(rsd, hid, torch.float64).float()
        tok_st = rr.resampler_ref(rsd, hid, torch.float64, store=True).float()
        tok_floor = rel_l2(tok_st, tok_ref)
    e_tok = rel_l2(tok, tok_ref)
    print(f"[tower -> plus tokens] rel_l2={e_tok:.3e} (Resampler-only storage floor {tok_floor:.3e}; the tower's own states carry < 2e-2)")
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (2 * B, NQ, 128) and torch.isfinite(tok).all()
    assert e_tok < 2e-2                                              # the bound of the tower's states (tests/test_vision_gpu.py)
    assert not torch.equal(tok[0], tok[1])                           # zero pixels are not the image
    hip.set_ip_tokens(tok)
    hip.set_ip_adapter_scale(scale)
    got = run()
    with torch.no_grad():
        set_ip(ref, tok_ref.to(BF).float(), scale)                   # the tokens enter the HIP projection rounded to bf16
        want = run_ref()
        set_ip(ref, tok_st.to(BF).float(), scale)                    # the floor of the chain: bf16-stored Resampler, then UNet
        with bf16_storage():
            stored = run_ref()
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[tiny unet + plus image prompt] eps rel_l2={e:.3e} (against the oracle WITHOUT the prompt {e_plain:.3e}), bf16-storage "
          f"floor {floor:.3e}, ratio {e / floor:.2f}; the prompt moves the oracle's eps by {shift:.3f}")
    assert shift >= 10 * EPS_LIMIT, shift
    assert e < EPS_LIMIT and e < e_plain
    if floor >= FLOOR_DEGENERATE:
        assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)
    assert torch.equal(run(), got)
