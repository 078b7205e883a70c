"""-m gpu: regional text prompts -- the fused per-region attention (pea_op_attention_fwd_regions) against an fp32 reference, its
exactness properties and refusals, and the UNet runtime (HipUNet.set_prompt_regions) against the restatement of
tests/regional_ref.py.

Tolerance of the kernel's O: the rule of tests/test_ip_multi_gpu.py (close_terms) term by term -- an element may be off by
2 x 2^-7 x (sum_r |w_r| |o_r| + rms(O)), rel-L2 below 6e-3.  It applies because the kernel rounds P of every region to bf16
un-normalised, as the plain kernel does, and scales each term by w_r afterwards, in fp32; O is rounded once."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from regional_ref import attach_regions, combine, half_masks, quadrant_masks, regions_terms, set_regions  # noqa: E402
from test_ip_adapter_gpu import _heads, _inputs, _tiny_ip_pair  # noqa: E402
from test_ip_multi_gpu import GRIDS, close_terms  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE  # noqa: E402

GRID = dict(GRIDS)
GRID.update({1: (1, 1)})
SOFT = [0.6, -1.0, 0.8, 0.5]                                         # per region; the second is negative wherever there are two


def _rects(R, h, w):
    """R rectangles that partition an 8h x 8w picture: columns for R <= 3 (R = 1: everything), quadrants for R = 4"""
    if R == 4:
        return quadrant_masks(8 * h, 8 * w)
    out = []
    for r in range(R):
        m = torch.zeros(8 * h, 8 * w)
        m[:, (8 * w * r) // R:(8 * w * (r + 1)) // R] = 1.0
        out.append(m)
    return out


def _weights(mode, B, Sq, R):
    """partition: rectangles through region_weights, most waves see one region | soft: every weight non-zero, one negative |
    batch: a table per sample, sample 0 one-hot on region 0"""
    from pea_diffusion_amd.regional import region_weights
    part = region_weights(_rects(R, *GRID[Sq]), None, *GRID[Sq])    # [1, R, Sq]
    if mode == "partition":
        return part
    g = torch.Generator().manual_seed(11)
    soft = torch.tensor(SOFT[:R])[None, :, None] * (0.25 + torch.rand(1, R, Sq, generator=g))
    if mode == "soft":
        return soft
    w = torch.cat([part, soft] + [soft * (1.0 + 0.25 * b) for b in range(2, B)])[:B].clone()
    w[0] = 0.0
    w[0, 0] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, R, Lr, prescaled):
    """inputs as test_ip_adapter_gpu._inputs makes them (the R regions back to back in k / v) and every region's fp32 term, once"""
    q, k, v, _, _ = _inputs(B, H, Sq, R * Lr, 1, prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    return tuple(t.cuda() for t in (q, k, v)), regions_terms(qr, k.float(), v.float(), H, R)


def _close(name, got, terms, w):
    """close_terms on O = 0 + sum_r 1 x w_r o_r; regional_ref.combine is the same sum"""
    R = len(terms)
    ref, _ = combine(terms, w)
    close_terms(name, got, torch.zeros_like(terms[0]), terms, [1.0] * R, [w[:, r] for r in range(R)])
    assert rel_l2(got, ref) < 6e-3


SHAPES = [(1, 1, 1, 1, 1), (2, 2, 16, 2, 16), (1, 2, 200, 2, 32), (1, 3, 128, 2, 77), (1, 2, 364, 3, 77), (1, 2, 260, 4, 33),
          (2, 2, 300, 4, 96), (2, 10, 4096, 2, 77)]                 # the last: 640 units over 512 workgroups, two per workgroup


@pytest.mark.parametrize("mode", ["partition", "soft", "batch"])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,R,Lr", SHAPES)
def test_attention_fwd_regions_vs_fp32(ops, B, H, Sq, R, Lr, prescaled, mode):
    (q, k, v), terms = _case(B, H, Sq, R, Lr, prescaled)
    w = _weights(mode, B, Sq, R)
    o = ops.attention_fwd_regions(q, k, v, H, R, w.cuda(), q_prescaled=prescaled)
    _close(f"attn-regions {mode} pre{int(prescaled)} B{B} H{H} Sq{Sq} R{R} Lr{Lr}", o, terms, w)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,R,Lr", [(1, 3, 128, 2, 77), (1, 2, 260, 4, 33), (2, 2, 300, 4, 96), (2, 10, 4096, 2, 77)])
def test_attention_fwd_regions_exactness(ops, B, H, Sq, R, Lr, prescaled):
    (q, k, v), _ = _case(B, H, Sq, R, Lr, prescaled)
    run = lambda w, kk=k, vv=v: ops.attention_fwd_regions(q, kk, vv, H, R, w.cuda(), q_prescaled=prescaled)
    # one-hot weights on region r: the plain kernel on a contiguous copy of that region's rows
    for r in (0, R - 1):
        w = torch.zeros(1, R, Sq)
        w[:, r] = 1.0
        rows = slice(r * Lr, (r + 1) * Lr)
        plain, _ = ops.attention_fwd(q, k[:, rows].contiguous(), v[:, rows].contiguous(), H, q_prescaled=prescaled)
        assert torch.equal(run(w), plain), r
    # a region that weighs 0 everywhere: its keys and values do not matter
    w = _weights("soft", B, Sq, R)
    w[:, 0] = 0.0
    k2, v2 = k.clone(), v.clone()
    k2[:, :Lr] = k2[:, :Lr] * 3
    v2[:, :Lr] = v2[:, :Lr] * 100
    a = run(w)
    assert torch.equal(run(w, k2, v2), a)
    # two runs, the same bits
    w = _weights("batch", B, Sq, R)
    a, b = run(w), run(w)
    assert torch.equal(a, b)
    # queries whose weights are all 0: exact zeros -- a whole wave's worth (rows 32..63), single rows beside weighted ones, the tail
    w = _weights("soft", 1, Sq, R).clone()
    dead = torch.zeros(Sq, dtype=torch.bool)
    dead[32:64] = True
    dead[5] = dead[Sq - 1] = dead[100] = True
    w[:, :, dead] = 0.0
    o = run(w)
    assert bool((o[:, dead] == 0).all()) and torch.equal(o[:, ~dead], run(_weights("soft", 1, Sq, R))[:, ~dead])


def test_attention_fwd_regions_spiked_key(ops):
    """one key of region 1 scores more than 100 above every other key of its region: that softmax collapses to one value row, and
    since every region has its own maximum the other regions' terms survive within the tolerance"""
    B, H, Sq, R, Lr, j = 1, 2, 260, 3, 77, 2
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)                                     # unit vector
    q = (4.0 * u + 0.5 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    k, v = bfr(B, R * Lr, H * 64, seed=2), bfr(B, R * Lr, H * 64, seed=3)
    k[:, Lr + j] = (512.0 * u).repeat(H).to(BF)
    logits = lambda kk: _heads(q.float(), H) @ _heads(kk.float(), H).transpose(-1, -2) * 0.125
    ls = logits(k[:, Lr:2 * Lr])
    rest = torch.cat([ls[..., :j], ls[..., j + 1:]], -1)
    assert (ls[..., j] - rest.max(-1).values).min() > 100
    assert logits(k[:, :Lr]).abs().max() < 30 and logits(k[:, 2 * Lr:]).abs().max() < 30
    terms = regions_terms(q.float(), k.float(), v.float(), H, R)
    value = v[:, Lr + j].float()[:, None, :]
    assert torch.equal(terms[1], value.expand_as(terms[1]))         # the reference itself: exactly one key
    dev = tuple(t.cuda() for t in (q, k, v))
    for r in range(R):                                               # every term on its own ...
        w = torch.zeros(1, R, Sq)
        w[:, r] = 1.0
        o = ops.attention_fwd_regions(*dev, H, R, w.cuda())
        _close(f"attn-regions spike in region 1, term {r}", o, terms, w)
        if r == 1:
            assert torch.equal(o.float().cpu(), value.expand_as(terms[1]))
    w = _weights("soft", B, Sq, R)                                   # ... and mixed
    _close("attn-regions spike in region 1, soft", ops.attention_fwd_regions(*dev, H, R, w.cuda()), terms, w)


def test_attention_fwd_regions_refusals(ops):
    """the list of tests/test_regional_cpu.py on the device: an O filled with 7.0 stays as it is.  nd is no argument of the entry
    point (it fixes head_dim 64): that refusal is reached through the planning entry and through the wrapper's own check"""
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    B, H, Sq = 2, 2, 128
    q = bfr(B, Sq, 128).cuda()
    filled = []

    def refused(what, R=2, Lr=77, ldk=128, Bw=1):
        rows = max(R, 1) * max(Lr, 1)
        k = bfr(B, rows, max(ldk, 128), seed=2).cuda()
        o = torch.full((B, Sq, 128), 7.0, dtype=BF).cuda()
        w = torch.ones(max(Bw, 1), max(R, 1), Sq).cuda()
        rc = lib().pea_op_attention_fwd_regions(ptr(q), 128, ptr(k), ldk, ptr(k), ldk, ptr(o), 128, B, H, Sq, R, Lr, ptr(w), Bw, 0.125, 0,
                                                stream_ptr())
        torch.cuda.synchronize()
        msg = lib().pea_last_error().decode()
        print(f"[attn-regions refused] {what}: rc={rc} {msg}")
        assert rc == -3 and msg and bool((o == 7.0).all()), what        # PEA_E_SHAPE
        filled.append(what)

    refused("R = 0", R=0)
    refused("R = 5", R=5)
    refused("Lr = 97", Lr=97)
    refused("ldk = 132", ldk=132)
    refused("Bw = 3", Bw=3)
    assert len(filled) == 5
    qd = (ctypes.c_int * 8)(B, H, Sq, 2, 77, 2, 0, 0)
    assert lib().pea_debug_attn_regions_dispatch(qd, (ctypes.c_int * 6)()) == -3 and b"head_dim 64" in lib().pea_last_error()
    wide = bfr(B, 154, 256).cuda()
    with pytest.raises(PeaError):
        ops.attention_fwd_regions(bfr(B, Sq, 256).cuda(), wide, wide, H, 2, torch.ones(1, 2, Sq).cuda())      # head_dim 128
    k = bfr(B, 154, 128, seed=2).cuda()
    with pytest.raises(PeaError):
        ops.attention_fwd_regions(q, k, k, H, 3, torch.ones(1, 3, Sq).cuda())                                 # 154 rows, 3 regions
    with pytest.raises(PeaError):
        ops.attention_fwd_regions(q, k, k, H, 2, torch.ones(1, 2, Sq - 1).cuda())


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
# measured on the CPU, oracle alone: with the context scaled by 5 two half-picture regions move eps by 0.305 against the plain
# 154-key attention (x 1: 0.028, x 4: 0.202), three column regions at 231 keys by 0.34
CTX_GAIN = 5.0


def _thirds(h, w):
    return _rects(3, h // 8, w // 8)


def _setup(B, L, hw=16):
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    ehs = (CTX_GAIN * ehs).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
    attach_regions(ref, (hw, hw))
    return cfg, ref, hip, (x, t, ehs, added), run_ref, run, plain_ref


def _check_eps(tag, got, want, stored, plain_ref):
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[{tag}] eps rel_l2={e:.3e} (against the oracle WITHOUT regions {e_plain:.3e}), bf16-storage floor {floor:.3e}, "
          f"ratio {e / floor:.2f}; the regions move the oracle's eps by {shift:.3f}")
    assert e < EPS_LIMIT and e < e_plain
    if floor >= FLOOR_DEGENERATE:
        assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)


def test_tiny_unet_two_regions(gpu):
    from oracle.bf16_store import bf16_storage
    from pea_diffusion_amd._lib import PeaError
    B, L = 2, 154
    cfg, ref, hip, _, run_ref, run, plain_ref = _setup(B, L)
    masks = half_masks(128, 128)                                     # 8 x the latent grid
    with torch.no_grad():
        assert torch.equal(run_ref(), plain_ref)                     # attached, nothing set: the plain attention
        set_regions(ref, masks)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
        set_regions(ref, masks, do_cfg=True)
        want_cfg = run_ref()
        with bf16_storage():
            stored_cfg = run_ref()
    # the oracle alone, before any GPU run: a UNet that ignores the regions cannot pass
    assert rel_l2(want, plain_ref) >= 10 * EPS_LIMIT and rel_l2(want_cfg, plain_ref) >= 10 * EPS_LIMIT
    assert rel_l2(want_cfg, want) >= 5 * EPS_LIMIT                  # measured 0.226: do_cfg is no detail either
    before = run()                                                   # the plain 154-key attention
    assert rel_l2(before, plain_ref) < EPS_LIMIT
    assert sorted(hip.ip_query_counts()) == [16, 64]
    hip.set_prompt_regions(masks)
    got = run()
    _check_eps("tiny unet + two regions", got, want, stored, plain_ref)
    assert rel_l2(got, want) < rel_l2(got, want_cfg)
    assert torch.equal(run(), got)                                   # bit-reproducible
    hip.set_prompt_regions(masks, do_cfg=True)
    got_cfg = run()
    _check_eps("tiny unet + two regions, do_cfg", got_cfg, want_cfg, stored_cfg, plain_ref)
    assert rel_l2(got_cfg, want_cfg) < rel_l2(got_cfg, want)
    assert torch.equal(got_cfg[1], got[1]) and not torch.equal(got_cfg[0], got[0])      # the samples do not mix
    # explicit weights of 1 are no weights
    hip.set_prompt_regions(masks, weights=[1.0, 1.0])
    assert torch.equal(run(), got)
    hip.clear_prompt_regions()
    assert torch.equal(run(), before)                                # the bits from before `set` come back
    with pytest.raises(PeaError, match="1..4 regions"):
        hip.set_prompt_regions([None] * 5)
    assert torch.equal(run(), before)


def test_tiny_unet_three_regions(gpu):
    from oracle.bf16_store import bf16_storage
    B, L = 2, 231
    cfg, ref, hip, _, run_ref, run, plain_ref = _setup(B, L)
    masks, weights = _thirds(128, 128), [1.0, 0.5, 2.0]
    with torch.no_grad():
        set_regions(ref, masks, weights)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
    assert rel_l2(want, plain_ref) >= 10 * EPS_LIMIT
    hip.set_prompt_regions(masks, weights)
    _check_eps("tiny unet + three regions", run(), want, stored, plain_ref)


def test_tiny_unet_regions_refusals(gpu):
    from ip_adapter_ref import make_image_proj
    from ip_multi_ref import attach_multi_ip, file_state_dict_of
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    from pea_diffusion_amd.unet import HipUNet
    masks = half_masks(128, 128)
    odd = HipUNet(pc.tiny_config(), 2, 16, 16, 155, needs_grad=False)
    with pytest.raises(PeaError, match="155 rows"):
        odd.set_prompt_regions(masks)                                # L = 155, R = 2
    long = HipUNet(pc.tiny_config(), 2, 16, 16, 194, needs_grad=False)
    with pytest.raises(PeaError, match="194 rows"):
        long.set_prompt_regions(masks)                               # 97 keys per region
    grad = HipUNet(pc.tiny_config(), 2, 16, 16, 154, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.set_prompt_regions(masks)
    # live image-prompt tokens: refused when the regions are set, and when the tokens arrive afterwards, at the forward (a context
    # that takes an adapter has at most 128 rows: two prompts of 64)
    B, L = 2, 128
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    before = run()
    ipref = UNet2DConditionRef(tiny_config())
    attach_multi_ip(ipref, (4,), (3,), (16, 16))
    hip.load_ip_adapter(file_state_dict_of(ipref, 0, make_image_proj(64, 128, 4, seed=4)))
    tok = torch.randn(B, 4, 128, generator=torch.Generator().manual_seed(7))
    hip.set_prompt_regions(masks)                                    # an adapter without tokens is no image prompt
    with_regions = run()
    assert not torch.equal(with_regions, before)
    hip.set_ip_tokens(tok)
    with pytest.raises(PeaError, match="live image prompts"):
        run()
    with pytest.raises(PeaError, match="live image prompts"):
        hip.set_prompt_regions(masks)
    hip.clear_ip_tokens()
    hip.set_prompt_regions(masks)
    assert torch.equal(run(), with_regions)
    # weights for one of the two query counts only: refused, with the missing count named
    hip.clear_prompt_regions()
    w64 = torch.full((1, 2, 64), 0.5).cuda()
    assert lib().pea_unet_set_prompt_regions(hip._h, 2, 64, ptr(w64), 1, stream_ptr()) == 0
    with pytest.raises(PeaError, match="16 queries"):
        run()
    assert lib().pea_unet_set_prompt_regions(hip._h, 3, 16, ptr(w64), 1, stream_ptr()) == -3       # another R while one is set
    assert lib().pea_unet_set_prompt_regions(hip._h, 2, 32, ptr(w64), 1, stream_ptr()) == -3       # no layer has 32 queries
    hip.clear_prompt_regions()
    assert torch.equal(run(), before)


def test_denoise_two_steps_with_regions(gpu):
    """two steps of sampler.denoise with DPMSolverMultistep on the regional context against the same loop on the oracle, within the
    bound tests/test_sampler_gpu.py uses for its own loop (3e-2 on the latents)"""
    from oracle.sampler_ref import DPMSolverMultistepRef, denoise_ref
    from pea_diffusion_amd.regional import compose_prompt_embeds
    from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
    B, L = 2, 154
    cfg, ref, hip, (x, _, _, added), _, _, _ = _setup(2 * B, L)
    g = torch.Generator().manual_seed(3)
    regions = [(CTX_GAIN * torch.randn(B, 77, cfg.cross_attention_dim, generator=g)).to(BF).float() for _ in range(2)]
    neg = (CTX_GAIN * torch.randn(B, 77, cfg.cross_attention_dim, generator=g)).to(BF).float()
    ehs = compose_prompt_embeds(regions, neg)
    assert tuple(ehs.shape) == (2 * B, L, cfg.cross_attention_dim)
    lat, masks = x[:B], half_masks(128, 128)
    kw = dict(num_inference_steps=2, guidance_scale=5.0)
    with torch.no_grad():
        plain = denoise_ref(lambda *a, **k: ref(*a, **k), DPMSolverMultistepRef(), lat.clone(), ehs, added, **kw)
        set_regions(ref, masks, do_cfg=True)
        want = denoise_ref(lambda *a, **k: ref(*a, **k), DPMSolverMultistepRef(), lat.clone(), ehs, added, **kw)
    hip.set_prompt_regions(masks, do_cfg=True)
    got = denoise(hip, DPMSolverMultistep(), lat.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()}, **kw)
    e, e_plain = rel_l2(got, want), rel_l2(got, plain)
    print(f"[denoise 2 steps, two regions, cfg 5.0] latents rel_l2={e:.3e} (against the oracle's loop WITHOUT regions {e_plain:.3e})")
    assert torch.isfinite(got).all() and e < 3e-2 and e < e_plain
