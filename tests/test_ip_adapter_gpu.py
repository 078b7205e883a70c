"""-m gpu: image prompts (IP-Adapter) on the HIP path -- the fused decoupled cross-attention kernel (pea_op_attention_fwd_ip)
against an fp32 reference, its exactness properties and refusals, the stacked to_k_ip | to_v_ip projection at full SDXL size,
and the tiny UNet, a 3-step loop and the tower -> adapter path against the restatement of tests/ip_adapter_ref.py.

Tolerance of the kernel's O: the attention-output rule of tests/test_ops_gpu.py (close_bf16 with 2 ulps: an element may be off by
2 x 2^-7 x (|ref| + rms)) applied per term of O = o_text + ip_scale * o_ip, i.e. 2 x 2^-7 x (|o_text| + |ip_scale| |o_ip| + rms(O));
that is the sum of what two separate launches may deviate by, with one output rounding fewer.  rel-L2 stays below 6e-3."""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
from ip_adapter_ref import attach_ip, file_state_dict, image_proj_ref, ip_tokens_ref, make_image_proj, set_ip  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, make_pair, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, close_bf16, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE, LOOP_FALLBACK  # noqa: E402


# ---------------------------------------------------------------------------------------------- kernel
def _heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2)


def _sdpa(q, k, v, H, kv_len=None):
    """fp32 attention per head, scale 1/8 -> (o [B,Sq,C], lse [B,H,Sq]); kv_len: keys >= kv_len[b] of sample b are cut"""
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * 0.125
    if kv_len is not None:
        cut = torch.arange(k.shape[1])[None, :] >= torch.as_tensor(kv_len)[:, None]
        s = s.masked_fill(cut[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ _heads(v, H)).transpose(1, 2).reshape(q.shape)
    return o, torch.logsumexp(s, -1)


def _inputs(B, H, Sq, Skv, N, prescaled):
    """q / k / v as tests/test_ops_gpu.py::test_attention_fwd_bwd makes them, image keys / values from two more seeds"""
    q, k, v = bfr(B, Sq, H * 64, seed=1), bfr(B, Skv, H * 64, seed=2), bfr(B, Skv, H * 64, seed=3)
    k2, v2 = bfr(B, N, H * 64, seed=5), bfr(B, N, H * 64, seed=6)
    if prescaled:
        q = (q.float() * ALPHA).to(BF)
    return q, k, v, k2, v2


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, Skv, N, prescaled):
    """inputs and the two fp32 terms, computed once per shape and shared by the ip_scale cases"""
    q, k, v, k2, v2 = _inputs(B, H, Sq, Skv, N, prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    o1, lse = _sdpa(qr, k.float(), v.float(), H)
    o2, _ = _sdpa(qr, k2.float(), v2.float(), H)
    return tuple(t.cuda() for t in (q, k, v, k2, v2)), o1, o2, lse


def close_two_terms(name, got, o1, o2, s):
    got, ref = got.detach().float().cpu(), o1 + s * o2
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    err = (got - ref).abs()
    tol = 2.0 * 2.0 ** -7 * (o1.abs() + abs(s) * o2.abs() + rms)
    bad = (err > tol).float().mean().item()
    e = rel_l2(got, ref)
    print(f"[{name}] max_abs={err.max().item():.3e} worst err/tol={(err / tol).max().item():.3f} rel_l2={e:.3e} rms={rms:.3e} frac_bad={bad:.2e}")
    assert torch.isfinite(got).all(), name
    assert bad == 0.0 and e < 6e-3, f"{name}: frac_bad={bad} rel_l2={e}"


SHAPES = [(1, 1, 64, 7, 1), (2, 2, 16, 16, 4), (1, 3, 128, 77, 4), (1, 2, 364, 77, 16), (1, 2, 260, 33, 5), (1, 2, 512, 100, 17),
          (1, 2, 640, 128, 32), (2, 10, 4096, 77, 4)]          # the last: 640 units -> two per workgroup, the next-unit Q prefetch


@pytest.mark.parametrize("ip_scale", [0.6, -1.0])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv,N", SHAPES)
def test_attention_fwd_ip_vs_fp32(ops, B, H, Sq, Skv, N, prescaled, ip_scale):
    (q, k, v, k2, v2), o1, o2, lref = _case(B, H, Sq, Skv, N, prescaled)
    o, lse = ops.attention_fwd_ip(q, k, v, k2, v2, H, ip_scale, q_prescaled=prescaled, want_lse=True)
    tag = f"attn-ip pre{int(prescaled)} s{ip_scale} B{B} H{H} Sq{Sq} Skv{Skv} N{N}"
    close_two_terms(tag + " O", o, o1, o2, ip_scale)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)      # the text softmax's, as the plain kernel writes it


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv,N", [(2, 2, 256, 77, 4), (1, 2, 364, 100, 16), (2, 10, 4096, 77, 4)])
def test_attention_fwd_ip_exactness(ops, B, H, Sq, Skv, N, prescaled):
    """weight 0: the plain kernel's O and lse bit for bit, whatever (finite) image keys there are; two runs agree exactly"""
    q, k, v, k2, v2 = (t.cuda() for t in _inputs(B, H, Sq, Skv, N, prescaled))
    plain, lse_p = ops.attention_fwd(q, k, v, H, q_prescaled=prescaled)
    o0, lse0 = ops.attention_fwd_ip(q, k, v, k2 * 3, v2 * 100, H, 0.0, q_prescaled=prescaled, want_lse=True)
    assert torch.equal(o0, plain) and torch.equal(lse0, lse_p)
    a = ops.attention_fwd_ip(q, k, v, k2, v2, H, 0.6, q_prescaled=prescaled)
    b = ops.attention_fwd_ip(q, k, v, k2, v2, H, 0.6, q_prescaled=prescaled)
    assert torch.equal(a, b) and not torch.equal(a, plain)


@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_fwd_ip_kv_len_masks_text_keys_only(ops, prescaled):
    B, H, Sq, Skv, N = 2, 2, 260, 77, 5
    q, k, v, k2, v2 = _inputs(B, H, Sq, Skv, N, prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    kv_len = [33, 9]
    o1, lref = _sdpa(qr, k.float(), v.float(), H, kv_len)           # text keys cut per sample ...
    o2, _ = _sdpa(qr, k2.float(), v2.float(), H)                    # ... every image key kept
    o, lse = ops.attention_fwd_ip(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), H, 0.6, q_prescaled=prescaled,
                                  kv_len=torch.tensor(kv_len, dtype=torch.int32).cuda(), want_lse=True)
    close_two_terms(f"attn-ip kv_len pre{int(prescaled)}", o, o1, o2, 0.6)
    close_f32("attn-ip kv_len lse", lse, lref, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("spike_on", ["image", "text"])
def test_attention_fwd_ip_spiked_key(ops, spike_on):
    """one key of one set aligned with every query and scaled until its logit leads its set by more than 100, the other set
    ordinary: each softmax has its own maximum, so the other set's term survives -- O = o_text + s * v_ip[j] (or the mirror)"""
    B, H, Sq, Skv, N, s, j = 1, 2, 260, 77, 4, 0.6, 2
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)                                     # unit vector
    q = (4.0 * u + 0.5 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    k, v, k2, v2 = bfr(B, Skv, H * 64, seed=2), bfr(B, Skv, H * 64, seed=3), bfr(B, N, H * 64, seed=5), bfr(B, N, H * 64, seed=6)
    (k2 if spike_on == "image" else k)[:, j] = (512.0 * u).repeat(H).to(BF)
    logits = lambda kk: _heads(q.float(), H) @ _heads(kk.float(), H).transpose(-1, -2) * 0.125
    ls = logits(k2 if spike_on == "image" else k)
    rest = torch.cat([ls[..., :j], ls[..., j + 1:]], -1)
    assert (ls[..., j] - rest.max(-1).values).min() > 100 and logits(k if spike_on == "image" else k2).abs().max() < 30
    o1, _ = _sdpa(q.float(), k.float(), v.float(), H)
    o2, _ = _sdpa(q.float(), k2.float(), v2.float(), H)
    if spike_on == "image":
        assert torch.equal(o2, v2[:, j].float()[:, None, :].expand_as(o2))      # the reference itself: exactly one key
    else:
        assert torch.equal(o1, v[:, j].float()[:, None, :].expand_as(o1))
    o = ops.attention_fwd_ip(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), H, s)
    close_two_terms(f"attn-ip spike on {spike_on} key", o, o1, o2, s)


def test_attention_fwd_ip_refusals(ops):
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    B, H, Sq, Skv = 1, 2, 128, 77
    q, k, v = bfr(B, Sq, 128).cuda(), bfr(B, Skv, 128).cuda(), bfr(B, Skv, 128).cuda()
    kv = lambda n: (bfr(B, n, 128, seed=5).cuda(), bfr(B, n, 128, seed=6).cuda())
    for what, call in (("N = 0", lambda: ops.attention_fwd_ip(q, k, v, *kv(0), H, 0.6)),
                       ("N = 33", lambda: ops.attention_fwd_ip(q, k, v, *kv(33), H, 0.6)),
                       ("causal", lambda: ops.attention_fwd_ip(q, k, v, *kv(4), H, 0.6, causal=True)),
                       ("129 text keys", lambda: ops.attention_fwd_ip(q, bfr(B, 129, 128).cuda(), bfr(B, 129, 128).cuda(), *kv(4), H, 0.6))):
        with pytest.raises(PeaError):
            call()
        print(f"[attn-ip refused] {what}: {lib().pea_last_error().decode()}")
    k2 = bfr(B, 4, 132, seed=5).cuda()                               # rows 132 elements apart: not a multiple of 8
    o = torch.full((B, Sq, 128), 7.0, dtype=BF).cuda()
    rc = lib().pea_op_attention_fwd_ip(ptr(q), 128, ptr(k), 128, ptr(v), 128, ptr(k2), 132, ptr(k2), 136, ptr(o), 128, None, B, H, Sq,
                                       Skv, 4, 0.125, 0.6, 0, 0, None, stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b"multiples of 8" in lib().pea_last_error() and bool((o == 7.0).all())     # refused before any launch


@pytest.mark.parametrize("R,C", [(1, 64), (3, 100), (8, 2048), (13, 1000), (64, 128)])
def test_layernorm_fwd_f32(ops, R, C):
    """the fp32 LayerNorm of the image projection against F.layer_norm in float64: rows not a multiple of the 4 a workgroup
    takes, widths not a multiple of the 64 lanes; an fp32 result, rtol 1e-3 / atol 1e-4"""
    g = torch.Generator().manual_seed(R * 10000 + C)
    x = torch.randn(R, C, generator=g) * 3.0 + 1.5
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    y, stats = ops.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5)
    assert stats is None and y.dtype == torch.float32 and tuple(y.shape) == (R, C)
    want = torch.nn.functional.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    close_f32(f"layernorm fp32 {R}x{C}", y, want.float(), rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------------------------------------- the stacked projection, SDXL
def test_ip_stack_mapping_full_size(gpu):
    """every one of the 140 to_k_ip / to_v_ip members of the SDXL stack lands in the column block the attention of its own layer
    reads: block i of the image K|V equals tokens @ W_i^T (W rounded to bf16), held to the rule for bf16-stored GEMM results.
    The file is built from `ip_adapter.layer_keys`, so this test pins the MAPPING from a file entry to its column block, not the
    numbering itself: that is pinned by the anchors and the oracle's module order in tests/test_ip_adapter_cpu.py."""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd._lib import lib
    from pea_diffusion_amd.unet import HipUNet
    cfg, N = pc.sdxl_config(), 4
    hip = HipUNet(cfg, 2, 16, 16, 77)
    hip.init_random(1)
    g = torch.Generator(device="cuda").manual_seed(2)
    sd = {"image_proj": make_image_proj(64, 2048, N, seed=4), "ip_adapter": {}}
    by_key = {}
    for (idx, pfx), (_, C) in zip(ipa.layer_keys(cfg), ipa._cross_layers(cfg)):
        for nm in ("to_k_ip", "to_v_ip"):
            w = (torch.randn(C, 2048, generator=g, device="cuda") * 2048 ** -0.5).to(BF).float()
            sd["ip_adapter"][f"{idx}.{nm}.weight"] = by_key[f"{pfx}.{nm}.weight"] = w
    hip.load_ip_adapter(sd)
    tok = torch.randn(2, N, 2048, generator=torch.Generator().manual_seed(3)).to(BF)
    hip.set_ip_tokens(tok.float())
    kv = hip.ip_kv()
    assert tuple(kv.shape) == (2 * N, 166400)
    name, off, n = ctypes.create_string_buffer(256), ctypes.c_int(), ctypes.c_int()
    i, seen, covered = 0, set(), 0
    while lib().pea_unet_stacked_layout(hip._h, 0, i, name, 256, ctypes.byref(off), ctypes.byref(n)) == 0:
        key = name.value.decode().replace(".to_k.weight", ".to_k_ip.weight").replace(".to_v.weight", ".to_v_ip.weight")
        want = tok.cuda().float().view(2 * N, 2048) @ by_key[key].T
        got = kv[:, off.value:off.value + n.value]
        assert got.shape == want.shape, key
        rms = want.pow(2).mean().sqrt()
        bad = ((got - want).abs() > 2.0 ** -7 * (want.abs() + rms)).float().mean().item()     # close_bf16(ulps=1), on the device
        assert bad == 0.0 and rel_l2(got, want) < 6e-3, (key, bad)
        seen.add(key)
        covered += n.value
        i += 1
    assert i == 140 and seen == set(by_key) and covered == 166400


# ---------------------------------------------------------------------------------------------- tiny UNet
N_TOK, GAIN = 4, 4.0       # measured on the CPU, oracle alone: torch's Linear init x 4 moves eps by 0.31 at scale 0.7 (x 1: 0.098)


def _tiny_ip_pair(B, L=77):
    from oracle.unet_ref import tiny_config
    cfg, ref, hip = make_pair(tiny_config, B, L, False)
    for p in ref.parameters():
        p.requires_grad_(False)
    return cfg, ref, hip


def test_tiny_unet_with_image_prompt(gpu):
    from oracle.bf16_store import bf16_storage
    from oracle.unet_ref import tiny15_config, tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    B, L, scale = 2, 77, 0.7
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    ehs = ehs.to(BF).float()
    tok = torch.randn(B, N_TOK, 128, generator=torch.Generator().manual_seed(7)).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda u=hip: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    before = run()
    table = hip.weight_table()
    with torch.no_grad():
        plain_ref = run_ref()
        attach_ip(ref, N_TOK, seed=3, gain=GAIN)
        set_ip(ref, tok, scale)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
    sd = file_state_dict(ref, make_image_proj(64, 128, N_TOK, seed=4))
    ad = hip.load_ip_adapter(sd)
    assert isinstance(ad, ipa.IPAdapter) and hip.weight_table() == table             # the UNet's own weights are what they were
    assert torch.equal(run(), before)                                               # loaded, no tokens: plain launches
    hip.set_ip_tokens(tok.cuda())
    hip.set_ip_adapter_scale(scale)
    got = run()
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[tiny unet + image prompt] eps rel_l2={e:.3e} (against the oracle WITHOUT the prompt {e_plain:.3e}), bf16-storage floor "
          f"{floor:.3e}, ratio {e / floor:.2f}; the prompt moves the oracle's eps by {shift:.3f}")
    assert shift >= 10 * EPS_LIMIT, shift                          # the oracle alone: a UNet that ignores the prompt cannot pass
    assert e < EPS_LIMIT and e < e_plain
    if floor >= FLOOR_DEGENERATE:
        assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)
    assert torch.equal(run(), got)                                  # bit-reproducible
    # weight 0, tokens cleared, adapter unloaded: each the context before load_ip_adapter, bit for bit
    hip.set_ip_adapter_scale(0.0)
    assert torch.equal(run(), before)
    hip.set_ip_adapter_scale(scale)
    assert torch.equal(run(), got)
    hip.clear_ip_tokens()
    assert torch.equal(run(), before)
    hip.set_ip_tokens(tok.cuda())
    hip.release_activations()                                       # the image K|V are not part of the activation arena
    assert torch.equal(run(), got)
    hip.unload_ip_adapter()
    assert torch.equal(run(), before)
    with pytest.raises(PeaError):
        hip.set_ip_tokens(tok.cuda())                               # nothing loaded
    hip.load_ip_adapter(ad)
    with pytest.raises(PeaError):
        hip.set_ip_tokens(tok[:, :3].cuda())
    # refusals: padded heads, a context with gradient support, a layer left out
    from ip_adapter_ref import ip_layers
    from oracle.unet_ref import UNet2DConditionRef
    ref15 = UNet2DConditionRef(tiny15_config())
    attach_ip(ref15, N_TOK, seed=3)
    with pytest.raises(PeaError, match="padded heads"):
        HipUNet(pc.tiny15_config(), B, 16, 16, L).load_ip_adapter(file_state_dict(ref15, make_image_proj(64, 128, N_TOK, seed=4)))
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        HipUNet(pc.tiny_config(), B, 16, 16, 12, needs_grad=True).load_ip_adapter(sd)
    with pytest.raises(PeaError, match="context length"):
        HipUNet(pc.tiny_config(), B, 16, 16, 160).load_ip_adapter(sd)
    assert len(ip_layers(ref)) == len(ipa.layer_keys(pc.tiny_config()))


def test_image_prompt_loop_tiny_vs_oracle(gpu):
    """3 DPM-Solver steps at guidance 5 (UNet batch 2B, the unconditional half first) with the tokens of IPAdapter.tokens(...,
    do_cfg=True), against the restated loop around the fp32 oracle with the restated tokens"""
    from oracle.bf16_store import bf16_storage
    from oracle.sampler_ref import DPMSolverMultistepRef, denoise_ref
    from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
    B, L, n, g, scale = 2, 77, 3, 5.0, 0.7
    cfg, ref, hip = _tiny_ip_pair(2 * B, L)
    x, _, ehs, added = cond_inputs(cfg, 2 * B, L, 16)
    x, ehs = x[:B], ehs.to(BF).float()
    proj = make_image_proj(64, 128, N_TOK, seed=4)
    embeds = torch.randn(B, 64, generator=torch.Generator().manual_seed(8))
    attach_ip(ref, N_TOK, seed=3, gain=GAIN)
    ad = hip.load_ip_adapter(file_state_dict(ref, proj))
    tok = ad.tokens(embeds.cuda(), do_cfg=True)
    tok_ref = ip_tokens_ref(proj, embeds, do_cfg=True).float()
    assert tuple(tok.shape) == (2 * B, N_TOK, 128)
    torch.testing.assert_close(tok.cpu(), tok_ref, rtol=1e-3, atol=1e-4)
    hip.set_ip_tokens(tok)
    hip.set_ip_adapter_scale(scale)
    loop = lambda: denoise_ref(lambda *a, **k: ref(*a, **k), DPMSolverMultistepRef(), x.clone(), ehs, added, n, guidance_scale=g)
    with torch.no_grad():
        set_ip(ref, None)
        without = loop()
        set_ip(ref, tok_ref.to(BF).float(), scale)                 # the tokens enter the HIP projection rounded to bf16
        want = loop()
        with bf16_storage():
            stored = loop()
    floor = rel_l2(stored, want)
    degenerate = floor < FLOOR_DEGENERATE
    limit = LOOP_FALLBACK if degenerate else STORAGE_FLOOR_FACTOR * floor
    run = lambda: denoise(hip, DPMSolverMultistep(), x.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()},
                          num_inference_steps=n, guidance_scale=g)
    got = run()
    e = rel_l2(got, want)
    print(f"[image prompt loop tiny, {n} DPM steps, guidance {g}] latents rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio "
          f"{e / max(floor, 1e-30):.2f}, limit {limit:.3e}; the prompt moves the oracle's latents by {rel_l2(want, without):.3f}")
    assert torch.isfinite(got).all() and e <= limit and e < rel_l2(got, without)
    assert torch.equal(run(), got)


def test_tower_to_adapter_tokens(gpu):
    """image -> tiny ViT tower -> image_embeds -> IPAdapter.tokens against the restated projection of the same embeddings: an
    fp32 result (bf16 GEMM operands, fp32 accumulator, fp32 LayerNorm), rtol 1e-3 / atol 1e-4"""
    import vision_ref as vr
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd.vision import HipImageEncoder
    vcfg = pc.tiny_vit_config()
    enc = HipImageEncoder(vcfg, 2)
    enc.load_state_dict(vr.random_state_dict(vcfg, seed=3))
    px = torch.randn(2, 3, vcfg.image_size, vcfg.image_size, generator=torch.Generator().manual_seed(5))
    embeds = enc.encode(px.cuda())[2]
    assert tuple(embeds.shape) == (2, vcfg.projection_dim) and torch.isfinite(embeds).all()
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    ref = UNet2DConditionRef(tiny_config())
    attach_ip(ref, 16, seed=3)
    proj = make_image_proj(vcfg.projection_dim, 128, 16, seed=4)
    ad = ipa.IPAdapter(file_state_dict(ref, proj), pc.tiny_config())
    for do_cfg in (False, True):
        got = ad.tokens(embeds, do_cfg=do_cfg)
        want = ip_tokens_ref(proj, embeds.cpu(), do_cfg=do_cfg).float()
        assert got.dtype == torch.float32 and tuple(got.shape) == ((4 if do_cfg else 2), 16, 128)
        close_f32(f"tower -> adapter tokens, do_cfg={do_cfg}", got, want, rtol=1e-3, atol=1e-4)
    assert torch.equal(got[0], got[1])                              # the unconditional half: one zero embedding, twice
