"""-m gpu: several image prompts in one fused attention launch (pea_op_attention_fwd_ipn) and in the UNet runtime
(pea_unet_ip_*_set / HipUNet's list forms), against the restatement of tests/ip_multi_ref.py.

Tolerance of the kernel's O: the two-term rule of tests/test_ip_adapter_gpu.py extended term by term -- an element may be off
by 2 x 2^-7 x (|o_text| + sum_j |w_j m_j| |o_j| + rms(O)), rel-L2 below 6e-3, the text lse at rtol 1e-3 / atol 2e-3.  The kernel
folds w_j m_j / sum_j into P before P's bf16 rounding: per set that is the one rounding of P the one-set kernel has, scaled."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from ip_adapter_ref import make_image_proj  # noqa: E402
from ip_multi_ref import (attach_multi_ip, combine, file_state_dict_of, grid_of, multi_ip_terms, rect_mask, sdpa,  # noqa: E402
                          set_multi_ip)
from test_ip_adapter_gpu import GAIN, _heads, _inputs, _tiny_ip_pair  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE  # noqa: E402

GRIDS = {64: (8, 8), 16: (4, 4), 128: (8, 16), 364: (14, 26), 260: (13, 20), 200: (10, 20), 300: (15, 20), 4096: (64, 64),
         256: (16, 16)}
WEIGHTS = [0.6, -1.0, 0.8, 0.5]                                     # per set; the second is negative wherever there are two


def _mask(Sq, variant):
    """[1, Sq] fp32: ip_adapter.downsample_mask of a binary rectangle -- with values below 0 and above 1"""
    from pea_diffusion_amd.ip_adapter import downsample_mask
    m = downsample_mask(rect_mask(*GRIDS[Sq], variant), *GRIDS[Sq])
    assert m.min() < 0 and m.max() > 1 and tuple(m.shape) == (1, Sq)
    return m


def _masks(mode, B, Sq, J):
    """none | shared: set 0 carries one mask for the whole batch | batch: every set carries a mask per sample, all different"""
    if mode == "none":
        return None
    if mode == "shared":
        return [_mask(Sq, 0)] + [None] * (J - 1)
    return [torch.cat([_mask(Sq, 2 * j + b) * (1.0 - 0.25 * b) for b in range(B)]) for j in range(J)]


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, Skv, sets, prescaled):
    """inputs (as test_ip_adapter_gpu._inputs makes them, the sets back to back) and every fp32 term, once per shape"""
    q, k, v, k2, v2 = _inputs(B, H, Sq, Skv, sum(sets), prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    o1, lse, terms = multi_ip_terms(qr, k.float(), v.float(), k2.float(), v2.float(), H, sets)
    return tuple(t.cuda() for t in (q, k, v, k2, v2)), o1, terms, lse


def close_terms(name, got, o1, terms, scales, masks):
    ref, mag = combine(o1, terms, scales, masks)
    got = got.detach().float().cpu()
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    err = (got - ref).abs()
    tol = 2.0 * 2.0 ** -7 * (mag + rms)
    bad = (err > tol).float().mean().item()
    e = rel_l2(got, ref)
    print(f"[{name}] max_abs={err.max().item():.3e} worst err/tol={(err / tol).max().item():.3f} rel_l2={e:.3e} rms={rms:.3e} frac_bad={bad:.2e}")
    assert torch.isfinite(got).all(), name
    assert bad == 0.0 and e < 6e-3, f"{name}: frac_bad={bad} rel_l2={e}"


def _run(ops, t, H, sets, scales, masks, mask_strides=None, **kw):
    q, k, v, k2, v2 = t
    dev = None if masks is None else [None if m is None else m.cuda() for m in masks]
    return ops.attention_fwd_ipn(q, k, v, k2, v2, H, sets, scales, dev, mask_strides=mask_strides, **kw)


SHAPES = [(1, 1, 64, 7, (1, 1)), (2, 2, 16, 16, (4, 4)), (1, 3, 128, 77, (4, 16)), (1, 2, 364, 77, (16, 16)),
          (1, 2, 260, 33, (5, 3, 7)), (1, 2, 200, 128, (4, 16, 4, 8)), (2, 2, 300, 77, (3, 29)), (2, 10, 4096, 77, (4, 16))]


@pytest.mark.parametrize("mode", ["none", "shared", "batch"])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv,sets", SHAPES)
def test_attention_fwd_ipn_vs_fp32(ops, B, H, Sq, Skv, sets, prescaled, mode):
    t, o1, terms, lref = _case(B, H, Sq, Skv, sets, prescaled)
    scales, masks = WEIGHTS[:len(sets)], _masks(mode, B, Sq, len(sets))
    strides = [Sq] * len(sets) if mode == "batch" else None         # per sample, also where B == 1
    o, lse = _run(ops, t, H, sets, scales, masks, strides, q_prescaled=prescaled, want_lse=True)
    tag = f"attn-ipn {mode} pre{int(prescaled)} B{B} H{H} Sq{Sq} Skv{Skv} sets{list(sets)}"
    close_terms(tag + " O", o, o1, terms, scales, masks)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv,sets", [(2, 2, 256, 77, (4, 16)), (1, 2, 364, 100, (5, 3, 7)), (2, 10, 4096, 77, (4, 16))])
def test_attention_fwd_ipn_exactness(ops, B, H, Sq, Skv, sets, prescaled):
    J, N = len(sets), sum(sets)
    t = q, k, v, k2, v2 = tuple(x.cuda() for x in _inputs(B, H, Sq, Skv, N, prescaled))
    w = WEIGHTS[:J]
    run = lambda scales, masks=None, tt=t: _run(ops, tt, H, sets, scales, masks, q_prescaled=prescaled, want_lse=True)
    # all weights 0: the plain kernel's O and lse, whatever (finite) image keys and masks there are
    plain, lse_p = ops.attention_fwd(q, k, v, H, q_prescaled=prescaled)
    o0, lse0 = run([0.0] * J, [_mask(Sq, 0)] * J, (q, k, v, k2 * 3, v2 * 100))
    assert torch.equal(o0, plain) and torch.equal(lse0, lse_p)
    # one set without a mask: attention_fwd_ip's O
    one = ops.attention_fwd_ipn(q, k, v, k2, v2, H, [N], [0.6], q_prescaled=prescaled)
    assert torch.equal(one, ops.attention_fwd_ip(q, k, v, k2, v2, H, 0.6, q_prescaled=prescaled))
    # two identical calls; a mask of ones is no mask
    a, lse_a = run(w)
    b, lse_b = run(w)
    assert torch.equal(a, b) and torch.equal(lse_a, lse_b) and not torch.equal(a, plain)
    ones = torch.ones(1, Sq)
    assert torch.equal(run(w, [ones] * J)[0], a)
    assert torch.equal(run(w, [None] * (J - 1) + [torch.ones(B, Sq)])[0], a)
    # a mask that is 0 on the first half of the queries of set j: those rows are the run with w_j = 0, the others the unmasked run
    half = torch.ones(1, Sq)
    half[:, :Sq // 2] = 0.0
    for j in range(J):
        got = run(w, [half if i == j else None for i in range(J)])[0]
        off = run([0.0 if i == j else w[i] for i in range(J)])[0]
        assert torch.equal(got[:, :Sq // 2], off[:, :Sq // 2]) and torch.equal(got[:, Sq // 2:], a[:, Sq // 2:]), j
        assert not torch.equal(off, a)


@pytest.mark.parametrize("spike_on", ["set0", "set1", "text"])
def test_attention_fwd_ipn_spiked_key(ops, spike_on):
    """the spike of test_attention_fwd_ip_spiked_key in set 0 of [4, 16], in set 1, in the text keys: the spiked softmax collapses
    to one value row, and since every set has its own maximum the other terms survive within the tolerance"""
    B, H, Sq, Skv, sets, w, j = 1, 2, 260, 77, (4, 16), [0.6, -1.0], 2
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)                                     # unit vector
    q = (4.0 * u + 0.5 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    k, v, k2, v2 = bfr(B, Skv, H * 64, seed=2), bfr(B, Skv, H * 64, seed=3), bfr(B, 20, H * 64, seed=5), bfr(B, 20, H * 64, seed=6)
    row = {"set0": j, "set1": 4 + j, "text": j}[spike_on]
    (k if spike_on == "text" else k2)[:, row] = (512.0 * u).repeat(H).to(BF)
    logits = lambda kk: _heads(q.float(), H) @ _heads(kk.float(), H).transpose(-1, -2) * 0.125
    parts = {"text": logits(k), "set0": logits(k2[:, :4]), "set1": logits(k2[:, 4:])}
    ls = parts.pop(spike_on)
    rest = torch.cat([ls[..., :j], ls[..., j + 1:]], -1)
    assert (ls[..., j] - rest.max(-1).values).min() > 100 and all(p.abs().max() < 30 for p in parts.values())
    o1, _, terms = multi_ip_terms(q.float(), k.float(), v.float(), k2.float(), v2.float(), H, sets)
    spiked = {"set0": terms[0], "set1": terms[1], "text": o1}[spike_on]
    value = (v if spike_on == "text" else v2)[:, row].float()[:, None, :]
    assert torch.equal(spiked, value.expand_as(spiked))             # the reference itself: exactly one key
    o = ops.attention_fwd_ipn(q.cuda(), k.cuda(), v.cuda(), k2.cuda(), v2.cuda(), H, sets, w)
    close_terms(f"attn-ipn spike in {spike_on}", o, o1, terms, w, None)


@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_fwd_ipn_kv_len_masks_text_keys_only(ops, prescaled):
    B, H, Sq, Skv, sets, w = 2, 2, 260, 77, (5, 3), [0.6, -1.0]
    q, k, v, k2, v2 = _inputs(B, H, Sq, Skv, sum(sets), prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    kv_len = [33, 9]
    o1, lref, terms = multi_ip_terms(qr, k.float(), v.float(), k2.float(), v2.float(), H, sets, kv_len)
    masks = _masks("shared", B, Sq, 2)
    o, lse = _run(ops, tuple(t.cuda() for t in (q, k, v, k2, v2)), H, sets, w, masks, q_prescaled=prescaled,
                  kv_len=torch.tensor(kv_len, dtype=torch.int32).cuda(), want_lse=True)
    close_terms(f"attn-ipn kv_len pre{int(prescaled)}", o, o1, terms, w, masks)
    close_f32("attn-ipn kv_len lse", lse, lref, rtol=1e-3, atol=2e-3)


def test_attention_fwd_ipn_refusals(ops):
    from pea_diffusion_amd._lib import PeaError, lib
    B, H, Sq, Skv = 1, 2, 128, 77
    q, k, v = bfr(B, Sq, 128).cuda(), bfr(B, Skv, 128).cuda(), bfr(B, Skv, 128).cuda()
    filled = []

    def refused(what, sets, k_=k, v_=v, ld2=128, **kw):
        """the library's own entry point on an O filled with 7.0, which a refusal before any launch leaves as it is"""
        import ctypes
        from pea_diffusion_amd._lib import ptr, stream_ptr
        n = max(sum(sets), 1)
        k2 = bfr(B, n, ld2, seed=5).cuda()
        o = torch.full((B, Sq, 128), 7.0, dtype=BF).cuda()
        m = torch.ones(B, Sq).cuda()
        st = ops.ip_sets(sets, [0.6] * len(sets), [m if kw.get("mstride") and i == 0 else None for i in range(len(sets))],
                         [kw.get("mstride", 0)] * len(sets))
        rc = lib().pea_op_attention_fwd_ipn(ptr(q), 128, ptr(k_), 128, ptr(v_), 128, ptr(k2), ld2, ptr(k2), ld2, ptr(o), 128, None,
                                            B, H, Sq, k_.shape[1], ctypes.byref(st), 0.125, 0, int(kw.get("causal", 0)), None,
                                            stream_ptr())
        torch.cuda.synchronize()
        msg = lib().pea_last_error().decode()
        print(f"[attn-ipn refused] {what}: rc={rc} {msg}")
        assert rc == -3 and msg and bool((o == 7.0).all()), what        # PEA_E_SHAPE
        filled.append(what)

    refused("J = 0", [])
    refused("J = 5", [2, 2, 2, 2, 2])
    refused("an empty set", [4, 0, 4])
    refused("sum n = 33", [16, 17])
    refused("causal", [4, 16], causal=1)
    refused("129 text keys", [4, 16], k_=bfr(B, 129, 128).cuda(), v_=bfr(B, 129, 128).cuda())
    refused("mask batch stride 1", [4, 16], mstride=1)
    refused("mask batch stride Sq - 1", [4, 16], mstride=Sq - 1)
    refused("ldk2 = 132", [4, 16], ld2=132)
    assert len(filled) == 9
    with pytest.raises(PeaError):
        ops.attention_fwd_ipn(q, k, v, bfr(B, 33, 128).cuda(), bfr(B, 33, 128).cuda(), H, [16, 17], [0.5, 0.5])


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
N_TOKS, SEEDS, SCALES = (4, 16), (3, 5), ({"down": 0.7, "up": 0.35, "mid": 0.7}, 0.4)


def _layer_scale_ref(name, spec):
    """the per-block dict restated on the oracle's module names"""
    return spec["down" if name.startswith("down_blocks") else "up" if name.startswith("up_blocks") else "mid"]


def _multi_setup(B, L=77):
    """a tiny pair, the oracle with two adapters attached, their files, tokens (bf16-representable) and the region mask"""
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    ehs = ehs.to(BF).float()
    toks = [torch.randn(B, n, 128, generator=torch.Generator().manual_seed(7 + j)).to(BF).float() for j, n in enumerate(N_TOKS)]
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
    layers = attach_multi_ip(ref, N_TOKS, SEEDS, (16, 16), gain=GAIN)
    files = [file_state_dict_of(ref, j, make_image_proj(64, 128, n, seed=4 + j)) for j, n in enumerate(N_TOKS)]
    mask = rect_mask(16, 16, 1)[None]                                # [1, 128, 128]: 8 x the latent grid
    return cfg, ref, hip, layers, files, toks, mask, run_ref, run, plain_ref


def test_tiny_unet_two_adapters_mask_and_block_scales(gpu):
    from oracle.bf16_store import bf16_storage
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    B = 2
    cfg, ref, hip, layers, files, toks, mask, run_ref, run, plain_ref = _multi_setup(B)
    before = run()
    per_layer = [[_layer_scale_ref(name, SCALES[0]) for name, _ in layers], SCALES[1]]
    with torch.no_grad():
        set_multi_ip(ref, toks, per_layer, [None, mask])
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
        set_multi_ip(ref, toks, per_layer, [None, None])
        no_mask = run_ref()
        set_multi_ip(ref, [toks[0], None], per_layer)
        first_only = run_ref()
    ads = hip.load_ip_adapter(files)
    assert [type(a) for a in ads] == [ipa.IPAdapter] * 2 and [a.n_tokens for a in ads] == list(N_TOKS)
    assert sorted(hip.ip_query_counts()) == [16, 64]
    assert torch.equal(run(), before)                                # loaded, no tokens: plain launches
    hip.set_ip_tokens(toks)
    hip.set_ip_adapter_scale(list(SCALES))
    hip.set_ip_adapter_masks([None, mask])
    got = run()
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    d_mask, d_second = rel_l2(no_mask, want), rel_l2(first_only, want)
    print(f"[tiny unet + two image prompts] eps rel_l2={e:.3e} (against the oracle WITHOUT prompts {e_plain:.3e}, without the mask "
          f"{rel_l2(got, no_mask):.3e}, without the second adapter {rel_l2(got, first_only):.3e}), bf16-storage floor {floor:.3e}, "
          f"ratio {e / floor:.2f}; the prompts move the oracle's eps by {shift:.3f}, the mask by {d_mask:.3f}, the second adapter by "
          f"{d_second:.3f}")
    assert shift >= 10 * EPS_LIMIT, shift                           # the oracle alone: a UNet that ignores the prompts cannot pass
    assert e < EPS_LIMIT and e < e_plain and e < rel_l2(got, no_mask) and e < rel_l2(got, first_only)
    if floor >= FLOOR_DEGENERATE:
        assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)
    assert torch.equal(run(), got)                                  # bit-reproducible
    # the packed buffer: adapter j in rows off_j .. off_j + n_j of every sample, block i of them tokens_j @ W_ji^T
    import ctypes
    kv = hip.ip_kv()
    cols = kv.shape[1]
    assert tuple(kv.shape) == (B * sum(N_TOKS), cols)
    kv = kv.view(B, sum(N_TOKS), cols)
    by_key = [{f"{name}.{nm}.weight": getattr(m, nm)[j].weight for name, m in layers for nm in ("to_k_ip", "to_v_ip")} for j in range(2)]
    name, off, n = ctypes.create_string_buffer(256), ctypes.c_int(), ctypes.c_int()
    i = 0
    while lib().pea_unet_stacked_layout(hip._h, 0, i, name, 256, ctypes.byref(off), ctypes.byref(n)) == 0:
        key = name.value.decode().replace(".to_k.weight", ".to_k_ip.weight").replace(".to_v.weight", ".to_v_ip.weight")
        for j, row0 in enumerate((0, N_TOKS[0])):
            want_kv = toks[j].cuda() @ by_key[j][key].T.cuda()
            got_kv = kv[:, row0:row0 + N_TOKS[j], off.value:off.value + n.value]
            rms = want_kv.pow(2).mean().sqrt()
            bad = ((got_kv - want_kv).abs() > 2.0 ** -7 * (want_kv.abs() + rms)).float().mean().item()    # close_bf16(ulps=1)
            assert bad == 0.0 and rel_l2(got_kv, want_kv) < 6e-3, (key, j, bad)
        i += 1
    assert i == 2 * len(layers)
    # all scales 0: the UNet without adapters, bit for bit; and back
    hip.set_ip_adapter_scale([0.0, 0.0])
    assert torch.equal(run(), before)
    hip.set_ip_adapter_scale(list(SCALES))
    assert torch.equal(run(), got)
    # clearing set 1: the bits of set 0 loaded alone (same per-block scales)
    hip.clear_ip_tokens(1)
    second_cleared = run()
    hip.set_ip_tokens([None, toks[1]])
    assert torch.equal(run(), got)
    # a mask for one of the two query counts only: refused, with the missing count named
    hip.set_ip_adapter_masks([None, None])
    m64 = ipa.downsample_mask(mask, 8, 8).cuda()
    assert lib().pea_unet_ip_set_mask(hip._h, 0, 64, ptr(m64), 1, stream_ptr()) == 0
    with pytest.raises(PeaError, match="16 queries"):
        run()
    hip.set_ip_adapter_masks([None, mask])
    assert torch.equal(run(), got)
    hip.unload_ip_adapter()
    assert torch.equal(run(), before)
    alone = hip.load_ip_adapter([files[0]])
    assert isinstance(alone, list) and len(alone) == 1
    hip.set_ip_tokens([toks[0]])
    hip.set_ip_adapter_scale([SCALES[0]])
    assert torch.equal(run(), second_cleared)
    # a list of one adapter is the scalar API, bit for bit
    hip.set_ip_adapter_scale([0.7])
    listed = run()
    hip.unload_ip_adapter()
    hip.load_ip_adapter(files[0])
    hip.set_ip_tokens(toks[0])
    hip.set_ip_adapter_scale(0.7)
    assert torch.equal(run(), listed) and not torch.equal(listed, before)
    # refusals of the list form
    with pytest.raises(PeaError, match="at most 32"):
        hip.load_ip_adapter([files[1], files[1], files[0]])
    with pytest.raises(PeaError):
        hip.load_ip_adapter([files[0]] * 5)


def test_base_and_plus_adapters_mixed(gpu):
    """a base file (4 tokens from image_embeds) and a plus file (4 tokens from the Resampler over hidden_states[-2]) in one
    load_ip_adapter call: tower -> both projections -> UNet, against the restatement fed the device's own tokens"""
    import resampler_ref as rr
    import vision_ref as vr
    from oracle.bf16_store import bf16_storage
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import ip_adapter as ipa
    from pea_diffusion_amd.vision import HipImageEncoder
    from test_model_gpu import make_pair
    B, L, NQ, scales = 1, 77, 4, [0.7, 0.5]
    vcfg = pc.tiny_vit_config()
    enc = HipImageEncoder(vcfg, B)
    enc.load_state_dict(vr.random_state_dict(vcfg, seed=3))
    px = torch.randn(B, 3, vcfg.image_size, vcfg.image_size, generator=torch.Generator().manual_seed(5))
    cfg, ref, hip = make_pair(tiny_config, 2 * B, L, False)
    for p in ref.parameters():
        p.requires_grad_(False)
    x, t, ehs, added = cond_inputs(cfg, 2 * B, L, 16)
    ehs = ehs.to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
    attach_multi_ip(ref, (4, NQ), (3, 5), (16, 16), gain=GAIN)
    base = file_state_dict_of(ref, 0, make_image_proj(vcfg.projection_dim, 128, 4, seed=4))
    plus = file_state_dict_of(ref, 1, rr.random_state_dict(rr.dims(vcfg.hidden_size, 128, 2, 2, NQ, 512, 128), seed=21))
    ads = hip.load_ip_adapter([ipa.IPAdapter(base, pc.tiny_config()), ipa.IPAdapterPlus(plus, pc.tiny_config())])
    assert [type(a) for a in ads] == [ipa.IPAdapter, ipa.IPAdapterPlus]
    toks = [ads[0].tokens(enc.encode(px.cuda())[2], do_cfg=True), ads[1].encode(enc, px.cuda(), do_cfg=True)]
    assert [tuple(t.shape) for t in toks] == [(2 * B, 4, 128), (2 * B, NQ, 128)] and all(torch.isfinite(t).all() for t in toks)
    hip.set_ip_tokens(toks)
    hip.set_ip_adapter_scale(scales)
    got = run()
    with torch.no_grad():
        set_multi_ip(ref, [t.cpu().to(BF).float() for t in toks], scales)        # the tokens enter the projection rounded to bf16
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[tiny unet + base and plus prompts] eps rel_l2={e:.3e} (against the oracle WITHOUT prompts {e_plain:.3e}), bf16-storage "
          f"floor {floor:.3e}, ratio {e / floor:.2f}; the prompts move the oracle's eps by {shift:.3f}")
    assert shift >= 10 * EPS_LIMIT, shift
    assert e < EPS_LIMIT and e < e_plain
    if floor >= FLOOR_DEGENERATE:
        assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)
