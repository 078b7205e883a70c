"""-m gpu: prompt-to-prompt editing -- the fused edit attention (pea_op_attention_fwd_edit) against an fp32 restatement, its
exactness properties, and the UNet runtime (HipUNet.set_prompt_edit) against the restatement of tests/p2p_ref.py on the oracle.

Tolerance of the kernel's O: the rule of tests/test_ip_multi_gpu.py (close_terms) -- an element may be off by
2 x 2^-7 x (mag + rms(O)), rel-L2 below 6e-3, with mag = sum_j (|c_j| (P0 |Mt|^T)_j + |d_j| P1_j) |V_j|.  It applies because the
kernel has three bf16 roundings of at most 2^-8 each (P0 un-normalised, the mixture, O): 3/4 of the rule's 2^-6."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from p2p_ref import attach_edit, edit_reference  # noqa: E402
from test_ip_adapter_gpu import _inputs, _tiny_ip_pair  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE  # noqa: E402


def _default_src(B):
    return [-1 if b % 2 == 0 else b - 1 for b in range(B)]          # [-1, 0] and [-1, 0, -1, 2]


def _tables(mode, B, L, src):
    """-> Mt bf16 [B, L, ldm], c, d fp32 [B, L] through the package's own builders (tests/test_p2p_cpu.py checks those);
    replace: a soft mapper with rows of 1/2 and a shift | gather: a one-hot gather with 0 / 1 alphas | reweight: factors 4
    and -1 on the identity | partial: the soft mapper with the window of every second key already over (c = 0, d = 1)"""
    from pea_diffusion_amd.prompt2prompt import equalizer, fold, gather_mapper, refine_mapper, replace_mapper
    w = torch.ones(1, L, dtype=torch.float64)
    alphas = eq = None
    if mode in ("replace", "partial"):
        M = replace_mapper(L, [((1, 2), (1, 3))]) if L >= 4 else torch.eye(L, dtype=torch.float64)
        if mode == "partial":
            w[:, 1::2] = 0.0
    elif mode == "gather":
        ids = list(range(100, 100 + max(L - 2, 1)))
        gather, alphas = refine_mapper(ids, ids[:2] + [7, 8][:max(L - len(ids), 0)] + ids[2:], L)
        M = gather_mapper(gather)
    else:
        M = torch.eye(L, dtype=torch.float64)
        eq = equalizer(L, {min(1, L - 1): 4.0, L // 2: -1.0} if L > 1 else {0: 4.0})
    c1, d1 = fold(w, alphas, eq)
    ldm = (L + 7) // 8 * 8
    Mt = torch.zeros(B, L, ldm)
    c, d = torch.zeros(B, L), torch.ones(B, L)
    for b in range(B):
        if src[b] >= 0 and src[b] != b:                            # (a sample that names itself is its own source: not edited)
            Mt[b, :, :L] = M.t().float() * (1.0 if b < 2 else 0.75)  # later samples: another table
            c[b], d[b] = c1[0].float(), d1[0].float()
    return Mt.to(BF), c, d


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, L, prescaled):
    q, k, v, _, _ = _inputs(B, H, Sq, L, 1, prescaled)
    qr = q.float() / ALPHA if prescaled else q.float()
    return tuple(t.cuda() for t in (q, k, v)), (qr, k.float(), v.float())


@functools.lru_cache(maxsize=None)
def _reference(B, H, Sq, L, src, mode, prescaled):
    """the fp32 restatement, once per case (a prescaled q is rounded to bf16 once more: its own reference)"""
    _, (qr, k, v) = _case(B, H, Sq, L, prescaled)
    Mt, c, d = _tables(mode, B, L, src)
    return edit_reference(qr, k, v, H, src, Mt.float()[:, :, :L], c, d)


def _close(name, got, ref, mag):
    """close_terms of tests/test_ip_multi_gpu.py with the edit's magnitude"""
    got = got.detach().float().cpu()
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    err = (got - ref).abs()
    tol = 2.0 * 2.0 ** -7 * (mag + rms)
    bad = (err > tol).float().mean().item()
    e = rel_l2(got, ref)
    print(f"[{name}] max_abs={err.max().item():.3e} worst err/tol={(err / tol).max().item():.3f} rel_l2={e:.3e} rms={rms:.3e} frac_bad={bad:.2e}")
    assert torch.isfinite(got).all(), name
    assert bad == 0.0 and e < 6e-3, f"{name}: frac_bad={bad} rel_l2={e}"


SHAPES = [(2, 1, 1, 1, None), (2, 2, 16, 16, None), (2, 2, 200, 32, None), (2, 3, 128, 77, None), (3, 2, 364, 77, (-1, 0, 0)),
          (4, 2, 260, 33, (-1, -1, 2, 2)), (2, 2, 300, 96, None), (4, 10, 4096, 77, None)]     # the last: five units per workgroup


@pytest.mark.parametrize("mode", ["replace", "gather", "reweight", "partial"])
@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,L,src", SHAPES)
def test_attention_fwd_edit_vs_fp32(ops, B, H, Sq, L, src, prescaled, mode):
    src = tuple(_default_src(B)) if src is None else src
    (q, k, v), _ = _case(B, H, Sq, L, prescaled)
    Mt, c, d = _tables(mode, B, L, src)
    o = ops.attention_fwd_edit(q, k, v, H, src, Mt.cuda(), c.cuda(), d.cuda(), q_prescaled=prescaled)
    ref, mag = _reference(B, H, Sq, L, src, mode, prescaled)
    _close(f"attn-edit {mode} pre{int(prescaled)} B{B} H{H} Sq{Sq} L{L} src{list(src)}", o, ref, mag)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,L,src", [(2, 3, 128, 77, (-1, 0)), (4, 2, 260, 33, (-1, -1, 2, 2)), (2, 2, 300, 96, (-1, 0)),
                                          (4, 10, 4096, 77, (-1, 0, -1, 2))])
def test_attention_fwd_edit_exactness(ops, B, H, Sq, L, src, prescaled):
    """at 128 queries and more pea_op_attention_fwd is xattn_fwd_kernel, whose bits the edit kernel reproduces"""
    (q, k, v), _ = _case(B, H, Sq, L, prescaled)
    plain, _ = ops.attention_fwd(q, k, v, H, q_prescaled=prescaled)
    Mt, c, d = (t.cuda() for t in _tables("replace", B, L, src))
    run = lambda Mt=Mt, c=c, d=d: ops.attention_fwd_edit(q, k, v, H, src, Mt, c, d, q_prescaled=prescaled)
    # c = 0, d = 1 on every sample: the plain launch's bits on the whole batch, the edited samples included
    assert torch.equal(run(c=torch.zeros_like(c), d=torch.ones_like(d)), plain)
    # unedited samples: the plain launch's bits whatever the tables hold -- NaN in their rows is never read
    un = [b for b in range(B) if src[b] < 0 or src[b] == b]
    ed = [b for b in range(B) if b not in un]
    Mn, cn, dn = Mt.clone(), c.clone(), d.clone()
    Mn[un], cn[un], dn[un] = float("nan"), float("nan"), float("nan")
    a = run()
    an = run(Mn, cn, dn)
    assert torch.equal(a[un], plain[un]) and torch.equal(an, a) and torch.isfinite(an.float()).all()
    assert not torch.equal(a[ed], plain[ed])
    # nobody edited: the tables may be absent
    none = ops.attention_fwd_edit(q, k, v, H, [-1] * B, None, None, None, q_prescaled=prescaled)
    assert torch.equal(none, plain)
    # two runs, the same bits
    assert torch.equal(run(), a)


def test_attention_fwd_edit_small_query_counts_keep_unedited_bits(ops):
    """below 128 queries pea_op_attention_fwd is another kernel: it writes the unedited samples, the edit kernel the edited ones"""
    for Sq, L in ((1, 1), (16, 16), (64, 77)):
        (q, k, v), _ = _case(2, 2, Sq, L, False)
        plain, _ = ops.attention_fwd(q, k, v, 2)
        Mt, c, d = (t.cuda() for t in _tables("reweight", 2, L, (-1, 0)))
        o = ops.attention_fwd_edit(q, k, v, 2, [-1, 0], Mt, c, d)
        assert torch.equal(o[0], plain[0]) and not torch.equal(o[1], plain[1])


def test_attention_fwd_edit_spiked_source_key(ops):
    """a spike of +60 and more on one source key: the source's softmax collapses
    to that key, and since each softmax has its own maximum the target's own term survives within the tolerance"""
    B, H, Sq, L, j = 2, 2, 260, 77, 5
    g = torch.Generator().manual_seed(9)
    u = torch.full((64,), 0.125)                                     # unit vector
    q = (4.0 * u + 0.5 * torch.randn(B, Sq, H, 64, generator=g)).reshape(B, Sq, H * 64).to(BF)
    k, v = bfr(B, L, H * 64, seed=2), bfr(B, L, H * 64, seed=3)
    k[0, j] = (160.0 * u).repeat(H).to(BF)                           # q . k = 640 +- 80, x 1/8: 60 and more above the rest
    s0 = (q[0].float().view(Sq, H, 64).transpose(0, 1) @ k[0].float().view(L, H, 64).transpose(0, 1).transpose(-1, -2)) * 0.125
    rest = torch.cat([s0[..., :j], s0[..., j + 1:]], -1)
    assert (s0[..., j] - rest.max(-1).values).min() > 40
    src = (-1, 0)
    Mt, c, d = _tables("partial", B, L, src)
    ref, mag = edit_reference(q.float(), k.float(), v.float(), H, src, Mt.float()[:, :, :L], c, d)
    o = ops.attention_fwd_edit(q.cuda(), k.cuda(), v.cuda(), H, src, Mt.cuda(), c.cuda(), d.cuda())
    _close("attn-edit spike on source key 5", o, ref, mag)


def test_attention_fwd_edit_refusals(ops):
    """the list of tests/test_p2p_cpu.py on the device: an O filled with 7.0 stays as it is"""
    from pea_diffusion_amd._lib import PeaError, lib, ptr, stream_ptr
    import ctypes
    B, H, Sq = 2, 2, 128
    q = bfr(B, Sq, 128).cuda()
    n = 0

    def refused(what, L=77, ldk=128, ldm=80, src=(-1, 0), B=B, table=True):
        nonlocal n
        k = bfr(max(B, 1), max(L, 1), max(ldk, 128), seed=2).cuda()
        o = torch.full((max(B, 1), Sq, 128), 7.0, dtype=BF).cuda()
        Mt = torch.zeros(max(B, 1), max(L, 1), max(ldm, 8), dtype=BF).cuda()
        cd = torch.ones(max(B, 1), max(L, 1)).cuda()
        hs = (ctypes.c_int * 40)(*(list(src) + [-1] * (40 - len(src))))
        rc = lib().pea_op_attention_fwd_edit(ptr(q), 128, ptr(k), ldk, ptr(k), ldk, ptr(o), 128, B, H, Sq, L, hs,
                                             ptr(Mt) if table else None, ldm, ptr(cd), ptr(cd), 0.125, 0, stream_ptr())
        torch.cuda.synchronize()
        msg = lib().pea_last_error().decode()
        print(f"[attn-edit refused] {what}: rc={rc} {msg}")
        assert rc == -3 and what in msg and bool((o == 7.0).all()), what          # PEA_E_SHAPE
        n += 1

    refused("out of range", src=(-1, 2))
    refused("itself edited", src=(1, 0))
    refused("at most 32 samples", B=33)
    refused("1..96 keys", L=97, ldm=104)
    refused("leading dimension", ldk=132)
    refused("leading dimension", ldm=84)
    refused("empty problem", L=0)
    refused("null table", table=False)
    assert n == 8
    wide = bfr(B, 77, 256).cuda()
    with pytest.raises(PeaError, match="head_dim"):
        ops.attention_fwd_edit(bfr(B, Sq, 256).cuda(), wide, wide, H, [-1, 0], None, None, None)


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
CTX_GAIN = 5.0                                                       # as tests/test_attn_maps_gpu.py: unscaled, the storage floor is degenerate
SRC_IDS = list(range(200, 230))
TGT_IDS = SRC_IDS[:4] + [901, 902] + SRC_IDS[4:11] + [903] + SRC_IDS[11:]


def _edit(L, T, smt, do_cfg=False, cross=0.5, self_steps=0.5):
    from pea_diffusion_amd.prompt2prompt import PromptEdit, equalizer, refine_mapper
    ed = dict(source=0, refine=refine_mapper(SRC_IDS, TGT_IDS, L), equalizer=equalizer(L, {2: 2.0}))
    return PromptEdit.compose(L, T, [None, ed], cross_replace_steps=cross, self_replace_steps=self_steps, self_max_tokens=smt, do_cfg=do_cfg)


def _setup(B, L=77, hw=16):
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    x, t = x[:1].expand(B, -1, -1, -1).contiguous(), t[1:2].expand(B).contiguous()       # the same latents and step for every prompt
    ehs = (CTX_GAIN * ehs).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    with torch.no_grad():
        plain_ref = run_ref()
    state = attach_edit(ref)
    return cfg, ref, hip, state, (x, t, ehs, added), run_ref, run, plain_ref


def _check_eps(tag, got, want, stored, plain_ref):
    e, e_plain, floor, shift = rel_l2(got, want), rel_l2(got, plain_ref), rel_l2(stored, want), rel_l2(want, plain_ref)
    print(f"[{tag}] eps rel_l2={e:.3e} (against the oracle WITHOUT the edit {e_plain:.3e}), bf16-storage floor {floor:.3e}, "
          f"ratio {e / floor:.2f}; the edit moves the oracle's eps by {shift:.3f}")
    assert e < EPS_LIMIT and e < e_plain
    assert floor >= FLOOR_DEGENERATE, floor                          # CTX_GAIN is there for this: the sharper bound never drops out
    assert e <= STORAGE_FLOOR_FACTOR * floor, (e, floor)


def test_tiny_unet_source_and_refined_prompt(gpu):
    """B = 2: the source and a refined, re-weighted prompt; self_max_tokens 16 and 64 -- the tiny UNet's self-attention has 64 and
    16 queries, so both sides of the threshold are exercised"""
    from oracle.bf16_store import bf16_storage
    B, L, T = 2, 77, 2
    cfg, ref, hip, state, _, run_ref, run, plain_ref = _setup(B, L)
    before = run()
    assert rel_l2(before, plain_ref) < EPS_LIMIT
    got = {}
    for smt in (16, 64):
        edit = _edit(L, T, smt)
        with torch.no_grad():
            state.set(edit, 0)
            want = run_ref()
            with bf16_storage():
                stored = run_ref()
            state.set(None)
        assert torch.equal(want[0], plain_ref[0])                    # the oracle's source does not move
        assert rel_l2(want[1], plain_ref[1]) >= 5 * EPS_LIMIT        # ... and an ignored edit cannot pass
        hip.set_prompt_edit(edit)
        hip.set_prompt_edit_step(0)
        got[smt] = run()
        _check_eps(f"tiny unet + refine edit, self_max_tokens {smt}", got[smt][1:], want[1:], stored[1:], plain_ref[1:])
        assert torch.equal(got[smt][0], before[0])                   # the source keeps the bits of a forward without an edit
        assert torch.equal(run(), got[smt])                          # bit-reproducible
        got[smt, "want"] = want
    assert not torch.equal(got[64][1], got[16][1])                   # the 64-query layers take the rule at 64 only
    assert rel_l2(got[64][1], got[64, "want"][1]) < rel_l2(got[64][1], got[16, "want"][1])
    # a step past every window: the plain launches, the bits of the forward without editing
    hip.set_prompt_edit_step(1)
    assert torch.equal(run(), before)
    hip.set_prompt_edit_step(0)
    assert torch.equal(run(), got[64])
    hip.clear_prompt_edit()
    assert torch.equal(run(), before)                                # the bits from before `set` come back


def test_tiny_unet_cfg_layout(gpu):
    from oracle.bf16_store import bf16_storage
    B, L, T = 4, 77, 2
    cfg, ref, hip, state, _, run_ref, run, plain_ref = _setup(B, L)
    before = run()
    edit = _edit(L, T, 64, do_cfg=True)
    assert edit.src.tolist() == [-1, -1, -1, 2]
    with torch.no_grad():
        state.set(edit, 0)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
    hip.set_prompt_edit(_edit(L, T, 64), do_cfg=True)                # composed without CFG, laid out by the UNet
    hip.set_prompt_edit_step(0)
    got = run()
    assert torch.equal(got[:3], before[:3]) and not torch.equal(got[3], before[3])      # the unconditional half and the source
    _check_eps("tiny unet + refine edit, CFG layout", got[3:], want[3:], stored[3:], plain_ref[3:])
    hip.clear_prompt_edit()
    assert torch.equal(run(), before)


def test_tiny_unet_edit_refusals(gpu):
    from ip_adapter_ref import make_image_proj
    from ip_multi_ref import attach_multi_ip, file_state_dict_of
    from oracle.unet_ref import UNet2DConditionRef, tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    T = 2
    grad = HipUNet(pc.tiny_config(), 2, 16, 16, 77, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.set_prompt_edit(_edit(77, T, 64))
    long = HipUNet(pc.tiny_config(), 2, 16, 16, 97, needs_grad=False)
    with pytest.raises(PeaError, match="1..96 rows"):
        long.set_prompt_edit(_edit(97, T, 64))
    B, L = 2, 77
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    before = run()
    edit = _edit(L, T, 64)
    with pytest.raises(PeaError, match="batch"):
        hip.set_prompt_edit(_edit(L, T, 64, do_cfg=True))            # tables for four samples
    with pytest.raises(PeaError, match="context of 40 rows, this UNet has 77"):
        hip.set_prompt_edit(_edit(40, T, 64))                        # tables for a shorter context: refused before the library copies
    assert torch.equal(run(), before)
    hip.set_prompt_edit(edit)
    edited = run()                                                   # step 0 is the default
    assert not torch.equal(edited, before)
    for step in (-1, T):
        hip.set_prompt_edit_step(step)
        with pytest.raises(PeaError, match="outside 0..1"):
            run()
    hip.set_prompt_edit_step(0)
    # maps, live image prompts (regions: the next test): refused at the forward when they arrive afterwards, and when the edit is set
    hip.clear_prompt_edit()
    hip.enable_attention_maps()
    with pytest.raises(PeaError, match="attention-map capture"):
        hip.set_prompt_edit(edit)
    hip.disable_attention_maps()
    hip.set_prompt_edit(edit)
    hip.enable_attention_maps()
    with pytest.raises(PeaError, match="attention-map capture"):
        run()
    hip.disable_attention_maps()
    assert torch.equal(run(), edited)
    hip.clear_prompt_edit()
    ipref = UNet2DConditionRef(tiny_config())
    attach_multi_ip(ipref, (4,), (3,), (16, 16))
    hip.load_ip_adapter(file_state_dict_of(ipref, 0, make_image_proj(64, 128, 4, seed=4)))
    hip.set_prompt_edit(edit)                                        # an adapter without tokens is no image prompt
    assert torch.equal(run(), edited)
    hip.set_ip_tokens(torch.randn(B, 4, 128, generator=torch.Generator().manual_seed(7)))
    with pytest.raises(PeaError, match="live image prompts"):
        run()
    with pytest.raises(PeaError, match="live image prompts"):
        hip.set_prompt_edit(edit)
    hip.clear_ip_tokens()
    hip.clear_prompt_edit()
    assert torch.equal(run(), before)


def test_tiny_unet_edit_refuses_regions(gpu):
    """a context of two prompts of 48 rows takes regions and, at 96 rows, an edit: never both"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    from regional_ref import half_masks
    L, T = 96, 2
    cfg, ref, hip = _tiny_ip_pair(2, L)
    x, t, ehs, added = cond_inputs(cfg, 2, L, 16)
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    hip.set_prompt_regions(half_masks(128, 128))
    with pytest.raises(PeaError, match="prompt regions"):
        hip.set_prompt_edit(_edit(L, T, 64))
    hip.clear_prompt_regions()
    hip.set_prompt_edit(_edit(L, T, 64))
    with_edit = run()
    hip.set_prompt_regions(half_masks(128, 128))
    with pytest.raises(PeaError, match="prompt regions"):
        run()
    hip.clear_prompt_regions()
    assert torch.equal(run(), with_edit)


def test_denoise_edit_two_steps(gpu):
    """two steps through denoise_edit, the window ending after the first, against the same two steps driven by hand"""
    from pea_diffusion_amd import ops as pops
    from pea_diffusion_amd.prompt2prompt import denoise_edit
    from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
    N, L, T, gs = 2, 77, 2, 5.0
    cfg, ref, hip, state, (x, _, ehs, added), _, _, _ = _setup(2 * N, L)
    lat = x[:1]
    dev = {k: v.cuda() for k, v in added.items()}
    kw = dict(num_inference_steps=T, guidance_scale=gs)
    edit = _edit(L, T, 64)
    assert edit.cd[0, 0, 1].abs().sum() > 0 and edit.cd[1, 0, 1].abs().sum() == 0 and edit.self_until == 1
    plain = denoise(hip, DPMSolverMultistep(), lat.expand(N, -1, -1, -1).contiguous().cuda(), ehs.cuda(), dev, **kw)
    got = denoise_edit(hip, DPMSolverMultistep(), lat.cuda(), ehs.cuda(), dev, edit, **kw)
    after = denoise(hip, DPMSolverMultistep(), lat.expand(N, -1, -1, -1).contiguous().cuda(), ehs.cuda(), dev, **kw)
    assert torch.equal(after, plain)                                 # denoise_edit cleared the edit
    # by hand: the loop of sampler.denoise, the step set in front of every forward
    sch = DPMSolverMultistep()
    ts = sch.set_timesteps(T)
    latents = (lat.expand(N, -1, -1, -1).float().cuda() * sch.init_noise_sigma).contiguous()
    hip.set_prompt_edit(edit, do_cfg=True)
    for i, t in enumerate(ts):
        hip.set_prompt_edit_step(i)
        xin = sch.scale_model_input(torch.cat([latents] * 2), t)
        eps = hip(xin, t, encoder_hidden_states=ehs.cuda(), added_cond_kwargs=dev, return_dict=False)[0]
        latents = sch.step(pops.cfg_combine(eps.float(), gs, 0.0), t, latents, return_dict=False)[0]
    hip.clear_prompt_edit()
    assert torch.isfinite(got).all() and torch.equal(got, latents)
    assert torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1])          # the source's picture is kept
