"""Prompt-to-prompt editing, the host side (no GPU): the mappers on hand-worked cases, the (Mt, c, d) form against the controllers
applied one after another, the schedule, and what pea_op_attention_fwd_edit launches or refuses (pea_debug_attn_edit_dispatch)."""
import ctypes

import pytest
import torch

from p2p_ref import chain_blend, chain_refine, chain_replace, chain_reweight

F64 = torch.float64


# ---------------------------------------------------------------------------------------------- mappers, known answers
def test_replace_mapper_equal_length_swap():
    from pea_diffusion_amd.prompt2prompt import replace_mapper
    # "a photo of a cat" -> "a photo of a dog": token 5 for token 5 (position 0 is the start token); nothing moves
    assert torch.equal(replace_mapper(8, [((5, 6), (5, 6))]), torch.eye(8, dtype=F64))
    # two tokens for two tokens, one to one
    assert torch.equal(replace_mapper(8, [((2, 4), (2, 4))]), torch.eye(8, dtype=F64))


def test_replace_mapper_one_to_two():
    from pea_diffusion_amd.prompt2prompt import replace_mapper
    M = replace_mapper(6, [((2, 3), (2, 4))])                        # source token 2 becomes target tokens 2 and 3
    want = torch.zeros(6, 6, dtype=F64)
    want[0, 0] = want[1, 1] = 1.0
    want[2, 2] = want[2, 3] = 0.5
    want[3, 4] = want[4, 5] = 1.0                                    # shifted by one behind the span; source token 5 falls off
    assert torch.equal(M, want)
    Mt = M.t()                                                       # the kernel's rows: target keys 2 and 3 read half of source key 2
    assert Mt[2].tolist() == [0, 0, 0.5, 0, 0, 0] and Mt[3].tolist() == [0, 0, 0.5, 0, 0, 0] and Mt[4].tolist() == [0, 0, 0, 1, 0, 0]
    # two source tokens become one: both feed it with weight 1 (1 / len(target))
    M = replace_mapper(5, [((1, 3), (1, 2))])
    assert M[1, 1] == 1 and M[2, 1] == 1 and M[3, 2] == 1 and M[4, 3] == 1 and M.sum() == 5


def test_refine_mapper_insertion_in_the_middle():
    from pea_diffusion_amd.prompt2prompt import gather_mapper, refine_mapper
    src = [49406, 320, 1125, 539, 2368, 49407]                       # start a photo of cat end
    tgt = [49406, 320, 1125, 539, 1746, 2368, 49407]                 # ... of FLUFFY cat end
    gather, alphas = refine_mapper(src, tgt, 8)
    assert gather.tolist() == [0, 1, 2, 3, -1, 4, 5, 7]
    assert alphas.tolist() == [1, 1, 1, 1, 0, 1, 1, 1]
    M = gather_mapper(gather)
    assert M[:, 4].abs().sum() == 0 and M[4, 5] == 1 and M[3, 3] == 1 and M.sum() == 7


def test_identical_prompts_are_the_identity():
    from pea_diffusion_amd.prompt2prompt import PromptEdit, cross_schedule, gather_mapper, refine_mapper, replace_mapper
    ids = [49406, 320, 1125, 539, 2368, 49407]
    L, T = 8, 5
    gather, alphas = refine_mapper(ids, ids, L)
    assert gather.tolist() == list(range(L)) and alphas.tolist() == [1.0] * L
    assert torch.equal(gather_mapper(gather), torch.eye(L, dtype=F64)) and torch.equal(replace_mapper(L, []), torch.eye(L, dtype=F64))
    pe = PromptEdit.compose(L, T, [None, dict(source=0, refine=(gather, alphas))], cross_replace_steps=0.4)
    w = cross_schedule(T, L, 0.4)
    assert pe.src.tolist() == [-1, 0] and torch.equal(pe.Mt[1], torch.eye(L, dtype=F64))
    assert torch.equal(pe.cd[:, 0, 1], w) and torch.equal(pe.cd[:, 1, 1], 1.0 - w)                 # c = w, d = 1 - w
    assert torch.equal(pe.cd[:, 0, 0], torch.zeros(T, L, dtype=F64)) and torch.equal(pe.cd[:, 1, 0], torch.ones(T, L, dtype=F64))


# ---------------------------------------------------------------------------------------------- the algebra
def _probs(L, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(2.0 * torch.randn(2, 3, 10, L, generator=g, dtype=F64), -1)     # [samples][heads][queries][keys]
    return p[0], p[1]


@pytest.mark.parametrize("case", ["replace", "refine", "refine+reweight", "reweight"])
def test_folded_form_equals_the_controller_chain(case):
    from pea_diffusion_amd.prompt2prompt import PromptEdit, equalizer, refine_mapper, replace_mapper
    L, T = 12, 4
    p0, p1 = _probs(L, 3)
    ed = dict(source=0, per_token={7: 0.25})                         # key 7 leaves the window after step 0, the rest after step 1
    M = gather = alphas = eq = None
    if case == "replace":
        M = ed["mapper"] = replace_mapper(L, [((2, 3), (2, 4)), ((6, 8), (7, 9))])
    elif case.startswith("refine"):
        src = [1, 10, 11, 12, 13, 14, 2]
        tgt = [1, 10, 77, 11, 12, 88, 99, 13, 14, 2]
        gather, alphas = ed["refine"] = refine_mapper(src, tgt, L)
        assert alphas.tolist().count(0.0) == 3
    if case.endswith("reweight"):
        eq = ed["equalizer"] = equalizer(L, {2: 4.0, 5: -1.0, 7: 0.5})          # key 2 is a NEW token in the refine case
    pe = PromptEdit.compose(L, T, [None, ed], cross_replace_steps=0.5)
    inside = outside = 0
    for t in range(T):
        w = pe.cd.new_tensor([1.0 if (t < 1 if j == 7 else t < 2) else 0.0 for j in range(L)])
        if M is not None:
            rep = chain_replace(p0, M)
        elif gather is not None:
            rep = chain_refine(p0, p1, gather, alphas)
        else:
            rep = p0
        if eq is not None:
            rep = chain_reweight(rep, eq)
        want = chain_blend(rep, p1, w)
        c, d = pe.cd[t, 0, 1], pe.cd[t, 1, 1]
        got = c * (p0 @ pe.Mt[1].t()) + d * p1
        assert torch.allclose(got, want, rtol=0, atol=1e-14), (case, t, (got - want).abs().max())
        if w.sum() == 0:
            outside += 1
            assert torch.equal(c, torch.zeros(L, dtype=F64)) and torch.equal(d, torch.ones(L, dtype=F64)) and torch.equal(got, p1)
        else:
            inside += 1
            assert not torch.allclose(got, p1, atol=1e-3)
    assert inside == 2 and outside == 2


def test_compose_cfg_layout_and_refusals():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import PromptEdit, equalizer
    L, T = 8, 4
    pe = PromptEdit.compose(L, T, [None, dict(source=0, equalizer=equalizer(L, {3: 2.0})), dict(source=0)], self_replace_steps=0.5)
    assert pe.src.tolist() == [-1, 0, 0] and pe.self_until == 2 and pe.self_max_tokens == 1024 and not pe.cfg
    both = pe.with_cfg()
    assert both.cfg and both.src.tolist() == [-1, -1, -1, -1, 3, 3] and tuple(both.Mt.shape) == (6, L, L) and tuple(both.cd.shape) == (T, 2, 6, L)
    assert torch.equal(both.cd[:, :, 3:], pe.cd) and both.cd[:, 0, :3].abs().max() == 0 and (both.cd[:, 1, :3] == 1).all()
    assert both.with_cfg() is both
    same = PromptEdit.compose(L, T, [None, dict(source=0, equalizer=equalizer(L, {3: 2.0})), dict(source=0)], self_replace_steps=0.5, do_cfg=True)
    assert torch.equal(same.cd, both.cd) and torch.equal(same.src, both.src)
    with pytest.raises(PeaError):
        PromptEdit.compose(L, T, [None, dict(source=1)])             # a source that is itself edited (here: itself)
    with pytest.raises(PeaError):
        PromptEdit.compose(L, T, [None, dict(source=0), dict(source=1)])
    with pytest.raises(PeaError):
        PromptEdit.compose(L, T, [None, dict(source=2)])
    with pytest.raises(PeaError):
        PromptEdit.compose(L, T, [None, dict(source=0, mapper=torch.eye(L), refine=(torch.arange(L), torch.ones(L)))])


def test_set_prompt_edit_refuses_another_context_length_before_the_library():
    """the C entry has no size arguments and copies by the context's own L: tables composed for another length (the number of
    tokens, say) must never reach it.  No handle, no device: the refusal comes first"""
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import PromptEdit
    from pea_diffusion_amd.unet import HipUNet
    u = HipUNet.__new__(HipUNet)
    u.B, u.L, u._h, u.device = 2, 77, None, "cpu"
    for L in (8, 96):
        with pytest.raises(PeaError, match=f"context of {L} rows, this UNet has 77"):
            u.set_prompt_edit(PromptEdit.compose(L, 2, [None, dict(source=0)]))
    u.B = 4
    with pytest.raises(PeaError, match="context of 8 rows, this UNet has 77"):
        u.set_prompt_edit(PromptEdit.compose(8, 2, [None, dict(source=0)]), do_cfg=True)


# ---------------------------------------------------------------------------------------------- the schedule
def test_cross_schedule():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import cross_schedule
    w = cross_schedule(10, 4, 0.4)
    assert w[:4].eq(1).all() and w[4:].eq(0).all()                   # steps 0..3 of 10
    assert cross_schedule(50, 2, 0.8)[:, 0].tolist() == [1.0] * 40 + [0.0] * 10
    assert cross_schedule(100, 1, 0.29).sum() == 29                  # 0.29 x 100 is 28.999... in binary: still 29 steps
    assert cross_schedule(3, 2, 1.0).eq(1).all() and cross_schedule(3, 2, 0.0).eq(0).all()
    w = cross_schedule(10, 4, 0.4, per_token={2: 0.8, 3: (0.2, 0.5)})
    assert w[:, 0].tolist() == w[:, 1].tolist() == [1.0] * 4 + [0.0] * 6
    assert w[:, 2].tolist() == [1.0] * 8 + [0.0] * 2 and w[:, 3].tolist() == [0.0] * 2 + [1.0] * 3 + [0.0] * 5
    for bad in (1.5, -0.1, (0.6, 0.4)):
        with pytest.raises(PeaError):
            cross_schedule(10, 4, bad)
    with pytest.raises(PeaError):
        cross_schedule(10, 4, 0.5, per_token={4: 0.5})


def test_equalizer():
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import equalizer
    assert equalizer(5, {1: 4.0, 3: -1.0}).tolist() == [1.0, 4.0, 1.0, -1.0, 1.0] and equalizer(3).tolist() == [1.0] * 3
    with pytest.raises(PeaError):
        equalizer(5, {5: 2.0})
    with pytest.raises(PeaError):
        equalizer(5, {1: float("nan")})


# ---------------------------------------------------------------------------------------------- the launcher, without a device
def _dispatch(B=2, H=2, Sq=128, Skv=77, nd=1, ldk=0, ldm=0, null_table=False, src=None):
    from pea_diffusion_amd._lib import lib
    src = ([-1] + [0] * (B - 1) if src is None else list(src))[:32]
    q = (ctypes.c_int * 40)(B, H, Sq, Skv, nd, ldk, ldm, int(null_table), *(src + [-1] * (32 - len(src))))
    out = (ctypes.c_int * 8)()
    rc = lib().pea_debug_attn_edit_dispatch(q, out)
    return rc, list(out), lib().pea_last_error().decode()


def _lds(KB):
    return 3 * KB * 4096 + KB * 32 * (KB * 64 + 16) + KB * 256 + 4 * 4096 + 8 * 4096


def test_edit_dispatch_lds_and_grid():
    for Skv in range(1, 97):
        KB = (Skv + 31) // 32
        for Sq in (1, 16, 1024, 4096):
            for B, H in ((2, 1), (4, 10), (4, 20)):
                rc, (kb, gx, gy, gz, lds, upw, plain_first, upw_e), msg = _dispatch(B, H, Sq, Skv, src=[-1, 0] * (B // 2))
                assert rc == 0, msg
                assert kb == KB and (gy, gz) == (1, 1)
                assert lds == _lds(KB) and lds <= 163840
                # below 128 queries the plain launch is another kernel: it runs first and keeps the unedited samples' bits
                assert plain_first == (1 if Sq < 128 else 0)
                # a 1-D grid of exactly the workgroups that have work: every unit of both kinds of sample, nobody idle ...
                nu, cd = (Sq + 127) // 128, lambda a, b: (a + b - 1) // b
                n_un = 0 if plain_first else B // 2
                assert 1 <= upw <= nu and 1 <= upw_e <= nu
                assert gx == H * (n_un * cd(nu, upw) + B // 2 * cd(nu, upw_e))
                assert (cd(nu, upw) - 1) * upw < nu and (cd(nu, upw_e) - 1) * upw_e < nu
                # ... in one round of the workgroups the CUs' LDS holds at once (here one per (sample, head) always fits)
                assert gx <= 256 * (2 if 2 * lds <= 163840 else 1)
    assert _lds(3) == 106752 and _lds(1) == 64256                    # the figures the header and DESIGN quote
    # units per workgroup (unedited, edited) by the measured times 3.0 + 2.0 u and 6.4 + 3.7 u us: SDXL at 1024 x 1024, CFG batch 4
    units = lambda *a, **k: tuple(_dispatch(*a, **k)[1][i] for i in (5, 7))
    assert units(4, 10, 4096, 77, src=[-1, -1, -1, 2]) == (8, 3)     # 30 x 4 + 10 x 11 = 230 workgroups, 19.0 | 17.5 us
    assert units(4, 10, 4096, 77, src=[-1, 0, -1, 2]) == (8, 4)      # 20 x 4 + 20 x 8 = 240
    assert units(4, 20, 1024, 77, src=[-1, -1, -1, 2]) == (4, 2)     # 60 x 2 + 20 x 4 = 200
    assert units(4, 10, 4096, 32, src=[-1, -1, -1, 2]) == (3, 2)     # two workgroups per CU: 30 x 11 + 10 x 16 = 490 of 512
    # more (sample, head) pairs than a round holds: one workgroup each, all units
    assert units(32, 40, 1024, 77, src=[-1, 0] * 16) == (8, 8)


def test_edit_dispatch_refusals():
    assert _dispatch()[0] == 0
    cases = (("out of range", dict(src=[-1, 2])), ("itself edited", dict(B=3, src=[-1, 0, 1])),
             ("at most 32 samples", dict(B=33)), ("1..96 keys", dict(Skv=97)), ("head_dim 64", dict(nd=2)),
             ("leading dimension", dict(ldk=132)), ("leading dimension", dict(ldm=84)), ("leading dimension", dict(ldm=72)),
             ("empty problem", dict(Sq=0)), ("empty problem", dict(Skv=0)), ("empty problem", dict(B=0)), ("empty problem", dict(H=0)),
             ("null table", dict(null_table=True)))
    for cause, kw in cases:
        rc, _, msg = _dispatch(**kw)
        assert rc == -3 and "attention_edit" in msg and cause in msg, (cause, kw, rc, msg)        # PEA_E_SHAPE, the cause named
    # a sample that names itself is its own source, that is, not edited: [-1, -1, 2, 2] is the CFG layout of two prompts
    assert _dispatch(src=[-1, 1], null_table=True)[0] == 0 and _dispatch(B=4, src=[-1, -1, 2, 2])[0] == 0
    # a null table is fine while nobody is edited; ldm may be wider than the keys
    assert _dispatch(src=[-1, -1], null_table=True)[0] == 0 and _dispatch(ldm=96)[0] == 0 and _dispatch(ldk=136)[0] == 0


def test_edit_entry_points_without_a_device():
    from pea_diffusion_amd import _lib
    L = _lib.lib()
    protos = _lib.parse_header()
    for name in ("pea_op_attention_fwd_edit", "pea_unet_set_prompt_edit", "pea_unet_set_prompt_edit_step", "pea_unet_clear_prompt_edit",
                 "pea_debug_attn_edit_dispatch"):
        assert name in protos and hasattr(L, name)
    assert len(protos["pea_op_attention_fwd_edit"][1]) == 20 and len(protos["pea_unet_set_prompt_edit"][1]) == 8
    fake = ctypes.c_void_p(4096)                                     # never followed: refused first
    src = (ctypes.c_int * 2)(-1, 0)
    call = lambda B=2, Skv=77, s=src, Mt=fake, ldm=80: L.pea_op_attention_fwd_edit(
        fake, 128, fake, 128, fake, 128, fake, 128, B, 2, 128, Skv, s, Mt, ldm, fake, fake, 0.125, 0, None)
    assert call(Skv=97) == -3 and b"1..96 keys" in L.pea_last_error()
    assert call(Mt=None) == -3 and b"null table" in L.pea_last_error()
    assert call(s=(ctypes.c_int * 2)(-1, 5)) == -3 and b"out of range" in L.pea_last_error()
    assert call(ldm=76) == -3 and call(s=None) == -1 and b"null src" in L.pea_last_error()
    assert L.pea_unet_set_prompt_edit(None, src, fake, fake, 2, 1, 1024, None) == -1 and b"pea_unet_set_prompt_edit" in L.pea_last_error()
    assert L.pea_unet_set_prompt_edit_step(None, 0) == -1 and b"pea_unet_set_prompt_edit_step" in L.pea_last_error()
    assert L.pea_unet_clear_prompt_edit(None) == -1 and b"pea_unet_clear_prompt_edit" in L.pea_last_error()
