"""-m gpu: perturbed-attention and smoothed-energy guidance -- the in-place query blur (pea_op_query_blur), the identity copy
(pea_op_attn_identity) and the three-way guidance combine (pea_op_cfg_pag_combine) against the fp32 restatement of
tests/pag_ref.py, their exactness properties, and the UNet runtime (HipUNet.set_attention_perturbation, pag.denoise_perturbed)
against the oracle with a perturbing self-attention.

Tolerances.  Query blur: bf16-stored, 1 bf16 ulp against the fp32 restatement rounded to bf16 (tests/test_ops_gpu.py: close_bf16).
Identity copy: bits.  Combine: the rule for fp32-stored results, rtol 1e-3 / atol 1e-4; at s = 0 the bits of cfg_combine.
Runtime: the oracle's own bf16-storage floor of the perturbed sample's eps, x STORAGE_FLOOR_FACTOR (tests/test_model_gpu.py),
measured in the run.

A forward that ignores the perturbation must not pass, so the oracle's perturbed eps has to lie at least 4 limits from its plain
eps.  With the tiny UNet's random weights a self-attention softmax is nearly flat and its layer a small part of eps: measured on the
CPU, the oracle alone (CTX_GAIN 5, the inputs of `_setup`, sample 2 of 3 perturbed), the mid block moves eps by 3.5 limits (PAG)
and 0.4 (SEG, infinite sigma).  The perturbed layers therefore get their query projection x 8 (QK_GAIN: a softmax with contrast)
and their output projection x 4 (OUT_GAIN), in the oracle and, through its state dict, on the device.  Measured with those gains,
distance / limit (limit = 1.5 x floor, floor 1.0e-2 .. 1.1e-2): the mid block (two layers of 16 tokens) PAG 8.8, SEG sigma inf 6.1,
SEG sigma 2 6.5; up_blocks.1.attentions.0 (64 tokens) PAG 17.6, SEG sigma inf 10.1, SEG sigma 2 10.2.  (SEG at sigma 0.5: 2.9 and
3.8 -- not used here.  The floor moves by some percent with the host's BLAS: the test's own run printed 8.2, 5.8, 17.5 and 10.1.)"""
import functools
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
from pag_ref import attach_perturb, blur_ref, combine_ref, denoise_perturbed_ref, set_perturb  # noqa: E402
from test_model_gpu import cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import BF, bfr, close_bf16, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import FLOOR_DEGENERATE, _floor_limit  # noqa: E402

INF = float("inf")
SIGMAS = [0.5, 2.0, 10.0, INF]
BLUR_SHAPES = [(1, 1, 1, 64), (1, 4, 4, 128), (2, 8, 8, 128), (1, 7, 13, 64), (1, 32, 32, 1280), (1, 64, 64, 640)]      # (n, h, w, C)


def _tables(h, w, sigma):
    from pea_diffusion_amd.pag import blur_matrix
    return torch.from_numpy(blur_matrix(h, sigma)).cuda(), torch.from_numpy(blur_matrix(w, sigma)).cuda()


@functools.lru_cache(maxsize=None)
def _rows(n, S, ld):
    """bf16 [n + 1, S, ld] on the host: one sample in front of the n that are blurred; computed once, never written"""
    return bfr(n + 1, S, ld, seed=7 * S + ld)


@pytest.mark.parametrize("shape", BLUR_SHAPES)
def test_query_blur_against_the_restatement(ops, shape):
    """pitch 3C with the Q columns first, one sample in front of the range: every sigma; the other columns and the sample in
    front keep their bits; the same bits every run"""
    n, h, w, C = shape
    src = _rows(n, h * w, 3 * C)
    for sigma in SIGMAS:
        Mh, Mw = _tables(h, w, sigma)
        buf = src.cuda()
        ops.query_blur_(buf[1:], (h, w), Mh, Mw, cols=C)
        got = buf.cpu()
        want = blur_ref(src[1:, :, :C].float(), h, w, sigma).to(BF)
        close_bf16(f"query_blur {shape} sigma {sigma}", got[1:, :, :C], want.float(), ulps=1.0)
        assert torch.equal(got[0], src[0]) and torch.equal(got[1:, :, C:], src[1:, :, C:])
        again = src.cuda()
        ops.query_blur_(again[1:], (h, w), Mh, Mw, cols=C)
        assert torch.equal(again.cpu(), got)
        if sigma == INF and h * w > 1:                               # the mean: every token of a channel holds the same value
            assert torch.equal(got[1:, :1, :C].expand(n, h * w, C), got[1:, :, :C]) and not torch.equal(got[1:, :, :C], src[1:, :, :C])


@pytest.mark.parametrize("shape,col0", [((2, 8, 8, 128), 128), ((1, 7, 13, 64), 64), ((1, 32, 32, 1280), 2560)])
def test_query_blur_at_a_column_offset(ops, shape, col0):
    n, h, w, C = shape
    src = _rows(n, h * w, 3 * C)
    Mh, Mw = _tables(h, w, 2.0)
    buf = src.cuda()
    ops.query_blur_(buf[1:], (h, w), Mh, Mw, cols=C, col0=col0)
    got = buf.cpu()
    want = blur_ref(src[1:, :, col0:col0 + C].float(), h, w, 2.0).to(BF)
    close_bf16(f"query_blur {shape} at column {col0}", got[1:, :, col0:col0 + C], want.float(), ulps=1.0)
    keep = torch.ones(3 * C, dtype=torch.bool)
    keep[col0:col0 + C] = False
    assert torch.equal(got[0], src[0]) and torch.equal(got[1:][:, :, keep], src[1:][:, :, keep])


def test_query_blur_refusals(ops):
    from pea_diffusion_amd._lib import PeaError
    Mh, Mw = _tables(65, 64, 2.0)
    with pytest.raises(PeaError, match="LDS"):                       # one row more than a workgroup's LDS holds
        ops.query_blur_(torch.zeros(1, 65 * 64, 64, dtype=BF, device="cuda"), (65, 64), Mh, Mw)
    Mh, Mw = _tables(4, 4, 2.0)
    buf = torch.zeros(1, 16, 192, dtype=BF, device="cuda")
    with pytest.raises(PeaError, match="whole heads"):
        ops.query_blur_(buf, (4, 4), Mh, Mw, cols=72)
    with pytest.raises(PeaError, match="offset"):
        ops.query_blur_(buf, (4, 4), Mh, Mw, cols=64, col0=136)
    with pytest.raises(PeaError, match="blur matrix"):
        ops.query_blur_(buf, (4, 4), Mh[:3], Mw)
    with pytest.raises(PeaError, match="grid"):
        ops.query_blur_(buf, (4, 5), Mh, Mw)
    assert not buf.any()


@pytest.mark.parametrize("rows,C,ldv,col0,ldo", [(1, 64, 64, 0, 64), (3 * 16, 128, 384, 256, 128), (2 * 1024, 1280, 3840, 2560, 1280 + 64),
                                                 (77, 64, 200, 72, 136)])
def test_attn_identity_is_a_pitched_copy(ops, rows, C, ldv, col0, ldo):
    v = bfr(rows, ldv, seed=rows + C)
    out0 = bfr(rows, ldo, seed=3)
    out = ops.attn_identity(v.cuda(), out0.cuda(), C, col0=col0).cpu()
    assert torch.equal(out[:, :C], v[:, col0:col0 + C]) and torch.equal(out[:, C:], out0[:, C:])      # bits; guard columns untouched


def test_cfg_pag_combine(ops):
    g = torch.Generator().manual_seed(5)
    B = 2
    e3 = torch.randn(3 * B, 4, 24, 20, generator=g)
    d3 = e3.cuda()
    for gs, s, phi in ((5.0, 3.0, 0.0), (7.5, 1.0, 0.7), (1.5, 0.25, 0.3)):
        close_f32(f"cfg_pag_combine g={gs} s={s} rescale={phi}", ops.cfg_pag_combine(d3, gs, s, phi), combine_ref(e3, gs, s, phi))
    for phi in (0.0, 0.7):                                           # s = 0: cfg_combine's bits on the first 2B samples
        assert torch.equal(ops.cfg_pag_combine(d3, 5.0, 0.0, phi), ops.cfg_combine(d3[:2 * B].contiguous(), 5.0, phi))
    assert not torch.equal(ops.cfg_pag_combine(d3, 5.0, 3.0, 0.7), ops.cfg_combine(d3[:2 * B].contiguous(), 5.0, 0.7))
    e2 = e3[:2 * B]
    close_f32("pag_combine without CFG", ops.cfg_pag_combine(e2.cuda(), 0.0, 3.0, 0.0, do_cfg=False), combine_ref(e2, 0.0, 3.0, 0.0, False))
    # ... where guidance_rescale is not applied, and s = 0 hands back the text prediction
    assert torch.equal(ops.cfg_pag_combine(e2.cuda(), 0.0, 3.0, 0.7, do_cfg=False), ops.cfg_pag_combine(e2.cuda(), 0.0, 3.0, 0.0, do_cfg=False))
    assert torch.equal(ops.cfg_pag_combine(e2.cuda(), 0.0, 0.0, 0.0, do_cfg=False).cpu(), e2[:B])
    odd = torch.randn(3, 3, 7, generator=g)                          # a ragged element count
    close_f32("cfg_pag_combine ragged", ops.cfg_pag_combine(odd.cuda(), 3.0, 0.5, 0.5), combine_ref(odd, 3.0, 0.5, 0.5))


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
CTX_GAIN = 5.0                                                       # as tests/test_sag_gpu.py
QK_GAIN, OUT_GAIN = 8.0, 4.0                                         # module docstring
MID = ["mid_block.attentions.0.transformer_blocks.0.attn1", "mid_block.attentions.0.transformer_blocks.1.attn1"]
UP = "up_blocks.1.attentions.0.transformer_blocks.0.attn1"           # 64 tokens


def _pair(B, L=77):
    """the tiny pair with QK_GAIN / OUT_GAIN on the layers the tests perturb"""
    from test_ip_adapter_gpu import _tiny_ip_pair
    cfg, ref, hip = _tiny_ip_pair(B, L)
    with torch.no_grad():
        for name in MID + [UP]:
            m = ref.get_submodule(name)
            m.to_q.weight.copy_((m.to_q.weight * QK_GAIN).to(BF).float())
            m.to_out[0].weight.copy_((m.to_out[0].weight * OUT_GAIN).to(BF).float())
    missing, unexpected = hip.load_state_dict(ref.state_dict())
    assert not missing and not unexpected
    return cfg, ref, hip


def _setup(B=3, L=77, hw=16):
    cfg, ref, hip = _pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    t = t[1:2].expand(B).contiguous()
    ehs = (CTX_GAIN * ehs).to(BF).float()

    def run_ref():
        with torch.no_grad():
            return ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    return cfg, ref, hip, run_ref, run


@pytest.mark.parametrize("layers", [None, [UP]], ids=["mid-block", "up-64-tokens"])
def test_tiny_unet_perturbed_sample_vs_oracle(gpu, layers):
    """batch 3, the last sample perturbed: samples 0 - 1 keep the feature-off bits; sample 2 against the oracle, which the
    perturbation moves by at least 4 limits; clear restores the first forward's bits; release_activations keeps the tables"""
    from oracle.bf16_store import bf16_storage
    cfg, ref, hip, run_ref, run = _setup()
    before = run()
    mods = attach_perturb(ref, MID if layers is None else layers, hip._grid_of)
    plain = run_ref()
    for mode, sigma in (("pag", INF), ("seg", INF)):
        hip.set_attention_perturbation(mode, layers=layers, samples=None if layers is None else 1, blur_sigma=sigma)
        got = run()
        assert torch.equal(got[:2], before[:2]) and not torch.equal(got[2], before[2])
        assert torch.equal(run(), got)                               # bit-reproducible (the blur runs in place on fresh queries)
        set_perturb(mods, mode, 2, sigma)
        want = run_ref()
        with bf16_storage():
            stored = run_ref()
        set_perturb(mods, None)
        assert torch.equal(want[:2], plain[:2])
        floor = rel_l2(stored[2], want[2])
        limit, rule = _floor_limit("tiny", floor)
        e, moved = rel_l2(got[2], want[2]), rel_l2(want[2], plain[2])
        print(f"[tiny unet, {mode} on {'the mid block' if layers is None else layers[0]}] perturbed eps rel_l2={e:.3e}, bf16-storage floor "
              f"{floor:.3e} (ratio {e / floor:.2f}, limit {limit:.3e}: {rule}); the perturbation moves the oracle's eps by {moved:.3e} "
              f"= {moved / limit:.1f} limits; ignoring it would score {rel_l2(before[2], want[2]):.3e}")
        assert floor >= FLOOR_DEGENERATE, floor
        assert moved >= 4.0 * limit, (moved, limit)
        assert torch.isfinite(got).all() and e <= limit, (e, limit)
        hip.release_activations()                                    # the tables are not part of the arenas
        assert torch.equal(run(), got)
        hip.clear_attention_perturbation()
        assert torch.equal(run(), before)


@pytest.mark.parametrize("sched,g,mode,sigma", [("dpm", 5.0, "pag", INF), ("euler", 0.0, "seg", 2.0)])
def test_denoise_perturbed_tiny_vs_oracle(gpu, sched, g, mode, sigma):
    """3 steps of pag.denoise_perturbed against the restated loop, n = 1: DPM-Solver under CFG (batch 3) with PAG, Euler without
    CFG (batch 2) with SEG at sigma 2; the mid block, scale 3"""
    from oracle.bf16_store import bf16_storage
    from oracle.sampler_ref import DPMSolverMultistepRef
    from pea_diffusion_amd.pag import denoise_perturbed
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerDiscrete
    from turbo_ref import EulerRef
    L, steps, s = 77, 3, 3.0
    k = 3 if g > 1.0 else 2
    cfg, ref, hip = _pair(k, L)
    x, _, ehs, added = cond_inputs(cfg, k, L, 16)
    x, ehs = x[:1], (CTX_GAIN * ehs).to(BF).float()[:k - 1]
    added = {key: v[:k - 1] for key, v in added.items()}
    run = lambda: denoise_perturbed(hip, DPMSolverMultistep() if sched == "dpm" else EulerDiscrete(), x.cuda(), ehs.cuda(),
                                    {key: v.cuda() for key, v in added.items()}, mode=mode, scale=s, blur_sigma=sigma,
                                    num_inference_steps=steps, guidance_scale=g)
    fwd = lambda: hip(torch.cat([x] * k).cuda(), torch.tensor([500] * k).cuda(), torch.cat([ehs, ehs[-1:]]).cuda(),
                      added_cond_kwargs={key: torch.cat([v, v[-1:]]).cuda() for key, v in added.items()})[0].clone()
    before = fwd()
    got = run()
    assert torch.equal(run(), got)                                   # bit-reproducible
    assert torch.equal(fwd(), before)                                # the perturbation is cleared behind the loop
    mods = attach_perturb(ref, MID, hip._grid_of)
    make = (lambda: DPMSolverMultistepRef()) if sched == "dpm" else (lambda: EulerRef(False))
    loop = lambda: denoise_perturbed_ref(lambda *a, **kw: ref(*a, **kw), make(), x.clone(), ehs, added, steps, g, s).float()
    with torch.no_grad():
        set_perturb(mods, mode, k - 1, sigma)
        want = loop()
        with bf16_storage():
            stored = loop()
        set_perturb(mods, None)
        plain = loop()                                               # t - p = 0: the plain (CFG) loop
    floor = rel_l2(stored, want)
    limit, rule = _floor_limit("tiny", floor)
    e = rel_l2(got, want)
    print(f"[denoise_perturbed tiny, {sched} {steps} steps, guidance {g}, {mode} sigma {sigma} scale {s}] latents rel_l2={e:.3e}, bf16-storage "
          f"floor {floor:.3e}, ratio {e / max(floor, 1e-30):.2f}, limit {limit:.3e} ({rule}); the guidance moves the oracle's latents by "
          f"{rel_l2(want, plain):.3f}; against the plain loop the device scores {rel_l2(got, plain):.3e}")
    assert torch.isfinite(got).all() and e <= limit, (e, limit)
    assert e < rel_l2(got, plain)                                    # a loop that ignores the perturbation cannot pass


def test_tiny_unet_perturbation_refusals(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import style_aligned as sa
    from pea_diffusion_amd._lib import PeaError, check, lib, stream_ptr
    from pea_diffusion_amd.prompt2prompt import PromptEdit
    from pea_diffusion_amd.unet import HipUNet
    grad = HipUNet(pc.tiny_config(), 3, 16, 16, 77, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.set_attention_perturbation("pag")
    h15 = HipUNet(pc.tiny15_config(), 3, 16, 16, 77)                 # a UNet whose self-attention heads are not 64 wide
    with pytest.raises(PeaError, match="head_dim"):
        h15.set_attention_perturbation("pag", layers=1.0)
    B, L = 3, 77
    cfg, ref, hip, run_ref, run = _setup(B, L)
    before = run()
    names = sa.layer_names(hip)
    with pytest.raises(PeaError, match="suffix"):
        hip.set_attention_perturbation("pag", samples=0)             # nobody is perturbed
    with pytest.raises(PeaError, match="suffix"):
        hip.set_attention_perturbation("pag", samples=B)             # nobody is left plain
    with pytest.raises(PeaError, match="mode"):
        hip.set_attention_perturbation("blur")
    with pytest.raises(PeaError, match="names no self-attention layer"):
        hip.set_attention_perturbation("pag", layers=["up_blocks.9"])
    two = HipUNet(pc.tiny_config(), 2, 16, 16, 77)
    with pytest.raises(PeaError, match="how many"):
        two.set_attention_perturbation("pag")                        # a batch that is no [uncond | cond | perturbed]
    assert torch.equal(run(), before)
    # SEG on every layer with the tables of no grid (the C ABI: the Python setter always sends them): the forward refuses
    check(lib().pea_unet_set_attn_perturb(hip._h, 2, 2, None, 0, 0, None, None, None, stream_ptr()))
    with pytest.raises(PeaError, match="no tables"):
        run()
    hip.clear_attention_perturbation()
    # prompt editing, set before and set after
    edit = PromptEdit.compose(L, 2, [None, dict(source=0), None])
    hip.set_prompt_edit(edit)
    with pytest.raises(PeaError, match="prompt editing"):
        hip.set_attention_perturbation("pag")
    hip.clear_prompt_edit()
    hip.set_attention_perturbation("pag")
    with pytest.raises(PeaError, match="prompt editing"):
        hip.set_prompt_edit(edit)
    perturbed = run()
    assert torch.equal(perturbed[:2], before[:2]) and not torch.equal(perturbed[2], before[2])
    # StyleAligned on a perturbed layer: refused by the forward; on the other layers: welcome
    hip.set_style_aligned(layers=[MID[0]])
    with pytest.raises(PeaError, match="StyleAligned"):
        run()
    hip.set_style_aligned(layers=[n for n in names if n not in MID])
    shared = run()
    assert torch.equal(shared[0], before[0]) and not torch.equal(shared[1], before[1]) and not torch.equal(shared[2], perturbed[2])
    hip.clear_attention_perturbation()
    hip.set_style_aligned(layers=[MID[1]])
    with pytest.raises(PeaError, match="StyleAligned"):
        hip.set_attention_perturbation("seg")                        # ... and refused when the perturbation arrives behind it
    hip.clear_style_aligned()
    # self-attention guidance capturing a perturbed layer, in both orders; capturing another layer: welcome
    hip.enable_sag()                                                 # the mid block's first layer
    with pytest.raises(PeaError, match="self-attention guidance"):
        hip.set_attention_perturbation("pag")
    hip.set_attention_perturbation("pag", layers=[UP])
    assert torch.equal(run()[:2], before[:2])
    hip.disable_sag()
    hip.enable_sag(names.index(UP))
    with pytest.raises(PeaError, match="self-attention guidance"):
        run()
    hip.disable_sag()
    hip.clear_attention_perturbation()
    assert torch.equal(run(), before)


def test_perturbation_beside_the_six_other_features(gpu):
    """the feature's own pairs, in both orders, on the context of scripts/feature_digest.py (batch 2, the second sample perturbed):
    image prompts, regions and heat maps are welcome and leave the plain sample the bits it has with them alone; prompt editing
    is refused at whichever setter comes second; StyleAligned and self-attention guidance are refused on a common layer (by the
    second setter where it can see it, else by the forward) and welcome on disjoint ones"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import style_aligned as sa
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import PromptEdit
    from pea_diffusion_amd.unet import HipUNet
    spec =importlib.util.spec_from_file_location("feature_digest", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                 "scripts", "feature_digest.py"))
    fd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fd)
    B, HW, L = fd.B, fd.HW, fd.L
    cfg = pc.tiny_config()
    hip = HipUNet(cfg, B, HW, HW, L, needs_grad=False)
    hip.init_random(3)
    hip.load_ip_adapter(fd._adapter_file(cfg))
    x, t = fd._rnd(B, 4, HW, HW, seed=1).cuda(), torch.tensor([250, 500]).cuda()
    ehs = fd._rnd(B, L, cfg.cross_attention_dim, seed=2).cuda()
    added = {"text_embeds": fd._rnd(B, cfg.pooled_dim, seed=3).cuda(), "time_ids": torch.tensor([[HW * 8, HW * 8, 0, 0, HW * 8, HW * 8]] * B).cuda()}
    tokens = fd._rnd(B, fd.N_TOK, cfg.cross_attention_dim, seed=4)
    left = torch.zeros(8 * HW, 8 * HW)
    left[:, : 4 * HW] = 1.0
    edit = PromptEdit.compose(L, fd.T, [None, dict(source=0)])

    def set_edit():
        hip.set_prompt_edit(edit)
        hip.set_prompt_edit_step(0)
    not_mid = [n for n in sa.layer_names(hip) if n not in MID]
    setters = {"ip": lambda: hip.set_ip_tokens(tokens), "regions": lambda: hip.set_prompt_regions([left, 1.0 - left]),
               "maps": hip.enable_attention_maps, "edit": set_edit, "style": lambda: hip.set_style_aligned(ref=[-1, 0]),
               "sag": hip.enable_sag, "style-elsewhere": lambda: hip.set_style_aligned(ref=[-1, 0], layers=not_mid),
               "sag-elsewhere": lambda: hip.enable_sag(UP)}
    perturb = lambda: hip.set_attention_perturbation("seg", samples=1, blur_sigma=2.0)

    def clear_all():
        hip.clear_ip_tokens()
        hip.clear_prompt_regions()
        hip.disable_attention_maps()
        hip.clear_prompt_edit()
        hip.clear_style_aligned()
        hip.disable_sag()
        hip.clear_attention_perturbation()
    run = lambda: hip(x, t, ehs, added_cond_kwargs=added)[0].clone()
    clear_all()
    plain = run()
    perturb()
    alone = run()
    assert torch.equal(alone[0], plain[0]) and not torch.equal(alone[1], plain[1])
    # feature -> (who refuses when the perturbation is set first, who when it is set second); None: welcome
    expect = {"ip": None, "regions": None, "maps": None, "edit": ("set", "set"), "style": ("forward", "set"), "sag": ("forward", "set"),
              "style-elsewhere": None, "sag-elsewhere": None}
    for name, refused in expect.items():
        for order in (0, 1):
            clear_all()
            setters[name]()
            feature_alone = run()
            clear_all()
            first, second = (perturb, setters[name]) if order == 0 else (setters[name], perturb)
            first()
            if refused is None:
                second()
                eps = run()
                assert torch.equal(eps[0], feature_alone[0]), (name, order)          # the plain sample: the feature's own bits
                assert not torch.equal(eps[1], feature_alone[1]) and torch.isfinite(eps).all(), (name, order)
                if name == "maps":
                    assert all(n > 0 for _, n in hip.attention_maps().values())
                if name == "sag-elsewhere":
                    assert torch.isfinite(hip.sag_colsum()).all()
            elif refused[order] == "set":
                with pytest.raises(PeaError, match="perturbed"):
                    second()
            else:
                second()
                with pytest.raises(PeaError, match="perturbed"):
                    run()
    clear_all()
    assert torch.equal(run(), plain)
