"""-m gpu: self-attention guidance -- the column-sum kernel (pea_op_attention_colsum), the fused degrade (pea_op_sag_degrade) and
the guidance combine (pea_op_cfg_sag_combine) against the fp32 restatement of tests/sag_ref.py, their exactness properties, and
the UNet runtime (HipUNet.enable_sag, sag.denoise_sag) against the oracle with a recording self-attention.

Tolerances.  Column sums with a torch fp32 lse, degrade, combine: the project's rule for fp32-stored results, rtol 1e-3 / atol 1e-4.
Column sums chained behind the project's own forward: rtol 3e-3 / atol 1e-4 -- tests/test_ops_gpu.py allows the forward's lse an
absolute 2e-3, which is a relative 2e-3 on every probability, on top of the rule's 1e-3.
Runtime: the oracle's own bf16-storage floor of the quantity, x STORAGE_FLOOR_FACTOR (tests/test_model_gpu.py).  A mask entry can
only flip where the column sum's deviation reaches its distance from 1, and that is an elementwise matter: for the masks the
floor is max |A_stored - A_fp32| over the entries, for the column sums as a whole it is the relative L2 distance, each measured in
the run and multiplied by the same factor.
Measured on the CPU, the oracle alone (tiny UNet, CTX_GAIN 5, the inputs of `_setup`): mid-block layer 0, 16 tokens x 2 samples:
column sums 0.84 .. 1.15, half of them above 1; floor 1.5e-3 (relative L2), 3.0e-3 (largest entry); 2 of 32 entries (6.2 %) lie
within 1.5 x 3.0e-3 of 1.  The 64-token layer up_blocks.1.attentions.0: 8.6 %.  Without the context gain the floors are
degenerate, as in the heat-map tests."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
from sag_ref import attach_sag, colsum_ref, combine_ref, degrade_ref, denoise_sag_ref  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, bfr, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE, _floor_limit  # noqa: E402

LN2 = math.log(2.0)
SHAPES = [(1, 1, 1, 1), (2, 2, 16, 16), (1, 3, 33, 33), (1, 2, 64, 64), (1, 2, 91, 91), (2, 3, 129, 129), (1, 2, 260, 33),
          (1, 1, 64, 7), (2, 5, 256, 256), (2, 20, 1024, 1024)]


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, Skv, prescaled, kind="plain"):
    """-> ((q, k) bf16 on the device, lse fp32 on the device, A fp32 [B, Skv] on the host); computed once, never written.
    kind "peaked": q x 4 (scores of standard deviation 4: a few keys take nearly all of a query's mass); "spike": the last query
    (a late, ragged query tile) is four times the last key, which takes all of that query's mass."""
    C = 64 * H
    q, k = bfr(B, Sq, C, seed=11).float(), bfr(B, Skv, C, seed=12).float()
    if kind == "peaked":
        q = q * 4.0
    if kind == "spike":
        q[0, Sq - 1] = 4.0 * k[0, Skv - 1]
    q = (q * ALPHA if prescaled else q).to(BF)
    k = k.to(BF)
    A, lse = colsum_ref(q, k, H, scale=LN2 if prescaled else 0.125)
    return (q.cuda(), k.cuda()), lse.contiguous().cuda(), A


def _sum_groups(part):
    """the consumer's sum: ascending g, plain fp32 adds"""
    A = part[:, 0].clone()
    for g in range(1, part.shape[1]):
        A = A + part[:, g]
    return A


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_colsum_against_the_restatement(ops, shape, prescaled):
    B, H, Sq, Skv = shape
    (q, k), lse, want = _case(B, H, Sq, Skv, prescaled)
    part = ops.attention_colsum(q, k, lse, H, q_prescaled=prescaled)
    G = ops.attention_colsum_groups(B, H, Sq, Skv)
    assert tuple(part.shape) == (B, G, Skv) and part.dtype == torch.float32
    got = _sum_groups(part).cpu()
    close_f32(f"colsum {shape} prescaled={prescaled}", got, want)
    close_f32(f"colsum {shape} mass", got.sum(1), torch.full((B,), float(Sq)))
    assert torch.equal(ops.attention_colsum(q, k, lse, H, q_prescaled=prescaled), part)      # the same bits every run


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("kind,shape", [("peaked", (2, 3, 129, 129)), ("peaked", (1, 2, 260, 33)), ("spike", (1, 2, 200, 200)),
                                        ("spike", (2, 3, 129, 129))])
def test_colsum_peaked_and_spiked(ops, kind, shape, prescaled):
    B, H, Sq, Skv = shape
    (q, k), lse, want = _case(B, H, Sq, Skv, prescaled, kind)
    got = _sum_groups(ops.attention_colsum(q, k, lse, H, q_prescaled=prescaled)).cpu()
    close_f32(f"colsum {kind} {shape} prescaled={prescaled}", got, want)
    if kind == "spike":
        assert float(want[0, Skv - 1]) > float(want[0].median()) + 0.9 / H     # the spiked key holds one query's whole mass in every head


@pytest.mark.parametrize("shape", [(2, 2, 16, 16), (1, 2, 91, 91), (2, 3, 129, 129), (1, 2, 260, 33), (2, 5, 256, 256), (2, 20, 1024, 1024)])
def test_colsum_behind_the_forward(ops, shape):
    """the lse of ops.attention_fwd (prescaled Q, the product path), then the column sums"""
    B, H, Sq, Skv = shape
    (q, k), _, want = _case(B, H, Sq, Skv, True)
    v = bfr(B, Skv, 64 * H, seed=13).cuda()
    _, lse = ops.attention_fwd(q, k, v, H, q_prescaled=True)
    got = _sum_groups(ops.attention_colsum(q, k, lse, H, q_prescaled=True)).cpu()
    close_f32(f"forward + colsum {shape}", got, want, rtol=3e-3, atol=1e-4)


def test_colsum_writes_nothing_else_and_ignores_padding_rows(ops):
    B, H, Sq, Skv = 1, 2, 91, 91
    (q, k), lse, _ = _case(B, H, Sq, Skv, False)
    G = ops.attention_colsum_groups(B, H, Sq, Skv)
    n = B * G * Skv
    buf = torch.full((n + 256,), 777.0, device="cuda")
    part = ops.attention_colsum(q, k, lse, H, out=buf)
    assert part.data_ptr() == buf.data_ptr() and torch.equal(buf[n:], torch.full((256,), 777.0, device="cuda"))
    assert torch.isfinite(part).all() and not (part == 777.0).any()
    # rows past Sq / Skv of an over-allocated buffer are legal padding: NaNs there change nothing
    pad = 37
    qb = torch.full((B, Sq + pad, 64 * H), float("nan"), dtype=BF, device="cuda")
    kb = torch.full((B, Skv + pad, 64 * H), float("nan"), dtype=BF, device="cuda")
    qb[:, :Sq], kb[:, :Skv] = q, k
    assert torch.equal(ops.attention_colsum(qb[:, :Sq], kb[:, :Skv], lse, H), part)
    # B = 2, three heads, a ragged last key block and query tile: nothing past [B][G][Skv]
    (q, k), lse, _ = _case(2, 3, 129, 129, True)
    n = 2 * ops.attention_colsum_groups(2, 3, 129, 129) * 129
    buf = torch.full((n + 256,), 777.0, device="cuda")
    ops.attention_colsum(q, k, lse, 3, q_prescaled=True, out=buf)
    assert torch.equal(buf[n:], torch.full((256,), 777.0, device="cuda")) and not (buf[:n] == 777.0).any()


def test_colsum_refusals(ops):
    from pea_diffusion_amd._lib import PeaError
    (q, k), lse, _ = _case(1, 2, 64, 64, False)
    with pytest.raises(PeaError, match="head_dim"):
        ops.attention_colsum(q, k, lse, 1)
    with pytest.raises(PeaError, match="lse"):
        ops.attention_colsum(q, k, lse[:, :1], 2)
    with pytest.raises(PeaError, match="null lse"):
        ops.attention_colsum(q, k, None, 2)
    with pytest.raises(PeaError, match="out"):
        ops.attention_colsum(q, k, lse, 2, out=torch.empty(8, device="cuda"))


# ---------------------------------------------------------------------------------------------- degrade and combine
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


COEF = tuple(_f32(v) for v in (5.9905, -5.9064, 0.16693, 0.98597))   # a DPM step at sigma 5.9: c_x, c_e, o_b, o_e


@functools.lru_cache(maxsize=None)
def _degrade_case(HW, hw, G, kind):
    """B = 2, C = 4.  part fp32 [B, G, h w] whose ascending sum is below 1 everywhere (kind "none"), above 1 everywhere ("all")
    or 0.5 .. 1.5 ("mixed")"""
    from pea_diffusion_amd.sag import nearest_tables
    g = torch.Generator().manual_seed(HW[0] * 1000 + HW[1] + G)
    B, C = 2, 4
    x, eps = 3.0 * torch.randn(B, C, *HW, generator=g), torch.randn(B, C, *HW, generator=g)
    A = {"none": 0.2, "all": 1.2, "mixed": 0.5}[kind] + (0.6 if kind != "mixed" else 1.0) * torch.rand(B, hw[0] * hw[1], generator=g)
    frac = torch.rand(B, G, hw[0] * hw[1], generator=g) + 0.1
    part = (A[:, None] * frac / frac.sum(1, keepdim=True)).contiguous()
    mask = (_sum_groups(part) > 1.0).view(B, *hw)
    iy, ix = nearest_tables(hw[0], hw[1], HW[0], HW[1])
    return x, eps, part, mask, iy.cuda(), ix.cuda()


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("HW,hw", [((5, 5), (3, 3)), ((8, 8), (2, 2)), ((56, 104), (7, 13)), ((128, 128), (32, 32))])
def test_sag_degrade_against_the_restatement(ops, HW, hw, G):
    for kind in ("none", "all", "mixed"):
        x, eps, part, mask, iy, ix = _degrade_case(HW, hw, G, kind)
        assert {"none": not mask.any(), "all": bool(mask.all()), "mixed": bool(mask.any() and not mask.all())}[kind]
        got = ops.sag_degrade(x.cuda(), eps.cuda(), part.cuda(), hw, iy, ix, *COEF).cpu()
        close_f32(f"sag_degrade {HW} from {hw} G={G} {kind}", got, degrade_ref(x, eps, mask, *COEF))
        if kind == "none":                                           # the written formula, every product and sum rounded once
            c_x, c_e, o_b, o_e = COEF
            assert torch.equal(got, o_b * (c_x * x + c_e * eps) + o_e * eps)
        if kind == "mixed":                                          # where the mask is false the same bits, where it is true others
            c_x, c_e, o_b, o_e = COEF
            plain = o_b * (c_x * x + c_e * eps) + o_e * eps
            up = mask[:, None].float()
            up = torch.nn.functional.interpolate(up, size=HW, mode="nearest").expand_as(x) > 0.5
            assert torch.equal(got[~up], plain[~up]) and not torch.equal(got[up], plain[up])


def test_sag_degrade_refusals(ops):
    from pea_diffusion_amd._lib import PeaError
    x, eps, part, mask, iy, ix = _degrade_case((8, 8), (2, 2), 1, "mixed")
    with pytest.raises(PeaError, match="reflect padding"):
        ops.sag_degrade(x[:, :, :4].contiguous().cuda(), eps[:, :, :4].contiguous().cuda(), part.cuda(), (2, 2), iy[:4].contiguous(), ix, *COEF)
    with pytest.raises(PeaError, match="index tables"):
        ops.sag_degrade(x.cuda(), eps.cuda(), part.cuda(), (2, 2), iy[:4].contiguous(), ix, *COEF)
    with pytest.raises(PeaError, match="part"):
        ops.sag_degrade(x.cuda(), eps.cuda(), part.cuda(), (3, 2), iy, ix, *COEF)


def test_cfg_sag_combine(ops):
    g = torch.Generator().manual_seed(5)
    B = 2
    e2, d = torch.randn(2 * B, 4, 24, 20, generator=g), torch.randn(B, 4, 24, 20, generator=g)
    for gs, s in ((5.0, 0.75), (7.5, 1.0), (1.5, 0.0)):
        close_f32(f"cfg_sag_combine g={gs} s={s}", ops.cfg_sag_combine(e2.cuda(), d.cuda(), gs, s), combine_ref(e2, d, gs, s))
        assert torch.equal(ops.cfg_sag_combine(e2.cuda(), d.cuda(), gs, 0.0), ops.cfg_combine(e2.cuda(), gs))    # s = 0: cfg_combine's bits
    close_f32("sag_combine without CFG", ops.cfg_sag_combine(e2[:B].cuda(), d.cuda(), 0.0, 0.75, do_cfg=False), combine_ref(e2[:B], d, 0.0, 0.75, False))
    assert torch.equal(ops.cfg_sag_combine(e2[:B].cuda(), d.cuda(), 0.0, 0.0, do_cfg=False).cpu(), e2[:B])
    odd = torch.randn(2, 3, 7, generator=g)                          # a ragged element count
    close_f32("cfg_sag_combine ragged", ops.cfg_sag_combine(torch.cat([odd, -odd]).cuda(), odd.cuda(), 3.0, 0.5),
              combine_ref(torch.cat([odd, -odd]), odd, 3.0, 0.5))


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
CTX_GAIN = 5.0                                                       # as tests/test_attn_maps_gpu.py: unscaled, the storage floor is degenerate
MASK_SHARE_CAP = 0.10                                                # entries within the limit of 1 (module docstring: 6.2 % measured)
MID = "mid_block.attentions.0.transformer_blocks.0.attn1"


def _setup(B, L=77, hw=16):
    from test_ip_adapter_gpu import _tiny_ip_pair
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    t = t[1:2].expand(B).contiguous()
    ehs = (CTX_GAIN * ehs).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    return cfg, ref, hip, run_ref, run


def _oracle_colsum(ref, name, run_ref):
    """-> (A fp32, A under bf16 storage) of layer `name`, each [B, S]"""
    from oracle.bf16_store import bf16_storage
    m = attach_sag(ref, name)
    with torch.no_grad():
        m.record = []
        run_ref()
        want = m.record[0]
        with bf16_storage():
            m.record = []
            run_ref()
            stored = m.record[0]
    m.record = None
    return want, stored


def _check_colsum(tag, got, want, stored):
    floor, floor_abs = rel_l2(stored, want), float((stored - want).abs().max())
    limit, limit_abs = STORAGE_FLOOR_FACTOR * floor, STORAGE_FLOOR_FACTOR * floor_abs
    e = rel_l2(got, want)
    near = (want - 1.0).abs() < limit_abs
    flips = (got > 1.0) != (want > 1.0)
    print(f"[{tag}] column sums {float(want.min()):.3f} .. {float(want.max()):.3f}, rel_l2={e:.3e}, bf16-storage floor {floor:.3e} "
          f"(ratio {e / floor:.2f}, limit {limit:.3e}); largest entry floor {floor_abs:.3e}: {int(near.sum())} of {near.numel()} entries "
          f"({float(near.float().mean()):.1%}) within {limit_abs:.3e} of 1, {int(flips.sum())} mask entries differ")
    assert floor >= FLOOR_DEGENERATE, floor
    assert e <= limit, (e, limit)
    assert not (flips & ~near).any()                                 # the masks differ only where the oracle cannot tell either
    assert float(near.float().mean()) <= MASK_SHARE_CAP
    assert 0.25 <= float((want > 1.0).float().mean()) <= 0.75         # ... and it is a mask: neither empty nor full


def test_tiny_unet_sag_capture(gpu):
    """capture on: the same eps, bit for bit; the column sums against the oracle's; the default layer and one by index"""
    from pea_diffusion_amd import style_aligned as sa
    B = 2
    cfg, ref, hip, run_ref, run = _setup(B)
    before = run()
    names = sa.layer_names(hip)
    for layer, name, samples in ((None, MID, None), (names.index("up_blocks.1.attentions.0.transformer_blocks.0.attn1"), None, (1, 1))):
        name = name or names[layer]
        hip.enable_sag(layer, samples=samples)
        assert torch.equal(run(), before)                            # the ordinary launch, its decision and its O do not change
        part = hip.sag_colsum()
        first, count = samples or (0, B)
        assert part.shape[0] == count and part.dtype == torch.float32
        got = part.sum(1).cpu()
        run()
        assert torch.equal(hip.sag_colsum(), part)                   # bit-reproducible
        want, stored = _oracle_colsum(ref, name, run_ref)
        assert tuple(got.shape) == (count, want.shape[1])
        close_f32(f"mass of {name}", got.sum(1), torch.full((count,), float(want.shape[1])))
        _check_colsum(f"tiny unet, column sums of {name}", got, want[first:first + count], stored[first:first + count])
        hip.release_activations()                                    # the lse and partial buffers are not part of the arenas
        assert torch.equal(run(), before) and torch.equal(hip.sag_colsum(), part)
        hip.disable_sag()
        assert torch.equal(run(), before)                            # the bits from before come back


def test_tiny_unet_sag_refusals(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd import style_aligned as sa
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.prompt2prompt import PromptEdit
    from pea_diffusion_amd.sag import denoise_sag
    from pea_diffusion_amd.unet import HipUNet
    grad = HipUNet(pc.tiny_config(), 2, 16, 16, 77, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.enable_sag()
    B, L = 2, 77
    cfg, ref, hip, run_ref, run = _setup(B, L)
    before = run()
    names = sa.layer_names(hip)
    with pytest.raises(PeaError, match="self-attention layers"):
        hip.enable_sag(len(names))
    with pytest.raises(PeaError, match="samples"):
        hip.enable_sag(samples=(1, 2))
    with pytest.raises(PeaError, match="names no self-attention layer"):
        hip.enable_sag("up_blocks.9")
    with pytest.raises(PeaError, match="enable_sag first"):
        hip.sag_colsum()
    edit = PromptEdit.compose(L, 2, [None, dict(source=0)])
    hip.set_prompt_edit(edit)
    with pytest.raises(PeaError, match="prompt editing"):
        hip.enable_sag()                                             # set while a prompt edit is live
    hip.clear_prompt_edit()
    hip.enable_sag()
    hip.set_prompt_edit(edit)                                        # ... and an edit that arrives afterwards: the forward refuses
    with pytest.raises(PeaError, match="prompt editing"):
        run()
    hip.clear_prompt_edit()
    assert torch.equal(run(), before)
    # StyleAligned on the captured layer: refused by the forward; on the other layers: welcome
    hip.set_style_aligned(layers=[MID])
    with pytest.raises(PeaError, match="StyleAligned"):
        run()
    hip.set_style_aligned(layers=[n for n in names if n != MID])
    shared = run()
    assert torch.equal(shared[0], before[0]) and not torch.equal(shared[1], before[1])
    hip.disable_sag()
    assert torch.equal(run(), shared)
    hip.set_style_aligned(layers=[MID])
    with pytest.raises(PeaError, match="StyleAligned"):
        hip.enable_sag()                                             # ... and refused when capture is switched on behind it
    hip.clear_style_aligned()
    assert torch.equal(run(), before)
    with pytest.raises(PeaError, match="guidance_rescale"):
        denoise_sag(hip, hip, None, torch.zeros(2, 4, 16, 16), None, None, guidance_rescale=0.5)
    # a UNet whose self-attention heads are not 64 wide
    h15 = HipUNet(pc.tiny15_config(), 2, 16, 16, 77)
    with pytest.raises(PeaError, match="head_dim"):
        h15.enable_sag(0)


@pytest.mark.parametrize("sched,g", [("dpm", 5.0), ("euler", 0.0)])
def test_denoise_sag_tiny_vs_oracle(gpu, sched, g):
    """3 steps of sag.denoise_sag against the restated loop: DPM-Solver under CFG (UNet batch 2B and a batch-B context sharing its
    weights for the degraded pass), Euler without CFG (one context for both passes).  The oracle's masks are its own except at the
    entries within the per-step limit of 1 (module docstring), where it is handed the device's decision: measured 2 - 3 % (DPM)
    and 6 - 8 % (Euler) of the 3 x 32 entries, and no other entry differs."""
    from oracle.bf16_store import bf16_storage
    from oracle.sampler_ref import DPMSolverMultistepRef
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.sag import denoise_sag
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerDiscrete
    from pea_diffusion_amd.unet import HipUNet
    from test_ip_adapter_gpu import _tiny_ip_pair
    from turbo_ref import EulerRef
    B, L, n, s = 2, 77, 3, 0.75
    UB = 2 * B if g > 1.0 else B
    cfg, ref, hip = _tiny_ip_pair(UB, L)
    x, _, ehs, added = cond_inputs(cfg, UB, L, 16)
    x, ehs = x[:B], (CTX_GAIN * ehs).to(BF).float()
    hip_sag = HipUNet(pc.tiny_config(), B, 16, 16, L, share_weights_from=hip) if UB != B else hip
    mod = attach_sag(ref, MID)
    make = (lambda: DPMSolverMultistepRef()) if sched == "dpm" else (lambda: EulerRef(False))
    kind = "alpha" if sched == "dpm" else "sigma"
    # the device loop, keeping every step's column sums
    seen = []
    colsum = hip.sag_colsum
    hip.sag_colsum = lambda: seen.append(colsum()) or seen[-1]
    run = lambda: denoise_sag(hip, hip_sag, DPMSolverMultistep() if sched == "dpm" else EulerDiscrete(), x.cuda(), ehs.cuda(),
                              {k: v.cuda() for k, v in added.items()}, sag_scale=s, num_inference_steps=n, guidance_scale=g)
    got = run()
    dev_A = [p.sum(1).cpu() for p in seen]
    del hip.sag_colsum
    assert len(dev_A) == n and torch.equal(run(), got)               # bit-reproducible

    def loop(fix=None, A_out=None):
        return denoise_sag_ref(lambda *a, **k: ref(*a, **k), mod, make(), x.clone(), ehs, added, n, g, s, (4, 4), kind=kind,
                               mask_fix=fix, A_out=A_out).float()
    # per step: the elementwise floor of the oracle's column sums, its own masks in both modes
    A32, A16 = [], []
    with torch.no_grad():
        loop(A_out=A32)
        with bf16_storage():
            loop(A_out=A16)
    limits = [STORAGE_FLOOR_FACTOR * float((a - b).abs().max()) for a, b in zip(A16, A32)]
    left_out, differ = [], []

    def fix(i, A, mask):
        near = ((A - 1.0).abs() < limits[i]).view_as(mask)
        dev = (dev_A[i] > 1.0).view_as(mask)
        left_out.append(float(near.float().mean()))
        differ.append(int(((dev != mask) & ~near).sum()))
        return torch.where(near, dev, mask)
    with torch.no_grad():
        want = loop(fix)
        with bf16_storage():
            stored = loop(fix)
        mod.record = None
        plain = loop(lambda i, A, mask: torch.zeros_like(mask))      # no entry degraded: the guidance term is nearly nothing
    floor = rel_l2(stored, want)
    limit, rule = _floor_limit("tiny", floor)
    e = rel_l2(got, want)
    print(f"[denoise_sag tiny, {sched} {n} steps, guidance {g}, sag {s}] latents rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio "
          f"{e / max(floor, 1e-30):.2f}, limit {limit:.3e} ({rule}); per step: mask limits {[f'{v:.1e}' for v in limits]}, entries left "
          f"out {[f'{v:.1%}' for v in left_out[:n]]}, other entries that differ {differ[:n]}; the degrade moves the oracle's latents "
          f"by {rel_l2(want, plain):.3f}")
    assert torch.isfinite(got).all() and e <= limit
    assert sum(differ[:n]) == 0                                      # outside the limit the device and the oracle decide alike
    assert e < rel_l2(got, plain)                                    # a loop that ignores the mask cannot pass
