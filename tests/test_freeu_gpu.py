"""FreeU on the GPU: the coefficient kernel and the fused concat against float64 at every shape class, the filter's literal
properties through the kernel, and `HipUNet.enable_freeu` against the fp32 oracle with FreeU bound onto its first two up blocks
(tests/freeu_ref.py)."""
import math

import pytest
import torch

from freeu_ref import fourier_filter, freeu_sums, freeu_unet, unfreeu_unet
from test_model_gpu import STORAGE_FLOOR_FACTOR, rel_l2, round_weights_bf16_
from test_ops_gpu import close_bf16, close_f32
from test_turbo_gpu import EPS_LIMIT, FLOOR_DEGENERATE

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X")
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------- op level
#         id            B   H   W   C1    C2   a depth-to-space   a is b
SHAPES = {"smallest": (1, 2, 2, 16, 8, False, False),          # H = 2: bin -1 is the Nyquist bin
          "odd": (2, 5, 7, 64, 24, False, False),              # C2 below a wave's channel span
          "d2s": (3, 6, 10, 128, 64, True, False),
          "same-tensor": (3, 6, 10, 64, 64, False, True),      # one tensor in both roles, hence C1 == C2
          "up0": (2, 32, 32, 1280, 640, False, False),
          "up1": (1, 64, 64, 640, 320, False, False)}          # the multi-slab reduction
FACTORS = [(0.5, 1.5), (0.2, 1.0), (1.0, 1.4)]
_cases = {}


def _case(name):
    """inputs and the float64 reference of one shape, made once: bf16 maps with a DC offset (S00 dominates, the other sums
    cancel), the skip's low-frequency part `low` = filter(skip, s = 2) - skip by torch.fft, so that filter(skip, s) =
    skip + (s - 1) low for every s, and the seven sums"""
    if name not in _cases:
        B, H, W, C1, C2, d2s, same = SHAPES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        b = (torch.randn(B, H, W, C2, generator=g) * 0.7 + 1.5).to(BF)
        a = b if same else (torch.randn(B, H, W, C1, generator=g) * 0.7 + 1.5).to(BF)
        b64 = b.double().permute(0, 3, 1, 2)
        low = (fourier_filter(b64, 1, 2.0) - b64).permute(0, 2, 3, 1).reshape(B * H * W, C2)
        _cases[name] = dict(a=a, b=b, low=low, coef=freeu_sums(b64)[0])
    return _cases[name]


def _run(ops, name, s, bs):
    """-> (y, coef) with every output buffer pre-filled with NaN, so that an unwritten element shows"""
    B, H, W, C1, C2, d2s, same = SHAPES[name]
    c = _case(name)
    bd = c["b"].cuda()
    ad = bd if same else (ops.nhwc_to_d2s(c["a"].cuda()) if d2s else c["a"].cuda())
    nan = lambda *shape, dtype: torch.full(shape, float("nan"), device="cuda", dtype=dtype)
    nbytes = ops.freeu_scratch_bytes(B, H, W, C2)
    y, coef = ops.freeu_concat(ad, bd, s, bs, d2s=d2s, y=nan(B * H * W, C1 + C2, dtype=BF), coef=nan(B, 7, C2, dtype=torch.float32),
                               scratch=nan(max(nbytes // 4, 1), dtype=torch.float32))
    return y, coef


@pytest.mark.parametrize("s,bs", FACTORS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_freeu_concat_vs_float64(gpu, name, s, bs):
    from pea_diffusion_amd import ops
    B, H, W, C1, C2, d2s, same = SHAPES[name]
    c = _case(name)
    a2, b2 = c["a"].reshape(-1, C1), c["b"].reshape(-1, C2)
    y, coef = _run(ops, name, s, bs)
    y = y.cpu()
    h = C1 // 2
    close_bf16(f"freeu {name} s={s} b={bs}: scaled half", y[:, :h], a2[:, :h].double() * bs, ulps=1)
    close_bf16(f"freeu {name} s={s} b={bs}: copied half", y[:, h:C1], a2[:, h:].double(), ulps=1)
    close_bf16(f"freeu {name} s={s} b={bs}: filtered skip", y[:, C1:], b2.double() + (s - 1.0) * c["low"], ulps=1)
    assert torch.equal(y[:, h:C1].view(torch.int16), a2[:, h:].view(torch.int16))
    if s == 1.0:
        assert coef is None and torch.equal(y[:, C1:].view(torch.int16), b2.view(torch.int16))
    else:
        # the fp32 rule for a kernel's fp32 results; the sums run over H W values, the absolute part scales with that
        close_f32(f"freeu {name}: coefficients", coef, c["coef"], rtol=1e-3, atol=1e-4 * H * W)
    if bs == 1.0:
        assert torch.equal(y[:, :h].view(torch.int16), a2[:, :h].view(torch.int16))
    y2, coef2 = _run(ops, name, s, bs)
    assert torch.equal(y2.cpu().view(torch.int16), y.view(torch.int16))                 # bit-reproducible
    assert coef is None or torch.equal(coef2.view(torch.int32), coef.view(torch.int32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_freeu_concat_with_unit_factors_is_concat2(gpu, name):
    from pea_diffusion_amd import ops
    B, H, W, C1, C2, d2s, same = SHAPES[name]
    c = _case(name)
    y, coef = _run(ops, name, 1.0, 1.0)
    bd = c["b"].cuda()
    ad = bd if same else (ops.nhwc_to_d2s(c["a"].cuda()) if d2s else c["a"].cuda())
    want = ops.concat2(ad, bd, d2s_hw=(H, W) if d2s else None)
    assert coef is None and torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_reduction_paths(gpu):
    """up block 1's production map takes the split reduction (the scratch holds [B][slabs][7][C2] partials, slabs > 1); the
    small maps take one slab and no scratch"""
    from pea_diffusion_amd import ops
    B, H, W, C1, C2, _, _ = SHAPES["up1"]
    assert ops.freeu_scratch_bytes(B, H, W, C2) // (4 * 7 * B * C2) > 1
    B, H, W, C1, C2, _, _ = SHAPES["up0"]
    assert ops.freeu_scratch_bytes(B, H, W, C2) // (4 * 7 * B * C2) > 1
    for name in ("smallest", "odd", "d2s"):
        B, H, W, C1, C2, _, _ = SHAPES[name]
        assert ops.freeu_scratch_bytes(B, H, W, C2) == 0


@pytest.mark.parametrize("s", [0.2, 0.5, 1.6])
def test_filter_properties_through_the_kernel(gpu, s):
    """the literals of tests/test_freeu_cpu.py: a constant map leaves as s times itself, a frequency-2 cosine at W = 10 as itself,
    sin(2 pi y / H) as (1 + s) / 2 times itself -- each within the bf16 rule of the expected map (the maps are bf16 values:
    their rounding residue, 2^-9 relative, is spread over all frequencies and far inside that rule)"""
    from pea_diffusion_amd import ops
    B, H, W, C = 2, 6, 10, 16
    yy = torch.arange(H, dtype=F64)[:, None].expand(H, W)
    xx = torch.arange(W, dtype=F64)[None, :].expand(H, W)
    maps = {"constant": (torch.full((H, W), 1.25, dtype=F64), s),
            "cos 2 tx": (torch.cos(2 * math.pi * 2 * xx / W), 1.0),
            "sin ty": (torch.sin(2 * math.pi * yy / H), (1 + s) / 2)}
    a = torch.zeros(B, H, W, 16, dtype=BF, device="cuda")
    for tag, (m, k) in maps.items():
        amp = torch.linspace(0.5, 2.0, B * C, dtype=F64).reshape(B, 1, 1, C)
        b = (m[None, :, :, None] * amp).to(BF)
        y, _ = ops.freeu_concat(a, b.cuda(), s, 1.0)
        close_bf16(f"freeu property '{tag}' s={s}", y[:, 16:], (b.double() * k).reshape(-1, C), ulps=1)


# ---------------------------------------------------------------------------------------------- model level
S1, S2, B1, B2 = 0.5, 0.2, 1.5, 1.4


def _inputs(cfg, B, L, H, W, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 4, H, W, generator=g)
    t = torch.tensor([10, 250, 500, 999][:B])
    ehs = torch.randn(B, L, cfg.cross_attention_dim, generator=g).to(BF).float()
    added = None
    if cfg.addition_embed_type == "text_time":
        added = {"text_embeds": torch.randn(B, cfg.pooled_dim, generator=g),
                 "time_ids": torch.tensor([[H * 8, W * 8, 0, 0, H * 8, W * 8]] * B)}
    return x, t, ehs, added


def _pair(name, B, H, W, L, **hip_kw):
    """the oracle with torch's default initialisation (seed 0), weights rounded to bf16, and a HipUNet holding them: the fill
    of tests/test_turbo_gpu.py / test_model_gpu.make_pair, at a latent that need not be square"""
    from oracle import unet_ref
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.unet import HipUNet
    cfg = getattr(unet_ref, name)()
    torch.manual_seed(0)
    ref = unet_ref.UNet2DConditionRef(cfg)
    round_weights_bf16_(ref)
    for p in ref.parameters():
        p.requires_grad_(False)
    hip = HipUNet(getattr(pc, name)(), B, H, W, L, **hip_kw)
    missing, unexpected = hip.load_state_dict(ref.state_dict())
    assert not missing and not unexpected
    return cfg, ref, hip


def _limit(floor):
    return EPS_LIMIT if floor < FLOOR_DEGENERATE else STORAGE_FLOOR_FACTOR * floor


def _oracle(ref, call, factors):
    """eps of the fp32 oracle with FreeU at `factors`, and of the same oracle in bf16-storage mode"""
    from oracle.bf16_store import bf16_storage
    freeu_unet(ref, *factors)
    try:
        with torch.no_grad():
            want = call(ref)
            with bf16_storage():
                stored = call(ref)
    finally:
        unfreeu_unet(ref)
    return want, stored


def _validity(tag, ref, call, want, limit):
    """a condition on the test, not a measurement of the kernels: on the oracle alone, each of the four factors set to 1 moves
    the output by at least 1.5 x the limit in use, so a path that forgets one factor or one up block cannot pass"""
    moves = {}
    for k, fname in enumerate(("s1", "s2", "b1", "b2")):
        f = [S1, S2, B1, B2]
        f[k] = 1.0
        freeu_unet(ref, *f)
        try:
            with torch.no_grad():
                moves[fname] = rel_l2(call(ref), want)
        finally:
            unfreeu_unet(ref)
    print(f"[{tag}] oracle alone, one factor set to 1 moves eps by " + ", ".join(f"{k} {v:.3e}" for k, v in moves.items())
          + f"; needed {1.5 * limit:.3e}")
    assert min(moves.values()) >= 1.5 * limit, f"invalid test: {moves} against 1.5 x {limit}"


@pytest.mark.parametrize("name,H,W", [("tiny_config", 16, 16), ("tiny_config", 24, 40), ("tiny15_config", 16, 16)])
def test_unet_with_freeu_vs_oracle(gpu, name, H, W):
    """tiny15: up block 0 is an UpBlock2D on a 2 x 2 map.  Fails on a HipUNet without the switch: FreeU moves the oracle's eps by
    9e-2 to 1.8e-1 at these factors, against a limit near 1.3e-2."""
    B, L = 2, 77
    cfg, ref, hip = _pair(name, B, H, W, L)
    x, t, ehs, added = _inputs(cfg, B, L, H, W)
    call = lambda m: m(x, t, ehs, added_cond_kwargs=added)[0]
    cadd = None if added is None else {k: v.cuda() for k, v in added.items()}
    run = lambda u: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    want, stored = _oracle(ref, call, (S1, S2, B1, B2))
    with torch.no_grad():
        plain = call(ref)
    floor = rel_l2(stored, want)
    limit = _limit(floor)
    tag = f"freeu {cfg.name} {H}x{W}"
    _validity(tag, ref, call, want, limit)
    h_plain = run(hip)
    hip.enable_freeu(S1, S2, B1, B2)
    assert hip.freeu == (S1, S2, B1, B2)
    got = run(hip)
    e = rel_l2(got, want)
    print(f"[{tag}] eps rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio {e / max(floor, 1e-30):.2f}, limit {limit:.3e}; "
          f"FreeU moves eps by {rel_l2(want, plain):.3e} (oracle) / {rel_l2(got, h_plain):.3e} (hip)")
    assert torch.isfinite(got).all() and e <= limit
    assert torch.equal(run(hip), got)                                   # bit-reproducible
    hip.release_activations()                                           # the coefficient buffer lives outside the arenas
    assert torch.equal(run(hip), got)
    hip.disable_freeu()
    assert hip.freeu is None and torch.equal(run(hip), h_plain)


def test_toggling(gpu):
    """off again is a context that never had it, bit for bit; enabling twice runs the last factors; a context sharing the
    weights carries its own switch"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    B, L = 2, 12
    cfg, ref, hip = _pair("tiny_config", B, 16, 16, L)
    x, t, ehs, added = _inputs(cfg, B, L, 16, 16)
    cadd = {k: v.cuda() for k, v in added.items()}
    run = lambda u: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].clone()
    never = HipUNet(pc.tiny_config(), B, 16, 16, L, share_weights_from=hip)
    p0 = run(never)
    assert torch.equal(run(hip), p0)
    hip.enable_freeu(S1, S2, B1, B2)
    first = run(hip)
    assert not torch.equal(first, p0) and torch.equal(run(never), p0)   # the twin did not follow
    hip.enable_freeu(0.9, 0.6, 1.1, 1.2)
    second = run(hip)
    assert not torch.equal(second, first) and not torch.equal(second, p0)
    never.enable_freeu(s1=0.9, s2=0.6, b1=1.1, b2=1.2)
    assert torch.equal(run(never), second)
    hip.enable_freeu(S1, S2, B1, B2)
    assert torch.equal(run(hip), first)
    hip.enable_freeu(1.0, 1.0, 1.0, 1.0)                                # unit factors: the fused concat's copy path
    assert torch.equal(run(hip), p0)
    hip.disable_freeu()
    never.disable_freeu()
    assert torch.equal(run(hip), p0) and torch.equal(run(never), p0)
    for bad in [(float("nan"), S2, B1, B2), (S1, float("inf"), B1, B2), (S1, S2, 0.0, B2), (S1, S2, B1, -1.0)]:
        with pytest.raises(PeaError, match="finite and positive"):
            hip.enable_freeu(*bad)
    assert hip.freeu is None and torch.equal(run(hip), p0)


def test_map_too_small_is_refused(gpu):
    """tiny15 has four levels: at an 8 x 8 latent up block 0 works on a 1 x 1 map, where the reference's window is degenerate"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    hip = HipUNet(pc.tiny15_config(), 1, 8, 8, 12)
    with pytest.raises(PeaError, match="1 x 1 map"):
        hip.enable_freeu(S1, S2, B1, B2)
    assert hip.freeu is None


def test_freeu_with_controlnet_residuals(gpu):
    """the residuals are in the skip tensors when the filter reads them, as in diffusers (added in front of the up path)"""
    B, L, H, W = 2, 12, 16, 16
    cfg, ref, hip = _pair("tiny_config", B, H, W, L, residual_inputs=True)
    x, t, ehs, added = _inputs(cfg, B, L, H, W)
    g = torch.Generator().manual_seed(5)
    res = [(torch.randn(B, C, h, w, generator=g) * 0.5).to(BF).float() for C, h, w in hip.residual_shapes()]
    down, mid = res[:-1], res[-1]
    call = lambda m: m(x, t, ehs, added_cond_kwargs=added, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0]
    cadd = {k: v.cuda() for k, v in added.items()}
    run = lambda u: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd, down_block_additional_residuals=[r.cuda() for r in down],
                      mid_block_additional_residual=mid.cuda())[0].clone()
    want, stored = _oracle(ref, call, (S1, S2, B1, B2))
    floor = rel_l2(stored, want)
    limit = _limit(floor)
    with torch.no_grad():
        no_res = _oracle(ref, lambda m: m(x, t, ehs, added_cond_kwargs=added)[0], (S1, S2, B1, B2))[0]
    hip.enable_freeu(S1, S2, B1, B2)
    got = run(hip)
    e = rel_l2(got, want)
    print(f"[freeu + residuals tiny] eps rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, limit {limit:.3e}; the residuals move the "
          f"oracle's eps by {rel_l2(want, no_res):.3e}")
    assert rel_l2(want, no_res) >= 1.5 * limit                         # the residuals matter to the case
    assert torch.isfinite(got).all() and e <= limit


def test_training_contexts_refuse_and_stay_as_they_were(gpu):
    from pea_diffusion_amd._lib import PeaError
    from test_model_gpu import _train_pair
    cfg, us, ut, ad_ref, ad_hip, hs, ht, batch, tr = _train_pair(2, 12)
    before = tr.training_step(batch, 0, sync=True)
    with pytest.raises(PeaError, match="inference feature"):
        hs.enable_freeu(S1, S2, B1, B2)
    assert hs.freeu is None
    after = tr.training_step(batch, 0, sync=True)
    for k in tr.LOG_KEYS:
        assert float(after[k]) == float(before[k]), k
