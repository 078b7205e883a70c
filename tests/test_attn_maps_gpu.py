"""-m gpu: cross-attention heat maps -- the kernel (pea_op_attention_maps) against the fp32 restatement of tests/attn_maps_ref.py,
its exactness properties, and the UNet runtime (HipUNet.enable_attention_maps, attention_maps.heat_maps) against the oracle
with recording attention modules.

Tolerance of the kernel: the maps are fp32 results of bf16 inputs (no bf16 rounding of P), so the project's rule for fp32-stored
results applies, rtol 1e-3 / atol 1e-4; and every (b, q) column sums to 1 within 2e-5: H rows of at most 128 fp32 terms, each
row normalised by its own sum."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
from attn_maps_ref import attach_maps, level_sums, maps_ref, reset_maps  # noqa: E402
from test_ip_adapter_gpu import _inputs, _tiny_ip_pair  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import ALPHA, BF, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import _floor_limit  # noqa: E402

SHAPES = [(1, 1, 1, 1), (2, 2, 16, 16), (1, 3, 200, 32), (1, 2, 129, 33), (1, 3, 128, 77), (1, 2, 364, 65), (2, 5, 300, 96),
          (1, 2, 260, 128), (2, 20, 1024, 77), (2, 10, 4096, 77)]


@functools.lru_cache(maxsize=None)
def _case(B, H, Sq, Skv, prescaled, gain=1, kv_len=None):
    """inputs as test_ip_adapter_gpu._inputs makes them (q times `gain`, a power of two: exact in bf16) and the fp32 maps, once"""
    q, k, _, _, _ = _inputs(B, H, Sq, Skv, 1, False)
    q = q * gain
    if prescaled:
        q = (q.float() * ALPHA).to(BF)
    qr = q.float() / ALPHA if prescaled else q.float()
    return (q.cuda(), k.cuda()), maps_ref(qr, k.float(), H, kv_len=None if kv_len is None else list(kv_len))


def _check(name, got, ref):
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
    col = (got.sum(1).cpu() - 1.0).abs().max().item()
    print(f"[{name}] worst |sum_key M - 1| = {col:.3e}")
    close_f32(name, got, ref)
    assert col <= 2e-5, col


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv", SHAPES)
def test_attention_maps_vs_fp32(ops, B, H, Sq, Skv, prescaled):
    (q, k), ref = _case(B, H, Sq, Skv, prescaled)
    m = ops.attention_maps(q, k, H, q_prescaled=prescaled)
    _check(f"attn-maps pre{int(prescaled)} B{B} H{H} Sq{Sq} Skv{Skv}", m, ref)


@pytest.mark.parametrize("prescaled", [False, True])
def test_attention_maps_peaked(ops, prescaled):
    """q times 4: logits of +-30 and more, probabilities above 0.5 -- without the maximum subtraction exp2 overflows"""
    (q, k), ref = _case(1, 3, 128, 77, prescaled, gain=4)
    qh = (q.float().cpu() / ALPHA if prescaled else q.float().cpu()).view(1, 128, 3, 64).transpose(1, 2)
    per_head = torch.softmax(qh @ k.float().cpu().view(1, 77, 3, 64).transpose(1, 2).transpose(-1, -2) * 0.125, -1)
    assert float(per_head.max()) > 0.5                               # (the maps themselves are means over three heads)
    _check(f"attn-maps peaked pre{int(prescaled)}", ops.attention_maps(q, k, 3, q_prescaled=prescaled), ref)


@pytest.mark.parametrize("prescaled", [False, True])
@pytest.mark.parametrize("B,H,Sq,Skv,kv_len", [(2, 3, 200, 77, (77, 52)), (2, 2, 129, 128, (128, 1))])
def test_attention_maps_kv_len(ops, B, H, Sq, Skv, kv_len, prescaled):
    (q, k), ref = _case(B, H, Sq, Skv, prescaled, kv_len=kv_len)
    m = ops.attention_maps(q, k, H, q_prescaled=prescaled, kv_len=torch.tensor(kv_len, dtype=torch.int32).cuda())
    for b, n in enumerate(kv_len):
        assert bool((m[b, n:] == 0.0).all()), b                      # cut keys: exact zeros
    _check(f"attn-maps kv_len {kv_len} pre{int(prescaled)}", m, ref)
    # a NaN in a cut key's row cannot reach a kept key's map
    k2 = k.clone()
    k2[1, kv_len[1]:] = float("nan")
    m2 = ops.attention_maps(q, k2, H, q_prescaled=prescaled, kv_len=torch.tensor(kv_len, dtype=torch.int32).cuda())
    assert torch.equal(m2, m)


@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 3, 128, 77), (1, 2, 364, 65), (2, 5, 300, 96), (2, 20, 1024, 77)])
def test_attention_maps_exactness(ops, B, H, Sq, Skv):
    (q, k), _ = _case(B, H, Sq, Skv, True)
    n = B * Skv * Sq
    a = ops.attention_maps(q, k, H, q_prescaled=True)
    assert torch.equal(ops.attention_maps(q, k, H, q_prescaled=True), a)        # two runs, the same bits
    z = torch.zeros(n, device="cuda")
    assert torch.equal(ops.attention_maps(q, k, H, q_prescaled=True, out=z, accumulate=True), a)
    seed = torch.rand(n, generator=torch.Generator().manual_seed(5)).cuda()
    acc = seed.clone()
    got = ops.attention_maps(q, k, H, q_prescaled=True, out=acc, accumulate=True)
    assert got.data_ptr() == acc.data_ptr()
    assert torch.equal(got, seed.view(B, Skv, Sq) + a)               # one fp32 add per element
    # a larger buffer: nothing past [B][Skv][Sq] is written, in either form
    for accumulate in (False, True):
        big = torch.full((n + 4096,), -7.0, device="cuda")
        big[:n] = seed
        got = ops.attention_maps(q, k, H, q_prescaled=True, out=big, accumulate=accumulate)
        assert bool((big[n:] == -7.0).all())
        assert torch.equal(got, seed.view(B, Skv, Sq) + a if accumulate else a)


def test_attention_maps_wrapper_refusals(ops):
    from pea_diffusion_amd._lib import PeaError
    (q, k), _ = _case(1, 3, 128, 77, True)
    with pytest.raises(PeaError):
        ops.attention_maps(q, k, 3, accumulate=True)                 # nothing to add into
    with pytest.raises(PeaError):
        ops.attention_maps(q, k, 3, out=torch.zeros(10, device="cuda"))
    with pytest.raises(PeaError):
        ops.attention_maps(q, k, 2)                                  # head_dim 96
    with pytest.raises(PeaError, match="1..128 keys"):
        ops.attention_maps(q, torch.zeros(1, 129, 192, dtype=BF, device="cuda"), 3)


# ---------------------------------------------------------------------------------------------- the runtime, tiny UNet
# measured on the CPU, oracle alone: with the context as cond_inputs draws it the tiny UNet's maps are nearly flat (0.045 .. 0.098 over
# five layers at 8 x 8) and the oracle's own bf16-storage floor is 1.0e-3 / 7.7e-4 per level, at the FLOOR_DEGENERATE line; with the
# context scaled by 5, as tests/test_regional_gpu.py scales it, the maps are peaked (up to 0.49 / 0.63) and the floor is 1.1e-2 / 1.0e-2
CTX_GAIN = 5.0


def _setup(B, L=77, hw=16):
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    ehs = (CTX_GAIN * ehs).to(BF).float()
    run_ref = lambda: ref(x, t, ehs, added_cond_kwargs=added)[0]
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    attach_maps(ref)
    return cfg, ref, hip, (x, t, ehs, added), run_ref, run


def _floor_check(tag, got, want, stored):
    """got / want / stored: {(h, w): (tensor, n)} or plain tensors keyed by a name -- per entry, the HIP maps within
    STORAGE_FLOOR_FACTOR x the oracle's own bf16-storage floor"""
    for key in want:
        e, floor = rel_l2(got[key], want[key]), rel_l2(stored[key], want[key])
        limit, how = _floor_limit(tag, floor)
        print(f"[{tag} {key}] maps rel_l2={e:.3e}, bf16-storage floor {floor:.3e}, ratio {e / max(floor, 1e-30):.2f}, limit {how}")
        assert e <= limit, (key, e, floor)


def test_tiny_unet_maps(gpu):
    from oracle.bf16_store import bf16_storage
    B, L = 2, 77
    cfg, ref, hip, _, run_ref, run = _setup(B, L)
    with torch.no_grad():
        reset_maps(ref)
        run_ref()
        want = level_sums(ref, (16, 16))
        reset_maps(ref)
        with bf16_storage():
            run_ref()
        stored = level_sums(ref, (16, 16))
        reset_maps(ref, select=lambda name: name.startswith("up_blocks"))
        run_ref()
        want_up = level_sums(ref, (16, 16))
    assert sorted(want) == [(4, 4), (8, 8)] and sorted(hip.ip_query_counts()) == [16, 64]
    off = run()
    hip.enable_attention_maps()
    on = run()
    assert torch.equal(on, off)                                      # capture does not touch the forward
    first = hip.attention_maps()
    assert sorted(first) == sorted(want)
    for hw, (t, n) in first.items():
        assert tuple(t.shape) == (B, L, *hw) and t.dtype == torch.float32 and n == want[hw][1]
        # every layer-forward adds a probability distribution over the keys
        assert float((t.sum(1) - n).abs().max()) <= 2e-5 * n
    _floor_check("tiny unet", {k: v[0] for k, v in first.items()}, {k: v[0] for k, v in want.items()},
                 {k: v[0] for k, v in stored.items()})
    # a second forward doubles the counters; reset + forward reproduces the first accumulators bit for bit
    run()
    for hw, (t, n) in hip.attention_maps().items():
        assert n == 2 * want[hw][1]
    hip.reset_attention_maps()
    for hw, (t, n) in hip.attention_maps().items():
        assert n == 0 and not bool(t.any())
    assert torch.equal(run(), off)
    again = hip.attention_maps()
    for hw in first:
        assert again[hw][1] == first[hw][1] and torch.equal(again[hw][0], first[hw][0])
    # a layer selection: the up blocks alone
    hip.enable_attention_maps({"up": 1.0})
    assert torch.equal(run(), off) and torch.equal(run(), off)
    sel = hip.attention_maps()
    for hw in want:
        n_up = want_up[hw][1] if hw in want_up else 0
        assert sel[hw][1] == 2 * n_up, (hw, sel[hw][1], n_up)
        if n_up == 0:
            assert not bool(sel[hw][0].any())
    assert sum(n for _, n in want_up.values()) < sum(n for _, n in want.values())
    hip.disable_attention_maps()
    assert torch.equal(run(), off)
    from pea_diffusion_amd._lib import PeaError
    with pytest.raises(PeaError, match="enable_attention_maps"):
        hip.attention_maps()


def test_denoise_three_steps_heat_maps(gpu):
    """sampler.denoise needs no change: enable before the loop, read after it -- the maps are sums over steps"""
    from oracle.bf16_store import bf16_storage
    from oracle.sampler_ref import DPMSolverMultistepRef, denoise_ref
    from pea_diffusion_amd.attention_maps import combine, heat_maps
    from pea_diffusion_amd.sampler import DPMSolverMultistep, denoise
    B, L = 2, 77
    cfg, ref, hip, (x, _, ehs, added), _, _ = _setup(B, L)
    lat = x[:1]
    kw = dict(num_inference_steps=3, guidance_scale=5.0)
    loop = lambda: denoise_ref(lambda *a, **k: ref(*a, **k), DPMSolverMultistepRef(), lat.clone(), ehs, added, **kw)
    with torch.no_grad():
        reset_maps(ref)
        loop()
        want = combine(level_sums(ref, (16, 16)))[B // 2:]
        reset_maps(ref)
        with bf16_storage():
            loop()
        stored = combine(level_sums(ref, (16, 16)))[B // 2:]
    hip.enable_attention_maps()
    out = denoise(hip, DPMSolverMultistep(), lat.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()}, **kw)
    assert torch.isfinite(out).all()
    got = heat_maps(hip, do_cfg=True)
    assert tuple(got.shape) == (1, L, 8, 8)
    for hw, (_, n) in hip.attention_maps().items():
        assert n % 3 == 0 and n > 0
    _floor_check("denoise 3 steps, cfg 5.0", {"heat": got}, {"heat": want}, {"heat": stored})
    assert torch.equal(heat_maps(hip, do_cfg=True, tokens=[3, 0]), got[:, [3, 0]])


def test_tiny_unet_maps_refusals(gpu):
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError, check, lib
    from pea_diffusion_amd.controlnet import HipControlNet
    from pea_diffusion_amd.unet import HipUNet
    from regional_ref import half_masks
    grad = HipUNet(pc.tiny_config(), 2, 16, 16, 77, needs_grad=True)
    with pytest.raises(PeaError, match="PEA_UNET_GRAD"):
        grad.enable_attention_maps()
    narrow = HipUNet(pc.tiny15_config(), 2, 16, 16, 77, needs_grad=False)
    with pytest.raises(PeaError, match="head_dim"):
        narrow.enable_attention_maps()
    long = HipUNet(pc.tiny_config(), 2, 16, 16, 154, needs_grad=False)
    with pytest.raises(PeaError, match="context length 154"):
        long.enable_attention_maps()
    cn = HipControlNet(pc.tiny_config(), 2, 16, 16, 77)
    with pytest.raises(PeaError, match="not a UNet handle"):
        check(lib().pea_unet_enable_attention_maps(cn._h, None, 0))
    # regions and capture together: refused at the forward, whichever came first; either alone runs
    B, L = 2, 128
    cfg, ref, hip = _tiny_ip_pair(B, L)
    x, t, ehs, added = cond_inputs(cfg, B, L, 16)
    run = lambda: hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs={k: v.cuda() for k, v in added.items()})[0].clone()
    before = run()
    hip.enable_attention_maps()
    hip.set_prompt_regions(half_masks(128, 128))
    with pytest.raises(PeaError, match="regional prompts"):
        run()
    hip.clear_prompt_regions()
    assert torch.equal(run(), before)
    with pytest.raises(PeaError, match="layer switches"):
        check(lib().pea_unet_enable_attention_maps(hip._h, (ctypes.c_float * 3)(1, 1, 1), 3))
    with pytest.raises(PeaError):
        hip.enable_attention_maps({"sideways": 1.0})
    hip.disable_attention_maps()
    assert torch.equal(run(), before)
