"""-m gpu: LoRA fusion on the HIP path -- the composition kernel against float64 torch, `HipUNet.fuse_lora / unfuse_lora`
against the CPU oracle UNet with the LoRA merged into its state dict in float64 (pea_diffusion_amd.lora.merged_weight), on
the tiny SDXL-shaped and SD1.5-shaped configs and once on the full SDXL.

So that no test can pass with the LoRA ignored, every random LoRA is scaled so that the ORACLE ALONE moves its eps by more than
ten times the test's limit (asserted on the CPU side of each test).  RHO is the LoRA delta's standard deviation per element
relative to the base weight's; chosen on the CPU: see the measured shifts at each use."""
import pytest
import torch

pytestmark = pytest.mark.gpu
from test_model_gpu import _fast_fill_, cond_inputs, gpu, make_pair, rel_l2, round_weights_bf16_  # noqa: E402,F401


def random_lora(sd, keys, rank, rho, seed=0):
    """{key: (down [r][...], up [Co][r] or [Co][r][1][1])}: delta = up @ down has per-element std rho * std(W)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in keys:
        W = sd[k]
        d0, kf = W.shape[0], W[0].numel()
        down = torch.randn((rank,) + tuple(W.shape[1:]), generator=g) / kf ** 0.5
        up = torch.randn((d0, rank) + ((1, 1) if W.dim() == 4 else ()), generator=g) * (rho * float(W.std()) * kf ** 0.5 / rank ** 0.5)
        out[k] = (down, up)
    return out


def spelled(lora, style, alpha_div=1.0):
    """the same LoRA as a file of that spelling; alpha_div: store alpha = rank / alpha_div and up * alpha_div (same product)"""
    sd = {}
    for k, (down, up) in lora.items():
        mod, rank = k[:-len(".weight")], down.shape[0]
        if style == "diffusers":
            sd[f"unet.{mod}.lora.down.weight"], sd[f"unet.{mod}.lora.up.weight"] = down, up
        elif style == "peft":
            sd[f"base_model.model.{mod}.lora_A.weight"], sd[f"base_model.model.{mod}.lora_B.weight"] = down, up
        else:
            base = "lora_unet_" + mod.replace(".", "_")
            sd[base + ".lora_down.weight"], sd[base + ".lora_up.weight"] = down, up * alpha_div
            sd[base + ".alpha"] = torch.tensor(rank / alpha_div)
    return sd


def merged_oracle(cfg, ref, lora, scale=1.0):
    from oracle.unet_ref import UNet2DConditionRef
    from pea_diffusion_amd.lora import merged_weight
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    for k, (down, up) in lora.items():
        sd[k] = merged_weight(sd[k], [(down, up, scale)])
    with torch.device("meta"):
        m = UNet2DConditionRef(cfg)
    m.load_state_dict(sd, assign=True)
    return m.eval()


# ---------------------------------------------------------------------------------------------- the kernel
COMPOSE_SHAPES = [(1280, 1280, 64), (10240, 1280, 64), (640, 5760, 64), (320, 2880, 4),          # production (Linear, GEGLU, convs)
                  (1280, 1280, 1), (1280, 640, 3), (640, 1280, 200), (77, 2885, 5), (40, 320, 8), (40, 2885, 33)]   # odd


@pytest.mark.parametrize("M,Kf,rank", COMPOSE_SHAPES)
def test_lora_compose_vs_float64(gpu, M, Kf, rank):
    """fp32-stored result: the per-kernel rule of tests/test_ops_gpu.py for fp32 outputs, rtol 1e-3 / atol 1e-4"""
    from pea_diffusion_amd import ops
    g = torch.Generator().manual_seed(M + Kf + rank)
    W = torch.randn(M, Kf, generator=g) / Kf ** 0.5
    down, up = torch.randn(rank, Kf, generator=g), torch.randn(M, rank, generator=g)
    s = 0.37 / rank
    want = W.double() + s * (up.double() @ down.double())
    got = ops.lora_compose(W.cuda(), down.cuda(), up.cuda(), s)
    err = (got.cpu().double() - want).abs().max().item()
    print(f"[lora_compose {M}x{Kf} r{rank}] max abs err {err:.2e}")
    assert torch.allclose(got.cpu().double(), want, rtol=1e-3, atol=1e-4)
    again = ops.lora_compose(W.cuda(), down.cuda(), up.cuda(), s)
    assert torch.equal(got, again)                                   # fixed order, no atomics: bit-reproducible


def test_lora_compose_accumulates_adapters_in_place(gpu):
    from pea_diffusion_amd import ops
    g = torch.Generator().manual_seed(0)
    M, Kf = 640, 2885
    W = torch.randn(M, Kf, generator=g) / Kf ** 0.5
    d1, u1, d2, u2 = (torch.randn(*s, generator=g) for s in [(64, Kf), (M, 64), (7, Kf), (M, 7)])
    want = W.double() + 0.01 * (u1.double() @ d1.double()) - 0.05 * (u2.double() @ d2.double())
    buf = W.cuda().clone()
    out = ops.lora_compose(buf, d1.cuda(), u1.cuda(), 0.01, out=buf)      # acc == out
    out = ops.lora_compose(buf, d2.cuda(), u2.cuda(), -0.05, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.allclose(buf.cpu().double(), want, rtol=1e-3, atol=1e-4)
    # a misaligned view (offset by one float) takes the scalar path and computes the same
    pad = torch.empty(M * Kf + 1, device="cuda")
    view = pad[1:].view(M, Kf)
    view.copy_(W)
    ops.lora_compose(view, d1.cuda(), u1.cuda(), 0.01, out=view)
    ops.lora_compose(view, d2.cuda(), u2.cuda(), -0.05, out=view)
    assert torch.equal(view, buf)


# ---------------------------------------------------------------------------------------------- the weight path, tiny UNets
RHO_TINY = 0.25      # oracle alone, measured on the CPU: eps shift 0.52 (tiny_config) / 0.54 (tiny15_config); required > 0.2


def _tiny_case(cfg_fn, B=2, L=77):
    from pea_diffusion_amd.lora import lcm_lora_target_keys
    cfg, ref, hip = make_pair(cfg_fn, B, L, needs_grad=False)
    base_sd = ref.state_dict()
    keys = lcm_lora_target_keys({k: tuple(v.shape) for k, v in base_sd.items()})
    lora = random_lora(base_sd, keys, 4, RHO_TINY)
    x, t, ehs, added = cond_inputs(cfg, B, L, cfg.sample_size)
    ehs = ehs.to(torch.bfloat16).float()
    merged = merged_oracle(cfg, ref, lora)
    with torch.no_grad():
        e_base = ref(x, t, ehs, added_cond_kwargs=added)[0]
        e_merged = merged(x, t, ehs, added_cond_kwargs=added)[0]
    cadd = {k: v.cuda() for k, v in added.items()} if added else None
    run = lambda u: u(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0]
    return cfg, ref, hip, base_sd, keys, lora, e_base, e_merged, run


@pytest.mark.parametrize("cfg_name", ["tiny_config", "tiny15_config"])
def test_fuse_lora_tiny_vs_merged_oracle(gpu, cfg_name):
    from oracle import unet_ref as ou
    cfg, ref, hip, base_sd, keys, lora, e_base, e_merged, run = _tiny_case(getattr(ou, cfg_name))
    kinds = {s: any(k.endswith(s + ".weight") for k in keys)
             for s in ("to_q", "proj_in", "conv1", "upsamplers.0.conv", "time_emb_proj", "ff.net.0.proj")}
    assert all(kinds.values()), kinds                     # Linear, proj_in (1x1 conv on SD1.5), 3x3, upsampler, time_emb_proj, GEGLU
    if cfg_name == "tiny15_config":
        assert base_sd[next(k for k in keys if k.endswith("proj_in.weight"))].dim() == 4
    shift = rel_l2(e_merged, e_base)
    print(f"[fuse_lora {cfg_name}] {len(keys)} keys; the oracle alone moves eps by rel_l2={shift:.3f}")
    assert shift > 0.2                                    # ten times the limit below: an ignored LoRA cannot pass
    e0 = run(hip)
    fused = hip.fuse_lora(base_sd, spelled(lora, "diffusers"))
    assert sorted(fused) == sorted(keys)
    e1 = run(hip)
    e = rel_l2(e1, e_merged)
    print(f"[fuse_lora {cfg_name}] eps rel_l2 vs merged oracle {e:.3e} (vs base oracle before fusing {rel_l2(e0, e_base):.3e})")
    assert e < 2e-2
    # the kohya (alpha = rank / 2, up doubled: the same product, all factors exact in fp32) and PEFT spellings: bit-identical
    for sd in (spelled(lora, "kohya", alpha_div=2.0), spelled(lora, "peft")):
        assert sorted(hip.fuse_lora(base_sd, sd)) == sorted(keys)
        assert torch.equal(run(hip), e1)
    # two adapters at half scale each accumulate to the same delta up to fp32 rounding of the sum: a few bf16 weights round the
    # other way, which the bf16 activations amplify to their own noise level, so the check is the one above, not equality
    hip.fuse_lora(base_sd, [(spelled(lora, "peft"), 0.5), (spelled(lora, "diffusers"), 0.5)])
    e2 = rel_l2(run(hip), e_merged)
    print(f"[fuse_lora {cfg_name}] two adapters at half scale: eps rel_l2 vs merged oracle {e2:.3e}")
    assert e2 < 2e-2
    # lora_scale
    hip.fuse_lora(base_sd, spelled(lora, "peft"), lora_scale=0.0)
    assert torch.equal(run(hip), e0)


def test_unfuse_refuse_and_shared_contexts(gpu):
    from oracle.unet_ref import tiny_config
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    cfg, ref, hip, base_sd, keys, lora, e_base, e_merged, run = _tiny_case(tiny_config)
    other = HipUNet(pc.tiny_config(), 2, cfg.sample_size, cfg.sample_size, 77, share_weights_from=hip)
    e0 = run(hip)
    assert torch.equal(run(other), e0)
    sd = spelled(lora, "kohya")
    hip.fuse_lora(base_sd, sd)
    e1 = run(hip)
    assert rel_l2(e1, e0) > 0.2
    assert torch.equal(run(other), e1)                            # a context sharing the weights returns the fused eps
    assert sorted(hip.unfuse_lora(base_sd)) == sorted(keys)
    assert torch.equal(run(hip), e0) and torch.equal(run(other), e0)          # bit-identical to never having fused
    hip.fuse_lora(base_sd, sd)
    assert torch.equal(run(hip), e1)                              # and the second fuse to the first
    # a later fuse of fewer keys puts the others back to the base
    few = {k: v for k, v in lora.items() if k.endswith("to_q.weight")}
    assert sorted(hip.fuse_lora(base_sd, spelled(few, "peft"))) == sorted(few)
    e_few = run(hip)
    hip.unfuse_lora(base_sd)
    hip.fuse_lora(base_sd, spelled(few, "peft"))
    assert torch.equal(run(hip), e_few)
    assert hip.unfuse_lora(base_sd) and hip.unfuse_lora(base_sd) == []
    # refusals: a borrower, an unknown key, a size mismatch at the C boundary -- none of them changes a weight
    with pytest.raises(PeaError, match="borrows"):
        other.fuse_lora(base_sd, sd)
    with pytest.raises(PeaError, match="no weight of this UNet"):
        hip.fuse_lora(base_sd, {"lora_unet_nothing.lora_down.weight": torch.zeros(4, 8)})
    import ctypes
    from pea_diffusion_amd._lib import lib, ptr
    k = keys[0]
    w = base_sd[k].float().cuda().contiguous()
    d, u = (t.float().cuda().contiguous() for t in lora[k])
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    ranks, scales = (ctypes.c_int * 1)(d.shape[0]), (ctypes.c_float * 1)(1.0)
    L = lib()
    assert L.pea_unet_load_weight_lora(hip._h, k.encode(), ptr(w), w.numel() - 1, 1, arr(d), arr(u), ranks, scales, None) == -3
    assert L.pea_unet_load_weight_lora(other._h, k.encode(), ptr(w), w.numel(), 1, arr(d), arr(u), ranks, scales, None) == -4
    assert L.pea_unet_load_weight_lora(hip._h, b"no.such.weight", ptr(w), w.numel(), 1, arr(d), arr(u), ranks, scales, None) == -5
    bias = next(b for b in base_sd if b.endswith(".bias"))
    assert L.pea_unet_load_weight_lora(hip._h, bias.encode(), ptr(w), base_sd[bias].numel(), 1, arr(d), arr(u), ranks, scales,
                                       None) == -3 and b"vector" in L.pea_last_error()
    torch.cuda.synchronize()
    assert torch.equal(run(hip), e0)


# ---------------------------------------------------------------------------------------------- full SDXL
RHO_SDXL = 0.25      # oracle alone, measured on the CPU: eps shift 0.50 at 64 x 64 latents, t = 500; required > 0.15


def test_fuse_lora_full_sdxl_vs_merged_oracle(gpu):
    """Full SDXL, batch 1, 64 x 64 latents, 77 tokens: a rank-64 LoRA on the whole LCM-LoRA target set, one UNet evaluation
    against the oracle with merged weights under the 1.5e-2 of the full-size forward tests."""
    import os
    from oracle import unet_ref as ou
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.lora import lcm_lora_target_keys, merged_weight
    from pea_diffusion_amd.unet import HipUNet
    torch.set_num_threads(min(64, len(os.sched_getaffinity(0))))
    cfg = ou.sdxl_config()
    B, L, hw = 1, 77, 64
    orig = torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_
    torch.nn.init.kaiming_uniform_ = lambda t, *a, **k: t
    torch.nn.init.uniform_ = lambda t, *a, **k: t
    try:
        ref = ou.UNet2DConditionRef(cfg)
    finally:
        torch.nn.init.kaiming_uniform_, torch.nn.init.uniform_ = orig
    _fast_fill_(ref, seed=5)
    round_weights_bf16_(ref)
    for p in ref.parameters():
        p.requires_grad_(False)
    base_sd = ref.state_dict()
    keys = lcm_lora_target_keys({k: tuple(v.shape) for k, v in base_sd.items()})
    assert len(keys) > 700
    lora = random_lora(base_sd, keys, 64, RHO_SDXL)
    hip = HipUNet(pc.sdxl_config(), B, hw, hw, L)
    hip.load_state_dict(base_sd)
    x, t, ehs, added = cond_inputs(cfg, B, L, hw)
    t = torch.tensor([500])
    ehs = ehs.to(torch.bfloat16).float()
    cadd = {k: v.cuda() for k, v in added.items()}
    with torch.no_grad():
        e_base = ref(x, t, ehs, added_cond_kwargs=added)[0]
    assert sorted(hip.fuse_lora(base_sd, spelled(lora, "kohya"))) == sorted(keys)
    got = hip(x.cuda(), t.cuda(), ehs.cuda(), added_cond_kwargs=cadd)[0].cpu()
    with torch.no_grad():                                     # merge into the oracle in place: one copy of the weights
        for k, (down, up) in lora.items():
            base_sd[k].copy_(merged_weight(base_sd[k], [(down, up, 1.0)]))
        e_merged = ref(x, t, ehs, added_cond_kwargs=added)[0]
    shift, e = rel_l2(e_merged, e_base), rel_l2(got, e_merged)
    print(f"[fuse_lora full SDXL, {len(keys)} keys, rank 64] oracle shift {shift:.3f}; eps rel_l2 vs merged oracle {e:.3e}")
    assert shift > 0.15                                       # ten times the limit
    assert torch.isfinite(got).all() and e < 1.5e-2
