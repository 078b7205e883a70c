"""-m gpu: semantic guidance -- the exact per-group quantile select (pea_op_abs_diff_quantile) and the masked combine with its
momentum (pea_op_cfg_sega_combine) against the restatement of tests/sega_ref.py, their exactness properties, and the loop
(sega.denoise_semantic) on the tiny UNet against a loop written here around the recorded combines.

Inputs are seeded randn rounded to bf16 and widened to fp32, what the UNet delivers.  For EVERY group that is ranked the test first
asserts, on the CPU, that the two order statistics around the cut are equal or lie more than 1e-5 (relative) apart: a condition on
the inputs, not a tolerance -- it guarantees that the rounding of the interpolated cut (an ulp, 6e-8) cannot move an element across
it.  The seeds below meet it in every group (the smallest relative gap of each case is printed; over all of them 1.0e-4).

Tolerances.  Order statistics: bits (a selection has no rounding).  The cut: rtol 1e-6, atol 0 against torch.quantile (about 8 fp32
ulp: lerp with and without a fused multiply-add).  The combine: the rule for fp32-stored results, rtol 1e-3 / atol 1e-4
(tests/test_ops_gpu.py: close_f32); a flipped mask element is an error of at least the cut's magnitude (about 1 at scale 5), far
outside it.  With every concept cooled and a zero momentum: the bits of ops.cfg_combine."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
import sega_ref as R  # noqa: E402
from test_model_gpu import cond_inputs, gpu  # noqa: E402,F401
from test_ops_gpu import BF, close_f32, ops  # noqa: E402,F401

#         B  C  h    w    K
SHAPES = [(1, 3, 1, 2, 1),                                           # the smallest group
          (1, 4, 8, 8, 1),
          (2, 4, 7, 9, 2),                                           # hw = 63: no multiple of 4 or of the wave
          (1, 4, 16, 16, 3),
          (3, 4, 32, 32, 8),                                         # K at its limit
          (1, 4, 128, 128, 2)]                                       # the production group, at the capacity edge of 16384
SCALES = [5.0, -5.0, 2.5, 7.0, -1.5, 5.0, 3.0, -6.0]                 # negative: a reversed concept
ALPHABET = torch.linspace(-1.875, 1.875, 16)                         # 16 values, exact in bf16


def quantiles(hw):
    """the last one gives an integral rank hw - 2 with weight 0, and the last pair"""
    return [0.0, 0.5, 0.9, 0.99, (hw - 2) / (hw - 1)]


@functools.lru_cache(maxsize=None)
def noise(shape, seed=0, ties=False):
    """eps fp32 [(2 + K) B, C, h, w] on the host: bf16-rounded randn, or draws from the 16-value alphabet; computed once, never
    written"""
    B, C, h, w, K = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * h * w + K)
    if ties:
        return ALPHABET[torch.randint(0, 16, ((2 + K) * B, C, h, w), generator=g)].contiguous()
    return torch.randn((2 + K) * B, C, h, w, generator=g).to(BF).float()


@functools.lru_cache(maxsize=None)
def reference(shape, q, seed=0, ties=False):
    """(bounds [K, B, C, 2], thr [K, B, C]) of the restatement with every concept at quantile q, after the condition on the gaps"""
    eps = noise(shape, seed, ties)
    K = shape[4]
    bounds = R.bounds_ref(eps, SCALES[:K], [q] * K)
    thr = torch.stack([R.threshold_ref(R.diff_ref(eps, K, c, SCALES[c]), q) for c in range(K)])
    assert_gaps(f"{shape} q={q:.6f} seed {seed}{' ties' if ties else ''}", bounds)
    return bounds, thr


def assert_gaps(name, bounds):
    lo, hi = bounds[..., 0], bounds[..., 1]
    rel = torch.where(hi > lo, (hi - lo) / hi, torch.ones_like(hi))
    print(f"[{name}] smallest relative gap between the order statistics around the cut: {float(rel.min()):.2e} over {lo.numel()} groups")
    assert bool(((hi == lo) | (hi - lo > 1e-5 * hi)).all()), name


def raw(fn, *args):
    from pea_diffusion_amd._lib import check, lib, stream_ptr
    check(getattr(lib(), fn)(*args, stream_ptr()))


def farr(v):
    return (ctypes.c_float * len(v))(*[float(a) for a in v])


def guarded(n, guard=64):
    """fp32 [n + guard] on the device, every element the sentinel"""
    return torch.full((n + guard,), -12345.0, device="cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", SHAPES)
def test_select_against_torch_quantile(ops, shape):
    B, C, h, w, K = shape
    eps = noise(shape)
    dev = eps.cuda()
    for q in quantiles(h * w):
        want_b, want_t = reference(shape, q)
        thr, bounds = ops.abs_diff_quantile(dev, SCALES[:K], [q] * K, [1.0] * K, want_bounds=True)
        assert torch.equal(bounds.cpu(), want_b), (shape, q)
        err = ((thr.cpu() - want_t).abs() / want_t.abs().clamp_min(1e-30)).max().item()
        print(f"[abs_diff_quantile {shape} q={q:.6f}] largest relative deviation of the cut {err:.2e}")
        torch.testing.assert_close(thr.cpu(), want_t, rtol=1e-6, atol=0.0)
        assert torch.equal(ops.abs_diff_quantile(dev, SCALES[:K], [q] * K, [1.0] * K), thr)          # without bounds; the same bits
    # a cooled concept is +inf and leaves the others alone; nothing behind thr and bounds is written; eps is not written
    q = 0.9
    want_b, want_t = reference(shape, q)
    n = K * B * C
    tbuf, bbuf = guarded(n), guarded(2 * n)
    weight = [0.0] + [1.0] * (K - 1)
    raw("pea_op_abs_diff_quantile", ptr(dev), ptr(tbuf), ptr(bbuf), B, C, h * w, K, farr(SCALES[:K]), farr([q] * K), farr(weight))
    thr, bounds = tbuf[:n].view(K, B, C).cpu(), bbuf[:2 * n].view(K, B, C, 2).cpu()
    assert bool(torch.isinf(thr[0]).all()) and bool((thr[0] > 0).all()) and bool(torch.isinf(bounds[0]).all())
    assert torch.equal(bounds[1:], want_b[1:])
    torch.testing.assert_close(thr[1:], want_t[1:], rtol=1e-6, atol=0.0)
    assert bool((tbuf[n:] == -12345.0).all()) and bool((bbuf[2 * n:] == -12345.0).all())
    assert torch.equal(dev.cpu(), eps)


@pytest.mark.parametrize("shape", SHAPES)
def test_select_with_ties(ops, shape):
    """values from a 16-letter alphabet: every order statistic is shared by many elements; the number of elements at or above the
    cut is the restatement's in every group"""
    B, C, h, w, K = shape
    eps = noise(shape, ties=True)
    dev = eps.cuda()
    d = torch.stack([R.diff_ref(eps, K, c, SCALES[c]).abs() for c in range(K)])                       # [K, B, C, h, w]
    tied = 0
    for q in quantiles(h * w):
        want_b, want_t = reference(shape, q, ties=True)
        thr, bounds = ops.abs_diff_quantile(dev, SCALES[:K], [q] * K, [1.0] * K, want_bounds=True)
        assert torch.equal(bounds.cpu(), want_b), (shape, q)
        count = lambda t: (d >= t[..., None, None]).flatten(3).sum(3)
        assert torch.equal(count(thr.cpu()), count(want_t)), (shape, q)
        tied += int((want_b[..., 0] == want_b[..., 1]).sum())
    assert tied > 0 or h * w < 8                                     # ties around the cut did occur


def _plan(K, step):
    """per-concept quantiles, weights and warm flags of a chained step: a cooled concept (K >= 2), then none warm, mixed, all warm"""
    qs = [[0.9, 0.5, 0.99, 0.0][c % 4] for c in range(K)]
    weight = [[1.0, 0.6, 1.5][c % 3] for c in range(K)]
    if K >= 2:
        weight[1] = 0.0 if step != 1 else 0.6                        # cooled in steps 0 and 2
    warm = [[0] * K, [c % 2 for c in range(K)] if K > 1 else [1], [1] * K][step]
    return qs, weight, warm


@pytest.mark.parametrize("shape", SHAPES)
def test_combine_three_chained_steps(ops, shape):
    B, C, h, w, K = shape
    g, mu, beta = 7.5, 0.1, 0.4
    mom = torch.zeros(B, C, h, w, device="cuda")
    mom_ref = torch.zeros(B, C, h, w)
    ws = ops.sega_workspace(B, C, K, "cuda")
    for step in range(3):
        eps = noise(shape, seed=step)
        qs, weight, warm = _plan(K, step)
        live = [c for c in range(K) if weight[c] != 0.0]
        for q in sorted(set(qs[c] for c in live)):
            reference(shape, q, seed=step)                           # the condition, for every group (at every concept's scale)
        want, mom_ref = R.combine_ref(eps, mom_ref, g, SCALES[:K], qs, weight, warm, mu, beta)
        dev = eps.cuda()
        got = ops.cfg_sega_combine(dev, mom, g, SCALES[:K], qs, weight, warm, mu, beta, workspace=ws)
        close_f32(f"cfg_sega_combine {shape} step {step} out (warm {warm}, weights {weight})", got, want)
        close_f32(f"cfg_sega_combine {shape} step {step} momentum", mom, mom_ref)
        assert torch.equal(dev.cpu(), eps)                           # eps is only read
        if step == 0:                                                # none warm: the momentum builds, out is cfg_combine's
            assert torch.equal(got, ops.cfg_combine(dev[:2 * B].contiguous(), g)) and bool(mom.any())
    assert bool(mom_ref.any())


@pytest.mark.parametrize("shape", [(2, 4, 7, 9, 2), (1, 4, 16, 16, 3), (1, 4, 128, 128, 2)])
def test_combine_properties(ops, shape):
    B, C, h, w, K = shape
    g = 7.5
    eps = noise(shape)
    dev = eps.cuda()
    n = B * C * h * w
    zeros = lambda: torch.zeros(B, C, h, w, device="cuda")
    # every concept cooled, zero momentum: cfg_combine's bits, whatever the warm flags; the momentum stays zero
    for warm in ([0] * K, [1] * K):
        mom = zeros()
        got = ops.cfg_sega_combine(dev, mom, g, SCALES[:K], [0.9] * K, [0.0] * K, warm)
        assert torch.equal(got, ops.cfg_combine(dev[:2 * B].contiguous(), g)) and not bool(mom.any())
    # q = 0 keeps every element: the unmasked sum
    wt = [1.0, 0.5, 2.0][:K]
    got = ops.cfg_sega_combine(dev, zeros(), g, SCALES[:K], [0.0] * K, wt, [1] * K)
    u, t = eps[:B], eps[B:2 * B]
    want = u + g * (t - u) + sum(wt[c] * SCALES[c] * (eps[(2 + c) * B:(3 + c) * B] - u) for c in range(K))
    close_f32(f"cfg_sega_combine {shape} at q = 0", got, want)
    # the same bits every run, out and momentum; guard regions behind out, momentum and the workspace; eps unwritten
    reference(shape, 0.9)
    runs = []
    for _ in range(2):
        obuf, mbuf, wbuf = guarded(n), guarded(n), guarded(K * B * C)
        mbuf[:n] = 0.25
        raw("pea_op_cfg_sega_combine", ptr(dev), ptr(mbuf), ptr(obuf), B, C, h * w, K, g, farr(SCALES[:K]), farr([0.9] * K), farr(wt),
            (ctypes.c_int * K)(*([1] * K)), 0.1, 0.4, ptr(wbuf))
        assert bool((obuf[n:] == -12345.0).all()) and bool((mbuf[n:] == -12345.0).all()) and bool((wbuf[K * B * C:] == -12345.0).all())
        runs.append((obuf[:n].cpu(), mbuf[:n].cpu(), wbuf[:K * B * C].cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    want, want_m = R.combine_ref(eps, torch.full((B, C, h, w), 0.25), g, SCALES[:K], [0.9] * K, wt, [1] * K, 0.1, 0.4)
    close_f32(f"cfg_sega_combine {shape} through the C ABI", runs[0][0].view(B, C, h, w), want)
    close_f32(f"cfg_sega_combine {shape} through the C ABI, momentum", runs[0][1].view(B, C, h, w), want_m)
    assert torch.equal(dev.cpu(), eps)
    assert ops.sega_workspace(B, C, K, "cuda").numel() == 4 * K * B * C


def test_wrapper_refusals(ops):
    from pea_diffusion_amd._lib import PeaError
    eps = torch.zeros(3, 4, 8, 8, device="cuda")
    mom = torch.zeros(1, 4, 8, 8, device="cuda")
    with pytest.raises(PeaError, match="noise_pred"):
        ops.abs_diff_quantile(eps.half(), [5.0], [0.9], [1.0])
    with pytest.raises(PeaError, match="noise_pred"):
        ops.abs_diff_quantile(eps, [5.0, 5.0], [0.9, 0.9], [1.0, 1.0])                               # 3 is no (2 + 2) B
    with pytest.raises(PeaError, match="one each"):
        ops.abs_diff_quantile(eps, [5.0], [0.9, 0.5], [1.0])
    with pytest.raises(PeaError, match="outside"):
        ops.abs_diff_quantile(eps, [5.0], [1.0], [1.0])
    with pytest.raises(PeaError, match="momentum"):
        ops.cfg_sega_combine(eps, mom[:, :2].contiguous(), 7.5, [5.0], [0.9], [1.0], [1])
    with pytest.raises(PeaError, match="warm"):
        ops.cfg_sega_combine(eps, mom, 7.5, [5.0], [0.9], [1.0], [1, 0])
    with pytest.raises(PeaError, match="hw=16900"):
        ops.abs_diff_quantile(torch.zeros(3, 1, 130, 130, device="cuda"), [5.0], [0.9], [1.0])
    assert not bool(mom.any())


# ---------------------------------------------------------------------------------------------- the loop, tiny UNet
CTX_GAIN = 5.0                                                       # as tests/test_pag_gpu.py: conditioning the tiny UNet listens to
STEPS, N_EDIT, G = 4, 2, 5.0
EDIT = dict(edit_guidance_scale=[5.0, 4.0], edit_threshold=[0.9, 0.75], reverse_editing_direction=[False, True], edit_warmup_steps=1,
            edit_cooldown_steps=[None, 3], edit_weights=[1.0, 0.8])


@functools.lru_cache(maxsize=None)
def _tiny():
    """the tiny UNet of tests/test_pag_gpu.py at batch 4 = [uncond | cond | edit_1 | edit_2] of one latent, and its inputs"""
    from test_ip_adapter_gpu import _tiny_ip_pair
    cfg, _, hip = _tiny_ip_pair(2 + N_EDIT, 77)
    x, _, ehs, added = cond_inputs(cfg, 2 + N_EDIT, 77, 16)
    ehs = (CTX_GAIN * ehs).to(BF).float().cuda()
    added = {key: v.cuda() for key, v in added.items()}
    return hip, x[:1].cuda(), ehs, added


def _semantic(monkeypatch, make, **edit):
    """-> (latents, records): sega.denoise_semantic with ops.cfg_sega_combine wrapped to record every step"""
    from pea_diffusion_amd import sega
    hip, x, ehs, added = _tiny()
    records, inner = [], sega.ops.cfg_sega_combine

    def recording(noise_pred, momentum, guidance_scale, edit_scale, quantile, weight, warm, *a, **kw):
        rec = dict(eps=noise_pred.clone(), before=momentum.clone(), lists=(edit_scale, quantile, weight, warm), g=guidance_scale, mom=momentum)
        rec["out"] = inner(noise_pred, momentum, guidance_scale, edit_scale, quantile, weight, warm, *a, **kw)
        rec["after"] = momentum.clone()
        rec["out"] = rec["out"].clone()
        records.append(rec)
        return rec["out"].clone()
    monkeypatch.setattr(sega.ops, "cfg_sega_combine", recording)
    got = sega.denoise_semantic(hip, make(), x.clone(), ehs[:2], {k: v[:2] for k, v in added.items()}, ehs[2:], {k: v[2:] for k, v in added.items()},
                                num_inference_steps=STEPS, guidance_scale=G, **edit)
    monkeypatch.setattr(sega.ops, "cfg_sega_combine", inner)
    return got.clone(), records


def _loop(make, combine):
    """the same UNet calls and scheduler steps, written out; combine(i, eps) -> the guided prediction of step i"""
    hip, x, ehs, added = _tiny()
    s = make()
    fused = getattr(s, "fused_model_input", False)
    timesteps = s.set_timesteps(STEPS)
    lat = (x.clone().float() * s.init_noise_sigma).contiguous()
    for i, t in enumerate(timesteps):
        xin = s.scale_model_input(lat, t, dup=1) if fused else s.scale_model_input(lat, t)
        eps = hip(torch.cat([xin] * (2 + N_EDIT)), t, encoder_hidden_states=ehs, added_cond_kwargs=added, return_dict=False)[0].float()
        lat = s.step(combine(i, eps), t, lat, return_dict=False)[0]
    return lat.clone()


@pytest.mark.parametrize("sched", ["dpm", "euler"])
def test_denoise_semantic_on_the_tiny_unet(gpu, monkeypatch, sched):
    """n = 1, K = 2, 4 steps, warm-up 1, the second concept reversed and cooled from step 3.  Every recorded combine against the
    restatement on the CPU; the K-lists against step_plan; the latents against the written-out loop around the recorded results;
    with every concept cooled from step 0 the latents of the plain CFG loop over the same batch-4 UNet, bit for bit; with the edits
    live, far from it.  (Not compared with an oracle-UNet loop: the device's bf16 eps differs from the oracle's at the storage floor,
    which moves elements across the cut -- that would measure mask flips, not the feature.)"""
    from pea_diffusion_amd import ops as o
    from pea_diffusion_amd import sega
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerDiscrete
    make = DPMSolverMultistep if sched == "dpm" else EulerDiscrete
    got, records = _semantic(monkeypatch, make, **EDIT)
    assert len(records) == STEPS and bool(torch.isfinite(got).all())
    assert all(r["mom"] is records[0]["mom"] for r in records) and not bool(records[0]["before"].any())
    for i, r in enumerate(records):
        lists = sega.step_plan(i, N_EDIT, **EDIT)
        assert r["lists"] == lists and r["g"] == G
        if i:
            assert torch.equal(r["before"], records[i - 1]["after"])
        want, want_m = R.combine_ref(r["eps"].cpu(), r["before"].cpu(), G, *lists, 0.1, 0.4)
        close_f32(f"denoise_semantic {sched} step {i} combine", r["out"], want)
        close_f32(f"denoise_semantic {sched} step {i} momentum", r["after"], want_m)

    def replay(i, eps):
        assert torch.equal(eps, records[i]["eps"])                   # the same UNet calls: the same bits
        return records[i]["out"].clone()
    assert torch.equal(_loop(make, replay), got)
    if sched == "euler":
        return
    plain = _loop(make, lambda i, eps: o.cfg_combine(eps[:2].contiguous(), G))
    cooled, recs = _semantic(monkeypatch, make, **dict(EDIT, edit_cooldown_steps=0))
    assert all(r["lists"][2] == [0.0, 0.0] for r in recs) and torch.equal(cooled, plain)
    far = ((got - plain).abs() > 4.0 * (1e-4 + 1e-3 * plain.abs())).float().mean().item()
    print(f"[denoise_semantic {sched}] {100 * far:.1f} % of the latents lie more than 4 tolerances from the plain CFG loop")
    assert far >= 0.01


def test_denoise_semantic_refuses_the_wrong_unet(gpu):
    from pea_diffusion_amd import sega
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.sampler import DPMSolverMultistep
    hip, x, ehs, added = _tiny()
    with pytest.raises(PeaError, match="UNet of batch 3"):
        sega.denoise_semantic(hip, DPMSolverMultistep(), x, ehs[:2], {k: v[:2] for k, v in added.items()}, ehs[2:3],
                              {k: v[2:3] for k, v in added.items()}, num_inference_steps=2)
