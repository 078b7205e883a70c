"""Semantic guidance without a GPU: the restatement's combine (tests/sega_ref.py) against a double loop in float64, the schedule of
`sega.step_plan` at its warm-up and cool-down boundaries, the control flow of `sega.denoise_semantic` with a stand-in UNet and
`ops.cfg_sega_combine` replaced by the restatement (batch layout, one momentum buffer, the per-step K-lists), the argument
refusals of both, and every refusal of the two C entry points that needs no device.
The kernels themselves are checked in tests/test_sega_gpu.py."""
import ctypes
import math

import pytest
import torch

import sega_ref as R
from pea_diffusion_amd import sampler, sega
from pea_diffusion_amd._lib import PeaError
from pea_diffusion_amd.sampler import DPMSolverMultistep


@pytest.mark.parametrize("K", [1, 2])
def test_combine_ref_against_a_double_loop(K):
    """float64, so the only difference is summation order: 1e-12"""
    g = torch.Generator().manual_seed(11 + K)
    B, C, h, w = 2, 3, 3, 5
    hw = h * w
    eps = torch.randn((2 + K) * B, C, h, w, generator=g, dtype=torch.float64)
    mom = torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    gs, mu, beta = 6.0, 0.3, 0.4
    scale, q, wt = [5.0, -3.0][:K], [0.9, 0.5][:K], [1.0, 0.7][:K]
    for warm in ([1, 1][:K], [0, 0][:K], [0, 1][:K]):
        mom0 = mom.clone()
        out, new = R.combine_ref(eps, mom, gs, scale, q, wt, warm, mu, beta)
        assert torch.equal(mom, mom0)                                # the restatement does not write its input
        for b in range(B):
            for ch in range(C):
                u, t = eps[b, ch].reshape(-1), eps[B + b, ch].reshape(-1)
                m0 = mom[b, ch].reshape(-1)
                e_all, e_warm = [0.0] * hw, [0.0] * hw
                for c in range(K):
                    e = eps[(2 + c) * B + b, ch].reshape(-1)
                    d = [scale[c] * float(e[i] - u[i]) for i in range(hw)]
                    v = sorted(abs(a) for a in d)
                    r = q[c] * (hw - 1)
                    k = int(math.floor(r))
                    thr = v[k] + (r - k) * (v[min(k + 1, hw - 1)] - v[k])
                    for i in range(hw):
                        m = d[i] if abs(d[i]) >= thr else 0.0        # (no value lies between v[k] and v[k + 1]: the cut's rounding is free)
                        e_all[i] += wt[c] * m
                        e_warm[i] += warm[c] * wt[c] * m
                for i in range(hw):
                    used = e_all[i] + mu * float(m0[i])
                    want = float(u[i]) + gs * float(t[i] - u[i]) + (e_warm[i] + mu * float(m0[i]) if any(warm) else 0.0)
                    assert abs(float(out[b, ch].reshape(-1)[i]) - want) <= 1e-12 * max(1.0, abs(want)), (warm, b, ch, i)
                    wantm = beta * float(m0[i]) + (1.0 - beta) * used
                    assert abs(float(new[b, ch].reshape(-1)[i]) - wantm) <= 1e-12 * max(1.0, abs(wantm)), (warm, b, ch, i)
    # none warm: the plain CFG expression, bit for bit; a cooled concept is skipped
    out, _ = R.combine_ref(eps, mom, gs, scale, q, wt, [0] * K, mu, beta)
    assert torch.equal(out, eps[:B] + gs * (eps[B:2 * B] - eps[:B]))
    out, new = R.combine_ref(eps, torch.zeros_like(mom), gs, scale, q, [0.0] * K, [1] * K, mu, beta)
    assert torch.equal(out, eps[:B] + gs * (eps[B:2 * B] - eps[:B])) and not new.any()


def test_bounds_ref_brackets_the_quantile():
    g = torch.Generator().manual_seed(3)
    K, B = 2, 2
    eps = torch.randn((2 + K) * B, 3, 7, 9, generator=g).to(torch.bfloat16).float()
    scale, q = [5.0, -2.0], [0.9, 62.0 / 62.0 - 1.0 / 62.0]
    b = R.bounds_ref(eps, scale, q)
    assert tuple(b.shape) == (K, B, 3, 2) and bool((b[..., 0] <= b[..., 1]).all())
    for c in range(K):
        thr = R.threshold_ref(R.diff_ref(eps, K, c, scale[c]), q[c])
        assert bool((thr >= b[c, ..., 0]).all()) and bool((thr <= b[c, ..., 1]).all())
    assert R.rank_ref(0.0, 63) == (0, 1) and R.rank_ref(0.5, 63) == (31, 32) and R.rank_ref(0.99, 2) == (0, 1)


def test_step_plan_boundaries_sign_and_broadcast():
    plan = lambda i, **kw: sega.step_plan(i, 2, **kw)
    assert plan(0) == ([5.0, 5.0], [0.9, 0.9], [1.0, 1.0], [0, 0])                # diffusers' defaults: warm-up 10, no cool-down
    assert plan(9)[3] == [0, 0] and plan(10)[3] == [1, 1] and plan(10 ** 6)[2] == [1.0, 1.0]
    kw = dict(edit_guidance_scale=[4.0, 7.0], edit_threshold=[0.95, 0.5], reverse_editing_direction=[False, True],
              edit_warmup_steps=[3, 5], edit_cooldown_steps=[None, 8], edit_weights=[1.0, 0.5])
    assert plan(2, **kw) == ([4.0, -7.0], [0.95, 0.5], [1.0, 0.5], [0, 0])        # i = warmup - 1
    assert plan(3, **kw)[3] == [1, 0] and plan(4, **kw)[3] == [1, 0] and plan(5, **kw)[3] == [1, 1]
    assert plan(7, **kw)[2] == [1.0, 0.5] and plan(8, **kw)[2] == [1.0, 0.0]      # i = cooldown - 1, cooldown
    assert plan(8, **kw)[0] == [4.0, -7.0] and plan(8, **kw)[3] == [1, 1]
    one = sega.step_plan(0, 3, edit_guidance_scale=2.0, reverse_editing_direction=True, edit_warmup_steps=0, edit_cooldown_steps=0)
    assert one == ([-2.0] * 3, [0.9] * 3, [0.0] * 3, [1] * 3)                     # scalars broadcast; cooled from step 0
    for bad, match in ((dict(K=0), "K=0"), (dict(K=9), "K=9"), (dict(edit_threshold=1.0), "edit_threshold"),
                       (dict(edit_threshold=-0.1), "edit_threshold"), (dict(edit_guidance_scale=-1.0), "negative"),
                       (dict(edit_weights=[1.0, -0.5]), "negative"), (dict(edit_warmup_steps=-1), "negative"),
                       (dict(edit_cooldown_steps=-2), "negative"), (dict(edit_weights=[1.0]), "entries")):
        a = dict(K=2)
        a.update(bad)
        with pytest.raises(PeaError, match=match):
            sega.step_plan(0, **a)


# ---------------------------------------------------------------------------------------------- the loop, the combine restated
class _ToyUNet:
    """a UNet-shaped stand-in of a fixed batch whose output depends on each sample's conditioning"""

    def __init__(self, B):
        self.B, self.calls = B, []
        self.mix = torch.linspace(-0.3, 0.4, 16).reshape(4, 4)

    def __call__(self, x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        assert x.shape[0] == self.B == encoder_hidden_states.shape[0] == added_cond_kwargs["text_embeds"].shape[0]
        self.calls.append((x.clone(), encoder_hidden_states, added_cond_kwargs))
        y = torch.einsum("oc,bchw->bohw", self.mix.to(x.dtype), x) * (1.0 + 1e-4 * float(t))
        gain = encoder_hidden_states.to(x.dtype).mean(dim=(1, 2)) + added_cond_kwargs["text_embeds"].to(x.dtype).mean(dim=1)
        return ((y * (1.0 + gain)[:, None, None, None]).to(torch.bfloat16),)


def _dpm_cpu(sample, eps, x0_prev, a_s, s_s, c_s, c0, c1):
    x0 = (sample - s_s * eps) / a_s
    sample.copy_(c_s * sample + c0 * x0 + c1 * x0_prev)
    x0_prev.copy_(x0)
    return sample


def test_denoise_semantic_loop_with_the_restated_combine(monkeypatch):
    n, K, steps, g = 2, 2, 4, 5.0
    records = []

    def combine(noise_pred, momentum, guidance_scale, edit_scale, quantile, weight, warm, momentum_scale=0.1, momentum_beta=0.4,
                workspace=None, out=None):
        assert workspace == "ws" and noise_pred.dtype == torch.float32 and tuple(noise_pred.shape) == ((2 + K) * n, 4, 8, 8)
        records.append((momentum, momentum.clone(), (edit_scale, quantile, weight, warm), guidance_scale, momentum_scale, momentum_beta))
        res, new = R.combine_ref(noise_pred, momentum, guidance_scale, edit_scale, quantile, weight, warm, momentum_scale, momentum_beta)
        momentum.copy_(new)
        return res
    monkeypatch.setattr(sega.ops, "cfg_sega_combine", combine)
    monkeypatch.setattr(sega.ops, "sega_workspace", lambda B, C, Kc, device: "ws" if (B, C, Kc) == (n, 4, K) else None)
    monkeypatch.setattr(sampler.ops, "dpm_update_", _dpm_cpu)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, 4, 8, 8, generator=gen)
    ehs, edit = torch.randn(2 * n, 7, 8, generator=gen) * 0.3, torch.randn(K * n, 7, 8, generator=gen) * 0.3
    added = {"text_embeds": torch.randn(2 * n, 6, generator=gen) * 0.3, "time_ids": torch.zeros(2 * n, 6)}
    eadded = {"text_embeds": torch.randn(K * n, 6, generator=gen) * 0.3, "time_ids": torch.ones(K * n, 6)}
    kw = dict(edit_guidance_scale=[5.0, 3.0], edit_threshold=[0.9, 0.5], reverse_editing_direction=[False, True], edit_warmup_steps=1,
              edit_cooldown_steps=[None, 3], edit_weights=[1.0, 0.8])
    toy = _ToyUNet((2 + K) * n)
    seen = []
    got = sega.denoise_semantic(toy, DPMSolverMultistep(), x.clone(), ehs, added, edit, eadded, edit_momentum_scale=0.2, edit_mom_beta=0.3,
                                num_inference_steps=steps, guidance_scale=g, callback=lambda i, t, lat: seen.append(i), **kw)
    assert len(toy.calls) == steps == len(records) and seen == list(range(steps))
    for xin, e, a in toy.calls:                                      # [uncond | cond | edit_1 | edit_2], the latents repeated
        assert torch.equal(e, torch.cat([ehs, edit])) and torch.equal(a["text_embeds"], torch.cat([added["text_embeds"], eadded["text_embeds"]]))
        assert torch.equal(a["time_ids"], torch.cat([added["time_ids"], eadded["time_ids"]]))
        assert all(torch.equal(xin[j * n:(j + 1) * n], xin[:n]) for j in range(2 + K))
    assert all(r[0] is records[0][0] for r in records)               # one momentum buffer ...
    assert not records[0][1].any() and records[1][1].any()           # ... zero before the first step, live behind it
    for i, r in enumerate(records):
        assert r[2] == sega.step_plan(i, K, **kw) and r[3:] == (g, 0.2, 0.3)
    assert [r[2][3] for r in records] == [[0, 0], [1, 1], [1, 1], [1, 1]] and [r[2][2][1] for r in records] == [0.8, 0.8, 0.8, 0.0]
    embeds = torch.cat([ehs, edit])
    both = {key: torch.cat([added[key], eadded[key]]) for key in added}
    want = R.denoise_semantic_ref(lambda x_, t, e, added_cond_kwargs=None: _ToyUNet((2 + K) * n)(x_, t, e, added_cond_kwargs),
                                  DPMSolverMultistep(), x.clone(), embeds, both, lambda i: sega.step_plan(i, K, **kw), steps, g, 0.2, 0.3)
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_denoise_semantic_argument_refusals():
    class Ctx:
        B = 4
    lat, emb, edit = torch.zeros(1, 4, 8, 8), torch.zeros(2, 77, 64), torch.zeros(2, 77, 64)
    call = lambda *a, **kw: sega.denoise_semantic(Ctx(), None, lat, *a, **kw)
    with pytest.raises(PeaError, match="guidance_scale"):
        call(emb, None, edit, None, guidance_scale=1.0)
    with pytest.raises(PeaError, match="K=9"):
        call(emb, None, torch.zeros(9, 77, 64), None)
    with pytest.raises(PeaError, match="edit_prompt_embeds"):
        call(emb, None, torch.zeros(0, 77, 64), None)                # K = 0
    with pytest.raises(PeaError, match="edit_prompt_embeds"):
        sega.denoise_semantic(Ctx(), None, torch.zeros(2, 4, 8, 8), torch.zeros(4, 77, 64), None, torch.zeros(3, 77, 64), None)
    with pytest.raises(PeaError, match="edit_threshold"):
        call(emb, None, edit, None, edit_threshold=1.0)
    with pytest.raises(PeaError, match="negative"):
        call(emb, None, edit, None, edit_guidance_scale=[5.0, -1.0])
    with pytest.raises(PeaError, match="negative"):
        call(emb, None, edit, None, edit_weights=-1.0)
    with pytest.raises(PeaError, match="negative"):
        call(emb, None, edit, None, edit_warmup_steps=-1)
    with pytest.raises(PeaError, match="edit_mom_beta"):
        call(emb, None, edit, None, edit_mom_beta=1.5)
    Ctx.B = 3
    with pytest.raises(PeaError, match="UNet of batch 4"):
        call(emb, None, edit, None)                                  # [uncond | cond | edit_1 | edit_2]
    Ctx.B = 4
    with pytest.raises(PeaError, match="prompt_embeds of batch 3"):
        call(torch.zeros(3, 77, 64), None, edit, None)
    added = {"text_embeds": torch.zeros(2, 6), "time_ids": torch.zeros(2, 6)}
    with pytest.raises(PeaError, match="come together"):
        call(emb, added, edit, None)
    with pytest.raises(PeaError, match="time_ids"):
        call(emb, added, edit, {"text_embeds": torch.zeros(2, 6), "time_ids": torch.zeros(1, 6)})


# ---------------------------------------------------------------------------------------------- the C ABI, without a device
def _abi():
    from pea_diffusion_amd._lib import lib
    L = lib()
    page = (ctypes.c_float * 64)()
    return L, ctypes.cast(page, ctypes.c_void_p)


def _f(*v):
    return (ctypes.c_float * len(v))(*v)


def _select(L, p, eps="p", thr="p", B=1, C=4, hw=64, K=1, scale=_f(5.0), q=_f(0.9), w=_f(1.0)):
    pick = lambda v: p if v == "p" else v
    return L.pea_op_abs_diff_quantile(pick(eps), pick(thr), None, B, C, hw, K, scale, q, w, None)


def _combine(L, p, eps="p", mom="p", out="p", B=1, C=4, hw=64, K=1, scale=_f(5.0), q=_f(0.9), w=_f(1.0),
             warm=(ctypes.c_int * 1)(1), beta=0.4, ws="p"):
    pick = lambda v: p if v == "p" else v
    return L.pea_op_cfg_sega_combine(pick(eps), pick(mom), pick(out), B, C, hw, K, 7.5, scale, q, w, warm, 0.1, beta, pick(ws), None)


SHARED_REFUSALS = [
    (dict(eps=None), b"null operand"), (dict(scale=None), b"null operand"), (dict(q=None), b"null operand"), (dict(w=None), b"null operand"),
    (dict(B=0), b"B=0"), (dict(C=0), b"C=0"), (dict(hw=1), b"hw=1"), (dict(hw=16385), b"hw=16385"), (dict(K=0), b"K=0"), (dict(K=9), b"K=9"),
    (dict(q=_f(1.0)), b"quantile 1 outside"), (dict(q=_f(-0.25)), b"quantile -0.25 outside"), (dict(w=_f(-1.0)), b"negative weight"),
    (dict(K=2, scale=_f(5.0, 5.0), q=_f(0.5, 1.5), w=_f(1.0, 1.0)), b"concept 1: quantile 1.5"),
]


def test_select_refusals_through_the_c_abi():
    L, p = _abi()
    for kw, msg in SHARED_REFUSALS + [(dict(thr=None), b"null operand")]:
        rc = _select(L, p, **kw)
        assert rc == -3 and msg in L.pea_last_error() and b"abs_diff_quantile" in L.pea_last_error(), (kw, L.pea_last_error())
    assert b"16384" in (_select(L, p, hw=20000), L.pea_last_error())[1]         # the limit is named


def test_combine_refusals_through_the_c_abi():
    L, p = _abi()
    two = dict(K=2, scale=_f(5.0, 5.0), q=_f(0.5, 0.5), w=_f(1.0, 1.0), warm=(ctypes.c_int * 2)(1, 0))
    for kw, msg in SHARED_REFUSALS + [(dict(mom=None), b"null operand"), (dict(out=None), b"null operand"), (dict(warm=None), b"null operand"),
                                      (dict(beta=-0.1), b"momentum_beta"), (dict(beta=1.5), b"momentum_beta"), (dict(ws=None), b"workspace"),
                                      (dict(two, ws=None), b"workspace")]:
        a = dict(kw)
        if a.get("K") == 2 and "warm" not in a:
            a["warm"] = (ctypes.c_int * 2)(1, 1)
        rc = _combine(L, p, **a)
        assert rc == -3 and msg in L.pea_last_error() and b"cfg_sega_combine" in L.pea_last_error(), (kw, L.pea_last_error())
    assert L.pea_op_sega_workspace_bytes(2, 4, 3) == 2 * 4 * 3 * 4 and L.pea_op_sega_workspace_bytes(1, 4, 8) == 128
    assert L.pea_op_sega_workspace_bytes(0, 4, 1) == 0
