"""MultiDiffusion panoramas without a GPU: the view geometry, weight tables and weight total of pea_diffusion_amd/panorama.py against
the restatement tests/panorama_ref.py and against known answers; the properties of the restated merge (partition of unity, the
single view); the loop logic in float64 (stepping through views against stepping the whole canvas with a pointwise model, and
diffusers' step-every-view-then-average against the merged-eps form with a position-dependent model, for the DPM-Solver and the
Euler reference); `model_input_scale()` of the four schedulers; the loop of `denoise_panorama` with the kernels replaced by the
restatement (chunking, padding, conditioning per chunk); and every refusal of the two kernels through the C ABI.
The kernels themselves are checked in tests/test_panorama_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import panorama_ref as R
from oracle.sampler_ref import DPMSolverMultistepRef
from pea_diffusion_amd import panorama, sampler
from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerAncestralDiscrete, EulerDiscrete, LCMScheduler
from turbo_ref import EulerRef

# (Hc, Wc, stride, wrap_x) at window 16 x 16 -> the x origins, the y origins
GEOMETRY = [
    ((16, 40, 8, False), [0], [0, 8, 16, 24]),
    ((24, 42, 8, False), [0, 8], [0, 8, 16, 24, 26]),               # 26: the last view flush with the edge
    ((20, 16, 8, False), [0, 4], [0]),
    ((16, 40, 8, True), [0], [0, 8, 16, 24, 32]),                   # 32: columns 32 .. 39, 0 .. 7 -- across the seam
    ((16, 44, 12, True), [0], [0, 12, 24, 36]),                     # 36: columns 36 .. 43, 0 .. 7
]
COUNTS = [4, 10, 2, 5, 4]
WIN = 16
KINDS = ("uniform", "ramp", "gaussian")


@pytest.mark.parametrize("case,count", list(zip(GEOMETRY, COUNTS)))
def test_view_geometry(case, count):
    (Hc, Wc, stride, wrap), ys, xs = case
    vs = panorama.views(Hc, Wc, WIN, WIN, stride, wrap)
    assert vs == [(y, x) for y in ys for x in xs] and len(vs) == count
    assert vs == R.views_ref(Hc, Wc, WIN, WIN, stride, wrap)
    triples = R.triples_ref(vs, 2)
    assert int(R.coverage_ref(triples, 2, Hc, Wc, WIN, WIN).min()) >= 1          # every element is covered
    for kind in KINDS:
        wy, wx = (panorama.view_weights(WIN, kind, WIN - stride) for _ in range(2))
        assert wy.dtype == torch.float32 and bool((wy > 0).all())
        assert torch.equal(wy, R.weights_ref(WIN, kind, WIN - stride))
        T = panorama.weight_total(vs, 2, Hc, Wc, wy, wx, wrap)
        assert T.dtype == torch.float32 and tuple(T.shape) == (2, Hc, Wc)
        assert torch.equal(T, R.total_ref(triples, 2, Hc, Wc, wy, wx)) and torch.equal(T, panorama.weight_total(triples, 2, Hc, Wc, wy, wx, wrap))
        assert float(T.min()) > 1e-30, (kind, float(T.min()))                    # far from denormal (gaussian corners: 4.6e-9)
    if wrap:
        assert any(x0 + WIN > Wc for _, x0 in vs)                                # a view straddles the seam


def test_view_geometry_refusals():
    from pea_diffusion_amd._lib import PeaError
    with pytest.raises(PeaError, match="window"):
        panorama.views(8, 40, 16, 16, 8)
    with pytest.raises(AssertionError, match="outside every window"):
        panorama.views(16, 64, 16, 16, 24)                                       # a stride past the window leaves gaps
    with pytest.raises(PeaError, match="kind"):
        panorama.view_weights(16, "cosine")
    with pytest.raises(PeaError, match="outside"):
        panorama.weight_total([(0, 0, 30)], 1, 16, 40, torch.ones(16), torch.ones(16))       # no wrap: columns 30 .. 45


def test_weight_tables_known_answers():
    assert panorama.view_weights(6, "ramp", 2).tolist() == pytest.approx([1 / 3, 2 / 3, 1, 1, 2 / 3, 1 / 3])
    g = panorama.view_weights(16, "gaussian")
    assert float(g[7]) == pytest.approx(math.exp(-0.25 / (256 * 0.02)) / math.sqrt(0.02 * math.pi), rel=1e-6)
    assert torch.equal(g, g.flip(0)) and torch.equal(panorama.view_weights(5, "uniform"), torch.ones(5))


@pytest.mark.parametrize("case", GEOMETRY)
def test_partition_of_unity(case):
    """merging a constant field returns it to within 2 ulp (measured: at most 6e-8 on 0.37)"""
    (Hc, Wc, stride, wrap), _, _ = case
    triples = R.triples_ref(R.views_ref(Hc, Wc, WIN, WIN, stride, wrap), 1)
    const = torch.full((len(triples), 4, WIN, WIN), 0.37)
    ulp = float(np.spacing(np.float32(0.37)))
    for kind in KINDS:
        wy = wx = R.weights_ref(WIN, kind, WIN - stride)
        got = R.merge_ref(const, triples, 1, Hc, Wc, wy, wx)
        err = float((got - 0.37).abs().max())
        print(f"[partition of unity {Hc} x {Wc} {kind}] max deviation {err:.2e} ({err / ulp:.1f} ulp)")
        assert err <= 2 * ulp


def test_single_view_is_the_identity():
    e = torch.randn(1, 4, WIN, WIN, generator=torch.Generator().manual_seed(0))
    ones = R.weights_ref(WIN, "uniform")
    assert torch.equal(R.merge_ref(e, [(0, 0, 0)], 1, WIN, WIN, ones, ones), e)


# ---------------------------------------------------------------------------------------------- loop logic, float64
def _f64_setup(wrap=False):
    Hc, Wc, stride = 24, 40, 8
    triples = R.triples_ref(R.views_ref(Hc, Wc, WIN, WIN, stride, wrap), 2)
    wy = wx = R.weights_ref(WIN, "gaussian", dtype=torch.float64)
    x = torch.randn(2, 4, Hc, Wc, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    return x, triples, wy, wx


@pytest.mark.parametrize("wrap", [False, True])
def test_views_of_a_pointwise_model_are_the_whole_canvas(wrap):
    """a pointwise stand-in UNet sees no window: three Euler steps on the canvas through the views equal the same steps on the
    whole canvas to 1e-12 (measured 4e-16 relative)"""
    x, triples, wy, wx = _f64_setup(wrap)
    model = lambda z, view=None: torch.tanh(0.7 * z) + 0.1 * z
    got = R.loop_merged_ref(model, EulerRef(False), x, 3, triples, WIN, WIN, wy, wx)
    s = EulerRef(False)
    s.set_timesteps(3)
    want = x * s.init_noise_sigma
    for t in s.timesteps:
        want = s.step(model(s.scale_model_input(want, t)), t, want)[0]
    err = float((got - want).abs().max() / want.abs().max())
    print(f"[pointwise model, wrap={wrap}] max deviation {err:.1e} of the largest latent")
    assert err <= 1e-12


@pytest.mark.parametrize("sched", ["dpm", "euler"])
def test_stepping_every_view_then_averaging_is_stepping_the_average(sched):
    """a position-dependent stand-in (a fixed 3 x 3 convolution, zero-padded at the WINDOW's edge): diffusers' form -- every view
    stepped with its own scheduler state, then averaged -- equals one step of the merged prediction, history included; 1e-10"""
    x, triples, wy, wx = _f64_setup()
    k = torch.randn(4, 4, 3, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 0.2
    model = lambda z, view=None: F.conv2d(z, k, padding=1)
    make = (lambda: DPMSolverMultistepRef()) if sched == "dpm" else (lambda: EulerRef(False))
    merged = R.loop_merged_ref(model, make(), x, 4, triples, WIN, WIN, wy, wx)
    per_view = R.loop_per_view_ref(model, make, x, 4, triples, WIN, WIN, wy, wx)
    err = float((merged - per_view).abs().max() / merged.abs().max())
    print(f"[per-view stepping vs merged eps, {sched}] max deviation {err:.1e} of the largest latent")
    assert err <= 1e-10
    whole = make()
    whole.set_timesteps(4)
    y = x * whole.init_noise_sigma
    for t in whole.timesteps:
        y = whole.step(model(whole.scale_model_input(y, t)), t, y)[0]
    # ... and this model does see the window: against the whole canvas the views differ by 1e4 times the bound above or more
    # (the gaussian weights are small at a window's edge, where the padding acts)
    assert float((merged - y).abs().max() / y.abs().max()) > 1e-6


# ---------------------------------------------------------------------------------------------- model_input_scale
def _euler_update_cpu_(sample, eps, noise, model_in, k_e, k_n, k_s, dup=1):
    """the contract of pea_op_euler_update in torch (include/pea_hip.h)"""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    x = sample
    if eps is not None:
        x = sample + f(k_e) * eps + (f(k_n) * noise if noise is not None else 0.0)
        sample.copy_(x)
    if model_in is not None:
        m = x * f(k_s)
        model_in.copy_(m.repeat((dup,) + (1,) * (m.dim() - 1)))
    return sample


@pytest.mark.parametrize("cls", [DPMSolverMultistep, LCMScheduler, EulerDiscrete, EulerAncestralDiscrete])
def test_model_input_scale_is_what_scale_model_input_applies(monkeypatch, cls):
    monkeypatch.setattr(sampler.ops, "euler_update_", _euler_update_cpu_)
    s = cls()
    s.set_timesteps(4)
    x = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1)) * 3.0
    for pos in (0, 2, 3):
        s._i = pos
        k = s.model_input_scale()
        assert isinstance(k, float)
        assert torch.equal(s.scale_model_input(x.clone(), s.timesteps[pos]), x * torch.tensor(k, dtype=torch.float32)), (cls.__name__, pos)
        if isinstance(s, EulerDiscrete):
            sigma = float(s.sigmas[pos])
            assert k == float(np.float32(1.0 / math.sqrt(sigma * sigma + 1.0))) and k < 1.0
        else:
            assert k == 1.0
    if isinstance(s, EulerDiscrete):
        with pytest.raises(ValueError, match="set_timesteps"):
            cls().model_input_scale()


# ---------------------------------------------------------------------------------------------- the loop, kernels restated
class _ToyUNet:
    """a UNet-shaped stand-in built for one batch and window: a channel mix that depends on the sample's conditioning"""

    def __init__(self, B, hw):
        self.B, self.H, self.W, self.calls = B, hw, hw, []
        self.mix = torch.linspace(-0.3, 0.4, 16).reshape(4, 4)

    def __call__(self, x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        assert x.shape[0] == self.B == encoder_hidden_states.shape[0] == added_cond_kwargs["text_embeds"].shape[0]
        self.calls.append(x.shape[0])
        y = torch.einsum("oc,bchw->bohw", self.mix.to(x.dtype), x) * (1.0 + 1e-4 * float(t))
        y = y + F.avg_pool2d(x, 3, 1, 1) * 0.3                                   # sees the window's edge
        gain = encoder_hidden_states.to(x.dtype).mean(dim=(1, 2)) + added_cond_kwargs["text_embeds"].to(x.dtype).mean(dim=1)
        return (y * (1.0 + gain)[:, None, None, None],)


class _AnyBatch(_ToyUNet):
    def __call__(self, x, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        self.B = x.shape[0]
        return super().__call__(x, t, encoder_hidden_states, added_cond_kwargs, return_dict)


@pytest.fixture
def restated_kernels(monkeypatch):
    calls = {"gather": 0, "merge": [], "factors": 0}

    def gather(canvas, views, vb, window, k_s=1.0, dup=1, wrap_x=False, out=None):
        calls["gather"] += 1
        got = R.gather_ref(canvas, views, vb, window[0], window[1], torch.tensor(k_s, dtype=torch.float32), dup)
        return got if out is None else out.copy_(got)

    def merge(canvas, eps, views, wy, wx, total, dup=1, guidance_scale=0.0, factor=None, first=True, last=True, wrap_x=False):
        calls["merge"].append((len(views), bool(first), bool(last)))
        vb = eps.shape[0] // dup
        if first:
            canvas.zero_()
        R.merge_partial_ref(canvas, R.guided_ref(eps, vb, dup, guidance_scale, factor), views, wy, wx)
        if last:
            canvas.div_(total[:, None])
        return canvas

    def factors(eps2, g, phi, out=None, workspace=None):
        calls["factors"] += 1
        u, t = eps2.chunk(2)
        f = R.rescale_factor_ref(u, t, g, phi).float()
        return f if out is None else out.copy_(f)

    def dpm(sample, eps, x0_prev, a_s, s_s, c_s, c0, c1):
        x0 = (sample - s_s * eps) / a_s
        sample.copy_(c_s * sample + c0 * x0 + c1 * x0_prev)
        x0_prev.copy_(x0)
        return sample
    monkeypatch.setattr(panorama.ops, "views_gather", gather)
    monkeypatch.setattr(panorama.ops, "views_merge_", merge)
    monkeypatch.setattr(panorama.ops, "cfg_rescale_factors", factors)
    monkeypatch.setattr(sampler.ops, "dpm_update_", dpm)
    monkeypatch.setattr(sampler.ops, "euler_update_", _euler_update_cpu_)
    return calls


@pytest.mark.parametrize("sched,g,phi,wrap,kind", [("dpm", 5.0, 0.7, False, "uniform"), ("euler", 0.0, 0.0, True, "gaussian"),
                                                   ("dpm", 5.0, 0.0, False, "ramp")])
def test_denoise_panorama_loop_with_restated_kernels(restated_kernels, sched, g, phi, wrap, kind):
    """N = 2 canvases of 16 x 40, 4 (5 with wrap) views each at vb = 3: chunks that mix the two images and a padded last chunk; the
    conditioning of every slot is its image's.  Against the restated loop, which calls the model view by view."""
    N, vb, steps = 2, 3, 3
    dup = 2 if g > 1.0 else 1
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(N, 4, 16, 40, generator=gen)
    ehs = torch.randn(dup * N, 7, 8, generator=gen) * 0.3
    added = {"text_embeds": torch.randn(dup * N, 6, generator=gen) * 0.3, "time_ids": torch.zeros(dup * N, 6)}
    toy = _ToyUNet(dup * vb, WIN)
    make, make_ref = ((DPMSolverMultistep, DPMSolverMultistepRef) if sched == "dpm" else (EulerDiscrete, lambda: EulerRef(False)))
    got = panorama.denoise_panorama(toy, make(), x.clone(), ehs, added, num_inference_steps=steps, guidance_scale=g,
                                    guidance_rescale=phi, stride=8, weights=kind, wrap_x=wrap)
    n_views = N * (5 if wrap else 4)
    n_chunks = -(-n_views // vb)
    assert toy.calls == [dup * vb] * (steps * n_chunks) and restated_kernels["gather"] == steps * n_chunks
    per_step = restated_kernels["merge"][:n_chunks]
    assert [m[0] for m in per_step] == [vb] * (n_chunks - 1) + [n_views - vb * (n_chunks - 1)]
    assert [m[1] for m in per_step] == [True] + [False] * (n_chunks - 1) and [m[2] for m in per_step] == [False] * (n_chunks - 1) + [True]
    assert restated_kernels["factors"] == (steps * n_chunks if phi > 0 else 0)
    want = R.denoise_panorama_ref(_AnyBatch(0, WIN), make_ref(), x.double(), ehs, added, steps, g, WIN, WIN, 8, weights=kind,
                                  wrap_x=wrap, phi=phi)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"[denoise_panorama, kernels restated, {sched} g={g} rescale={phi} wrap={wrap} {kind}] max deviation {err:.1e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, 4, 16, 40) and err < 1e-5


def test_denoise_panorama_refusals():
    from pea_diffusion_amd._lib import PeaError
    x, ehs = torch.zeros(1, 4, 16, 40), torch.zeros(2, 7, 8)
    with pytest.raises(PeaError, match="batch 3"):
        panorama.denoise_panorama(_ToyUNet(3, 16), DPMSolverMultistep(), x, ehs, None, guidance_scale=5.0)
    with pytest.raises(PeaError, match="batch 34"):
        panorama.denoise_panorama(_ToyUNet(34, 16), DPMSolverMultistep(), x, ehs, None, guidance_scale=5.0)
    with pytest.raises(PeaError, match="smaller"):
        panorama.denoise_panorama(_ToyUNet(2, 32), DPMSolverMultistep(), x, ehs, None, guidance_scale=5.0)
    with pytest.raises(PeaError, match="prompt_embeds"):
        panorama.denoise_panorama(_ToyUNet(2, 16), DPMSolverMultistep(), x, ehs[:1], None, guidance_scale=5.0)


# ---------------------------------------------------------------------------------------------- the C ABI, without a device
def _abi():
    from pea_diffusion_amd._lib import lib
    L = lib()
    page = (ctypes.c_float * 64)()
    return L, ctypes.cast(page, ctypes.c_void_p)


def _slots(*views):
    return (ctypes.c_int * (3 * len(views)))(*[v for view in views for v in view])


def _gather(L, p, canvas="p", out="p", slots=_slots((0, 0, 0)), n_valid=1, vb=1, dup=1, N=1, C=4, Hc=16, Wc=40, h=16, w=16, wrap=0):
    pick = lambda v: p if v == "p" else v
    return L.pea_op_views_gather(pick(canvas), pick(out), slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap, 1.0, None)


def _merge(L, p, eps="p", canvas="p", slots=_slots((0, 0, 0)), n_valid=1, vb=1, dup=1, N=1, C=4, Hc=16, Wc=40, h=16, w=16, wrap=0,
           factor=None, wy="p", wx="p", total="p"):
    pick = lambda v: p if v == "p" else v
    return L.pea_op_views_merge(pick(eps), pick(canvas), slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap, 5.0, pick(factor), pick(wy),
                                pick(wx), pick(total), 1, 1, None)


REFUSALS = [
    (dict(vb=0, n_valid=0), b"vb=0"), (dict(vb=17, n_valid=1), b"vb=17"),
    (dict(n_valid=0), b"n_valid=0"), (dict(n_valid=2, vb=1, slots=_slots((0, 0, 0), (0, 0, 8))), b"n_valid=2"),
    (dict(dup=0), b"dup=0"), (dict(dup=3), b"dup=3"),
    (dict(h=17), b"window is larger"), (dict(w=41), b"window is larger"),
    (dict(slots=_slots((0, 0, 25))), b"no wrap_x"), (dict(slots=_slots((0, 0, -1))), b"no wrap_x"),
    (dict(slots=_slots((0, 1, 0))), b"no wrap in y"), (dict(slots=_slots((0, -1, 0)), wrap=1), b"no wrap in y"),
    (dict(slots=_slots((0, 0, 40)), wrap=1), b"x0=40"), (dict(slots=_slots((0, 0, -1)), wrap=1), b"x0=-1"),
    (dict(slots=_slots((1, 0, 0))), b"n=1 of 1"), (dict(slots=_slots((-1, 0, 0))), b"n=-1"),
    (dict(slots=None), b"null operand"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS)
def test_kernel_refusals_need_no_device(kw, msg):
    L, p = _abi()
    for op in (_gather, _merge):
        rc = op(L, p, **kw)
        assert rc == -3 and msg in L.pea_last_error(), (op.__name__, kw, rc, L.pea_last_error())


def test_null_operands_and_the_factor_rule_need_no_device():
    L, p = _abi()
    for missing in ("canvas", "out"):
        assert _gather(L, p, **{missing: None}) == -3 and b"null operand" in L.pea_last_error(), missing
    for missing in ("eps", "canvas", "wy", "wx", "total"):
        assert _merge(L, p, **{missing: None}) == -3 and b"null operand" in L.pea_last_error(), missing
    assert _merge(L, p, factor="p", dup=1) == -3 and b"dup=1" in L.pea_last_error()       # factors belong to the guided form
    assert _gather(L, p, slots=_slots((0, 0, 32))) == -3 and b"no wrap_x" in L.pea_last_error()      # fine with wrap_x, refused without
    for a in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.pea_op_cfg_rescale_factors(a[0], 2, 64, 5.0, 0.7, a[1], a[2], None) == -3 and b"null operand" in L.pea_last_error()
    assert L.pea_op_cfg_rescale_factors(p, 0, 64, 5.0, 0.7, p, p, None) == -3 and b"B=0" in L.pea_last_error()
