"""-m gpu: MultiDiffusion panoramas -- the view gather (pea_op_views_gather) and the overlap merge (pea_op_views_merge) against the
plain-torch restatement tests/panorama_ref.py, their exactness properties and bit identities with `ops.cfg_combine`, the loop
`panorama.denoise_panorama` on the tiny UNet (bit-equal to `sampler.denoise` when the canvas is the window; against the restated
loop over the oracle UNet on a 16 x 40 canvas), and `panorama.decode_tiled` on the tiny VAE decoder.

Tolerances.  Gather and merge: the project's rule for fp32-stored results, rtol 1e-3 / atol 1e-4 (`close_f32`).  The loop: the
oracle's own bf16-storage floor of the final latents, measured in the run, x STORAGE_FLOOR_FACTOR (tests/test_model_gpu.py); that
floor has to be at least FLOOR_DEGENERATE (tests/test_turbo_gpu.py).  Everything called "equal" is `torch.equal`."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
import panorama_ref as R  # noqa: E402
from test_model_gpu import STORAGE_FLOOR_FACTOR, cond_inputs, gpu, rel_l2  # noqa: E402,F401
from test_ops_gpu import BF, close_f32, ops  # noqa: E402,F401
from test_turbo_gpu import FLOOR_DEGENERATE, _unaligned  # noqa: E402

WIN = 16
CTX_GAIN = 5.0                                                       # as tests/test_sag_gpu.py: unscaled, the storage floor is degenerate

# name -> (N, C, Hc, Wc, views of one image or None (panorama.views at `stride`), stride, wrap_x, vb, dup, weights, factor)
CASES = {
    # w, Wc and every x0 multiples of 4: the 16-byte path; 4 views, two full chunks
    "vector": (1, 4, 16, 40, None, 8, False, 2, 2, "uniform", False),
    # Wc = 42: the scalar path; 2 x 10 views with the flush origins y0 = 8, x0 = 26, five chunks that cross the image boundary
    "odd_width": (2, 3, 24, 42, None, 8, False, 4, 1, "gaussian", False),
    # 5 views at vb = 2: three chunks, the last one padded; the view at x0 = 32 = Wc - 8 wraps and stays on the 16-byte path
    "wrap": (1, 4, 16, 40, None, 8, True, 2, 2, "ramp", True),
    # an origin that is no multiple of 4 (x0 = 6): the scalar path on an aligned canvas; a padded chunk
    "x0_6": (1, 4, 16, 40, [(0, 0), (0, 6), (0, 16), (0, 24)], 8, False, 3, 2, "gaussian", True),
    # stride 12 on 44 wrapped columns, two images, three chunks (3 + 3 + 2)
    "wrap_44": (2, 4, 16, 44, None, 12, True, 3, 1, "uniform", False),
    # canvas taller than the window only, 16 slots
    "tall": (2, 4, 20, 16, None, 8, False, 16, 2, "ramp", True),
}
G, K_S = 5.0, 0.3713


@functools.lru_cache(maxsize=None)
def _case(name):
    """host data of a case, computed once and never written: the canvas, per chunk (views, eps with NaN in the padded slots,
    factor), the tables, T, and the restatement's gather per chunk and merged canvas"""
    from pea_diffusion_amd import panorama
    N, C, Hc, Wc, vs, stride, wrap, vb, dup, kind, with_factor = CASES[name]
    vs = vs if vs is not None else panorama.views(Hc, Wc, WIN, WIN, stride, wrap)
    triples = R.triples_ref(vs, N)
    gen = torch.Generator().manual_seed(len(name) * 100 + Wc)
    x = torch.randn(N, C, Hc, Wc, generator=gen) * 3.0
    wy = wx = R.weights_ref(WIN, kind, WIN - stride)
    T = R.total_ref(triples, N, Hc, Wc, wy, wx)
    chunks, acc = [], torch.zeros(N, C, Hc, Wc)
    for k in range(0, len(triples), vb):
        views = triples[k:k + vb]
        eps = torch.randn(dup * vb, C, WIN, WIN, generator=gen)
        factor = (0.5 + torch.rand(vb, generator=gen)) if with_factor else None
        R.merge_partial_ref(acc, R.guided_ref(eps, vb, dup, G, factor), views, wy, wx)
        for d in range(dup):                                         # what the UNet returns for a padded slot is not to be read
            eps[d * vb + len(views):(d + 1) * vb] = float("nan")
        if factor is not None:
            factor[len(views):] = float("nan")
        chunks.append((views, eps, factor, R.gather_ref(x, views, vb, WIN, WIN, torch.tensor(K_S), dup)))
    return x, chunks, wy, wx, T, acc / T[:, None]


def _merge_all(ops, name, shift=False):
    """the case's chunks merged on the device into a canvas that starts as NaN; shift: every operand the kernel tests for alignment
    sits behind a pointer offset by 4 bytes.  -> (canvas, the canvas after every chunk)"""
    N, C, Hc, Wc, _, _, wrap, vb, dup, _, _ = CASES[name]
    x, chunks, wy, wx, T, _ = _case(name)
    put = (lambda t: _unaligned(t.cuda()).view(t.shape)) if shift else (lambda t: t.cuda())
    canvas = put(torch.full((N, C, Hc, Wc), float("nan")))
    Td, wyd, wxd = put(T), wy.cuda(), wx.cuda()
    after = []
    for ci, (views, eps, factor, _) in enumerate(chunks):
        ops.views_merge_(canvas, put(eps), views, wyd, wxd, Td, dup, G, None if factor is None else factor.cuda(), first=ci == 0,
                         last=ci == len(chunks) - 1, wrap_x=wrap)
        after.append(canvas.clone())
    return canvas, after


@pytest.mark.parametrize("name", list(CASES))
def test_gather_against_the_restatement(ops, name):
    N, C, Hc, Wc, _, _, wrap, vb, dup, _, _ = CASES[name]
    x, chunks, *_ = _case(name)
    xd = x.cuda()
    for views, _, _, want in chunks:
        got = ops.views_gather(xd, views, vb, (WIN, WIN), K_S, dup, wrap)
        assert tuple(got.shape) == (dup * vb, C, WIN, WIN) and got.dtype == torch.float32
        close_f32(f"views_gather {name}", got, want)
        assert torch.equal(got.cpu(), want)                          # one fp32 product per element: the restatement's bits
        for s in range(len(views), vb):                              # padded slots repeat the last valid slot
            assert torch.equal(got[s], got[len(views) - 1]) and torch.equal(got[(dup - 1) * vb + s], got[len(views) - 1])
        assert dup == 1 or torch.equal(got[vb:], got[:vb])
        # the scalar path behind pointers offset by 4 bytes, and a second run: the same bits
        out = _unaligned(torch.full((got.numel(),), float("nan"), device="cuda")).view(got.shape)
        ops.views_gather(_unaligned(xd).view(x.shape), views, vb, (WIN, WIN), K_S, dup, wrap, out=out)
        assert torch.equal(out, got) and torch.equal(ops.views_gather(xd, views, vb, (WIN, WIN), K_S, dup, wrap), got)


@pytest.mark.parametrize("name", list(CASES))
def test_merge_against_the_restatement(ops, name):
    N, C, Hc, Wc, _, _, wrap, vb, dup, _, _ = CASES[name]
    x, chunks, wy, wx, T, want = _case(name)
    got, after = _merge_all(ops, name)
    assert torch.isfinite(got).all()                                 # neither the canvas's NaNs nor a padded slot's reach the result
    close_f32(f"views_merge {name}", got, want)
    again, _ = _merge_all(ops, name)
    assert torch.equal(again, got)                                   # the same bits every run
    shifted, _ = _merge_all(ops, name, shift=True)
    assert torch.equal(shifted, got)                                 # ... and on the scalar path
    # a chunk that is neither first nor last leaves every element outside its views as it was
    for ci in range(1, len(chunks) - 1):
        cover = R.coverage_ref(chunks[ci][0], N, Hc, Wc, WIN, WIN) > 0
        keep = (~cover)[:, None].expand(N, C, Hc, Wc).cuda()
        assert keep.any() and torch.equal(after[ci][keep], after[ci - 1][keep]) and not torch.equal(after[ci], after[ci - 1])
    if name in ("wrap", "odd_width", "wrap_44"):
        assert len(chunks) >= 3


def test_merge_bit_identities(ops):
    """canvas = window, one view per image, uniform weights: `cfg_combine`'s bits at guidance_rescale 0 and 0.7; a tiling without
    overlap: `cfg_combine` per tile; dup = 1: eps itself"""
    gen = torch.Generator().manual_seed(9)
    ones = torch.ones(WIN, device="cuda")
    eps2 = torch.randn(4, 4, WIN, WIN, generator=gen).cuda()
    views = [(0, 0, 0), (1, 0, 0)]
    T = torch.ones(2, WIN, WIN, device="cuda")
    for phi in (0.0, 0.7):
        factor = ops.cfg_rescale_factors(eps2, G, phi) if phi > 0 else None
        canvas = torch.full((2, 4, WIN, WIN), float("nan"), device="cuda")
        ops.views_merge_(canvas, eps2, views, ones, ones, T, 2, G, factor)
        assert torch.equal(canvas, ops.cfg_combine(eps2, G, phi)), phi
    # two tiles side by side on one 16 x 32 canvas, in two chunks of one view as well as in one chunk of two
    want = ops.cfg_combine(eps2, G)
    T = torch.ones(1, WIN, 2 * WIN, device="cuda")
    canvas = torch.full((1, 4, WIN, 2 * WIN), float("nan"), device="cuda")
    ops.views_merge_(canvas, eps2, [(0, 0, 0), (0, 0, WIN)], ones, ones, T, 2, G)
    assert torch.equal(canvas[0, :, :, :WIN], want[0]) and torch.equal(canvas[0, :, :, WIN:], want[1])
    split = torch.full_like(canvas, float("nan"))
    for s in range(2):
        one = torch.stack([eps2[s], eps2[2 + s]])
        ops.views_merge_(split, one, [(0, 0, s * WIN)], ones, ones, T, 2, G, first=s == 0, last=s == 1)
    assert torch.equal(split, canvas)
    # dup = 1
    e = torch.randn(1, 3, WIN, WIN, generator=gen).cuda()
    canvas = torch.full((1, 3, WIN, WIN), float("nan"), device="cuda")
    ops.views_merge_(canvas, e, [(0, 0, 0)], ones, ones, torch.ones(1, WIN, WIN, device="cuda"), 1)
    assert torch.equal(canvas, e)


def test_rescale_factors_are_cfg_combine_s(ops):
    gen = torch.Generator().manual_seed(10)
    eps2 = torch.randn(6, 4, WIN, WIN, generator=gen)
    f = ops.cfg_rescale_factors(eps2.cuda(), G, 0.7)
    close_f32("cfg_rescale_factors", f, R.rescale_factor_ref(eps2[:3], eps2[3:], G, 0.7).float())
    plain, scaled = ops.cfg_combine(eps2.cuda(), G), ops.cfg_combine(eps2.cuda(), G, 0.7)
    assert torch.equal(plain * f.view(-1, 1, 1, 1), scaled)


def test_refusals_through_ops(ops):
    from pea_diffusion_amd._lib import PeaError
    x = torch.zeros(1, 4, 16, 40, device="cuda")
    with pytest.raises(PeaError, match="no wrap_x"):
        ops.views_gather(x, [(0, 0, 32)], 1, (WIN, WIN))
    with pytest.raises(PeaError, match="views for a chunk"):
        ops.views_gather(x, [(0, 0, 0)] * 3, 2, (WIN, WIN))
    with pytest.raises(PeaError, match="vb=17"):
        ops.views_gather(x, [(0, 0, 0)], 17, (WIN, WIN))
    ones, T, e = torch.ones(WIN, device="cuda"), torch.ones(1, 16, 40, device="cuda"), torch.zeros(1, 4, WIN, WIN, device="cuda")
    with pytest.raises(PeaError, match="dup=1"):
        ops.views_merge_(x, e, [(0, 0, 0)], ones, ones, T, 1, factor=torch.ones(1, device="cuda"))
    with pytest.raises(PeaError, match="total"):
        ops.views_merge_(x, e, [(0, 0, 0)], ones, ones, T[:, :8].contiguous(), 1)


# ---------------------------------------------------------------------------------------------- the loop, tiny UNet
def _tiny(UB, N, dup, Wc, L=77):
    """the tiny UNet pair at batch UB, latents [N, 4, 16, Wc] and per-image conditioning [dup N] (the context gain of the SAG tests)"""
    from test_ip_adapter_gpu import _tiny_ip_pair
    cfg, ref, hip = _tiny_ip_pair(UB, L)
    _, _, ehs, added = cond_inputs(cfg, dup * N, L, 16)
    x = torch.randn(N, 4, 16, Wc, generator=torch.Generator().manual_seed(21))
    return ref, hip, x, (CTX_GAIN * ehs).to(BF).float(), added


@pytest.mark.parametrize("sched,g,phi", [("dpm", 5.0, 0.7), ("ancestral", 0.0, 0.0)])
def test_canvas_of_one_window_is_denoise(gpu, sched, g, phi):
    """canvas = window: `denoise_panorama` gives the bits of `sampler.denoise` on the same context, seed and scheduler"""
    from pea_diffusion_amd.panorama import denoise_panorama
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerAncestralDiscrete, denoise
    N = 2
    dup = 2 if g > 1.0 else 1
    _, hip, x, ehs, added = _tiny(dup * N, N, dup, 16)
    make = DPMSolverMultistep if sched == "dpm" else EulerAncestralDiscrete
    args = lambda: (hip, make(), x.cuda(), ehs.cuda(), {k: v.cuda() for k, v in added.items()})
    kw = lambda: dict(num_inference_steps=3, guidance_scale=g, guidance_rescale=phi, generator=torch.Generator().manual_seed(4))
    want = denoise(*args(), **kw()).clone()
    got = denoise_panorama(*args(), **kw())
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert torch.equal(denoise_panorama(*args(), weights="uniform", stride=4, **kw()), want)


@pytest.mark.parametrize("sched,g,N,kind,wrap", [("dpm", 5.0, 2, "uniform", False), ("euler", 0.0, 1, "gaussian", True)])
def test_denoise_panorama_tiny_vs_oracle(gpu, sched, g, N, kind, wrap):
    """3 steps on 16 x 40 canvases, stride 8, vb = 2, against the restated loop over the oracle UNet: DPM-Solver under CFG with
    uniform weights (2 canvases, 8 views, chunks that cross the image boundary), Euler without guidance with gaussian weights and
    wrap (5 views, the last chunk padded).  Measured on an MI355X (ratio = error / bf16-storage floor; the limit is 1.5):
    dpm: rel_l2 8.4e-3 on a floor of 8.5e-3, ratio 0.99; euler: 2.1e-3 on 2.3e-3, ratio 0.94."""
    from oracle.bf16_store import bf16_storage
    from oracle.sampler_ref import DPMSolverMultistepRef
    from pea_diffusion_amd.panorama import denoise_panorama
    from pea_diffusion_amd.sampler import DPMSolverMultistep, EulerDiscrete
    from turbo_ref import EulerRef
    n, vb = 3, 2
    dup = 2 if g > 1.0 else 1
    ref, hip, x, ehs, added = _tiny(dup * vb, N, dup, 40)
    make_ref = (lambda: DPMSolverMultistepRef()) if sched == "dpm" else (lambda: EulerRef(False))
    loop = lambda: R.denoise_panorama_ref(lambda *a, **k: ref(*a, **k), make_ref(), x.clone(), ehs, added, n, g, WIN, WIN, 8,
                                          weights=kind, wrap_x=wrap).float()
    with torch.no_grad():
        want = loop()
        with bf16_storage():
            stored = loop()
    floor = rel_l2(stored, want)
    limit = STORAGE_FLOOR_FACTOR * floor
    run = lambda: denoise_panorama(hip, DPMSolverMultistep() if sched == "dpm" else EulerDiscrete(), x.cuda(), ehs.cuda(),
                                   {k: v.cuda() for k, v in added.items()}, num_inference_steps=n, guidance_scale=g, stride=8,
                                   weights=kind, wrap_x=wrap)
    got = run()
    e = rel_l2(got, want)
    print(f"[denoise_panorama tiny, {sched} {n} steps, guidance {g}, {N} x 16 x 40, {kind}, wrap={wrap}] latents rel_l2={e:.3e}, "
          f"bf16-storage floor {floor:.3e}, ratio {e / max(floor, 1e-30):.2f}, limit {limit:.3e} ({STORAGE_FLOOR_FACTOR} x floor)")
    assert floor >= FLOOR_DEGENERATE, floor
    assert torch.isfinite(got).all() and tuple(got.shape) == (N, 4, 16, 40) and e <= limit
    assert torch.equal(run(), got)                                   # bit-reproducible


# ---------------------------------------------------------------------------------------------- tiled decode, tiny VAE
def test_decode_tiled_of_one_tile_is_decode(gpu):
    from pea_diffusion_amd.panorama import decode_tiled
    from test_vae_gpu import _dec_pair
    ref, dec = _dec_pair("tiny_vae_config", 2, 16, 16)
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)).cuda() / ref.config.scaling_factor
    want = dec.decode(z)[0].clone()
    got = decode_tiled(dec, z)
    f = dec.scale_factor
    assert tuple(got.shape) == (2, 3, 16 * f, 16 * f) and torch.equal(got, want)


def test_decode_tiled_against_the_restated_merge(gpu):
    """a 16 x 40 canvas through a batch-3 decoder of 16 x 16 tiles at stride 8: 4 tiles, two calls, the second padded; against the
    restatement's merge of the decoder's own per-tile outputs"""
    from pea_diffusion_amd.panorama import decode_tiled
    from test_vae_gpu import _dec_pair
    ref, dec = _dec_pair("tiny_vae_config", 3, 16, 16)
    z = torch.randn(1, 4, 16, 40, generator=torch.Generator().manual_seed(5)) / ref.config.scaling_factor
    triples = R.triples_ref(R.views_ref(16, 40, 16, 16, 8), 1)
    tiles = []
    for k in range(0, len(triples), 3):
        chunk = triples[k:k + 3]
        tiles.append(dec.decode(R.gather_ref(z, chunk, 3, 16, 16).cuda())[0][:len(chunk)].cpu())
    f = dec.scale_factor
    want = R.decode_tiled_ref(torch.cat(tiles), triples, 1, 16, 40, 16, 16, f, 8)
    got = decode_tiled(dec, z.cuda(), stride=8)
    assert tuple(got.shape) == (1, 3, 16 * f, 40 * f)
    close_f32("decode_tiled 16 x 40", got, want)
    assert torch.equal(decode_tiled(dec, z.cuda(), stride=8), got)
