"""Kernels on the operand layouts the UNet hands them (-m gpu): column slices of wider buffers, leading dimensions that
change the epilogue the GEMM launcher picks, the fused Q|K|V buffer and the stacked cross-attention K|V buffer of the
attention operators, and the non-square latent grids of the aspect-ratio buckets at full SDXL channel widths.

Conventions are those of tests/test_ops_gpu.py: the reference is plain torch fp32 on the same bf16-rounded inputs, with
its close_bf16 / close_f32 tolerances (the same formulas, evaluated where the result lives).  Every strided destination is a
*canvas*: a buffer wider and taller than the result (column offset, ld > N, slack rows around the [M, N] window) filled
with a sentinel bit pattern before the call; after the call every element outside the window must still hold it, bit for
bit.  Where the same kernel form runs on a contiguous layout, strided and contiguous results must be bitwise equal.
"""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENT16 = -0x5433                   # bf16 bits 0xabcd
SENT32 = 0x7fabcdef                # a NaN pattern for fp32 destinations
ALPHA = 0.125 * math.log2(math.e)  # softmax scale x log2(e) of head_dim 64 (what a prescaled Q carries)
GEMM_VARIANTS = [18, 19, 22, 23, 24, 25, 27, 28, 29, 30, 31, 33, 34, 35, 39, 40]     # test_gemm_every_variant_ragged_shapes
CONV_VARIANTS = [22, 23, 24, 25, 27, 28, 29, 30, 31, 33]                             # test_conv3x3_every_variant
VARIANT_IDS = dict(ids=lambda v: "default" if v < 0 else f"v{v}")                   # (-1: the launcher's own choice)
RAGGED = [(308, 640, 128), (1000, 104, 192), (4100, 1288, 256), (130, 3840, 64), (33000, 336, 128), (64, 160, 640)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a MI355X (torch.cuda.is_available() is False)")
    from pea_diffusion_amd import ops as o
    return o


def L():
    from pea_diffusion_amd._lib import lib
    return lib()


def call(rc):
    from pea_diffusion_amd._lib import check
    check(rc)


def vp(t):
    """device pointer of a tensor or of a view into one (slices of wider buffers are the point here)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bfr(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def close_bf16(name, got, ref, ulps=1.0):
    """tests/test_ops_gpu.py close_bf16 (1 bf16 ulp of |ref| + rms, no element outside, rel_l2 < 6e-3) on got's device"""
    got = got.detach().float()
    ref = ref.detach().float().to(got.device)
    rms = ref.pow(2).mean().sqrt().item() + 1e-30
    err = (got - ref).abs()
    tol = ulps * (2.0 ** -7) * (ref.abs() + rms)
    bad = (err > tol).float().mean().item()
    rel_l2 = ((got - ref).pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-30)).item()
    print(f"[{name}] max_abs={err.max().item():.3e} rel_l2={rel_l2:.3e} rms={rms:.3e} frac_bad={bad:.2e}")
    assert torch.isfinite(got).all(), name
    assert bad == 0.0 and rel_l2 < 6e-3, f"{name}: frac_bad={bad} rel_l2={rel_l2}"


def close_f32(name, got, ref, rtol=1e-3, atol=1e-4):
    got = got.detach().float()
    ref = ref.detach().float().to(got.device)
    print(f"[{name}] max_abs={(got - ref).abs().max().item():.3e} ref_max={ref.abs().max().item():.3e}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)


def rel_l2(got, ref):
    got, ref = got.detach().float(), ref.detach().float().to(got.device)
    return ((got - ref).pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-30)).item()


def bits_equal(name, a, b):
    assert a.shape == b.shape, name
    a = a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32)
    b = b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32)
    n = int((a != b).sum())
    assert n == 0, f"{name}: {n} element(s) differ bitwise"


class Canvas:
    """A [r0 + M + slack, ld] destination filled with the sentinel; `win(i)` are the [M, n_i] windows at columns c_i of rows
    r0 .. r0 + M.  `check` asserts that nothing outside the windows changed."""

    def __init__(self, M, ld, windows, r0=1, slack=3, dtype=BF):
        self.dtype, self.ld, self.M, self.r0 = dtype, ld, M, r0
        self.buf = torch.empty(r0 + M + slack, ld, device="cuda", dtype=dtype)
        self.bits = self.buf.view(torch.int16 if dtype == BF else torch.int32)
        self.sent = SENT16 if dtype == BF else SENT32
        self.bits.fill_(self.sent)
        self.outside = torch.ones(self.buf.shape, device="cuda", dtype=torch.bool)
        self.wins = []
        for (c0, n) in windows:
            assert c0 + n <= ld
            self.outside[r0:r0 + M, c0:c0 + n] = False
            self.wins.append(self.buf[r0:r0 + M, c0:c0 + n])

    def win(self, i=0):
        return self.wins[i]

    def check(self, name):
        torch.cuda.synchronize()
        n = int((self.bits[self.outside] != self.sent).sum())
        assert n == 0, f"{name}: {n} element(s) outside the result window were written"

    def untouched(self, name):
        torch.cuda.synchronize()
        n = int((self.bits != self.sent).sum())
        assert n == 0, f"{name}: {n} element(s) of the destination were written by a refused call"


def strided(t, pad, c0):
    """a copy of the 2-D tensor t as columns [c0, c0 + cols) of a [rows, cols + pad] buffer (lda > K)"""
    R, Cc = t.shape
    buf = torch.randn(R, Cc + pad, device="cuda").to(t.dtype)
    v = buf[:, c0:c0 + Cc]
    v.copy_(t)
    return v


# ------------------------------------------------------------------------------------ GEMM family
# destination layouts: (ldc - N, column offset, 16-byte aligned C with ldc % 8 == 0)
C_LAYOUTS = {"pair": (24, 8, True),      # batched-load epilogue and its 32-column paired stores
             "ld4": (12, 0, False),      # ldc % 8 == 4: the general store path
             "off4": (16, 4, False)}     # C offset by 4 columns: 8-byte but not 16-byte aligned


def gemm_raw(a, w, c, ldc, M, N, K, alpha=1.0, bias=None, rowvec=None, rpb=1, act=0, pre=None, ldpre=0, res=None, ldres=0,
             out_f32=0, accum=0):
    call(L().pea_op_gemm(vp(a), a.stride(0), vp(w), w.stride(0), vp(c), ldc, M, N, K, alpha, vp(bias), vp(rowvec),
                         rowvec.stride(0) if rowvec is not None else 0, rpb, act, vp(pre), ldpre, vp(res), ldres, out_f32, accum,
                         stream()))


def _gemm_layout_cases(ops, variant, M, N, K, g):
    a = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    bias = torch.randn(N, generator=g)
    rpb = 64 if M < 1000 else 128                            # 64 x k rows per sample: the row vector's batched-load form
    rv = torch.randn((M + rpb - 1) // rpb, N, generator=g).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    ref = a.float() @ w.float().T
    base = ref * 0.5 + bias + rv.float().repeat_interleave(rpb, 0)[:M]
    epi_ref = base + res.float()
    ad = strided(a.cuda(), 40, 8)                            # lda = K + 40, A at a 16-byte column offset
    wd, bd, rvd = w.cuda(), bias.cuda(), rv.cuda()
    staged = variant in (34, 35)                             # staged / deferred epilogues: bf16 output, bias only
    tag = f"v{variant} {M}x{N}x{K}"
    # contiguous references of the same kernel form
    cont = torch.empty(M, N, device="cuda", dtype=BF)
    gemm_raw(ad, wd, cont, N, M, N, K)
    cont_epi = torch.empty(M, N, device="cuda", dtype=BF)
    if not staged:
        gemm_raw(ad, wd, cont_epi, N, M, N, K, 0.5, bd, rvd, rpb, res=res.cuda(), ldres=N)
    else:
        gemm_raw(ad, wd, cont_epi, N, M, N, K, 1.0, bd)
    general = {}
    for name, (pad, c0, aligned) in C_LAYOUTS.items():
        fast = aligned and N % 16 == 0
        cv = Canvas(M, N + pad, [(c0, N)])
        gemm_raw(ad, wd, cv.win(), cv.ld, M, N, K)
        cv.check(f"{tag} plain {name}")
        close_bf16(f"{tag} plain {name}", cv.win(), ref)
        bits_equal(f"{tag} plain {name} vs contiguous", cv.win(), cont)       # (no epilogue terms: one rounding either way)
        ce = Canvas(M, N + pad, [(c0, N)])
        if staged:
            gemm_raw(ad, wd, ce.win(), ce.ld, M, N, K, 1.0, bd)
            want = ref + bias
        else:
            rs = strided(res.cuda(), 40, c0)                 # the residual with its own ld (and the same alignment as C)
            gemm_raw(ad, wd, ce.win(), ce.ld, M, N, K, 0.5, bd, rvd, rpb, res=rs, ldres=rs.stride(0))
            want = epi_ref
        ce.check(f"{tag} epilogue {name}")
        close_bf16(f"{tag} epilogue {name}", ce.win(), want)
        if fast or N % 16 != 0:
            bits_equal(f"{tag} epilogue {name} vs contiguous", ce.win(), cont_epi)
        else:
            general.setdefault("epi", []).append(ce.win().clone())
        if staged:
            continue
        # activation + pre-activation + residual: the general epilogue on every layout; preact / res with their own ld
        cp = Canvas(M, N + pad, [(c0, N)])
        cpre = Canvas(M, N + 20, [(4, N)], r0=2)
        rs = strided(res.cuda(), 36, 4)
        gemm_raw(ad, wd, cp.win(), cp.ld, M, N, K, 0.5, bd, rvd, rpb, act=2, pre=cpre.win(), ldpre=cpre.ld, res=rs,
                 ldres=rs.stride(0))
        cp.check(f"{tag} silu+preact {name}")
        cpre.check(f"{tag} preact canvas {name}")
        close_bf16(f"{tag} silu+res {name}", cp.win(), F.silu(base) + res.float())
        close_bf16(f"{tag} preact {name}", cpre.win(), base)
        general.setdefault("act", []).append(cp.win().clone())
        general.setdefault("pre", []).append(cpre.win().clone())
    # results of one general-epilogue kernel form on different layouts agree bit for bit.  Against the batched-load form
    # (contiguous / aligned C) they may differ in the last bit: gemm_epilogue16_fast sums bias + row vector first and applies
    # acc * alpha + that sum as ONE fma, the general epilogue rounds acc * alpha, adds the bias, then the row vector; those
    # results are held to the tolerance above
    for k, outs in general.items():
        for o in outs[1:]:
            bits_equal(f"{tag} {k} general-epilogue layouts", o, outs[0])
    if staged:
        return
    # fp32 output into a strided fp32 destination (ldc % 8 == 4, 16-byte column offset), and fp32 accumulate into it
    cf = Canvas(M, N + 12, [(4, N)], dtype=torch.float32)
    gemm_raw(ad, wd, cf.win(), cf.ld, M, N, K, out_f32=1)
    cf.check(f"{tag} fp32 out")
    close_f32(f"{tag} fp32 out", cf.win(), ref, rtol=2e-3, atol=2e-3)
    cf.win().copy_(torch.ones(M, N, device="cuda"))
    gemm_raw(ad, wd, cf.win(), cf.ld, M, N, K, out_f32=1, accum=1)
    cf.check(f"{tag} fp32 accumulate")
    close_f32(f"{tag} fp32 accumulate", cf.win(), ref + 1.0, rtol=2e-3, atol=2e-3)
    # accumulate into a strided bf16 gradient buffer: the residual aliases the output (same pointer, same ld)
    cg = Canvas(M, N + 16, [(4, N)])
    cg.win().copy_(res.cuda())
    gemm_raw(ad, wd, cg.win(), cg.ld, M, N, K, res=cg.win(), ldres=cg.ld)
    cg.check(f"{tag} bf16 accumulate")
    close_bf16(f"{tag} bf16 accumulate", cg.win(), ref + res.float())
    # the fused Q|K|V projection's column scale on a strided output
    qc = (N // 3) // 16 * 16
    for name in ("pair", "ld4"):
        pad, c0, _ = C_LAYOUTS[name]
        cq = Canvas(M, N + pad, [(c0, N)])
        call(L().pea_op_gemm_qscale(vp(ad), ad.stride(0), vp(wd), K, vp(cq.win()), cq.ld, M, N, K, vp(bd), qc, ALPHA, stream()))
        cq.check(f"{tag} qscale {name}")
        want = ref + bias
        want[:, :qc] *= ALPHA
        close_bf16(f"{tag} qscale {name}", cq.win(), want)


@pytest.mark.parametrize("variant", [-1] + GEMM_VARIANTS, **VARIANT_IDS)
def test_gemm_layouts(ops, variant):
    """pea_op_gemm / pea_op_gemm_qscale with A a column slice (lda > K), C in the three destination layouts, the residual and
    the pre-activation with their own ld and offset, a per-sample row vector of 64 x k rows, fp32 output / accumulate and the
    bf16 accumulate-into form; the ragged shapes of test_gemm_every_variant_ragged_shapes (N = 336 ends inside a 32-column
    store pair, N = 104 / 1288 are not multiples of 16)"""
    g = torch.Generator().manual_seed(100 + variant)
    try:
        L().pea_debug_set_gemm_variant(variant)
        for (M, N, K) in RAGGED:
            _gemm_layout_cases(ops, variant, M, N, K, g)
    finally:
        L().pea_debug_set_gemm_variant(-1)


def test_gemm_refused_layouts_leave_the_destination_alone(ops):
    """Layouts SHAPECHK forbids raise PeaError before any launch: lda % 8 != 0, ldc % 4 != 0, qscale_cols % 16 != 0"""
    from pea_diffusion_amd._lib import PeaError
    M, N, K = 256, 320, 128
    a = bfr(M, K + 16, seed=1).cuda()
    w = bfr(N, K, seed=2, scale=K ** -0.5).cuda()
    a8 = a[:, :K]
    cases = [("lda % 8", a, K + 4, N + 8), ("ldc % 4", a8, K + 16, N + 2)]
    for name, at, lda, ldc in cases:
        cv = Canvas(M, ldc, [(0, N)])
        with pytest.raises(PeaError, match="lda|ldc"):
            call(L().pea_op_gemm(vp(at), lda, vp(w), K, vp(cv.win()), ldc, M, N, K, 1.0, None, None, 0, 1, 0, None, 0, None, 0, 0,
                                 0, stream()))
        cv.untouched(f"gemm {name}")
    cv = Canvas(M, N + 8, [(0, N)])
    with pytest.raises(PeaError, match="qscale_cols"):
        call(L().pea_op_gemm_qscale(vp(a8), K + 16, vp(w), K, vp(cv.win()), cv.ld, M, N, K, None, 104, ALPHA, stream()))
    cv.untouched("gemm qscale_cols % 16")
    # attention: leading dimensions must be multiples of 8; the backward needs Sq % 4 == 0
    B, H, S = 1, 2, 92
    C = H * 64
    qkv = bfr(B * S + 1, 3 * C + 4, seed=3).cuda()
    o = Canvas(B * S, C, [(0, C)])
    lse = torch.empty(B, H, S, device="cuda")
    with pytest.raises(PeaError, match="multiples of 8"):
        call(L().pea_op_attention_fwd(vp(qkv), 3 * C + 4, vp(qkv[:, C:]), 3 * C + 4, vp(qkv[:, 2 * C:]), 3 * C + 4,
                                      vp(o.win()), C, vp(lse), B, H, S, S, 0.125, 1, stream()))
    o.untouched("attention ldq % 8")
    Sq = 91                                           # an SD1.5 mid block at a 56 x 104 latent: 7 x 13 tokens
    q, kv = bfr(Sq, C, seed=4).cuda(), bfr(77, 2 * C, seed=5).cuda()
    oo, ll = ops.attention_fwd(q.view(1, Sq, C), kv[:, :C].contiguous().view(1, 77, C), kv[:, C:].contiguous().view(1, 77, C), H)
    dq = Canvas(Sq, C, [(0, C)])
    dkv = Canvas(77, 2 * C, [(0, C), (C, C)])
    delta = torch.empty(2, 1, H, Sq, device="cuda")
    with pytest.raises(PeaError, match="multiple of 4"):
        call(L().pea_op_attention_bwd(vp(q), C, vp(kv), 2 * C, vp(kv[:, C:]), 2 * C, vp(oo), C, vp(q), C, vp(ll), vp(delta),
                                      vp(dq.win()), C, vp(dkv.win(0)), 2 * C, vp(dkv.win(1)), 2 * C, 1, H, Sq, 77, 0.125, 0, 0, 1,
                                      None, stream()))
    dq.untouched("attention bwd Sq % 4 (dQ)")
    dkv.untouched("attention bwd Sq % 4 (dK|dV)")


def _geglu_factors(pre):
    h, gate = pre[:, 0::2], pre[:, 1::2]
    phi = 0.5 * (1.0 + torch.erf(gate / 2 ** 0.5))
    return gate * phi, h * (phi + gate * torch.exp(-0.5 * gate * gate) / (2 * torch.pi) ** 0.5)


@pytest.mark.parametrize("variant", [-1] + GEMM_VARIANTS, **VARIANT_IDS)
def test_gemm_geglu_strided(ops, variant):
    """GEGLU in the FF projection's epilogue with A a column slice; y and the stash at offsets inside wider buffers (y 8-byte
    aligned: the GEGLU fast form allows it; the stash 16-byte aligned, then 8-byte: the general store path), both stash forms;
    a ragged row count, N = 1288 (not a multiple of 16: the general epilogue) and an SDXL FF shape, under every variant"""
    try:
        for (M, N, K) in [(308, 2560, 320), (1000, 1288, 192), (1456, 2560, 320)]:
            g = torch.Generator().manual_seed(M + N)
            a = torch.randn(M, K, generator=g).to(BF)
            w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
            bias = torch.randn(N, generator=g) * 0.1
            pre = a.float() @ w.float().t() + bias
            ad, wd, bd = strided(a.cuda(), 24, 8), w.cuda(), bias.cuda()
            yref = pre[:, 0::2] * F.gelu(pre[:, 1::2])
            fa, fb = _geglu_factors(pre)
            L().pea_debug_set_gemm_variant(variant)
            for stash_grad in (1, 0):
                outs = {}
                for st_off in (8, 4):
                    y = Canvas(1, M * (N // 2) + 12, [(4, M * (N // 2))], r0=0, slack=1)      # y at +8 bytes
                    st = Canvas(1, M * N + 16, [(st_off, M * N)], r0=0, slack=1)             # stash at +16 / +8 bytes
                    yv, stv = y.win().view(M, N // 2), st.win().view(M, N)
                    call(L().pea_op_gemm_geglu(vp(ad), ad.stride(0), vp(wd), K, vp(bd), vp(yv), vp(stv), M, N, K, stash_grad, 0,
                                               stream()))
                    tag = f"v{variant} geglu {M}x{N}x{K} grad-form {stash_grad} stash +{2 * st_off}B"
                    y.check(tag + " y")
                    st.check(tag + " stash")
                    close_bf16(tag + " y", yv, yref, ulps=2.0)
                    close_bf16(tag + " stash", stv, torch.stack([fa, fb], -1).reshape(M, N) if stash_grad else pre, ulps=2.0)
                    outs[st_off] = (yv.clone(), stv.clone())
                y0, st0 = ops.gemm_geglu(a.cuda(), wd, bd, stash_grad=bool(stash_grad))
                bits_equal(f"v{variant} geglu y (grad form {stash_grad}) offset vs fresh", outs[8][0], y0)
                bits_equal(f"v{variant} geglu stash (grad form {stash_grad}) offset vs fresh", outs[8][1], st0)
    finally:
        L().pea_debug_set_gemm_variant(-1)


@pytest.mark.parametrize("variant", [-1] + GEMM_VARIANTS, **VARIANT_IDS)
def test_gemm_geglu_bwd_strided(ops, variant):
    """the FF output projection's dgrad with the GEGLU backward in its epilogue: A and the stash column slices of wider
    buffers, d(pre) written at a column offset with ldc > 2N; both stash forms; a ragged M with N = 1296 (ends inside a
    160-column tile) and SDXL shapes; every pinned variant (the launcher maps them onto its 256-, 128- and 64-row forms);
    bitwise equal to the contiguous call"""
    try:
        for (M, N, K) in [(308, 1296, 256), (1000, 2560, 320), (392, 5120, 1280)]:
            for form in (0, 1):
                g = torch.Generator().manual_seed(M + N + form)
                a = (torch.randn(M, K, generator=g) * 0.5).to(BF)
                w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
                pre = (torch.randn(M, 2 * N, generator=g) * 1.2).to(BF)
                fa, fb = _geglu_factors(pre.float())
                if form == 1:
                    pre = torch.stack([fa, fb], -1).reshape(M, 2 * N).to(BF)
                    fa, fb = pre.float()[:, 0::2], pre.float()[:, 1::2]
                dy = a.float() @ w.float().t()
                ref = torch.stack([dy * fa, dy * fb], -1).reshape(M, 2 * N)
                ad, pd, wd = strided(a.cuda(), 40, 8), strided(pre.cuda(), 48, 16), w.cuda()
                cv = Canvas(M, 2 * N + 24, [(8, 2 * N)])
                L().pea_debug_set_gemm_variant(variant)
                call(L().pea_op_gemm_geglu_bwd(vp(ad), ad.stride(0), vp(wd), K, vp(pd), pd.stride(0), vp(cv.win()), cv.ld, M, N, K,
                                               form, stream()))
                tag = f"v{variant} geglu bwd form {form} {M}x{N}x{K} strided"
                cv.check(tag)
                close_bf16(tag, cv.win(), ref)
                bits_equal(tag + " vs contiguous", cv.win(), ops.gemm_geglu_bwd(a.cuda(), wd, pre.cuda(), form=form))
    finally:
        L().pea_debug_set_gemm_variant(-1)


@pytest.mark.parametrize("variant", [-1] + GEMM_VARIANTS, **VARIANT_IDS)
def test_ln_linear_offsets(ops, variant):
    """LayerNorm folded into its Linear with the outputs at offsets inside wider buffers (its ABI has no leading dimensions:
    the canary is what a row or column overrun would hit); plain and GEGLU forms; a ragged M with N = 1296 and SDXL shapes;
    every pinned variant (the launcher maps them onto its five folded-LayerNorm forms); bitwise equal to the fresh-tensor call"""
    try:
        for (M, N, K) in [(308, 1296, 256), (1000, 1920, 640), (392, 3840, 1280)]:
            g = torch.Generator().manual_seed(N)
            x = (torch.randn(M, K, generator=g) * 1.3 + 0.5).to(BF)
            w = bfr(N, K, seed=2, scale=K ** -0.5)
            gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
            bias = torch.randn(N, generator=g)
            ref = F.layer_norm(x.float(), (K,), gamma, beta, 1e-5) @ w.float().T + bias
            xd, gd, bd, wd, bsd = x.cuda(), gamma.cuda(), beta.cuda(), w.cuda(), bias.cuda()
            wf, sv, tv, stt = (torch.empty(N, K, device="cuda", dtype=BF), torch.empty(N, device="cuda"),
                               torch.empty(N, device="cuda"), torch.empty(M, 2, device="cuda"))
            tag = f"v{variant} ln_linear {M}x{N}x{K}"
            L().pea_debug_set_gemm_variant(variant)
            y = Canvas(M, N, [(0, N)], r0=2, slack=2)
            call(L().pea_op_ln_linear(vp(xd), vp(gd), vp(bd), vp(wd), vp(bsd), vp(y.win()), None, M, N, K, 1e-5, vp(wf), vp(sv),
                                      vp(tv), vp(stt), stream()))
            y.check(tag)
            close_bf16(tag + " at an offset", y.win(), ref, ulps=2.0)
            bits_equal(tag + " offset vs fresh", y.win(), ops.ln_linear(xd, gd, bd, wd, bsd))
            gy = Canvas(M, N // 2, [(0, N // 2)], r0=3, slack=2)
            y2 = Canvas(M, N, [(0, N)], r0=1, slack=2)
            call(L().pea_op_ln_linear(vp(xd), vp(gd), vp(bd), vp(wd), vp(bsd), vp(y2.win()), vp(gy.win()), M, N, K, 1e-5, vp(wf),
                                      vp(sv), vp(tv), vp(stt), stream()))
            gy.check(tag + " geglu y")
            y2.check(tag + " geglu preact")
            close_bf16(tag + " geglu preact", y2.win(), ref, ulps=2.0)
            close_bf16(tag + " geglu y", gy.win(), ref[:, 0::2] * F.gelu(ref[:, 1::2]), ulps=3.0)
            gy0, y20 = ops.ln_linear(xd, gd, bd, wd, bsd, geglu=True)
            bits_equal(tag + " geglu y offset vs fresh", gy.win(), gy0)
            bits_equal(tag + " geglu preact offset vs fresh", y2.win(), y20)
    finally:
        L().pea_debug_set_gemm_variant(-1)


# ------------------------------------------------------------------------------------ attention
def kv_stack(cfg):
    """(column offset, padded width Cp) of every cross-attention layer's K block in the stacked K|V projection, in the order
    graph.hip builds them (down blocks, mid block, up blocks; K at kv_off, V at kv_off + Cp), and the stack's width"""
    from pea_diffusion_amd.config import depth_tables
    down, up, mid = depth_tables(cfg)
    n = len(cfg.block_out_channels)
    layers = []

    def add(level, depth):
        C, h = cfg.block_out_channels[level], cfg.num_attention_heads[level]
        cp = h * ((C // h + 63) // 64 * 64)
        for _ in range(depth):
            layers.append(cp)
    for i in range(n):
        if cfg.down_block_types[i].startswith("CrossAttn"):
            for j in range(cfg.layers_per_block):
                add(i, down[i][j])
    if mid >= 0:
        add(n - 1, mid)
    for i in range(n):
        if cfg.up_block_types[i].startswith("CrossAttn"):
            for j in range(cfg.layers_per_block + 1):
                add(n - 1 - i, up[i][j])
    offs, w = [], 0
    for cp in layers:
        offs.append((w, cp))
        w += 2 * cp
    return offs, w


@pytest.mark.parametrize("cfg_name,width", [("sdxl_config", 166400), ("sd15_config", None)])
def test_stacked_kv_layout_matches_the_model(ops, cfg_name, width):
    """kv_stack (what the cross-attention test takes its K|V offset from) against the library's own record of the stacked
    K|V projection (pea_unet_stacked_layout): every layer's to_k / to_v column block, in order; SDXL: 70 layers, 166 400 columns"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd.unet import HipUNet
    cfg = getattr(pc, cfg_name)()
    offs, w = kv_stack(cfg)
    if width is not None:
        assert w == width
    u = HipUNet(cfg, 1, 16, 16, 77)
    got = []
    try:
        i = 0
        while True:
            name = ctypes.create_string_buffer(256)
            off, n = ctypes.c_int(), ctypes.c_int()
            if L().pea_unet_stacked_layout(u._h, 0, i, name, 256, ctypes.byref(off), ctypes.byref(n)) != 0:
                break
            got.append((name.value.decode(), off.value, n.value))
            i += 1
    finally:
        del u
    want = []
    for o, cp in offs:
        want += [("to_k", o, cp), ("to_v", o + cp, cp)]
    assert len(got) == len(want), (len(got), len(want))
    for (name, o, n), (kind, wo, wn) in zip(got, want):
        assert f"attn2.{kind}." in name and (o, n) == (wo, wn), (name, o, n, kind, wo, wn)


def attn_ref(q, k, v, H, dp, scale):
    B, Sq, C = q.shape
    qh, kh, vh = [t.view(B, -1, H, dp).transpose(1, 2) for t in (q, k, v)]
    s = qh @ kh.transpose(-1, -2) * scale
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Sq, C)
    return o, torch.logsumexp(s, -1)


def _heads_inputs(rows, H, d, dp, seed, scale=1.0):
    """[rows, H*dp] bf16 with each head's columns d..dp zero (the padded-head storage)"""
    x = torch.zeros(rows, H, dp, dtype=BF)
    x[..., :d] = bfr(rows, H, d, seed=seed, scale=scale)
    return x.reshape(rows, H * dp)


def attn_bwd_raw(q, ldq, k, ldk, v, ldv, o, do, lse, dq, lddq, dk, lddk, dv, lddv, B, H, Sq, Skv, scale, nd, prescaled,
                 accum=0, scratch=None):
    delta = torch.empty(2, B, H, Sq, device="cuda")
    fn = L().pea_op_attention_bwd_prescaled if prescaled else L().pea_op_attention_bwd
    call(fn(vp(q), ldq, vp(k), ldk, vp(v), ldv, vp(o), o.stride(0), vp(do), do.stride(0), vp(lse), vp(delta), vp(dq), lddq, vp(dk),
            lddk, vp(dv), lddv, B, H, Sq, Skv, scale, accum, accum, nd, vp(scratch), stream()))


def _scratch(B, H, Sq, Skv, nd):
    nb = L().pea_op_attention_bwd_scratch_bytes(B, H, Sq, Skv, nd)
    return torch.empty(nb, device="cuda", dtype=torch.uint8) if nb else None


# (B, H, tokens, head_dim d, prescaled): SDXL 10 / 20 heads of 64 at bucket token counts (14x28, 14x26, 18x22, 28x56, 36x44,
# 28x52); SD1.5 heads of 80 / 160 stored padded to 128 / 192 columns (nd 2 / 3)
SELF_CASES = [(1, 10, 1584, 64, True), (1, 10, 1456, 64, False), (2, 20, 392, 64, True), (1, 20, 364, 64, False),
              (1, 20, 396, 64, True), (1, 10, 1568, 64, True), (1, 8, 1456, 80, True), (1, 8, 364, 160, False)]


@pytest.mark.parametrize("B,H,S,d,prescaled", SELF_CASES)
def test_self_attention_fused_qkv_layout(ops, B, H, S, d, prescaled):
    """Self-attention as the UNet runs it: Q, K and V are the three column blocks of one [B*S, 3C] buffer (ld 3C, offsets C
    and 2C); dQ, dK and dV go to the three blocks of one [B*S, 3C] gradient buffer (here with pad columns and slack rows as
    canary), plain and accumulate-into; a dQ-only and a dK/dV-only call leave the other blocks untouched"""
    dp = (d + 63) // 64 * 64
    nd, C, scale = dp // 64, H * dp, d ** -0.5
    alpha = scale * math.log2(math.e)
    rows = B * S
    q = _heads_inputs(rows, H, d, dp, 1, alpha if prescaled else 1.0)
    k, v, do = _heads_inputs(rows, H, d, dp, 2), _heads_inputs(rows, H, d, dp, 3), _heads_inputs(rows, H, d, dp, 4)
    qr = (q.float() / alpha if prescaled else q.float()).view(B, S, C).requires_grad_(True)
    kr, vr = [t.float().view(B, S, C).requires_grad_(True) for t in (k, v)]
    oref, lref = attn_ref(qr, kr, vr, H, dp, scale)
    oref.backward(do.float().view(B, S, C))
    grads = [t.grad.reshape(rows, C) for t in (qr, kr, vr)]
    qkv = torch.cat([q, k, v], 1).cuda()
    Q, K, V = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    tag = f"self-attn B{B} H{H} S{S} d{d} pre{int(prescaled)}"
    oc = Canvas(rows, C + 32, [(16, C)])
    lse = torch.empty(B, H, S, device="cuda")
    fn = L().pea_op_attention_fwd_prescaled if prescaled else L().pea_op_attention_fwd
    call(fn(vp(Q), 3 * C, vp(K), 3 * C, vp(V), 3 * C, vp(oc.win()), oc.ld, vp(lse), B, H, S, S, scale, nd, stream()))
    oc.check(tag + " O")
    close_bf16(tag + " O", oc.win(), oref.reshape(rows, C), ulps=2.0)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)
    o0, lse0 = ops.attention_fwd(Q.contiguous().view(B, S, C), K.contiguous().view(B, S, C), V.contiguous().view(B, S, C), H,
                                 scale=scale, q_prescaled=prescaled)
    bits_equal(tag + " O strided vs contiguous", oc.win(), o0.view(rows, C))
    bits_equal(tag + " lse strided vs contiguous", lse, lse0)
    O = oc.win().contiguous()
    dod = do.cuda()
    ld = 3 * C + 64
    blocks = [(0, C), (C, C), (2 * C, C)]
    g = Canvas(rows, ld, blocks)
    attn_bwd_raw(Q, 3 * C, K, 3 * C, V, 3 * C, O, dod, lse, g.win(0), ld, g.win(1), ld, g.win(2), ld, B, H, S, S, scale, nd,
                 prescaled, scratch=_scratch(B, H, S, S, nd))
    g.check(tag + " dQ|dK|dV")
    for name, got, r in zip(("dQ", "dK", "dV"), (g.win(0), g.win(1), g.win(2)), grads):
        close_bf16(f"{tag} {name}", got, r, ulps=4.0)
    c0 = ops.attention_bwd(Q.contiguous().view(B, S, C), K.contiguous().view(B, S, C), V.contiguous().view(B, S, C), O.view(B, S, C),
                           dod.view(B, S, C), lse, H, scale=scale, q_prescaled=prescaled)
    for name, got, r in zip(("dQ", "dK", "dV"), (g.win(0), g.win(1), g.win(2)), c0):
        bits_equal(f"{tag} {name} strided vs contiguous", got, r.view(rows, C))
    # accumulate-into: the blocks already hold another consumer's share
    x0 = [bfr(rows, C, seed=20 + i).cuda() for i in range(3)]
    ga = Canvas(rows, ld, blocks)
    for i in range(3):
        ga.win(i).copy_(x0[i])
    attn_bwd_raw(Q, 3 * C, K, 3 * C, V, 3 * C, O, dod, lse, ga.win(0), ld, ga.win(1), ld, ga.win(2), ld, B, H, S, S, scale, nd,
                 prescaled, accum=1, scratch=_scratch(B, H, S, S, nd))
    ga.check(tag + " accumulate")
    for i, name in enumerate(("dQ", "dK", "dV")):
        close_bf16(f"{tag} {name} accumulate", ga.win(i), x0[i].float() + grads[i].cuda(), ulps=4.0)
    # one gradient at a time: the other column blocks stay sentinel
    gq = Canvas(rows, ld, [(0, C)])
    attn_bwd_raw(Q, 3 * C, K, 3 * C, V, 3 * C, O, dod, lse, gq.win(), ld, None, ld, None, ld, B, H, S, S, scale, nd, prescaled)
    gq.check(tag + " dQ only")
    close_bf16(f"{tag} dQ only", gq.win(), grads[0], ulps=4.0)
    gkv = Canvas(rows, ld, [(C, C), (2 * C, C)])
    attn_bwd_raw(Q, 3 * C, K, 3 * C, V, 3 * C, O, dod, lse, None, ld, gkv.win(0), ld, gkv.win(1), ld, B, H, S, S, scale, nd,
                 prescaled)
    gkv.check(tag + " dK|dV only")
    close_bf16(f"{tag} dK only", gkv.win(0), grads[1], ulps=4.0)
    close_bf16(f"{tag} dV only", gkv.win(1), grads[2], ulps=4.0)


# (B, H, Sq, d, prescaled); Skv = 77 keys of the stacked K|V buffer
CROSS_CASES = [(1, 10, 1584, 64, True), (1, 10, 1456, 64, False), (2, 20, 392, 64, True), (1, 20, 364, 64, False),
               (1, 20, 396, 64, True), (1, 10, 1568, 64, False), (1, 8, 1456, 80, True), (1, 8, 364, 160, False)]


@pytest.mark.parametrize("B,H,Sq,d,prescaled", CROSS_CASES)
def test_cross_attention_stacked_kv_layout(ops, B, H, Sq, d, prescaled):
    """Cross-attention as the UNet runs it: K and V are column slices at a deep offset of the stacked K|V projection of every
    cross-attention layer (SDXL: 166 400 columns; SD1.5 stack for the padded heads), dK / dV go back into the same layout;
    every pea_debug_set_xattn_bwd_v2 form that applies to 77 keys, with and without the query-split scratch, plain and
    accumulate-into; bitwise equal to the contiguous call of the same form"""
    from pea_diffusion_amd import config as pc
    Skv = 77
    dp = (d + 63) // 64 * 64
    nd, C, scale = dp // 64, H * dp, d ** -0.5
    alpha = scale * math.log2(math.e)
    offs, KVW = kv_stack(pc.sdxl_config() if d == 64 else pc.sd15_config())
    kvo = [o for o, cp in offs if cp == C][-1]
    rows, krows = B * Sq, B * Skv
    q = _heads_inputs(rows, H, d, dp, 11, alpha if prescaled else 1.0)
    k, v = _heads_inputs(krows, H, d, dp, 12), _heads_inputs(krows, H, d, dp, 13)
    do = _heads_inputs(rows, H, d, dp, 14)
    qr = (q.float() / alpha if prescaled else q.float()).view(B, Sq, C).requires_grad_(True)
    kr, vr = [t.float().view(B, Skv, C).requires_grad_(True) for t in (k, v)]
    oref, lref = attn_ref(qr, kr, vr, H, dp, scale)
    oref.backward(do.float().view(B, Sq, C))
    grads = [t.grad.reshape(-1, C).cuda() for t in (qr, kr, vr)]
    kvall = torch.zeros(krows, KVW, device="cuda", dtype=BF)
    K, V = kvall[:, kvo:kvo + C], kvall[:, kvo + C:kvo + 2 * C]
    K.copy_(k.cuda())
    V.copy_(v.cuda())
    Q, dod = q.cuda(), do.cuda()
    tag = f"xattn B{B} H{H} Sq{Sq} d{d} pre{int(prescaled)} kv@{kvo}/{KVW}"
    oc = Canvas(rows, C, [(0, C)])
    lse = torch.empty(B, H, Sq, device="cuda")
    fn = L().pea_op_attention_fwd_prescaled if prescaled else L().pea_op_attention_fwd
    call(fn(vp(Q), C, vp(K), KVW, vp(V), KVW, vp(oc.win()), C, vp(lse), B, H, Sq, Skv, scale, nd, stream()))
    oc.check(tag + " O")
    close_bf16(tag + " O", oc.win(), oref.reshape(rows, C), ulps=2.0)
    close_f32(tag + " lse", lse, lref, rtol=1e-3, atol=2e-3)
    Kc, Vc = k.cuda().view(B, Skv, C), v.cuda().view(B, Skv, C)
    o0, _ = ops.attention_fwd(Q.view(B, Sq, C), Kc, Vc, H, scale=scale, q_prescaled=prescaled)
    bits_equal(tag + " O strided vs contiguous", oc.win(), o0.view(rows, C))
    O = oc.win().contiguous()
    forms = (3, 2, 0) if nd == 1 else (3,)
    try:
        for ver in forms:
            L().pea_debug_set_xattn_bwd_v2(ver)
            for use_scratch in (True, False):
                scr = _scratch(B, H, Sq, Skv, nd) if use_scratch else None
                if use_scratch and scr is None:
                    continue                          # (no query split at this size: the same launch as without)
                t2 = f"{tag} v{ver} scratch{int(scr is not None)}"
                dq = Canvas(rows, C + 16, [(8, C)])
                dkv = Canvas(krows, KVW, [(kvo, C), (kvo + C, C)], r0=0, slack=1)
                attn_bwd_raw(Q, C, K, KVW, V, KVW, O, dod, lse, dq.win(), dq.ld, dkv.win(0), KVW, dkv.win(1), KVW, B, H, Sq, Skv,
                             scale, nd, prescaled, scratch=scr)
                dq.check(t2 + " dQ")
                dkv.check(t2 + " dK|dV")
                for name, got, r in zip(("dQ", "dK", "dV"), (dq.win(), dkv.win(0), dkv.win(1)), grads):
                    close_bf16(f"{t2} {name}", got, r, ulps=4.0)
                # the contiguous call of the same form
                cq, ck, cvv = (torch.empty(rows, C, device="cuda", dtype=BF), torch.empty(krows, C, device="cuda", dtype=BF),
                               torch.empty(krows, C, device="cuda", dtype=BF))
                attn_bwd_raw(Q, C, Kc, C, Vc, C, O, dod, lse, cq, C, ck, C, cvv, C, B, H, Sq, Skv, scale, nd, prescaled,
                             scratch=_scratch(B, H, Sq, Skv, nd) if scr is not None else None)
                for name, got, r in zip(("dQ", "dK", "dV"), (dq.win(), dkv.win(0), dkv.win(1)), (cq, ck, cvv)):
                    bits_equal(f"{t2} {name} strided vs contiguous", got, r)
                # accumulate-into (dQ and the K|V gradient stack already hold other shares)
                x0 = [bfr(rows, C, seed=30).cuda(), bfr(krows, C, seed=31).cuda(), bfr(krows, C, seed=32).cuda()]
                dq.win().copy_(x0[0])
                dkv.win(0).copy_(x0[1])
                dkv.win(1).copy_(x0[2])
                attn_bwd_raw(Q, C, K, KVW, V, KVW, O, dod, lse, dq.win(), dq.ld, dkv.win(0), KVW, dkv.win(1), KVW, B, H, Sq, Skv,
                             scale, nd, prescaled, accum=1, scratch=scr)
                dq.check(t2 + " dQ accumulate")
                dkv.check(t2 + " dK|dV accumulate")
                for x, name, got, r in zip(x0, ("dQ", "dK", "dV"), (dq.win(), dkv.win(0), dkv.win(1)), grads):
                    close_bf16(f"{t2} {name} accumulate", got, x.float() + r, ulps=4.0)
    finally:
        L().pea_debug_set_xattn_bwd_v2(3)


# ------------------------------------------------------------------------------------ conv geometry
def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def conv_raw(x, wp, B, Hs, Ws, Cin, Cout, stride=1, ups=False, tr2=False, bias=None, rowvec=None, res=None):
    """pea_op_conv3x3 into a canvas: the output rows at an offset inside a buffer with slack rows on both sides"""
    sh = 1 if (ups or tr2) else 0
    Hv, Wv = Hs << sh, Ws << sh
    Ho, Wo = ((Hv + 1) // 2, (Wv + 1) // 2) if stride == 2 else (Hv, Wv)
    cv = Canvas(B * Ho * Wo, Cout, [(0, Cout)], r0=2, slack=3)
    call(L().pea_op_conv3x3(vp(x), vp(wp), vp(cv.win()), B, Hs, Ws, Cin, Cout, stride, int(ups), int(tr2), vp(bias), vp(rowvec),
                            rowvec.stride(0) if rowvec is not None else 0, vp(res), stream()))
    return cv, (B, Ho, Wo, Cout)


# (B, Hs, Ws, Cin, Cout, stride, upsample2x): latents of the 448x896 (56x112 -> 28x56 -> 14x28), 576x704 (72x88 -> 36x44 ->
# 18x22) and 832x448 (104x56 -> 52x28 -> 26x14) buckets at SDXL widths, the up path's concatenated inputs, both kinds of
# resampling, and one odd-sized image
CONV_FWD = [(1, 56, 112, 320, 320, 1, False), (2, 36, 44, 640, 640, 1, False), (1, 26, 14, 1280, 1280, 1, False),
            (1, 28, 56, 960, 640, 1, False), (1, 14, 28, 2560, 1280, 1, False), (1, 18, 22, 1920, 1280, 1, False),
            (1, 56, 112, 320, 320, 2, False), (2, 52, 28, 640, 640, 2, False), (1, 36, 44, 640, 640, 2, False),
            (1, 9, 11, 1280, 1280, 1, True), (1, 26, 14, 640, 640, 1, True), (2, 13, 19, 320, 320, 1, False),
            (2, 13, 19, 320, 320, 2, False)]
CONV_SWEEP = [0, 2, 7, 9, 12]          # the subset of CONV_FWD run under every variant: wide, tall, s2, upsample, odd


def _conv_case(case, seed):
    B, Hs, Ws, Cin, Cout, stride, ups = case
    g = torch.Generator().manual_seed(seed)
    x = bfr(B, Cin, Hs, Ws, seed=seed)
    wq = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(BF).float()
    bias = torch.randn(Cout, generator=g)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if ups else x.float()
    ref = _nhwc(F.conv2d(xin, wq, bias, stride=stride, padding=1))
    return x, wq, bias, ref


@pytest.mark.parametrize("variant", [-1] + CONV_VARIANTS, ids=lambda v: "default" if v < 0 else f"v{v}")
def test_conv_bucket_geometry(ops, variant):
    """conv3x3 forward (stride 1, stride-2 downsample, folded nearest-2x upsample) on non-square bucket latents at full channel
    widths; B = 2 cases put row tiles across samples; the default choice runs every shape, each variant the sweep subset"""
    cases = range(len(CONV_FWD)) if variant < 0 else CONV_SWEEP
    try:
        for i in cases:
            case = CONV_FWD[i]
            B, Hs, Ws, Cin, Cout, stride, ups = case
            x, wq, bias, ref = _conv_case(case, 10 + i)
            wp = ops.pack_conv(wq.cuda())
            L().pea_debug_set_gemm_variant(variant)
            cv, shape = conv_raw(_nhwc(x).cuda(), wp, B, Hs, Ws, Cin, Cout, stride, ups, bias=bias.cuda())
            tag = f"v{variant} conv B{B} {Hs}x{Ws} {Cin}->{Cout} s{stride} ups{int(ups)}"
            cv.check(tag)
            close_bf16(tag, cv.win().view(shape), ref)
    finally:
        L().pea_debug_set_gemm_variant(-1)


@pytest.mark.parametrize("variant", [-1] + CONV_VARIANTS, ids=lambda v: "default" if v < 0 else f"v{v}")
def test_conv_bucket_epilogue_and_dgrad(ops, variant):
    """the resnet's temb row vector + residual epilogue, and the three data-gradient forms (plain, zero-stuffed transposed
    conv of a stride-2 conv, dgrad at the upsampled resolution then sumpool2) on non-square latents"""
    try:
        # temb + res: B = 2 (one row vector per sample, a sample boundary inside row tiles)
        for (B, Hs, Ws, C) in ([(2, 18, 22, 640), (1, 104, 56, 320)] if variant < 0 else [(2, 18, 22, 640)]):
            x, wq, bias, _ = _conv_case((B, Hs, Ws, C, C, 1, False), 40 + Hs)
            temb, res = bfr(B, C, seed=4), bfr(B, Hs, Ws, C, seed=5)
            ref = F.conv2d(x.float(), wq, bias, padding=1) + temb.float()[:, :, None, None] + res.float().permute(0, 3, 1, 2)
            wp = ops.pack_conv(wq.cuda())
            L().pea_debug_set_gemm_variant(variant)
            cv, shape = conv_raw(_nhwc(x).cuda(), wp, B, Hs, Ws, C, C, bias=bias.cuda(), rowvec=temb.cuda(), res=res.cuda())
            tag = f"v{variant} conv+temb+res B{B} {Hs}x{Ws} C{C}"
            cv.check(tag)
            close_bf16(tag, cv.win().view(shape), _nhwc(ref))
            L().pea_debug_set_gemm_variant(-1)
        # dgrad: (B, Hs, Ws, Cin, Cout, stride, ups) of the FORWARD conv
        dg = [(1, 28, 56, 640, 640, 1, False), (1, 26, 14, 1920, 1280, 1, False), (1, 56, 112, 320, 320, 2, False),
              (2, 52, 28, 640, 640, 2, False), (1, 14, 28, 640, 640, 1, True), (1, 13, 19, 320, 320, 2, False)]
        for i, (B, Hs, Ws, Cin, Cout, stride, ups) in enumerate(dg if variant < 0 else [dg[0], dg[3], dg[4]]):
            g = torch.Generator().manual_seed(60 + i)
            x = bfr(B, Cin, Hs, Ws, seed=60 + i).float().requires_grad_(True)
            wq = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(BF).float()
            xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
            y = F.conv2d(xin, wq, None, stride=stride, padding=1)
            dy = bfr(*y.shape, seed=70 + i)
            y.backward(dy.float())
            wd = ops.pack_conv(wq.cuda(), dgrad=True)
            _, _, Ho, Wo = y.shape
            tag = f"v{variant} dgrad B{B} {Hs}x{Ws} {Cin}->{Cout} s{stride} ups{int(ups)}"
            L().pea_debug_set_gemm_variant(variant)
            if stride == 2:
                cv, shape = conv_raw(_nhwc(dy).cuda(), wd, B, Ho, Wo, Cout, Cin, tr2=True)
                if shape[1:3] != (Hs, Ws):                # odd input: the transposed form yields 2*Ho x 2*Wo, crop it
                    got = cv.win().view(shape)[:, :Hs, :Ws]
                else:
                    got = cv.win().view(shape)
            else:
                cv, shape = conv_raw(_nhwc(dy).cuda(), wd, B, Ho, Wo, Cout, Cin)
                got = cv.win().view(shape)
                if ups:
                    got = ops.sumpool2(got.contiguous())
            cv.check(tag)
            close_bf16(tag, got, _nhwc(x.grad), ulps=2.0)
            L().pea_debug_set_gemm_variant(-1)
    finally:
        L().pea_debug_set_gemm_variant(-1)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 26, 14, 640, 640), (2, 9, 11, 640, 640), (1, 13, 7, 1280, 1280)])
def test_upconv_subpixel_buckets(ops, B, H, W, Cin, Cout):
    """the sub-pixel upsampler (four 2 x 2 kernels, depth-to-space output) and its data gradient on non-square latents; the
    bounds of test_upconv_subpixel_fwd_dgrad (they carry the merged taps' weight rounding)"""
    x = bfr(B, Cin, H, W, seed=1).float().requires_grad_(True)
    wq = (torch.randn(Cout, Cin, 3, 3, generator=torch.Generator().manual_seed(2)) * (9 * Cin) ** -0.5).to(BF).float()
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(3))
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wq, bias, padding=1)
    dy = bfr(*ref.shape, seed=7)
    ref.backward(dy.float())
    y = ops.upconv_subpixel(_nhwc(x.detach().to(BF)).cuda(), ops.pack_conv_subpixel(wq.cuda()), bias=bias.cuda())
    e = rel_l2(ops.d2s_to_nhwc(y), _nhwc(ref.detach()))
    res = bfr(B, H, W, Cin, seed=9)
    dx = ops.upconv_subpixel_dgrad(ops.nhwc_to_d2s(_nhwc(dy).cuda()), ops.pack_conv_subpixel(wq.cuda(), dgrad=True), res=res.cuda())
    e2 = rel_l2(dx, _nhwc(x.grad) + res.float())
    y3 = ops.conv3x3(_nhwc(x.detach().to(BF)).cuda(), ops.pack_conv(wq.cuda()), bias=bias.cuda(), upsample2x=True)
    e3 = rel_l2(ops.d2s_to_nhwc(y), y3)
    print(f"[upconv subpixel B{B} {H}x{W} {Cin}->{Cout}] fwd rel_l2={e:.2e} dgrad rel_l2={e2:.2e} vs 3x3 form {e3:.2e}")
    assert e < 4e-3 and e2 < 5e-3 and e3 < 5e-3


@pytest.mark.parametrize("H,W", [(56, 112), (104, 56)])
def test_conv_in_out_buckets(ops, H, W):
    """the UNet's 4-channel ends at a wide and a tall bucket latent: conv_in (4 -> 320), conv_out (320 -> 4) and its dgrad"""
    g = torch.Generator().manual_seed(H)
    x = torch.randn(1, 4, H, W, generator=g)
    w_in, b_in = torch.randn(320, 4, 3, 3, generator=g) * 0.2, torch.randn(320, generator=g)
    close_bf16(f"conv_in {H}x{W}", ops.conv_in(x.cuda(), w_in.cuda(), b_in.cuda()), _nhwc(F.conv2d(x, w_in, b_in, padding=1)))
    h = (torch.randn(1, 320, H, W, generator=g) * 1.5).to(BF)
    w_out = torch.randn(4, 320, 3, 3, generator=g) * (1.0 / (3.0 * 320 ** 0.5))
    b_out = torch.randn(4, generator=g)
    wp = ops.pack_conv_out(w_out.cuda())
    close_f32(f"conv_out {H}x{W}", ops.conv_out(_nhwc(h).cuda(), wp, b_out.cuda()), F.conv2d(h.float(), w_out, b_out, padding=1))
    hh = torch.zeros(1, 320, H, W, requires_grad=True)
    dy = torch.randn(1, 4, H, W, generator=g)
    F.conv2d(hh, w_out, None, padding=1).backward(dy)
    close_bf16(f"conv_out dgrad {H}x{W}", ops.conv_out_dgrad(dy.cuda(), wp, 320), _nhwc(hh.grad))


# ------------------------------------------------------------------------------------ norms
def _groupnorm_case(ops, B, HW, C, silu):
    x = (bfr(B, HW, C, seed=1).float() * 1.5 + 0.7).to(BF)
    g = torch.Generator().manual_seed(2)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    xr = x.float().requires_grad_(True)
    z = F.group_norm(xr.permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    yr = F.silu(z) if silu else z
    y, stats = ops.groupnorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), 32, 1e-5, silu)
    close_bf16(f"groupnorm fwd B{B} HW{HW} C{C} silu{silu}", y, yr)
    mean_ref = x.float().reshape(B, HW, 32, C // 32).mean(dim=(1, 3))
    var_ref = x.float().reshape(B, HW, 32, C // 32).var(dim=(1, 3), unbiased=False)
    st = stats.cpu().reshape(B, 32, 2)
    assert torch.allclose(st[..., 0], mean_ref, rtol=1e-4, atol=1e-5), "groupnorm: saved mean"
    assert torch.allclose(st[..., 1], (var_ref + 1e-5).rsqrt(), rtol=1e-4, atol=1e-5), "groupnorm: saved rstd"
    dy = bfr(B, HW, C, seed=3)
    yr.backward(dy.float())
    dx = ops.groupnorm_bwd(x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda(), stats, 32, silu)
    close_bf16(f"groupnorm bwd B{B} HW{HW} C{C} silu{silu}", dx, xr.grad, ulps=2.0)
    prev = bfr(B, HW, C, seed=4)
    acc = prev.cuda().clone()
    ops.groupnorm_bwd(x.cuda(), dy.cuda(), gamma.cuda(), beta.cuda(), stats, 32, silu, accum_into=acc)
    close_bf16(f"groupnorm bwd accumulate B{B} HW{HW} C{C}", acc, xr.grad + prev.float(), ulps=2.0)


# bucket pixel counts (14x26, 18x22, 14x28, 36x44, 72x88, 28x52) at the UNet's widths, the up path's concatenations included
@pytest.mark.parametrize("B,HW,C,silu", [(1, 364, 1280, True), (2, 396, 2560, True), (1, 392, 1920, False), (2, 1584, 640, True),
                                         (1, 6336, 320, True), (1, 1584, 960, False), (2, 1456, 640, True), (1, 392, 2560, False),
                                         (1, 364, 320, True), (1, 6336, 640, False)])
def test_groupnorm_buckets(ops, B, HW, C, silu):
    _groupnorm_case(ops, B, HW, C, silu)


# VAE widths: 4 / 8 / 16 channels per group; one large image on the three-launch path
@pytest.mark.parametrize("B,HW,C,silu", [(1, 4096, 128, True), (2, 1024, 128, False), (1, 16384, 256, True), (1, 1024, 256, False),
                                         (1, 4096, 512, True), (2, 576, 512, False), (1, 256 * 256, 128, True)])
def test_groupnorm_vae_widths(ops, B, HW, C, silu):
    _groupnorm_case(ops, B, HW, C, silu)


@pytest.mark.parametrize("R,C", [(784, 640), (1584, 640), (2912, 640), (364, 1280), (792, 1280), (1456, 1280)])
def test_layernorm_buckets(ops, R, C):
    """LayerNorm at the transformer widths with bucket row counts (B x tokens)"""
    x = (bfr(R, C, seed=1).float() * 2 - 0.5).to(BF)
    g = torch.Generator().manual_seed(2)
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, generator=g)).requires_grad_(True)
    xr = x.float().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), gamma, beta, 1e-5)
    y, stats = ops.layernorm_fwd(x.cuda(), gamma.detach().cuda(), beta.detach().cuda())
    close_bf16(f"layernorm fwd {R}x{C}", y, yr)
    dy = bfr(R, C, seed=3)
    yr.backward(dy.float())
    dx, dg, db = ops.layernorm_bwd(x.cuda(), dy.cuda(), gamma.detach().cuda(), stats, want_param_grads=True)
    close_bf16(f"layernorm bwd {R}x{C}", dx, xr.grad, ulps=2.0)
    close_f32("layernorm dgamma", dg, gamma.grad, rtol=2e-3, atol=2e-3)
    close_f32("layernorm dbeta", db, beta.grad, rtol=2e-3, atol=2e-3)


# ------------------------------------------------------------------------------------ model-level edge
def test_training_context_refuses_token_counts_the_backward_cannot_take(ops):
    """an SD1.5-shaped UNet at a 56 x 104 latent has a 7 x 13 = 91-token mid block; the attention backward needs multiples of
    4, so a training context is refused when it is created (not in its first backward); an inference context is fine"""
    from pea_diffusion_amd import config as pc
    from pea_diffusion_amd._lib import PeaError
    from pea_diffusion_amd.unet import HipUNet
    with pytest.raises(PeaError, match="91 tokens"):
        HipUNet(pc.tiny15_config(), 1, 56, 104, 12, needs_grad=True)
    u = HipUNet(pc.tiny15_config(), 1, 56, 104, 12, needs_grad=False)
    del u


# ------------------------------------------------------------------------------------ child processes
def _child(env_extra, select):
    import subprocess
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", select],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_child_gemm_layouts_on_the_slow_epilogue(ops):
    """PEA_GEMM_SLOW_EPILOGUE=1 takes the batched-load epilogue away from every launch: the default-choice layout cases again"""
    _child({"PEA_GEMM_SLOW_EPILOGUE": "1"}, "test_gemm_layouts and default")


def test_child_layouts_on_a_smaller_device(ops):
    """tile rules and persistent grids follow the CU count (PEA_CU_LIMIT): the GEMM and conv layout cases limited to 40 CUs"""
    _child({"PEA_CU_LIMIT": "40"}, "(test_gemm_layouts or test_gemm_geglu or test_ln_linear_offsets or test_conv_bucket_geometry "
                                   "or test_conv_bucket_epilogue_and_dgrad) and default")


def test_child_groupnorm_buckets_three_launch_path(ops):
    """PEA_GN_UNFUSED=1: the bucket shapes on the three-launch path (the one-kernel forms take them by default)"""
    _child({"PEA_GN_UNFUSED": "1"}, "test_groupnorm_buckets")
