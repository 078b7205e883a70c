"""Kernel-level parity (-m gpu) of the GEMM / implicit-GEMM conv forms that only the model tape fills -- GemmP fields no older
pea_op_* entry can set: split-K partials (the stacked K|V projection's backward), the quick-GELU activation (CLIP towers), the
tanh-form GEGLU (T5 v1.1), the asymmetric-padding stride-2 conv (VAE encoder downsampler), convs with an activation on
channel-padded layouts (ControlNet conditioning embedding) and the next-op weight prefetch -- each through its thin entry
(pea_op_gemm_splitk, pea_op_gemm_geglu_tanh, pea_op_conv3x3_ex, pea_op_pack_conv_padded, pea_debug_set_gemm_prefetch) against a
float64 reference of the same operation on the same bf16-rounded inputs, rounded once where the kernel stores.

Tolerances are those tests/test_ops_gpu.py states (close_bf16 / close_f32 are imported from there), none is fitted to a result:
  * fp32 split-K partials: close_f32 defaults (rtol 1e-3, atol 1e-4), meant at unit scale: W carries K^-0.5, so the FULL product
    has unit scale and every partial is smaller.  An empty split's tile is exact zeros.  The reduced bf16 result: close_bf16, 1 ulp.
  * bf16-stored forward results (quick-GELU, both conv groups): close_bf16 at 1 ulp.
  * tanh GEGLU: the budgets test_gemm_geglu_forward_and_stash_forms states for the erf form -- y and the stash at 2 ulps (two
    rounded factors enter y).
  * prefetch, repeated runs, layouts of the same launch: the bits.
close_bf16's absolute term scales with the root-mean-square of the reference it is handed, so rows / columns planted far out
(pre-activations near +-60, gates at +-12 and +-40) are compared on their own and never widen the budget of the ordinary ones.
Every strided or partial output starts as sentinels, and everything outside the specified region must still carry them.  Each
case prints its worst error (close_bf16 / close_f32 print max_abs and rel_l2)."""
import ctypes
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
from glue_ref import bfr, bits, gelu64, rnd, same_bits, sentinel, untouched  # noqa: E402
from test_layouts_gpu import CONV_VARIANTS  # noqa: E402
from test_ops_gpu import close_bf16, close_f32, ops  # noqa: E402,F401

BF = torch.bfloat16


def L():
    from pea_diffusion_amd._lib import lib
    return lib()


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


def ceil64(n):
    return (n + 63) // 64 * 64


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_tanh64(g):
    return 0.5 * g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (g + 0.044715 * g ** 3)))


def silu64(x):
    return x * torch.sigmoid(x)


# ------------------------------------------------------------------------------------ split-K partials
# M, N, K-steps (K = 64 x steps), ksplit, alpha.  A split owns per = ceil(steps / ksplit) K-steps from s * per on, or what is left:
SPLITK = [(154, 136, 8, 2, 1.0),        # even split, ragged M and N
          (154, 136, 10, 4, 0.5),       # steps 3, 3, 3, 1
          (154, 136, 9, 4, 1.0),        # steps 3, 3, 3, 0: an empty last split (loader and consumers meet at the prologue barrier only)
          (77, 2048, 1, 2, 1.0),        # one step, empty second split, many n-tiles
          (308, 768, 40, 3, 1.0),       # steps 14, 14, 12: deeper than the kernel's 4-stage LDS ring
          (130, 132, 64, 32, 1.0)]      # the tape's cap of 32 splits


@pytest.mark.parametrize("M,N,steps,ksplit,alpha", SPLITK, ids=[f"{m}x{n}-{s}steps-{k}splits" for m, n, s, k, _ in SPLITK])
def test_splitk_partials(ops, M, N, steps, ksplit, alpha):
    K = 64 * steps
    a, w = bfr(M, K, seed=M + steps), bfr(N, K, seed=N + ksplit, scale=K ** -0.5)
    ad, wd = a.cuda(), w.cuda()
    a64, w64 = a.double(), w.double()
    ldc = N + 4
    stride = M * ldc + 8
    per = -(-steps // ksplit)
    tag = f"splitk {M}x{N}x{K}/{ksplit}"
    part = sentinel(ksplit * stride + 8, torch.float32)
    ops.gemm_splitk(ad, wd, ksplit, part, ldc, stride, alpha=alpha)
    for s in range(ksplit):
        k0, k1 = min(s * per, steps) * 64, min((s + 1) * per, steps) * 64
        tile = part[s * stride:s * stride + M * ldc].view(M, ldc)
        ref = alpha * (a64[:, k0:k1] @ w64[:, k0:k1].T)                 # (an empty K range gives zeros)
        close_f32(f"{tag} partial {s} (K-steps {k0 // 64}..{k1 // 64})", tile[:, :N], ref)
        if k0 == k1:
            assert bool((tile[:, :N] == 0).all()), f"{tag}: the empty split {s} did not store zeros"
        assert untouched(tile[:, N:]), f"{tag}: partial {s} wrote between its rows"
        assert untouched(part[s * stride + M * ldc:(s + 1) * stride]), f"{tag}: partial {s} wrote behind its last row"
    assert untouched(part[ksplit * stride:])
    again = sentinel(ksplit * stride + 8, torch.float32)
    ops.gemm_splitk(ad, wd, ksplit, again, ldc, stride, alpha=alpha)
    assert same_bits(part, again), f"{tag}: a second run gives other bits"
    # the reduce reads rows N apart (the tape's layout: ldc = N, split_stride = M N): the same launch on that layout gives the
    # same bits, and those go through the reduce
    dense = sentinel(ksplit * M * N + 8, torch.float32)
    ops.gemm_splitk(ad, wd, ksplit, dense, N, M * N, alpha=alpha)
    assert untouched(dense[ksplit * M * N:])
    for s in range(ksplit):
        assert same_bits(dense[s * M * N:(s + 1) * M * N].view(M, N), part[s * stride:s * stride + M * ldc].view(M, ldc)[:, :N].contiguous()), \
            f"{tag}: partial {s} depends on the layout of the partials"
    full = alpha * (a64 @ w64.T)
    prev = bfr(M, N, seed=7)
    for accum in (0, 1):
        out = sentinel(M * N + 8)
        out[:M * N] = prev.cuda().reshape(-1)
        ops.splitk_reduce_(dense, ksplit, M * N, out, N, M, N, accum=bool(accum))
        close_bf16(f"{tag} reduced accum={accum}", out[:M * N].view(M, N), rnd(full + accum * prev.double()))
        assert untouched(out[M * N:])


# ------------------------------------------------------------------------------------ quick-GELU (act 3)
@pytest.mark.parametrize("M,N", [(154, 264), (17, 1280)])          # N = 264 ends inside a 16-column tile
def test_quick_gelu_epilogue(ops, M, N):
    K = 128
    a32 = randn(M, K, seed=M) * 4.0
    a32[0] *= 15.0                                                  # two planted rows: pre-activations of sigma ~ 60, so that
    a32[1] *= -15.0                                                 # exp(-1.702 x) overflows on one side and vanishes on the other
    a, w = a32.to(BF), bfr(N, K, seed=2, scale=K ** -0.5)
    bias, res = randn(N, seed=3) * 2.0, bfr(M, N, seed=4)
    pre = a.double() @ w.double().T + bias.double()
    assert pre[2:].min() <= -12 and pre[2:].max() >= 12 and pre[:2].min() <= -60 and pre[:2].max() >= 60, "the inputs miss the tails"
    ref = quick_gelu64(pre)
    buf = sentinel(M * N + 8)
    out, got_pre = ops.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), act=3, res=res.cuda(), want_preact=True, out=buf[:M * N].view(M, N))
    tag = f"quick-gelu {M}x{N}x{K}"
    for name, rows in (("", slice(2, M)), (" planted rows", slice(0, 2))):
        close_bf16(f"{tag} + res{name}", out[rows], rnd(ref[rows] + res.double()[rows]))
        close_bf16(f"{tag} preact{name}", got_pre[rows], rnd(pre[rows]))
    assert untouched(buf[M * N:])
    plain = ops.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), act=3)                   # no residual: the tails themselves
    for name, rows in (("", slice(2, M)), (" planted rows", slice(0, 2))):
        close_bf16(f"{tag}{name}", plain[rows], rnd(ref[rows]))
    plain = plain.float().cpu()
    assert torch.isfinite(plain).all()
    far = pre <= -60.0                                              # 1.702 x < -88.7: exp overflows, the sigmoid is 0
    assert far.any() and bool((plain[far] == 0).all()), f"{tag}: the far negative tail is not +-0"
    silu = ops.gemm(a.cuda(), w.cuda(), bias=bias.cuda(), act=2)
    assert not torch.equal(silu.cpu(), plain.to(BF)), "act 3 gives what act 2 gives"


def test_quick_gelu_conv(ops):
    B, H, W, Cin, Cout = 2, 6, 10, 64, 64
    x = bfr(B, Cin, H, W, seed=1, scale=4.0)
    wq = (randn(Cout, Cin, 3, 3, seed=2) * (9 * Cin) ** -0.5).to(BF)
    bias = randn(Cout, seed=3)
    ref = quick_gelu64(F.conv2d(x.double(), wq.double(), bias.double(), padding=1))
    buf = sentinel(B * H * W * Cout + 8)
    ops.conv3x3_ex(nhwc(x).cuda(), ops.pack_conv(wq.float().cuda()), bias=bias.cuda(), act=3, out=buf)
    close_bf16("quick-gelu conv 2x6x10 64->64", buf[:-8].view(B, H, W, Cout), rnd(nhwc(ref)))
    assert untouched(buf[-8:])


# ------------------------------------------------------------------------------------ tanh-form GEGLU
GATES = (12.0, -12.0, 40.0, -40.0)     # exp2's argument in gelu_tanh overflows / vanishes: y saturates to h * gate and to +-0


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N", [336, 2560])                          # inner 168 ends inside a 160-column tile
def test_tanh_geglu(ops, N, with_bias):
    M, K, inner = 154, 128, N // 2
    a32, w32 = randn(M, K, seed=N), randn(N, K, seed=N + 1) * K ** -0.5
    a32[:, 0] = 1.0                                                 # column 0 of A is 1: W[n][0] acts as a bias that needs none
    cols = [3, inner // 2 + 1, inner - 2, inner - 1]                # planted gates, the last two in the ragged last tile
    bias = randn(N, seed=5) * 0.1 if with_bias else None
    for c, g in zip(cols, GATES):
        w32[2 * c + 1] = 0.0
        w32[2 * c + 1, 0] = g
        if with_bias:
            bias[2 * c + 1] = 0.0
    a, w = a32.to(BF), w32.to(BF)
    pre = a.double() @ w.double().T + (bias.double() if with_bias else 0.0)
    h, gate = pre[:, 0::2], pre[:, 1::2]
    assert all(bool((gate[:, c] == g).all()) for c, g in zip(cols, GATES))
    yref = h * gelu_tanh64(gate)
    rest = torch.ones(inner, dtype=torch.bool)
    rest[cols] = False
    rest2 = rest.repeat_interleave(2)                               # the same columns of the interleaved (h, gate) stash
    tag = f"tanh geglu {M}x{N}x{K} {'bias' if with_bias else 'no bias'}"
    bd = bias.cuda() if with_bias else None
    ys = []
    for mode, rows in (("no stash", None), ("stash", M), ("stash_rows=77", 77)):
        ybuf = sentinel(M * inner + 8)
        sbuf = sentinel(M * N + 8) if rows else None
        y, st = ops.gemm_geglu(a.cuda(), w.cuda(), bd, want_stash=False, stash_grad=False, stash_rows=0 if rows in (None, M) else rows,
                               tanh=True, y=ybuf[:M * inner].view(M, inner), stash=sbuf[:M * N].view(M, N) if rows else None)
        assert untouched(ybuf[M * inner:])
        yc = y.float().cpu()
        assert torch.isfinite(yc).all()
        close_bf16(f"{tag} y ({mode})", y[:, rest], rnd(yref[:, rest]), ulps=2.0)
        for c, g in zip(cols, GATES):
            if g > 0:                                               # saturated: exactly h * gate
                close_bf16(f"{tag} y gate {g:+.0f} ({mode})", y[:, c], rnd(h[:, c] * g), ulps=2.0)
            else:
                assert bool((yc[:, c] == 0).all()), f"{tag}: gate {g} does not give +-0"
        if rows:
            close_bf16(f"{tag} stash ({mode})", st[:rows][:, rest2], rnd(pre[:rows][:, rest2]), ulps=2.0)
            stc = st.float().cpu()
            for c, g in zip(cols, GATES):
                close_bf16(f"{tag} stash h at gate {g:+.0f} ({mode})", st[:rows, 2 * c], rnd(pre[:rows, 2 * c]), ulps=2.0)
                assert bool((stc[:rows, 2 * c + 1] == g).all())
            assert untouched(st[rows:]) and untouched(sbuf[M * N:]), f"{tag}: rows past the stash were written"
        ys.append(y)
    assert same_bits(ys[0], ys[1]) and same_bits(ys[0], ys[2]), f"{tag}: y depends on the stash"
    y_erf, _ = ops.gemm_geglu(a.cuda(), w.cuda(), bd, want_stash=False, stash_grad=False)
    close_bf16(f"{tag} erf form, same inputs", y_erf[:, rest], rnd((h * gelu64(gate))[:, rest]), ulps=2.0)
    assert not torch.equal(y_erf, ys[0]), f"{tag}: the tanh flag changes nothing"
    # the two gate forms differ by less than the 2-ulp budget (|gelu_new - gelu| <= 4.8e-4), so the budget alone cannot tell them
    # apart: where the two references round to different bf16 values, each result must side with its own.  (A right result
    # misses its own reference only where its fp32 error of ~1e-6 relative flips the bf16 rounding, a chance of ~1e-6 / 2^-8 per
    # element, while it misses the other form's reference at every one of these elements: a factor of 10 is far inside that.)
    t_ref, e_ref = rnd(yref[:, rest]).float(), rnd((h * gelu64(gate))[:, rest]).float()
    differ = t_ref != e_ref
    got_t, got_e = ys[0][:, rest].float().cpu()[differ], y_erf[:, rest].float().cpu()[differ]
    t_ref, e_ref = t_ref[differ], e_ref[differ]
    d_tt, d_te = (got_t - t_ref).abs().sum().item(), (got_t - e_ref).abs().sum().item()
    d_ee, d_et = (got_e - e_ref).abs().sum().item(), (got_e - t_ref).abs().sum().item()
    print(f"[{tag}] {int(differ.sum())} elements tell the forms apart: tanh result |.-tanh|={d_tt:.3e} |.-erf|={d_te:.3e}; "
          f"erf result |.-erf|={d_ee:.3e} |.-tanh|={d_et:.3e}")
    assert differ.sum() > 100 and d_tt < 0.1 * d_te and d_ee < 0.1 * d_et, f"{tag}: the result does not follow its own gate form"


# ------------------------------------------------------------------------------------ VAE encoder downsampler (pad_off = 1)
VAE_DOWN = [(1, 8, 12, 128, 128), (2, 6, 10, 64, 192), (1, 16, 4, 256, 256)]


@functools.lru_cache(maxsize=None)
def vae_down_case(B, H, W, Cin, Cout):
    """inputs and the float64 reference F.conv2d(F.pad(x, (0,1,0,1)), w, b, stride=2), computed once per shape"""
    x = bfr(B, Cin, H, W, seed=H + W)
    wq = (randn(Cout, Cin, 3, 3, seed=2) * (9 * Cin) ** -0.5).to(BF)
    bias = randn(Cout, seed=3)
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), wq.double(), bias.double(), stride=2)
    return nhwc(x), wq.float(), bias, rnd(nhwc(ref))


def run_vae_down(ops, shape, tag):
    B, H, W, Cin, Cout = shape
    x, wq, bias, ref = vae_down_case(*shape)
    Ho, Wo = H // 2, W // 2
    buf = sentinel(B * Ho * Wo * Cout + 8)
    wp = ops.pack_conv(wq.cuda())
    ops.conv3x3_ex(x.cuda(), wp, bias=bias.cuda(), stride=2, pad_off=1, out=buf)
    y = buf[:-8].view(B, Ho, Wo, Cout)
    assert tuple(ref.shape) == (B, Ho, Wo, Cout)
    close_bf16(f"{tag} {B}x{H}x{W} {Cin}->{Cout}", y, ref)
    assert untouched(buf[-8:])
    return y, ref


@pytest.mark.parametrize("shape", VAE_DOWN, ids=lambda s: "x".join(map(str, s)))
def test_vae_downsampler(ops, shape):
    run_vae_down(ops, shape, "vae down")


@pytest.mark.parametrize("variant", [-1] + CONV_VARIANTS, ids=lambda v: "default" if v < 0 else f"v{v}")
def test_vae_downsampler_every_variant(ops, variant):
    """the first shape under every kernel form; its rightmost column and bottom row are the outputs whose tap window reaches the
    zero padding, so a window one pixel off fails there by name"""
    try:
        L().pea_debug_set_gemm_variant(variant)
        y, ref = run_vae_down(ops, VAE_DOWN[0], f"vae down v{variant}")
        close_bf16(f"vae down v{variant} rightmost column", y[:, :, -1], ref[:, :, -1])
        close_bf16(f"vae down v{variant} bottom row", y[:, -1], ref[:, -1])
    finally:
        L().pea_debug_set_gemm_variant(-1)


# ------------------------------------------------------------------------------------ ControlNet conditioning convs
# real Cin -> Cout, stride, residual: SiLU in the epilogue, the input stored 64-padded, the output Cout wide in rows ceil64(Cout) wide
COND_CONVS = [(16, 16, 1, False), (16, 32, 2, False), (32, 96, 2, True), (96, 256, 2, False)]


@pytest.mark.parametrize("cin,Cout,stride,with_res", COND_CONVS, ids=[f"{a}to{b}-s{s}" + ("-res" if r else "") for a, b, s, r in COND_CONVS])
def test_conditioning_conv_padded_layouts(ops, cin, Cout, stride, with_res):
    B, H, W = 2, 16, 24
    Cs, width = ceil64(cin), ceil64(Cout)
    x = bfr(B, cin, H, W, seed=cin)
    wq = (randn(Cout, cin, 3, 3, seed=Cout) * (9 * cin) ** -0.5).to(BF)
    bias = randn(Cout, seed=3)
    xs = torch.zeros(B, H, W, Cs, dtype=BF)
    xs[..., :cin] = nhwc(x)
    wp = ops.pack_conv(wq.float().cuda(), cin_stored=Cs)
    packed = wp.view(Cout, 9, Cs)
    assert same_bits(packed[:, :, :cin].contiguous(), wq.permute(0, 2, 3, 1).reshape(Cout, 9, cin).contiguous().cuda()), "padded pack: weights"
    assert bool((bits(packed[:, :, cin:]) == 0).all()), "padded pack: padding channels are not zero"
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    rows = B * Ho * Wo
    ref = silu64(F.conv2d(x.double(), wq.double(), bias.double(), stride=stride, padding=1))
    assert tuple(ref.shape) == (B, Cout, Ho, Wo)
    ref = nhwc(ref).view(rows, Cout)
    res = None
    if with_res:
        res = bfr(rows, width, seed=9)                              # a residual in the same padded layout
        ref = ref + res.double()[:, :Cout]
    buf = sentinel(rows * width + 8)
    ops.conv3x3_ex(xs.cuda(), wp, bias=bias.cuda(), stride=stride, act=2, res=res.cuda() if with_res else None, out=buf, ldc=width)
    y = buf[:-8].view(rows, width)
    close_bf16(f"cond conv {cin}->{Cout} s{stride} res={int(with_res)}", y[:, :Cout], rnd(ref))
    assert untouched(y[:, Cout:]), "the padding columns of the output rows were written"
    assert untouched(buf[-8:])


# ------------------------------------------------------------------------------------ next-op weight prefetch
def env_int(name):
    """what atoi makes of an environment variable (None: unset)"""
    v = os.environ.get(name)
    if v is None:
        return None
    m = re.match(r"\s*[+-]?\d+", v)
    return int(m.group()) if m else 0


def test_prefetch_changes_neither_the_output_nor_its_target(ops):
    """a launch armed with a prefetch target gives the bits of the unarmed launch and leaves the target as it was; the target is a
    live tensor of the full size every time (a parity test on valid memory)"""
    if env_int("PEA_GEMM_PF") == 0:
        pytest.fail("PEA_GEMM_PF switches the prefetch off in this environment: this test would pass without testing anything")
    if env_int("PEA_GEMM_PF_MAX_MB") is not None and env_int("PEA_GEMM_PF_MAX_MB") < 3:
        pytest.fail("PEA_GEMM_PF_MAX_MB caps the prefetch below the sizes this test arms")
    MiB = 1 << 20
    sizes = [4, 128, 8192, 3 * 8192 + 132, 3 * MiB]
    T = torch.arange(80 * MiB // 4, dtype=torch.int32, device="cuda") * 40503 + 12345         # 80 MiB, a pattern
    keep = T.clone()
    a1, w1, b1 = bfr(128, 256, seed=1).cuda(), bfr(128, 256, seed=2, scale=1 / 16).cuda(), randn(128, seed=3).cuda()
    a2, w2, b2 = bfr(4100, 256, seed=4).cuda(), bfr(1288, 256, seed=5, scale=1 / 16).cuda(), randn(1288, seed=6).cuda()
    a3, w3 = bfr(1000, 128, seed=7).cuda(), bfr(336, 128, seed=8, scale=128 ** -0.5).cuda()
    x = bfr(2, 20, 20, 64, seed=9).cuda()
    wp = ops.pack_conv((randn(192, 64, 3, 3, seed=10) / 24).cuda())
    bc = randn(192, seed=11).cuda()

    def one_tile_kernel():                                          # variant 25: the one-tile-per-workgroup kernel's DMA waves
        L().pea_debug_set_gemm_variant(25)
        try:
            return ops.gemm(a3, w3)
        finally:
            L().pea_debug_set_gemm_variant(-1)

    launches = [("one tile 128x128x256", lambda: ops.gemm(a1, w1, bias=b1), sizes),
                ("persistent 4100x1288x256", lambda: ops.gemm(a2, w2, bias=b2), sizes + [80 * MiB]),      # above the 64 MiB cap
                ("conv 2x20x20 64->192", lambda: ops.conv3x3(x, wp, bias=bc), sizes),
                ("one-tile-per-workgroup kernel 1000x336x128", one_tile_kernel, sizes)]
    try:
        for name, launch, arm in launches:
            base = launch()
            for nbytes in arm:
                assert nbytes <= T.numel() * 4
                L().pea_debug_set_gemm_prefetch(ctypes.c_void_p(T.data_ptr()), nbytes)
                got = launch()
                assert same_bits(got, base), f"{name}: armed with {nbytes} bytes the output changes"
                assert torch.equal(T, keep), f"{name}: armed with {nbytes} bytes the prefetch target changed"
            print(f"[prefetch {name}] {len(arm)} armed launches: output and target bits unchanged (0 differing elements)")
    finally:
        L().pea_debug_set_gemm_prefetch(None, 0)
        L().pea_debug_set_gemm_variant(-1)
