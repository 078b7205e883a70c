"""Kernel-level parity (-m gpu) of the glue kernels between the GEMM / conv / norm / attention families: the maps, selects,
copies, transposes, layout changes, column sums, RMSNorm and LayerNorm statistics, the row softmax, the VAE ends, the text
glue, the split-K reduce, and the KD loss' nan_guard / grad_scale / tmap forms -- each through its pea_op_* entry against a
float64 reference of the same operation on the same bf16-rounded inputs, rounded once where the kernel stores.

Tolerances are those tests/test_ops_gpu.py states (close_bf16 / close_f32 are imported from there):
  * data movers and selects: the bits (torch.equal on integer views);
  * bf16-stored arithmetic: close_bf16, 1 ulp forward, 2 ulps backward;
  * fp32-stored outputs: close_f32 defaults (rtol 1e-3, atol 1e-4); saved statistics as test_groupnorm (rtol 1e-4, atol 1e-5).
  * column sums (fp32 sums of R bf16 values of root-mean-square `rms`): rtol 1e-3 and atol = 1e-4 * sqrt(R) * rms.  Derivation:
    a sum of R zero-mean terms has standard deviation sqrt(R) * rms -- that is the scale of the output tensor, and close_f32's
    atol of 1e-4 is meant at unit scale.  The kernels' own error is far below it: every output is the end of an addition chain
    of at most D = 16 + ppb + ceil(nblk / 16) + 16 fp32 additions (per thread, across the pixel lanes, across the block partials,
    across the 16 waves), so |err| <= D * 2^-24 * sum|x| <= D * 2^-24 * R * rms in the worst case and about 2^-24 * sqrt(D R) * rms
    typically: at the largest case here (R = 1637, C = 320, D = 40) 3.9e-3 * rms worst case against an atol of 4.0e-3 * rms.
    A nonzero mean adds R * mean to the result, which the relative term covers.  The worst error observed is printed per case.

Wherever a kernel writes a strided or partial output the buffer is pre-filled with a sentinel bit pattern, and every element
outside the specified region must still carry it.  Loop-cap crossings (second trip of a grid-stride loop): gelu_bwd
(EW_GRID, 8192 workgroups), nchw <-> nhwc with depth-to-space rows, fill_random, residual_import (2048 workgroups), splitk_reduce
(2048 workgroups)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
from glue_ref import (BF, bfr, bits, f32r, gelu64, gelu_grad64, hf_t5_bucket, rnd, same_bits, sentinel, silu64, silu_grad64,  # noqa: E402
                      t5_dist_table, untouched)
from test_ops_gpu import close_bf16, close_f32, ops  # noqa: E402,F401

RAGGED = 8 * (256 * 3 + 5)                       # four workgroups, the last one with 5 of its 256 lanes at work
PAST_EW_CAP = 8 * (8192 * 256 + 3)               # the EW_GRID cap plus three vectors: a second trip for the first lanes


def span12(n, seed):
    """bf16 values over [-12, 12] (both tails of erf and of the sigmoid) with exact zeros and the end points"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 24 - 12).to(BF)
    x[0], x[1], x[2], x[3] = 0.0, 12.0, -12.0, -0.0
    return x


# ------------------------------------------------------------------------------------ maps
@pytest.mark.parametrize("n", [8, RAGGED])
def test_maps_forward(ops, n):
    x, b = span12(n, 1), bfr(n, seed=2, scale=3.0)
    xd = x.double()
    for name, fn, ref in (("silu", ops.silu_fwd, silu64(xd)), ("gelu", ops.gelu_fwd, gelu64(xd))):
        y = sentinel(n + 8)
        fn(x.cuda(), y, n=n)
        close_bf16(f"{name}_fwd n={n}", y[:n], rnd(ref))
        assert untouched(y[n:]), name
    y = sentinel(n + 8)
    ops.add(x.cuda(), b.cuda(), y, n=n)
    close_bf16(f"add n={n}", y[:n], rnd(xd + b.double()))
    assert untouched(y[n:])


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("n", [8, RAGGED])
def test_maps_backward_and_accum(ops, n, accum):
    x, dy, prev = span12(n, 3), bfr(n, seed=4, scale=2.0), bfr(n, seed=5, scale=2.0)
    xd, dd, pd = x.double(), dy.double(), prev.double() * accum
    for name, fn, ref in (("silu_bwd", ops.silu_bwd, dd * silu_grad64(xd)), ("gelu_bwd", ops.gelu_bwd, dd * gelu_grad64(xd))):
        buf = sentinel(n + 8)
        buf[:n] = prev.cuda()
        fn(x.cuda(), dy.cuda(), buf, accum=bool(accum), n=n)
        close_bf16(f"{name} n={n} accum={accum}", buf[:n], rnd(ref + pd), ulps=2.0)
        assert untouched(buf[n:]), name
    buf = sentinel(n + 8)
    buf[:n] = prev.cuda()
    ops.accum_(x.cuda(), buf, accum=bool(accum), n=n)
    if accum:
        close_bf16(f"accum n={n}", buf[:n], rnd(xd + pd))
    else:
        assert same_bits(buf[:n].cpu(), x)                        # accum = 0 is a copy
    assert untouched(buf[n:])


def test_map_loop_past_the_grid_cap(ops):
    """gelu_bwd with accumulate at 8 (8192 * 256 + 3) elements: the first three lanes take a second trip of the loop"""
    n = PAST_EW_CAP
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(n, generator=g) * 24 - 12).to(BF)
    dy = torch.randn(n, generator=g).to(BF)
    prev = torch.randn(n, generator=g).to(BF)
    buf = sentinel(n + 8)
    buf[:n] = prev.cuda()
    ops.gelu_bwd(x.cuda(), dy.cuda(), buf, accum=True, n=n)
    ref = rnd(dy.double() * gelu_grad64(x.double()) + prev.double())
    close_bf16("gelu_bwd past the cap", buf[:n], ref, ulps=2.0)
    close_bf16("gelu_bwd past the cap, second trip", buf[n - 24:n], ref[n - 24:], ulps=2.0)
    assert untouched(buf[n:])


# ------------------------------------------------------------------------------------ sumpool2, geglu_bwd_il
@pytest.mark.parametrize("accum", [0, 1])
def test_sumpool2_non_square(ops, accum):
    B, H, W, C = 2, 3, 5, 24
    x, prev = bfr(B, 2 * H, 2 * W, C, seed=1), bfr(B, H, W, C, seed=2)
    y = sentinel(B * H * W * C + 8)
    y[:-8] = prev.reshape(-1).cuda()
    ops.sumpool2_(x.cuda(), y[:-8].view(B, H, W, C), accum=bool(accum))
    ref = x.double().view(B, H, 2, W, 2, C).sum((2, 4)) + prev.double() * accum
    close_bf16(f"sumpool2 accum={accum}", y[:-8].view(B, H, W, C), rnd(ref))
    assert untouched(y[-8:])


@pytest.mark.parametrize("inner", [4, 324])
def test_geglu_bwd_interleaved(ops, inner):
    rows = 5
    hg, dy = bfr(rows, 2 * inner, seed=1, scale=1.5), bfr(rows, inner, seed=2)
    out = sentinel(rows * 2 * inner + 8)
    ops.geglu_bwd_il(hg.cuda(), dy.cuda(), out[:-8].view(rows, 2 * inner))
    ref = hg.double() * dy.double().repeat_interleave(2, dim=1)
    close_bf16(f"geglu_bwd_il inner={inner}", out[:-8].view(rows, 2 * inner), rnd(ref), ulps=2.0)
    assert untouched(out[-8:])


# ------------------------------------------------------------------------------------ select_rows
MASKS = [[1, 0, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1]]


@pytest.mark.parametrize("mask", MASKS, ids=["mixed", "none", "all"])
@pytest.mark.parametrize("tail", [0, 8 * 19])
@pytest.mark.parametrize("per", [8, 8 * 77])
def test_select_rows(ops, per, tail, mask):
    B, ys = 4, per + tail
    c, u = bfr(B, per, seed=1), bfr(B, per, seed=2)
    m = torch.tensor(mask, dtype=torch.uint8)
    want = torch.where(m.bool()[:, None], u, c)
    y = sentinel(B * ys + 8)
    ops.select_rows_(c.cuda(), u.cuda(), m.cuda(), y, B, per, ys if tail else 0)
    yv = y[:-8].view(B, ys)
    assert same_bits(yv[:, :per].cpu(), want)
    assert untouched(yv[:, per:]) and untouched(y[-8:])
    # one sample per call with an offset mask pointer (the trainer's compacted teacher rows): B = 1, mask + j
    y1 = sentinel(B * ys + 8)
    cd, ud, md = c.cuda(), u.cuda(), m.cuda()
    for j in (2, 0, 3, 1):
        ops.select_rows_(cd[j:j + 1], ud[j:j + 1], md[j:], y1[j * ys:], 1, per, 0)
    y1v = y1[:-8].view(B, ys)
    assert same_bits(y1v[:, :per].cpu(), want)
    assert untouched(y1v[:, per:]) and untouched(y1[-8:])


@pytest.mark.parametrize("mask", MASKS, ids=["mixed", "none", "all"])
@pytest.mark.parametrize("tail", [0, 8 * 19])
@pytest.mark.parametrize("per", [8, 8 * 77])
def test_select_rows_bwd(ops, per, tail, mask):
    B, ds = 4, per + tail
    dy = bfr(B, ds, seed=3)
    dy[:, 1] = -0.0                                             # a negative zero travels as it is; the unselected side is +0
    m = torch.tensor(mask, dtype=torch.uint8)
    dc, du = sentinel(B * per + 8), sentinel(B * per + 8)
    ops.select_rows_bwd_(dy.cuda(), m.cuda(), dc, du, B, per, ds if tail else 0)
    src = dy[:, :per].contiguous()
    zero = torch.zeros(B, per, dtype=BF)
    sel = m.bool()[:, None]
    assert same_bits(dc[:-8].view(B, per).cpu(), torch.where(sel, zero, src))
    assert same_bits(du[:-8].view(B, per).cpu(), torch.where(sel, src, zero))
    for b in range(B):                                          # exact zeros: all bits clear, no -0.0
        off = dc if mask[b] else du
        assert int(bits(off[b * per:(b + 1) * per]).abs().max()) == 0
    assert untouched(dc[-8:]) and untouched(du[-8:])


# ------------------------------------------------------------------------------------ token mean
@pytest.mark.parametrize("B,L,C", [(3, 77, 40), (2, 1, 8)])
def test_mean_tokens_fwd_bwd(ops, B, L, C):
    x = bfr(B, L, C, seed=1, shift=3.0)                         # a mean of about 3: a wrong divisor shows
    y = sentinel(B * C + 8)
    ops.mean_tokens(x.cuda(), y[:-8].view(B, C))
    close_bf16(f"mean_tokens {B}x{L}x{C}", y[:-8].view(B, C), rnd(x.double().mean(1)))
    assert untouched(y[-8:])
    dy, prev = bfr(B, C, seed=2, shift=3.0), bfr(B, L, C, seed=3)
    for accum in (0, 1):
        dx = sentinel(B * L * C + 8)
        dx[:-8] = prev.reshape(-1).cuda()
        ops.mean_tokens_bwd_(dy.cuda(), dx[:-8].view(B, L, C), accum=bool(accum))
        ref = (dy.double() / L)[:, None, :].expand(B, L, C) + prev.double() * accum
        close_bf16(f"mean_tokens_bwd {B}x{L}x{C} accum={accum}", dx[:-8].view(B, L, C), rnd(ref), ulps=2.0)
        assert untouched(dx[-8:])


# ------------------------------------------------------------------------------------ column sums
def close_colsum(name, got, ref, rows, rms):
    atol = 1e-4 * math.sqrt(rows) * rms                         # derivation in the module docstring
    worst = (got.detach().double().cpu() - ref.double()).abs().max().item()
    print(f"[{name}] worst error {worst:.3e} against atol {atol:.3e} ({worst / atol:.2e} of it)")
    close_f32(name, got, ref, rtol=1e-3, atol=atol)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("C", [8, 64, 72])
@pytest.mark.parametrize("R", [1, 15, 16, 17, 616])
def test_colsum(ops, R, C, accum):
    x, prev = bfr(R, C, seed=R + C), f32r(C, seed=7, scale=3.0)
    db = sentinel(C + 8, torch.float32)
    db[:C] = prev.cuda()
    ops.colsum_(x.cuda(), db, accum=bool(accum))
    rms = x.double().pow(2).mean().sqrt().item()
    close_colsum(f"colsum {R}x{C} accum={accum}", db[:C], x.double().sum(0) + prev.double() * accum, R, rms)
    assert untouched(db[C:])


# colsum_geometry: ppb = max(256 / (C / 8), 1) pixels per workgroup pass, 16 ppb pixels per workgroup, nblk = ceil(HW / (16 ppb))
COLSUM_BATCHED = [(300, 8, 0),                      # ppb = 256: one workgroup, HW below its share
                  (40, 2048, 0),                    # ppb = 1: three workgroups
                  (1, 320, 0), (7, 320, 0),         # ppb = 6: fewer pixels than lanes, one ragged pass
                  (96, 320, 0), (97, 320, 0),       # 16 ppb exactly, and one pixel into a second workgroup
                  (1637, 320, 0),                   # 18 partial blocks: the reduce kernel's first two waves take two each
                  (97, 320, 24), (40, 2048, 8)]     # ldo > C: the gap stays as it was


@pytest.mark.parametrize("HW,C,gap", COLSUM_BATCHED)
def test_colsum_batched(ops, HW, C, gap):
    B, ldo = 2, C + gap
    x = bfr(B, HW, C, seed=HW + C, shift=0.25)
    out = sentinel(B * ldo + 8, torch.float32)
    ops.colsum_batched_(x.cuda(), out, ldo=ldo)
    ov = out[:-8].view(B, ldo)
    rms = x.double().pow(2).mean().sqrt().item()
    close_colsum(f"colsum_batched HW={HW} C={C} ldo={ldo}", ov[:, :C], x.double().sum(1), HW, rms)
    assert untouched(ov[:, C:]) and untouched(out[-8:])


# ------------------------------------------------------------------------------------ copy2d
@pytest.mark.parametrize("accum", [0, 1])
def test_copy2d_strided(ops, accum):
    rows, C, ldx, ldy = 5, 24, 40, 56
    x, prev = bfr(rows, ldx, seed=1), bfr(rows, C, seed=2)
    y = sentinel(rows * ldy + 8)
    yv = y[:-8].view(rows, ldy)
    yv[:, :C] = prev.cuda()
    ops.copy2d_(x.cuda(), ldx, y, ldy, rows, C, accum=bool(accum))
    if accum:
        close_bf16("copy2d accumulate", yv[:, :C], rnd(x[:, :C].double() + prev.double()))
    else:
        assert same_bits(yv[:, :C].cpu(), x[:, :C].contiguous())
    assert untouched(yv[:, C:]) and untouched(y[-8:])


def test_copy2d_broadcasts_one_row(ops):
    rows, C, ldy = 5, 24, 56
    x = bfr(C, seed=3)
    y = sentinel(rows * ldy + 8)
    ops.copy2d_(x.cuda(), 0, y, ldy, rows, C)
    yv = y[:-8].view(rows, ldy)
    assert same_bits(yv[:, :C].cpu(), x[None, :].expand(rows, C).contiguous())
    assert untouched(yv[:, C:]) and untouched(y[-8:])


# ------------------------------------------------------------------------------------ transposes and layout changes
@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (64, 32), (77, 100)])
def test_transposes(ops, R, C, pad):
    ldy = R + pad
    xb = bfr(R, C, seed=R)
    xf = f32r(R, C, seed=C) * (1 + 2.0 ** -9)                   # fp32 values that need the rounding
    for x, want in ((xb, xb.t().contiguous()), (xf, xf.to(BF).t().contiguous())):
        y = sentinel(C * ldy + 8)
        ops.transpose_(x.cuda(), y, R, C, ldy)
        yv = y[:-8].view(C, ldy)
        assert same_bits(yv[:, :R].cpu(), want), str(x.dtype)
        assert untouched(yv[:, R:]) and untouched(y[-8:])


def _layout_case(ops, B, C, hw, d2s):
    H, W = hw
    HW = H * W
    t = bfr(B, H, W, C, seed=H + C)                                             # the logical NHWC tensor
    stored = ops.nhwc_to_d2s(t) if d2s else t                                   # how it lies in memory
    nchw = t.permute(0, 3, 1, 2).reshape(B, C, HW).float().contiguous()
    y = sentinel(B * C * HW + 8, torch.float32)
    ops.nhwc_to_nchw_f32(stored.cuda(), B, HW, C, d2s_hw=hw if d2s else None, y=y)
    assert same_bits(y[:-8].view(B, C, HW).cpu(), nchw) and untouched(y[-8:])
    z = sentinel(B * HW * C + 8)
    ops.nchw_f32_to_nhwc(nchw.cuda(), B, HW, C, d2s_hw=hw if d2s else None, y=z)
    assert same_bits(z[:-8].view(stored.shape).cpu(), stored.contiguous()) and untouched(z[-8:])
    back = ops.nhwc_to_nchw_f32(z[:-8], B, HW, C, d2s_hw=hw if d2s else None)   # round trip: the identity
    assert same_bits(back.cpu(), nchw)


@pytest.mark.parametrize("d2s", [False, True], ids=["plain", "d2s"])
def test_nhwc_nchw_layouts(ops, d2s):
    _layout_case(ops, 2, 5, (4, 6), d2s)


def test_nhwc_nchw_past_the_grid_cap(ops):
    """64 x 66 x 500 = 2,112,000 elements, more than 8192 x 256: depth-to-space rows on the loop's second trip"""
    _layout_case(ops, 1, 500, (64, 66), True)


# ------------------------------------------------------------------------------------ weight repacks
def _pad_gather_ref(src, mode, d, dp, st_n, st_k):
    w = torch.zeros(st_n, st_k)
    for rp in range(st_n):
        for kp in range(st_k):
            r, k, pad = rp, kp, False
            if mode == 1:
                h, j = divmod(rp, dp)
                pad, r = j >= d, h * d + j
            elif mode == 2:
                h, j = divmod(kp, dp)
                pad, k = j >= d, h * d + j
            elif mode == 3:
                r = st_n // 2 + rp // 2 if rp & 1 else rp // 2
            w[rp, kp] = 0.0 if pad else src[r, k]
    return w.to(BF)


@pytest.mark.parametrize("with_wt", [True, False])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pad_gather(ops, mode, with_wt):
    d, dp, heads = 40, 64, 3
    N_t, K_t, st_n, st_k = {0: (24, 16, 24, 16), 1: (heads * d, 16, heads * dp, 16), 2: (16, heads * d, 16, heads * dp),
                            3: (10, 16, 10, 16)}[mode]
    src = f32r(N_t, K_t, seed=mode) * (1 + 2.0 ** -9)
    ldw, ldwt = st_k + 8, st_n + 16
    w, wt = sentinel(st_n * ldw + 8), sentinel(st_k * ldwt + 8)
    ops.pad_gather_(src.cuda(), mode, d, dp, w, ldw, wt if with_wt else None, ldwt, st_n, st_k)
    want = _pad_gather_ref(src, mode, d, dp, st_n, st_k)
    wv = w[:-8].view(st_n, ldw)
    assert same_bits(wv[:, :st_k].cpu(), want)                  # every stored element written, zeros (all bits clear) in the padding
    assert untouched(wv[:, st_k:]) and untouched(w[-8:])
    if with_wt:
        tv = wt[:-8].view(st_k, ldwt)
        assert same_bits(tv[:, :st_n].cpu(), want.t().contiguous())
        assert untouched(tv[:, st_n:]) and untouched(wt[-8:])
    else:
        assert untouched(wt)


def test_pad_head_vec_and_permute_geglu_vec(ops):
    heads, d, dp = 3, 40, 64
    src = f32r(heads * d, seed=1)
    dst = sentinel(heads * dp + 4, torch.float32)
    ops.pad_head_vec(src.cuda(), heads, d, dp, dst=dst)
    want = torch.zeros(heads, dp)
    want[:, :d] = src.view(heads, d)
    assert same_bits(dst[:-4].cpu(), want.reshape(-1)) and untouched(dst[-4:])
    inner = 5
    v = f32r(2 * inner, seed=2)
    out = sentinel(2 * inner + 4, torch.float32)
    ops.permute_geglu_vec(v.cuda(), out)
    assert same_bits(out[:-4].cpu(), torch.stack([v[:inner], v[inner:]], 1).reshape(-1)) and untouched(out[-4:])


# ------------------------------------------------------------------------------------ casts
def test_casts(ops):
    i = torch.tensor([0, 1, -1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 40 + 2 ** 16, 2 ** 40 + 2 ** 16 + 1,
                      -(2 ** 62), 2 ** 63 - 1, 49407, 999], dtype=torch.int64)
    y = sentinel(i.numel() + 4, torch.float32)
    ops.cast_i64_f32(i.cuda(), y)
    assert same_bits(y[:-4].cpu(), i.to(torch.float32)) and untouched(y[-4:])        # round to nearest even, as the CPU cast
    f = torch.tensor([0.0, -0.0, 1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8), 3.0e38, 3.4e38,
                      float("inf"), float("-inf"), float("nan"), 0.1, -7.3], dtype=torch.float32)
    b = sentinel(f.numel() + 8)
    ops.cast_f32_bf16(f.cuda(), b)
    got, want = b[:f.numel()].cpu(), f.to(BF)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == 1
    assert torch.equal(bits(got)[~nan], bits(want)[~nan])                            # ties to even, overflow to Inf, signed zeros
    assert untouched(b[f.numel():])
    x = bfr(RAGGED + 3, seed=9)
    z = sentinel(x.numel() + 4, torch.float32)
    ops.cast_bf16_f32(x.cuda(), z)
    assert same_bits(z[:-4].cpu(), x.float()) and untouched(z[-4:])


# ------------------------------------------------------------------------------------ split-K reduce
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("gap", [0, 12])
@pytest.mark.parametrize("M,N", [(5, 8), (37, 132)])
@pytest.mark.parametrize("nsplit", [1, 3])
def test_splitk_reduce(ops, nsplit, M, N, gap, accum):
    ldo, stride = N + gap, M * N + 20                           # partials further apart than one matrix
    part = f32r(nsplit * stride, seed=M + nsplit)
    prev = bfr(M, N, seed=3)
    out = sentinel(M * ldo + 8)
    ov = out[:-8].view(M, ldo)
    ov[:, :N] = prev.cuda()
    ops.splitk_reduce_(part.cuda(), nsplit, stride, out, ldo, M, N, accum=bool(accum))
    ref = sum(part[s * stride:s * stride + M * N].double().view(M, N) for s in range(nsplit)) + prev.double() * accum
    close_bf16(f"splitk_reduce {nsplit}x{M}x{N} ldo={ldo} accum={accum}", ov[:, :N], rnd(ref))
    assert untouched(ov[:, N:]) and untouched(out[-8:])


def test_splitk_reduce_past_the_grid_cap(ops):
    M, N, nsplit = 1040, 2020, 2                                # M N / 4 = 525,200 > 2048 x 256
    stride = M * N + 4
    part = f32r(nsplit * stride, seed=5)
    out = sentinel(M * N + 8)
    ops.splitk_reduce_(part.cuda(), nsplit, stride, out, N, M, N)
    ref = part[:M * N].double() + part[stride:stride + M * N].double()
    close_bf16("splitk_reduce past the cap", out[:-8], rnd(ref))
    assert untouched(out[-8:])


# ------------------------------------------------------------------------------------ norms
NORM_ROWS = [1, 2, 3, 9]              # one wave with its second row absent, a full pair, odd counts, more than one workgroup
NORM_COLS = [8, 512, 520, 1664, 2048, 2568, 4096]     # 1, 64, 65, 208, 256, 321, 512 chunks: NCH = 1, 1, 2, 4, 4, 8, 8


def _norm_inputs(R, C):
    x = (bfr(R, C, seed=R * 7 + C).float() * 2 - 0.5).to(BF)
    g = torch.Generator().manual_seed(C)
    return x, 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


@pytest.mark.parametrize("C", NORM_COLS)
def test_rmsnorm_and_layernorm_stats(ops, C):
    for R in NORM_ROWS:
        x, gamma, _ = _norm_inputs(R, C)
        xd = x.double()
        y = sentinel((R + 1) * C)
        ops.rmsnorm_fwd_(x.cuda(), gamma.cuda(), y, R, C, eps=1e-6)
        ref = xd * torch.rsqrt(xd.pow(2).mean(1, keepdim=True) + 1e-6) * gamma.double()
        close_bf16(f"rmsnorm {R}x{C}", y[:R * C].view(R, C), rnd(ref))
        assert untouched(y[R * C:]), f"rmsnorm {R}x{C}: row {R} was written"
        st = sentinel((R + 1) * 2, torch.float32)
        ops.layernorm_stats_(x.cuda(), st, R, C, eps=1e-5)
        got = st[:2 * R].view(R, 2).cpu()
        mean, var = xd.mean(1), xd.var(1, unbiased=False)
        assert torch.allclose(got[:, 0], mean.float(), rtol=1e-4, atol=1e-5), f"layernorm_stats {R}x{C}: mean"
        assert torch.allclose(got[:, 1], (var + 1e-5).rsqrt().float(), rtol=1e-4, atol=1e-5), f"layernorm_stats {R}x{C}: rstd"
        assert untouched(st[2 * R:]), f"layernorm_stats {R}x{C}: row {R} was written"


@pytest.mark.parametrize("C", [2568, 4096])
def test_layernorm_eight_chunk_instance(ops, C):
    """321 .. 512 chunks per row: ln_fwd_kernel<8> / ln_bwd_kernel<8>, full (4096) and with a ragged last chunk column (2568)"""
    for R in NORM_ROWS:
        x, gamma, beta = _norm_inputs(R, C)
        xd, gd, bd = x.double(), gamma.double(), beta.double()
        mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
        rstd = (var + 1e-5).rsqrt()
        xh = (xd - mean) * rstd
        y, st = sentinel((R + 1) * C), sentinel((R + 1) * 2, torch.float32)
        ops.layernorm_fwd_(x.cuda(), gamma.cuda(), beta.cuda(), y, st, R, C)
        close_bf16(f"layernorm fwd {R}x{C}", y[:R * C].view(R, C), rnd(xh * gd + bd))
        got = st[:2 * R].view(R, 2).cpu()
        assert torch.allclose(got[:, 0], mean[:, 0].float(), rtol=1e-4, atol=1e-5)
        assert torch.allclose(got[:, 1], rstd[:, 0].float(), rtol=1e-4, atol=1e-5)
        assert untouched(y[R * C:]) and untouched(st[2 * R:])
        dy, prev = bfr(R, C, seed=3), bfr(R, C, seed=4)
        d = dy.double() * gd
        ref = rstd * (d - d.mean(1, keepdim=True) - xh * (d * xh).mean(1, keepdim=True))
        stats = torch.cat([mean, rstd], 1).float().cuda()
        for accum in (0, 1):
            dx = sentinel((R + 1) * C)
            dx[:R * C] = prev.reshape(-1).cuda()
            ops.layernorm_bwd_(x.cuda(), dy.cuda(), gamma.cuda(), stats, dx, R, C, accum=bool(accum))
            close_bf16(f"layernorm bwd {R}x{C} accum={accum}", dx[:R * C].view(R, C), rnd(ref + prev.double() * accum), ulps=2.0)
            assert untouched(dx[R * C:])


# ------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("cols", [8, 512, 2048, 2056, 4096])
def test_softmax_rows(ops, cols, pad):
    """8: one lane of the workgroup has data; 512: one wave; 2048: one full trip; 2056: a second trip for one lane; 4096: two"""
    rows, ld, scale = 3, cols + pad, 0.5
    x = bfr(rows, cols, seed=cols, scale=3.0)
    x[0, cols // 3] = 40.0                                       # a spike far above the rest
    x[1, :] = 1.75                                               # an all-equal row
    buf = sentinel(rows * ld + 8)
    bv = buf[:-8].view(rows, ld)
    bv[:, :cols] = x.cuda()
    ops.softmax_rows_(buf, rows, cols, ld, scale)
    ref = torch.softmax(x.double() * float(torch.tensor(scale, dtype=torch.float32)), -1)
    close_bf16(f"softmax_rows cols={cols} ld={ld}", bv[:, :cols], rnd(ref))
    assert same_bits(bv[1, :cols].cpu(), rnd(torch.full((cols,), 1.0 / cols, dtype=torch.float64)))
    assert untouched(bv[:, cols:]) and untouched(buf[-8:])


# ------------------------------------------------------------------------------------ residual import, VAE ends
@pytest.mark.parametrize("B,C,HW", [(2, 5, 12), (1, 5, 104860)], ids=["small", "past-the-cap"])     # 524,300 > 2048 x 256
def test_residual_import(ops, B, C, HW):
    s32 = float(torch.tensor(0.1, dtype=torch.float32))
    src = f32r(B, C, HW, seed=1) * (1 + 2.0 ** -9)
    for dtype in (0, 1, 2):
        if dtype == 0:
            s, ref = src, src.double().permute(0, 2, 1) * s32
        elif dtype == 1:
            s = src.to(BF)
            ref = s.double().permute(0, 2, 1) * s32
        else:
            s = src.to(BF).permute(0, 2, 1).contiguous()
            ref = s.double() * s32
        dst = sentinel(B * HW * C + 8)
        ops.residual_import(s.cuda(), dtype, B, C, HW, 0.1, dst=dst)
        close_bf16(f"residual_import dtype={dtype} {B}x{C}x{HW}", dst[:-8].view(B, HW, C), rnd(ref))
        assert untouched(dst[-8:])


@pytest.mark.parametrize("C2", [8, 2])
def test_vae_posterior(ops, C2):
    B, H, W, L, scaling = 2, 4, 5, C2 // 2, 0.13025
    g = torch.Generator().manual_seed(C2)
    h = torch.randn(B, C2, H, W, generator=g)
    h[:, L:] *= 30.0                                             # log-variances beyond both clamps
    wq = torch.eye(C2) + 0.1 * torch.randn(C2, C2, generator=g)
    bq = 0.1 * torch.randn(C2, generator=g)
    noise = torch.randn(B, L, H, W, generator=g)
    mom = torch.einsum("oc,bchw->bohw", wq.double(), h.double()) + bq.double()[None, :, None, None]
    assert float(mom[:, L:].min()) < -30 and float(mom[:, L:].max()) > 20
    lv = mom[:, L:].clamp(-30.0, 20.0)
    lat = (mom[:, :L] + torch.exp(0.5 * lv) * noise.double()) * scaling
    hc, wc, bc, nc = h.cuda(), wq.cuda(), bq.cuda(), noise.cuda()
    m1, l1 = ops.vae_posterior(hc, wc, bc, nc, scaling)
    close_f32(f"vae_posterior C2={C2} moments", m1, mom)
    close_f32(f"vae_posterior C2={C2} latents", l1, lat)
    m2, l2 = ops.vae_posterior(hc, wc, bc, None, scaling)                    # no noise: the scaled mean
    close_f32(f"vae_posterior C2={C2} mode", l2, mom[:, :L] * scaling)
    assert same_bits(m2.cpu(), m1.cpu())
    m3, l3 = ops.vae_posterior(hc, wc, bc, nc, scaling, want_moments=False)
    m4, l4 = ops.vae_posterior(hc, wc, bc, nc, scaling, want_latents=False)
    assert m3 is None and l4 is None and same_bits(l3.cpu(), l1.cpu()) and same_bits(m4.cpu(), m1.cpu())


@pytest.mark.parametrize("C", [4, 1])
def test_vae_post_quant(ops, C):
    B, H, W, inv = 2, 4, 5, 1.0 / 0.13025
    g = torch.Generator().manual_seed(C)
    z, w, b = torch.randn(B, C, H, W, generator=g), torch.randn(C, C, generator=g), torch.randn(C, generator=g)
    got = ops.vae_post_quant(z.cuda(), w.cuda(), b.cuda(), inv)
    ref = torch.einsum("oc,bchw->bohw", w.double(), z.double() * float(torch.tensor(inv, dtype=torch.float32))) + b.double()[None, :, None, None]
    close_f32(f"vae_post_quant C={C}", got, ref)


# ------------------------------------------------------------------------------------ text glue
def test_embed_tokens_three_forms(ops):
    vocab, width, B, L = 11, 16, 2, 5
    tok, pos, ty = bfr(vocab, width, seed=1), bfr(L, width, seed=2), bfr(width, seed=3)
    ids = torch.tensor([[0, 3, -1, vocab, vocab - 1], [7, 7, 10 ** 12, -5, 2]], dtype=torch.int64)
    rows = tok[ids.clamp(0, vocab - 1)]                                      # ids outside the table clamp to its ends
    t5 = ops.embed_tokens(ids.cuda(), tok.cuda())
    assert same_bits(t5.cpu(), rows)
    clip = ops.embed_tokens(ids.cuda(), tok.cuda(), pos.cuda())
    close_bf16("embed_tokens + positions", clip, rnd(rows.double() + pos.double()[None]))
    bert = ops.embed_tokens(ids.cuda(), tok.cuda(), pos.cuda(), ty.cuda())
    close_bf16("embed_tokens + positions + type 0", bert, rnd(rows.double() + pos.double()[None] + ty.double()[None, None]))


def test_gather_eos(ops):
    B, L, width, eos = 5, 6, 24, 9
    x = bfr(B, L, width, seed=1)
    ids = torch.tensor([[1, 2, 3, 4, 5, 6],        # no EOS: the last row
                        [1, 9, 3, 9, 5, 6],        # the first of two
                        [9, 2, 3, 4, 5, 6],        # at position 0
                        [1, 2, 3, 4, 5, 9],        # at the end
                        [8, 8, 9, 9, 9, 1]], dtype=torch.int64)
    got = ops.gather_eos(ids.cuda(), x.cuda(), eos)
    assert same_bits(got.cpu(), x[torch.arange(B), torch.tensor([5, 1, 0, 5, 2])])
    ids2 = torch.tensor([[1, 7, 3, 7, 5, 6],       # eos < 0: the argmax of the ids, the first of equal maxima
                         [4, 4, 4, 4, 4, 4],
                         [0, 1, 2, 3, 4, 5],
                         [5, 4, 3, 2, 1, 0],
                         [1, 2, 9, 3, 9, 9]], dtype=torch.int64)
    got = ops.gather_eos(ids2.cuda(), x.cuda(), -1)
    assert same_bits(got.cpu(), x[torch.arange(B), torch.tensor([1, 0, 5, 0, 2])])


def test_kv_len_is_last_non_pad_plus_one(ops):
    pad = 0
    ids = torch.tensor([[5, 6, 7, 0, 0, 0],        # right padding: 3
                        [0, 0, 0, 0, 0, 0],        # pads only: 1 (a row keeps one key)
                        [5, 0, 7, 0, 0, 0],        # a pad id inside the prompt, a real token behind it: 3, not 1
                        [5, 6, 7, 8, 9, 4],        # no padding: L
                        [0, 0, 0, 0, 0, 3]], dtype=torch.int64)
    out = sentinel(5 + 3, torch.int32)
    from pea_diffusion_amd._lib import check, lib, ptr, stream_ptr
    check(lib().pea_op_kv_len(ptr(ids.cuda()), ptr(out), 5, 6, pad, stream_ptr()))
    assert out[:5].cpu().tolist() == [3, 1, 3, 6, 6] and untouched(out[5:])
    assert ops.kv_len(ids.cuda(), pad).cpu().tolist() == [3, 1, 3, 6, 6]


@pytest.mark.parametrize("L,pitch", [(7, 64), (7, 128), (70, 128)])          # (a row of 70 keys has no pitch of 64)
def test_t5_rel_bias(ops, L, pitch):
    H, nbk, maxd = 3, 32, 128
    rel = f32r(nbk, H, seed=L)
    tab = t5_dist_table(L, nbk, maxd)
    pos = torch.arange(L)
    bucket = hf_t5_bucket(pos[None, :] - pos[:, None], nbk, maxd)            # [q][k], key - query
    assert torch.equal(bucket, (pos[None, :] > pos[:, None]).long() * (nbk // 2) + tab.long()[(pos[None, :] - pos[:, None]).abs()])
    bias = sentinel(H * L * pitch + 8, torch.float32)
    ops.t5_rel_bias_(rel.cuda(), tab.cuda(), bias, H, L, pitch)
    bv = bias[:-8].view(H, L, pitch)
    want = rel[bucket].permute(2, 0, 1).contiguous() * torch.tensor(1.4426950408889634, dtype=torch.float32)
    assert same_bits(bv[:, :, :L].cpu(), want)                               # a table lookup and one fp32 product
    assert untouched(bv[:, :, L:]) and untouched(bias[-8:])


# ------------------------------------------------------------------------------------ KD loss forms, AdamW, RNG fill
KD_SHAPES = [(4, 16, 4, 4), (4, 8, 4, 4), (4, 24, 2, 2)]
ZH = [1, 0, 0, 1]


def _kd_inputs():
    fs = [bfr(*s, seed=10 + i) for i, s in enumerate(KD_SHAPES)]
    ft = [bfr(*s, seed=30 + i) for i, s in enumerate(KD_SHAPES)]
    g = torch.Generator().manual_seed(5)
    es, e, et = [torch.randn(4, 4, 4, 4, generator=g) for _ in range(3)]
    return fs, ft, es, e, et, torch.tensor(ZH)


def _kd_run(ops, fs, ft, es, e, et, z, **kw):
    c = lambda ts: [t.cuda() for t in ts]
    losses, dt, de = ops.kd_loss(c(fs), c(ft), es.cuda(), e.cuda(), et.cuda(), z.cuda(), **kw)
    return losses.cpu(), [d.cpu() for d in dt], de.cpu()


def _kd_ref(fs, ft, es, e, et, z, nan_guard=False):
    from oracle.step_ref import kd_losses
    fsr = [t.double().requires_grad_(True) for t in fs]
    esr = es.double().requires_grad_(True)
    out = kd_losses(esr, e.double(), et.double(), fsr, [t.double() for t in ft], z, nan_guard=nan_guard)
    out[0].backward()
    grads = [r.grad if r.grad is not None else torch.zeros_like(r) for r in fsr]
    return torch.stack([torch.as_tensor(v, dtype=torch.float64) for v in out]).detach(), grads, esr.grad


def test_kd_loss_grad_scale(ops):
    """grad_scale multiplies every seed and leaves the four losses alone"""
    inp = _kd_inputs()
    l1, d1, e1 = _kd_run(ops, *inp)
    l4, d4, e4 = _kd_run(ops, *inp, grad_scale=0.25)
    assert same_bits(l4, l1)
    ref_l, ref_d, ref_e = _kd_ref(*inp)
    close_f32("kd losses", l4, ref_l, rtol=1e-3, atol=1e-5)
    close_f32("kd deps, grad_scale 0.25", e4, 0.25 * ref_e, rtol=1e-3, atol=1e-9)
    for i, (d, r) in enumerate(zip(d4, ref_d)):
        close_bf16(f"kd dtap{i}, grad_scale 0.25", d, rnd(0.25 * r), ulps=2.0)
        assert same_bits(d, (d1[i].float() * 0.25).to(BF))                   # a power of two: the unscaled seeds, exactly


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_kd_loss_nan_guard_drops_the_tap(ops, bad):
    """a non-finite value in a sample WITH KD weight: the tap leaves the loss, its seeds are exact zeros, the rest is as before"""
    fs, ft, es, e, et, z = _kd_inputs()
    clean = _kd_run(ops, fs, ft, es, e, et, z, nan_guard=True)
    fs = [t.clone() for t in fs]
    fs[1][1, 3, 2, 1] = bad                                                  # sample 1: zh = 0
    losses, dt, de = _kd_run(ops, fs, ft, es, e, et, z, nan_guard=True)
    ref_l, _, _ = _kd_ref(fs, ft, es, e, et, z, nan_guard=True)
    assert torch.isfinite(losses).all()
    close_f32("kd losses, tap 1 dropped", losses, ref_l, rtol=1e-3, atol=1e-5)
    assert int(bits(dt[1]).abs().max()) == 0                                 # exact zeros, every sample of the tap
    assert same_bits(dt[0], clean[1][0]) and same_bits(dt[2], clean[1][2]) and same_bits(de, clean[2])
    assert same_bits(losses[1:3], clean[0][1:3])                             # the two noise terms do not move
    # without the guard the value reaches the loss and the live sample's seeds: that is the unguarded contract
    l0, d0, _ = _kd_run(ops, fs, ft, es, e, et, z, nan_guard=False)
    assert not torch.isfinite(l0[3]) and not torch.isfinite(l0[0]) and torch.isfinite(l0[1:3]).all()
    assert same_bits(d0[0], clean[1][0])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_kd_loss_nan_guard_does_not_inspect_masked_samples(ops, bad):
    """a non-finite value in a MASKED sample (zh = 1, KD weight 0).  The reference script and oracle.step_ref.kd_losses test
    mse * (1 - zh), where NaN * 0 is NaN, and drop the tap; the kernel never reads masked samples (with compacted teacher rows
    there is nothing to read) and KEEPS it: losses and seeds are those of the clean batch, bit for bit, with and without the
    guard, in the student tap or in the teacher tap.  Pinned here; the difference is stated at KdLossP::nan_guard and in DESIGN.md."""
    fs, ft, es, e, et, z = _kd_inputs()
    clean = _kd_run(ops, fs, ft, es, e, et, z, nan_guard=True)
    for which in (0, 1):
        fs2, ft2 = [t.clone() for t in fs], [t.clone() for t in ft]
        (fs2, ft2)[which][1][0, 3, 2, 1] = bad                               # sample 0: zh = 1
        for guard in (True, False):
            losses, dt, de = _kd_run(ops, fs2, ft2, es, e, et, z, nan_guard=guard)
            assert same_bits(losses, clean[0]) and same_bits(de, clean[2])
            assert all(same_bits(a, b) for a, b in zip(dt, clean[1]))
        ref_l, _, _ = _kd_ref(fs2, ft2, es, e, et, z, nan_guard=True)
        full, _, _ = _kd_ref(fs, ft, es, e, et, z, nan_guard=True)
        assert float(ref_l[3]) < float(full[3])                              # the reference composition drops the tap


def test_kd_loss_compacted_teacher_rows(ops):
    """teacher tensors holding only the rows of the samples with KD weight, addressed through tmap: the uncompacted call's bits"""
    fs, ft, es, e, et, z = _kd_inputs()
    full = _kd_run(ops, fs, ft, es, e, et, z)
    live = [1, 2]
    c = lambda ts: [t.cuda() for t in ts]
    tmap = torch.tensor([-1, 0, 1, -1], dtype=torch.int32).cuda()
    losses, dt, de = ops.kd_loss_tmap(c(fs), c([t[live].contiguous() for t in ft]), es.cuda(), e.cuda(), et[live].contiguous().cuda(),
                                      z.cuda(), tmap)
    assert same_bits(losses.cpu(), full[0]) and same_bits(de.cpu(), full[2])
    assert all(same_bits(a.cpu(), b) for a, b in zip(dt, full[1]))
    # the rows in the other order: the map is what is followed, not the position
    tmap2 = torch.tensor([-1, 1, 0, -1], dtype=torch.int32).cuda()
    rev = [2, 1]
    l2, dt2, de2 = ops.kd_loss_tmap(c(fs), c([t[rev].contiguous() for t in ft]), es.cuda(), e.cuda(), et[rev].contiguous().cuda(),
                                    z.cuda(), tmap2)
    assert same_bits(l2.cpu(), full[0]) and same_bits(de2.cpu(), full[2]) and all(same_bits(a.cpu(), b) for a, b in zip(dt2, full[1]))


def test_adamw_grad_scale_ragged(ops):
    from pea_diffusion_amd._lib import check, lib, ptr, stream_ptr
    n, gs, lr, b1, b2, eps, wd = 1003, 0.125, 1e-2, 0.9, 0.999, 1e-8, 0.01
    g = torch.Generator().manual_seed(0)
    w0 = torch.randn(n, generator=g)
    w, m, v = w0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    buf = sentinel(n + 5, torch.float32)
    buf[:n] = w0.cuda()
    md, vd = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * 8
        gi = gr.double() * gs
        m = b1 * m + (1 - b1) * gi
        v = b2 * v + (1 - b2) * gi * gi
        w = w * (1 - lr * wd) - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
        check(lib().pea_op_adamw(ptr(buf), ptr(gr.cuda()), ptr(md), ptr(vd), n, lr, b1, b2, eps, wd, step, gs, stream_ptr()))
    close_f32("adamw grad_scale", buf[:n], w, rtol=1e-4, atol=1e-6)
    close_f32("adamw m", md, m, rtol=1e-4, atol=1e-6)
    assert untouched(buf[n:])


def test_fill_random_is_a_function_of_seed_and_index(ops):
    small, big = 1000, 8192 * 256 + 500                                      # the second past the loop's grid cap
    for dtype, scale in ((BF, 0.5), (torch.float32, 0.5), (BF, 0.02)):
        a, b = sentinel(small + 8, dtype), sentinel(big + 8, dtype)
        ops.fill_random_(a, 1234, scale, n=small)
        ops.fill_random_(b, 1234, scale, n=big)
        assert same_bits(a[:small].cpu(), b[:small].cpu()) and untouched(a[small:]) and untouched(b[big:])
        c = sentinel(small, dtype)
        ops.fill_random_(c, 1235, scale)
        assert not same_bits(c.cpu(), a[:small].cpu())
        vals = b[:big].float().cpu()
        lo, hi = float(vals.min()), float(vals.max())
        print(f"[fill_random {dtype} scale={scale}] min={lo!r} max={hi!r} mean={float(vals.mean()):.3e}")
        assert -scale <= lo and hi < scale                                   # [-scale, scale), after the bf16 rounding too
        assert lo < -0.99 * scale and hi > 0.99 * scale and abs(float(vals.mean())) < 0.01 * scale
        b2 = sentinel(big + 4096 + 8, dtype)                                 # a third length: the second trip's indices are its own
        ops.fill_random_(b2, 1234, scale, n=big + 4096)
        assert same_bits(b2[:big].cpu(), b[:big].cpu()) and untouched(b2[big + 4096:])
        assert not same_bits(b[big - 500:big].cpu(), b[:500].cpu())
