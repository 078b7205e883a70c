"""Operator-level Python bindings over the C ABI (include/pea_hip.h, `pea_op_*`).

Thin: torch tensors provide device memory and the current stream, nothing else.  Every function
takes/returns CUDA(HIP) tensors; bf16 activations are token-major ("NHWC").
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from ._lib import PeaError, check, lib, ptr, stream_ptr

BF = torch.bfloat16


def _dev(t):
    return t.device


def gemm(a, w, bias=None, rowvec=None, rows_per_batch=1, act=0, res=None, want_preact=False, out_f32=False,
         alpha=1.0, out=None, accum_f32=False):
    """act(alpha * a @ w.T + bias + rowvec[m // rows_per_batch]) + res ; a [M,K] bf16, w [N,K] bf16."""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else BF)
    pre = torch.empty(M, N, device=a.device, dtype=BF) if want_preact else None
    check(lib().pea_op_gemm(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, alpha,
                            ptr(bias), ptr(rowvec), rowvec.stride(0) if rowvec is not None else 0, rows_per_batch,
                            act, ptr(pre), N, ptr(res), res.stride(0) if res is not None else 0,
                            int(out.dtype == torch.float32), int(accum_f32), stream_ptr()))
    return (out, pre) if want_preact else out


def gemm_geglu(a, w, bias=None, want_stash=True, stash_grad=True, stash_rows=0, tanh=False, y=None, stash=None):
    """FF projection with GEGLU in its epilogue (pea_op_gemm_geglu): w [N,K] rows interleaved (h_i, gate_i);
    returns (h * gelu(gate) [M,N/2], stash [M,N] or None).  stash_grad: the stash holds (gelu(gate), h * gelu'(gate)).
    tanh: the gate goes through gelu_new, the tanh form (pea_op_gemm_geglu_tanh; no stash_grad with it).
    y / stash: caller-provided [M,N/2] / [M,N] buffers."""
    M, K = a.shape
    N = w.shape[0]
    if y is None:
        y = torch.empty(M, N // 2, device=a.device, dtype=BF)
    st = stash if stash is not None else (torch.zeros(M, N, device=a.device, dtype=BF) if want_stash else None)
    if tanh:
        check(lib().pea_op_gemm_geglu_tanh(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(y), ptr(st), M, N, K,
                                           int(stash_grad), stash_rows, 1, stream_ptr()))
        return y, st
    check(lib().pea_op_gemm_geglu(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(bias), ptr(y), ptr(st), M, N, K,
                                  int(stash_grad), stash_rows, stream_ptr()))
    return y, st


def gemm_splitk(a, w, ksplit, part, ldc, split_stride, alpha=1.0):
    """split-K GEMM (pea_op_gemm_splitk): fp32 partial s of alpha * a @ w.T over its own K-step range, [M,N] with rows ldc
    apart at part[s * split_stride:]; `part` is a flat fp32 buffer the caller owns.  splitk_reduce_ adds the partials."""
    M, K = a.shape
    N = w.shape[0]
    assert part.dtype == torch.float32 and part.numel() >= (ksplit - 1) * split_stride + (M - 1) * ldc + N
    check(lib().pea_op_gemm_splitk(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(part), ldc, split_stride, M, N, K, alpha,
                                   ksplit, stream_ptr()))
    return part


def gemm_geglu_bwd(a, w, pre, form=0):
    """dgrad GEMM of the FF output projection with the GEGLU backward in its epilogue (pea_op_gemm_geglu_bwd):
    dy = a @ w.T ([M,N], never stored); pre [M,2N] interleaved (h, gate) [form 0] or (gelu(gate), h gelu'(gate)) [form 1]
    -> d(pre) [M,2N] interleaved (dh, dgate)."""
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, 2 * N, device=a.device, dtype=BF)
    check(lib().pea_op_gemm_geglu_bwd(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(pre), pre.stride(0), ptr(out), out.stride(0),
                                      M, N, K, form, stream_ptr()))
    return out


def ln_linear(x, gamma, beta, w, bias=None, eps=1e-5, geglu=False):
    """LayerNorm folded into its consuming Linear (pea_op_ln_linear): x [M,K] bf16, w [N,K] bf16 -> LN(x) @ w.T + bias.
    geglu=True: w rows interleaved (h_i, gate_i); returns (h * gelu(gate) [M,N/2], pre-activation [M,N])."""
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=BF)
    gy = torch.empty(M, N // 2, device=x.device, dtype=BF) if geglu else None
    wf = torch.empty(N, K, device=x.device, dtype=BF)
    sv = torch.empty(N, device=x.device, dtype=torch.float32)
    tv = torch.empty(N, device=x.device, dtype=torch.float32)
    st = torch.empty(M, 2, device=x.device, dtype=torch.float32)
    check(lib().pea_op_ln_linear(ptr(x), ptr(gamma), ptr(beta), ptr(w), ptr(bias), ptr(y), ptr(gy), M, N, K, eps, ptr(wf),
                                 ptr(sv), ptr(tv), ptr(st), stream_ptr()))
    return (gy, y) if geglu else y


def pack_conv(w_fp32, dgrad=False, cin_stored=None):
    """cin_stored: the forward pack for an input stored that many channels wide (zero weights in the padding channels)"""
    Co, Ci = w_fp32.shape[:2]
    if cin_stored is not None:
        assert not dgrad, "the padded pack is a forward pack"
        out = torch.empty(Co, 9 * cin_stored, device=w_fp32.device, dtype=BF)
        check(lib().pea_op_pack_conv_padded(ptr(w_fp32.contiguous()), ptr(out), Co, Ci, cin_stored, stream_ptr()))
        return out
    out = torch.empty((Ci, 9 * Co) if dgrad else (Co, 9 * Ci), device=w_fp32.device, dtype=BF)
    check(lib().pea_op_pack_conv(ptr(w_fp32.contiguous()), ptr(out), Co, Ci, int(dgrad), stream_ptr()))
    return out


def conv3x3(x, w_packed, bias=None, stride=1, upsample2x=False, transposed2=False, rowvec=None, res=None):
    """x [B,H,W,Cin] bf16 NHWC; w_packed [Cout, 9*Cin] -> [B,Ho,Wo,Cout]."""
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    sh = 1 if (upsample2x or transposed2) else 0
    Hv, Wv = H << sh, W << sh
    Ho, Wo = ((Hv + 1) // 2, (Wv + 1) // 2) if stride == 2 else (Hv, Wv)
    y = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=BF)
    check(lib().pea_op_conv3x3(ptr(x), ptr(w_packed), ptr(y), B, H, W, Cin, Cout, stride, int(upsample2x),
                               int(transposed2), ptr(bias), ptr(rowvec),
                               rowvec.stride(0) if rowvec is not None else 0, ptr(res), stream_ptr()))
    return y


def conv3x3_ex(x, w_packed, bias=None, stride=1, pad_off=0, act=0, res=None, out=None, ldc=None):
    """pea_op_conv3x3_ex: x [B,H,W,Cs] bf16 NHWC with Cs the stored channel width; w_packed [Cout, 9*Cs].  pad_off=1 (stride 2):
    F.pad(x, (0,1,0,1)) then stride 2 without padding.  act: 0 none, 1 GELU, 2 SiLU, 3 quick-GELU.  out / ldc: a caller's
    buffer whose rows are ldc >= Cout wide (only the first Cout columns of a row are written); res [rows, ldres] likewise.
    Returns [B,Ho,Wo,Cout], or `out` as given."""
    B, H, W, Cs = x.shape
    Cout = w_packed.shape[0]
    Ho, Wo = ((H // 2, W // 2) if pad_off else ((H + 1) // 2, (W + 1) // 2)) if stride == 2 else (H, W)
    ldc = Cout if ldc is None else ldc
    if out is None:
        assert ldc == Cout
        out = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=BF)
    else:
        assert out.numel() >= (B * Ho * Wo - 1) * ldc + Cout
    check(lib().pea_op_conv3x3_ex(ptr(x), ptr(w_packed), w_packed.stride(0), ptr(out), ldc, B, H, W, Cs, Cout, stride, pad_off,
                                  act, ptr(bias), ptr(res), res.shape[-1] if res is not None else 0, stream_ptr()))
    return out


def pack_conv_subpixel(w_fp32, dgrad=False):
    """[Co,Ci,3,3] fp32 -> the sub-pixel form of conv3x3(nearest_2x(.)): [4,Co,4*Ci] (forward) or [Ci,16*Co] (data gradient)"""
    Co, Ci = w_fp32.shape[:2]
    out = torch.empty((Ci, 16 * Co) if dgrad else (4, Co, 4 * Ci), device=w_fp32.device, dtype=BF)
    check(lib().pea_op_pack_conv_subpixel(ptr(w_fp32.contiguous()), ptr(out), Co, Ci, int(dgrad), stream_ptr()))
    return out


def upconv_subpixel(x, w_packed, bias=None):
    """x [B,H,W,Cin] -> conv3x3(nearest_2x(x)) stored depth-to-space [B,H,W,4,Cout] (block (y&1)*2 + (x&1))"""
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[1]
    y = torch.empty(B, H, W, 4, Cout, device=x.device, dtype=BF)
    check(lib().pea_op_upconv_subpixel(ptr(x), ptr(w_packed), ptr(y), B, H, W, Cin, Cout, ptr(bias), stream_ptr()))
    return y


def upconv_subpixel_dgrad(dy_d2s, wt_packed, res=None):
    """dy [B,H,W,4,Cout] (depth-to-space) -> dx [B,H,W,Cin] (+ res)"""
    B, H, W, _, Cout = dy_d2s.shape
    Cin = wt_packed.shape[0]
    dx = torch.empty(B, H, W, Cin, device=dy_d2s.device, dtype=BF)
    check(lib().pea_op_upconv_subpixel_dgrad(ptr(dy_d2s), ptr(wt_packed), ptr(dx), B, H, W, Cin, Cout, ptr(res), stream_ptr()))
    return dx


def d2s_to_nhwc(y):
    """[B,H,W,4,C] depth-to-space -> [B,2H,2W,C]"""
    B, H, W, _, C = y.shape
    return y.view(B, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * H, 2 * W, C)


def nhwc_to_d2s(y):
    """[B,2H,2W,C] -> [B,H,W,4,C]"""
    B, H2, W2, C = y.shape
    return y.view(B, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2 // 2, W2 // 2, 4, C).contiguous()


def concat2(a, b, d2s_hw=None):
    """rows-wise channel concat; d2s_hw = (H, W): `a` is stored depth-to-space at that full resolution"""
    C1, C2 = a.shape[-1], b.shape[-1]
    rows = b.numel() // C2
    y = torch.empty(rows, C1 + C2, device=a.device, dtype=BF)
    H, W = d2s_hw if d2s_hw else (0, 0)
    check(lib().pea_op_concat2(ptr(a), C1, ptr(b), C2, ptr(y), rows, H, W, stream_ptr()))
    return y


def freeu_scratch_bytes(B, H, W, C2):
    """device bytes of the split reduction's partials behind `freeu_concat` (host only); 0: one slab per map, no scratch"""
    return int(lib().pea_op_freeu_scratch_bytes(B, H, W, C2))


def freeu_concat(a, b, s, bscale, d2s=False, y=None, coef=None, scratch=None):
    """FreeU on the operands of an up-path concat (diffusers 0.23 `apply_freeu`): b [B,H,W,C2] is the skip tensor, a [B,H,W,C1]
    the hidden state (d2s: stored depth-to-space, [B,H/2,W/2,4,C1]).  -> (y [B*H*W, C1+C2] = (bscale * a[..., :C1/2] |
    a[..., C1/2:] | fourier_filter(b, threshold 1, scale s)), coef fp32 [B,7,C2]: the filter's seven sums per channel map, or
    None with s == 1, which needs none).  y / coef / scratch: buffers to use instead of fresh ones."""
    B, H, W, C2 = b.shape
    C1 = a.shape[-1]
    if y is None:
        y = torch.empty(B * H * W, C1 + C2, device=b.device, dtype=BF)
    if s != 1.0:
        if coef is None:
            coef = torch.empty(B, 7, C2, device=b.device, dtype=torch.float32)
        nbytes = freeu_scratch_bytes(B, H, W, C2)
        if scratch is None and nbytes:
            scratch = torch.empty(nbytes // 4, device=b.device, dtype=torch.float32)
        check(lib().pea_op_freeu_coef(ptr(b), B, H, W, C2, ptr(coef), ptr(scratch), stream_ptr()))
    else:
        coef = None
    check(lib().pea_op_concat2_freeu(ptr(a), C1, ptr(b), C2, ptr(coef), ptr(y), B, H, W, float(s), float(bscale),
                                     H if d2s else 0, W if d2s else 0, stream_ptr()))
    return y, coef


def split2(dy, C1, C2, da=None, db=None, accum_a=False, accum_b=False, d2s_hw=None):
    rows = dy.numel() // (C1 + C2)
    H, W = d2s_hw if d2s_hw else (0, 0)
    check(lib().pea_op_split2(ptr(dy), C1, C2, ptr(da), int(accum_a), ptr(db), int(accum_b), rows, H, W, stream_ptr()))


def conv_in(x_nchw, w, bias):
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    y = torch.empty(B, H, W, Cout, device=x_nchw.device, dtype=BF)
    check(lib().pea_op_conv_in(ptr(x_nchw), ptr(w.contiguous()), ptr(bias), ptr(y), B, Cin, H, W, Cout, stream_ptr()))
    return y


def conv_in_gather(latents, mask, masked_latents, w, bias, B):
    """conv_in of an inpainting UNet over `cat([latents[b % lb], mask[b % cb], masked_latents[b % cb]], dim=1)` for b < B,
    without materialising the concatenation (bf16 NHWC out)."""
    lb, C, H, W = latents.shape
    cb = mask.shape[0]
    Cout = w.shape[0]
    y = torch.empty(B, H, W, Cout, device=latents.device, dtype=BF)
    check(lib().pea_op_conv_in_gather(ptr(latents), ptr(mask), ptr(masked_latents), ptr(w.contiguous()), ptr(bias), ptr(y), B,
                                      C, lb, cb, H, W, Cout, stream_ptr()))
    return y


def inpaint_prepare(image, mask):
    """image [N,3,H,W], mask [N,1,H,W] fp32 in [0, 1] -> (init_image = 2 image - 1, masked_image = init_image * (mask < 0.5),
    latent_mask = (mask >= 0.5)[:, :, ::8, ::8])"""
    N, _, H, W = image.shape
    init = torch.empty_like(image)
    masked = torch.empty_like(image)
    lmask = torch.empty(N, 1, H // 8, W // 8, device=image.device, dtype=torch.float32)
    check(lib().pea_op_inpaint_prepare(ptr(image), ptr(mask), N, H, W, ptr(init), ptr(masked), ptr(lmask), stream_ptr()))
    return init, masked, lmask


def pack_conv_out(w):
    Co, Ci = w.shape[:2]
    out = torch.empty(Co, 3, 3, Ci, device=w.device, dtype=torch.float32)
    check(lib().pea_op_pack_conv_out(ptr(w.contiguous()), ptr(out), Co, Ci, stream_ptr()))
    return out


def conv_out(x_nhwc, w_packed, bias):
    B, H, W, Cin = x_nhwc.shape
    Cout = w_packed.shape[0]
    y = torch.empty(B, Cout, H, W, device=x_nhwc.device, dtype=torch.float32)
    check(lib().pea_op_conv_out(ptr(x_nhwc), ptr(w_packed), ptr(bias), ptr(y), B, Cin, H, W, Cout, stream_ptr()))
    return y


def conv_out_dgrad(dy_nchw, w_packed, Cin):
    B, Cout, H, W = dy_nchw.shape
    dx = torch.empty(B, H, W, Cin, device=dy_nchw.device, dtype=BF)
    check(lib().pea_op_conv_out_dgrad(ptr(dy_nchw), ptr(w_packed), ptr(dx), B, Cin, H, W, Cout, stream_ptr()))
    return dx


def groupnorm_fwd(x, gamma, beta, groups=32, eps=1e-5, silu=False):
    B, HW, C = x.shape
    y = torch.empty_like(x)
    stats = torch.empty(B, groups, 2, device=x.device, dtype=torch.float32)
    scratch = torch.empty(lib().pea_op_groupnorm_scratch_bytes(B, HW, C, groups), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_groupnorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(stats), ptr(scratch), B, HW, C, groups,
                                     eps, int(silu), stream_ptr()))
    return y, stats


def groupnorm_bwd(x, dy, gamma, beta, stats, groups=32, silu=False, accum_into=None):
    B, HW, C = x.shape
    dx = accum_into if accum_into is not None else torch.empty_like(x)
    scratch = torch.empty(lib().pea_op_groupnorm_scratch_bytes(B, HW, C, groups), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_groupnorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(beta), ptr(stats), ptr(dx), ptr(scratch), B, HW,
                                     C, groups, int(silu), int(accum_into is not None), stream_ptr()))
    return dx


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """bf16 rows -> (bf16 rows, stats [R,2]); fp32 rows -> (fp32 rows, None)"""
    R, C = x.shape
    y = torch.empty_like(x)
    if x.dtype == torch.float32:
        check(lib().pea_op_layernorm_fwd_f32(ptr(x), ptr(gamma), ptr(beta), ptr(y), R, C, eps, stream_ptr()))
        return y, None
    stats = torch.empty(R, 2, device=x.device, dtype=torch.float32)
    check(lib().pea_op_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(stats), R, C, eps, stream_ptr()))
    return y, stats


def layernorm_bwd(x, dy, gamma, stats, want_param_grads=False, accum_into=None):
    R, C = x.shape
    dx = accum_into if accum_into is not None else torch.empty_like(x)
    dg = torch.zeros(C, device=x.device, dtype=torch.float32) if want_param_grads else None
    db = torch.zeros(C, device=x.device, dtype=torch.float32) if want_param_grads else None
    check(lib().pea_op_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(stats), ptr(dx), ptr(dg), ptr(db), R, C,
                                     int(accum_into is not None), stream_ptr()))
    return (dx, dg, db) if want_param_grads else dx


def gemm_qscale(a, w, bias=None, qscale_cols=0, qscale=1.0):
    """a @ w.T + bias with the first qscale_cols output columns multiplied by qscale (the Q block of a fused Q|K|V projection)"""
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=a.device, dtype=BF)
    check(lib().pea_op_gemm_qscale(ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias),
                                   qscale_cols, qscale, stream_ptr()))
    return out


def _attn_fwd_out(q, heads, scale, want_lse=True):
    """what every attention forward wrapper starts from -> B, Sq, C, the scale (default head_dim^-0.5), o, lse (or None)"""
    B, Sq, C = q.shape
    o = torch.empty(B, Sq, C, device=q.device, dtype=BF)
    lse = torch.empty(B, heads, Sq, device=q.device, dtype=torch.float32) if want_lse else None
    return B, Sq, C, (scale if scale is not None else (C // heads) ** -0.5), o, lse


def attention_fwd(q, k, v, heads, scale=None, q_prescaled=False):
    """q [B,Sq,H*D], k/v [B,Skv,H*D] bf16 (D = 64, 128 or 192: zero-padded heads) -> (o, lse [B,H,Sq]).
    q_prescaled: q already holds (unscaled q) * scale * log2(e)."""
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale)
    Skv = k.shape[1]
    nd = C // heads // 64
    fn = lib().pea_op_attention_fwd_prescaled if q_prescaled else lib().pea_op_attention_fwd
    check(fn(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, ptr(lse),
                                     B, heads, Sq, Skv, scale, nd, stream_ptr()))
    return o, lse


def attention_fwd_ip(q, k, v, k_ip, v_ip, heads, ip_scale, scale=None, q_prescaled=False, kv_len=None, want_lse=False,
                     causal=False):
    """Decoupled cross-attention of an image prompt in one launch (pea_op_attention_fwd_ip):
    softmax(scale q k^T) v + ip_scale * softmax(scale q k_ip^T) v_ip, head_dim 64.  q [B,Sq,H*64], k/v [B,Skv<=128,H*64],
    k_ip/v_ip [B,N<=32,>=H*64] bf16; kv_len (int32 [B]) masks text keys only; the lse is the text softmax's.
    -> o, or (o, lse [B,H,Sq]) with want_lse.  causal=True exists to be refused."""
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale, want_lse)
    check(lib().pea_op_attention_fwd_ip(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(k_ip), k_ip.stride(1),
                                        ptr(v_ip), v_ip.stride(1), ptr(o), C, ptr(lse), B, heads, Sq, k.shape[1], k_ip.shape[1],
                                        scale, float(ip_scale), int(q_prescaled), int(causal), ptr(kv_len), stream_ptr()))
    return (o, lse) if want_lse else o


class IpSets(ctypes.Structure):
    """pea_attn_ip_sets of include/pea_hip.h"""
    _fields_ = [("n_sets", ctypes.c_int), ("n_keys", ctypes.c_int * 4), ("weight", ctypes.c_float * 4),
                ("mask", ctypes.c_void_p * 4), ("mask_stride", ctypes.c_longlong * 4)]


def ip_sets(n_keys, scales, masks=None, mask_strides=None) -> IpSets:
    """the per-set table of attention_fwd_ipn.  The struct has room for four sets: of more, the first four are written and
    n_sets carries the real count, which the library refuses"""
    n_keys, scales = list(n_keys), list(scales)
    masks = [None] * len(n_keys) if masks is None else list(masks)
    if not (len(n_keys) == len(scales) == len(masks)):
        raise PeaError(f"ip_sets: {len(n_keys)} key counts, {len(scales)} scales, {len(masks)} masks")
    st = IpSets()
    st.n_sets = len(n_keys)
    for j, (n, w, m) in enumerate(list(zip(n_keys, scales, masks))[:4]):
        st.n_keys[j], st.weight[j] = int(n), float(w)
        if m is not None:
            assert m.dtype == torch.float32 and m.dim() == 2 and m.stride(1) == 1, "mask: fp32 [1|B, Sq]"
            st.mask[j] = m.data_ptr()
            st.mask_stride[j] = (0 if m.shape[0] == 1 else m.stride(0)) if mask_strides is None else int(mask_strides[j])
    return st


def attention_fwd_ipn(q, k, v, k2, v2, heads, n_keys, scales, masks=None, scale=None, q_prescaled=False, kv_len=None,
                      want_lse=False, causal=False, mask_strides=None):
    """Several image prompts in one launch (pea_op_attention_fwd_ipn):
    softmax(scale q k^T) v + sum_j scales[j] * masks[j][b, q] * softmax(scale q k2_j^T) v2_j, head_dim 64, one softmax per set.
    q [B,Sq,H*64], k/v [B,Skv<=128,H*64]; k2/v2 [B,sum(n_keys)<=32,>=H*64] bf16 hold the 1..4 sets back to back, set j in rows
    sum(n_keys[:j]) .. + n_keys[j].  masks: None, or per set None / fp32 [1,Sq] (shared by the batch) / [B,Sq], any finite
    values.  kv_len (int32 [B]) masks text keys only; the lse is the text softmax's.  -> o, or (o, lse [B,H,Sq]) with want_lse.
    causal=True and mask_strides (the batch stride handed over instead of the tensor's) exist to be refused."""
    sets = ip_sets(n_keys, scales, masks, mask_strides)
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale, want_lse)
    check(lib().pea_op_attention_fwd_ipn(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(k2), k2.stride(1),
                                         ptr(v2), v2.stride(1), ptr(o), C, ptr(lse), B, heads, Sq, k.shape[1], ctypes.byref(sets),
                                         scale, int(q_prescaled), int(causal), ptr(kv_len), stream_ptr()))
    return (o, lse) if want_lse else o


def attention_fwd_regions(q, k, v, heads, R, w, q_prescaled=False, scale=None):
    """Regional text prompts in one launch (pea_op_attention_fwd_regions):
    o[b, q] = sum_r w[b, r, q] * softmax(scale q k_r^T) v_r, head_dim 64, one softmax per region.  q [B,Sq,H*64] bf16; k/v
    [B,R*Lr,>=H*64] bf16 hold the R <= 4 regions back to back, region r in rows r*Lr .. (r+1)*Lr, Lr <= 96; w fp32 [1|B,R,Sq],
    any finite values, used as they are (`regional.region_weights` makes them sum to 1 per query).  -> o."""
    B, Sq, C, scale, o, _ = _attn_fwd_out(q, heads, scale)
    R = int(R)
    if C != heads * 64:
        raise PeaError(f"attention_fwd_regions: head_dim {C // heads} (the kernel is built for 64)")
    if w.dtype != torch.float32 or w.dim() != 3 or w.shape[1] != R or w.shape[2] != Sq:
        raise PeaError(f"attention_fwd_regions: w {tuple(w.shape)} {w.dtype}, expected fp32 [1|{B}, {R}, {Sq}]")
    Lr = k.shape[1] // R if R > 0 and k.shape[1] % R == 0 else -1
    if Lr < 0:
        raise PeaError(f"attention_fwd_regions: {k.shape[1]} key rows are no {R} regions of equal length")
    w = w.contiguous()
    check(lib().pea_op_attention_fwd_regions(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, B, heads, Sq,
                                             R, Lr, ptr(w), w.shape[0], scale, int(q_prescaled), stream_ptr()))
    return o


def attention_maps(q, k, heads, scale=None, q_prescaled=False, kv_len=None, out=None, accumulate=False):
    """Cross-attention heat maps in one launch (pea_op_attention_maps):
    m[b, key, q] = mean_h softmax_key(scale q_h k_h^T), head_dim 64, fp32, probabilities never rounded to bf16.  q [B,Sq,H*64] bf16;
    k [B,Skv,>=H*64] bf16, 1 <= Skv <= 128; kv_len: optional int32 [B] (keys at or past it map to exact zeros).  out: a contiguous
    fp32 buffer of at least B*Skv*Sq elements to write (or, accumulate=True, add) into; the maps are its first B*Skv*Sq elements.
    -> fp32 [B, Skv, Sq] (a view of `out` when given).  The same bits every run."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    if C != heads * 64:
        raise PeaError(f"attention_maps: head_dim {C // max(heads, 1)} (the kernel is built for 64)")
    scale = float(scale) if scale is not None else 64 ** -0.5
    n = B * Skv * Sq
    if out is None:
        if accumulate:
            raise PeaError("attention_maps: accumulate=True needs the buffer to add into (out=)")
        out = torch.empty(n, device=q.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n or out.device != q.device:
        raise PeaError(f"attention_maps: out {tuple(out.shape)} {out.dtype}, expected contiguous fp32 with at least {n} elements")
    if kv_len is not None:
        if kv_len.dtype != torch.int32 or kv_len.numel() != B:
            raise PeaError(f"attention_maps: kv_len {tuple(kv_len.shape)} {kv_len.dtype}, expected int32 [{B}]")
        kv_len = kv_len.contiguous()
    check(lib().pea_op_attention_maps(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(out), B, heads, Sq, Skv, scale, int(q_prescaled),
                                      ptr(kv_len), int(bool(accumulate)), stream_ptr()))
    return out.view(-1)[:n].view(B, Skv, Sq)


def attention_fwd_edit(q, k, v, heads, src, Mt, c, d, q_prescaled=False, scale=None):
    """Prompt-to-prompt editing in one launch over the batch (pea_op_attention_fwd_edit), head_dim 64, at most 96 keys, B <= 32:
    sample b with s = src[b] >= 0:  o[b] = (c[b] * (softmax(scale q[s] k[s]^T) Mt[b]^T) + d[b] * softmax(scale q[b] k[b]^T)) v[b],
    src[b] < 0: plain attention (the sample's table rows are never read).  q [B,Sq,H*64], k/v [B,Skv,>=H*64] bf16; src: B ints
    (host); Mt bf16 [B,Skv,ldm>=Skv] (row = target key, column = source key; ldm a multiple of 8); c, d fp32 [B,Skv].  -> o."""
    B, Sq, C, scale, o, _ = _attn_fwd_out(q, heads, scale, want_lse=False)
    if C != heads * 64:
        raise PeaError(f"attention_fwd_edit: head_dim {C // heads} (the kernel is built for 64)")
    Skv = k.shape[1]
    src = [int(x) for x in (src.tolist() if hasattr(src, "tolist") else src)]
    if len(src) != B:
        raise PeaError(f"attention_fwd_edit: {len(src)} sources for a batch of {B}")
    hsrc = (ctypes.c_int * max(B, 1))(*src)
    ldm = 0
    if Mt is not None:
        if Mt.dtype != BF or Mt.dim() != 3 or Mt.shape[0] != B or Mt.shape[1] != Skv or Mt.stride(2) != 1 or Mt.stride(0) != Skv * Mt.stride(1):
            raise PeaError(f"attention_fwd_edit: Mt {tuple(Mt.shape)} {Mt.dtype}, expected bf16 [{B}, {Skv}, >= {Skv}] with dense rows")
        ldm = Mt.stride(1)
    for name, t in (("c", c), ("d", d)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B, Skv) or not t.is_contiguous()):
            raise PeaError(f"attention_fwd_edit: {name} {tuple(t.shape)} {t.dtype}, expected fp32 [{B}, {Skv}]")
    check(lib().pea_op_attention_fwd_edit(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, B, heads, Sq, Skv,
                                          hsrc, None if Mt is None else ctypes.c_void_p(Mt.data_ptr()), ldm, ptr(c), ptr(d), scale,
                                          int(q_prescaled), stream_ptr()))
    return o


def _rows(name, t, B, S, who):
    """a [B, S, >= C] bf16 operand whose rows may sit inside a wider buffer (the Q | K | V projection's) -> its address"""
    if t.dtype != BF or t.dim() != 3 or t.shape[0] != B or t.shape[1] != S or t.stride(2) != 1 or t.stride(0) != S * t.stride(1):
        raise PeaError(f"{who}: {name} {tuple(t.shape)} {t.dtype} strides {t.stride()}, expected bf16 [{B}, {S}, C] with dense samples")
    return ctypes.c_void_p(t.data_ptr())


def _host_ref(ref, B, who):
    ref = [int(x) for x in (ref.tolist() if hasattr(ref, "tolist") else ref)]
    if len(ref) != B:
        raise PeaError(f"{who}: {len(ref)} references for a batch of {B}")
    return (ctypes.c_int * max(B, 1))(*ref)


def attn_adain_coef(q, k, heads, ref, q_prescaled=False, scale=None, adain_queries=True, adain_keys=True, out=None):
    """The AdaIN coefficients of StyleAligned sharing (pea_op_attn_adain_coef), head_dim 64: q, k [B,S,H*64] bf16 (rows may be
    column slices of a wider buffer); ref: B ints (host), ref[b] >= 0 the style reference of target b.  -> fp32 [B,4,H*64] =
    (a_q, s_q, a_k, s_k) with a = sigma(X[ref]) / sigma(X[b]), s = mu(X[ref]) - a mu(X[b]) over the tokens; rows of plain samples
    are left as they were (zeros in a fresh buffer).  q_prescaled: q holds q * scale * log2(e); the variance epsilon follows."""
    B, S, C = q.shape
    who = "attn_adain_coef"
    if C != heads * 64:
        raise PeaError(f"{who}: head_dim {C // heads} (the kernel is built for 64)")
    scale = scale if scale is not None else 64 ** -0.5
    href = _host_ref(ref, B, who)
    coef = out if out is not None else torch.zeros(B, 4, C, device=q.device, dtype=torch.float32)
    nbytes = int(lib().pea_op_attn_adain_scratch_bytes(B, heads, S))
    scratch = torch.empty(max(nbytes, 16) // 4, device=q.device, dtype=torch.float32)
    check(lib().pea_op_attn_adain_coef(_rows("q", q, B, S, who), q.stride(1), _rows("k", k, B, S, who), k.stride(1), B, heads, S, href,
                                       scale, int(q_prescaled), int(adain_queries), int(adain_keys),
                                       ptr(coef), ptr(scratch), stream_ptr()))
    return coef


def attention_fwd_shared(q, k, v, heads, ref, coef, q_prescaled=False, scale=None, shared_score_scale=1.0, shared_score_shift=0.0):
    """StyleAligned shared self-attention in one launch over the batch (pea_op_attention_fwd_shared), head_dim 64, B <= 32:
    target b with r = ref[b] >= 0 and coef[b] = (a_q, s_q, a_k, s_k):  q' = a_q q + s_q,
      o[b] = softmax([scale q' (a_k k[b] + s_k)^T | shared_score_scale scale q' k[r]^T + shared_score_shift]) [v[b]; v[r]],
    ref[b] < 0: plain attention, the bits of attention_fwd (the sample's coef row is never read).  q, k, v [B,S,H*64] bf16 (rows
    may be column slices of a wider buffer); coef fp32 [B,4,H*64] from attn_adain_coef, or None while no sample is a target.  -> o."""
    B, Sq, C, scale, o, _ = _attn_fwd_out(q, heads, scale, want_lse=False)
    who = "attention_fwd_shared"
    Skv = k.shape[1]
    href = _host_ref(ref, B, who)
    if coef is not None and (coef.dtype != torch.float32 or tuple(coef.shape) != (B, 4, C) or not coef.is_contiguous()):
        raise PeaError(f"{who}: coef {tuple(coef.shape)} {coef.dtype}, expected fp32 [{B}, 4, {C}]")
    check(lib().pea_op_attention_fwd_shared(_rows("q", q, B, Sq, who), q.stride(1), _rows("k", k, B, Skv, who), k.stride(1),
                                            _rows("v", v, B, Skv, who), v.stride(1), ptr(o), C, B, heads, Sq, Skv, href, ptr(coef), scale,
                                            int(q_prescaled), float(shared_score_scale), float(shared_score_shift), C // heads // 64,
                                            stream_ptr()))
    return o


def attention_fwd_fewq(q, k, v, k2=None, v2=None, heads=1, scale=None, q_prescaled=False, want_lse=False, kv_rows=None,
                       kv2_rows=None):
    """Few-query attention over the union of two key sets in one launch (pea_op_attention_fwd_fewq):
    softmax(scale [q k^T | q k2^T]) [v ; v2], ONE softmax, head_dim 64.  q [B,Sq<=32,H*64], k/v [B,Skv,>=H*64], k2/v2
    [B,N<=32,>=H*64] bf16 or both None.  kv_rows / kv2_rows: use only the first so many rows of each sample of k, v / k2, v2
    (buffers with rows to spare: the batch stride stays that of the tensor only for B == 1).  -> o, or (o, lse [B,H,Sq])."""
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale if scale is not None else 0.125, want_lse)
    Skv = k.shape[1] if kv_rows is None else kv_rows
    Skv2 = 0 if k2 is None else (k2.shape[1] if kv2_rows is None else kv2_rows)
    check(lib().pea_op_attention_fwd_fewq(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(k2),
                                          0 if k2 is None else k2.stride(1), ptr(v2), 0 if v2 is None else v2.stride(1), ptr(o), C,
                                          ptr(lse), B, heads, Sq, Skv, Skv2, scale, C // heads // 64, int(q_prescaled), stream_ptr()))
    return (o, lse) if want_lse else o


def attention_fwd_masked(q, k, v, heads, causal=False, kv_len=None, scale=None, want_lse=False):
    """text-encoder attention: head_dim 64, optional causal mask and per-sample key counts (int32 [B])
    -> o, or (o, lse [B,H,Sq]) with want_lse"""
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale, want_lse)
    Skv = k.shape[1]
    check(lib().pea_op_attention_fwd_masked(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, ptr(lse),
                                            B, heads, Sq, Skv, scale, int(causal), ptr(kv_len), stream_ptr()))
    return (o, lse) if want_lse else o


def attention_bias_pitch(Skv):
    """row pitch (elements) of the score bias of attention_fwd_text: whole 64-key tiles"""
    return (Skv + 63) // 64 * 64


def attention_fwd_text(q, k, v, heads, scale=None, q_prescaled=False, causal=False, kv_len=None, bias=None, want_lse=True):
    """pea_op_attention_fwd_text: everything the forward launcher takes at head_dim 64.  kv_len int32 [B] (values 1..Skv);
    bias fp32 [H, Sq, attention_bias_pitch(Skv)], contiguous, in the log2 domain (natural-log bias x log2 e), shared by the
    batch -- the columns past Skv are read but never used.  -> (o, lse [B,H,Sq]), or o alone without want_lse."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (heads, Sq, attention_bias_pitch(Skv))
                             or not bias.is_contiguous()):
        raise PeaError(f"attention_fwd_text: bias must be contiguous fp32 [{heads}, {Sq}, {attention_bias_pitch(Skv)}]")
    B, Sq, C, scale, o, lse = _attn_fwd_out(q, heads, scale, want_lse)
    check(lib().pea_op_attention_fwd_text(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, ptr(lse),
                                          B, heads, Sq, Skv, scale, int(q_prescaled), int(causal), ptr(kv_len), ptr(bias),
                                          stream_ptr()))
    return (o, lse) if want_lse else o


def attention_bwd(q, k, v, o, do, lse, heads, scale=None, q_prescaled=False):
    """-> (dq, dk, dv); with q_prescaled dq is still the gradient w.r.t. the UNSCALED q"""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    nd = C // heads // 64
    scale = scale if scale is not None else (C // heads) ** -0.5
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(2, B, heads, Sq, device=q.device, dtype=torch.float32)     # scratch: -delta and -lse*log2(e) per row
    nb = lib().pea_op_attention_bwd_scratch_bytes(B, heads, Sq, Skv, nd)
    scratch = torch.empty(nb, device=q.device, dtype=torch.uint8) if nb else None
    fn = lib().pea_op_attention_bwd_prescaled if q_prescaled else lib().pea_op_attention_bwd
    check(fn(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, ptr(do),
                                     C, ptr(lse), ptr(delta), ptr(dq), C, ptr(dk), C, ptr(dv), C, B, heads, Sq, Skv,
                                     scale, 0, 0, nd, ptr(scratch), stream_ptr()))
    return dq, dk, dv


def attention_bwd_masked(q, k, v, o, do, lse, heads, scale=None, q_prescaled=False, kv_len=None, use_scratch=True):
    """pea_op_attention_bwd_masked -> (dq, dk, dv): attention_bwd with per-sample key counts (int32 [B], values 1..Skv, those
    of the forward that made o and lse); rows >= kv_len[b] of dk / dv come back as zeros.  use_scratch=False: without the
    query-split scratch."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    nd = C // heads // 64
    scale = scale if scale is not None else (C // heads) ** -0.5
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(2, B, heads, Sq, device=q.device, dtype=torch.float32)
    nb = lib().pea_op_attention_bwd_scratch_bytes(B, heads, Sq, Skv, nd) if use_scratch else 0
    scratch = torch.empty(nb, device=q.device, dtype=torch.uint8) if nb else None
    check(lib().pea_op_attention_bwd_masked(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(v), v.stride(1), ptr(o), C, ptr(do),
                                            C, ptr(lse), ptr(delta), ptr(dq), C, ptr(dk), C, ptr(dv), C, B, heads, Sq, Skv,
                                            scale, 0, 0, nd, ptr(scratch), int(q_prescaled), ptr(kv_len), stream_ptr()))
    return dq, dk, dv


def geglu_fwd(hg):
    rows, two = hg.shape
    y = torch.empty(rows, two // 2, device=hg.device, dtype=BF)
    check(lib().pea_op_geglu_fwd(ptr(hg), ptr(y), rows, two // 2, stream_ptr()))
    return y


def geglu_bwd(hg, dy):
    d = torch.empty_like(hg)
    check(lib().pea_op_geglu_bwd(ptr(hg), ptr(dy), ptr(d), hg.shape[0], hg.shape[1] // 2, stream_ptr()))
    return d


def sumpool2(x):
    B, H2, W2, C = x.shape
    y = torch.empty(B, H2 // 2, W2 // 2, C, device=x.device, dtype=BF)
    check(lib().pea_op_sumpool2(ptr(x), ptr(y), B, H2 // 2, W2 // 2, C, 0, stream_ptr()))
    return y


def timestep_embed(t_f32, dim):
    y = torch.empty(t_f32.numel(), dim, device=t_f32.device, dtype=BF)
    check(lib().pea_op_timestep_embed(ptr(t_f32), ptr(y), t_f32.numel(), dim, stream_ptr()))
    return y


def add_noise(x0, eps, t, ac):
    xt = torch.empty_like(x0)
    check(lib().pea_op_add_noise(ptr(x0), ptr(eps), ptr(t), ptr(ac), ptr(xt), x0.shape[0], x0[0].numel(), stream_ptr()))
    return xt


def kd_loss(taps_s: Sequence[torch.Tensor], taps_t: Sequence[torch.Tensor], eps_s, eps, eps_t, zh,
            feat_weight=0.1, nan_guard=False, grad_scale=1.0, want_grads=True):
    """-> (losses fp32[4] device, [dL/dtap_s], dL/d eps_s).  taps: bf16 [B, ...] paired layouts."""
    n = len(taps_s)
    B = eps_s.shape[0]
    dev = eps_s.device
    dt = [torch.empty_like(t) for t in taps_s] if want_grads else []
    de = torch.empty_like(eps_s) if want_grads else None
    arr = ctypes.c_void_p * max(n, 1)
    a_s = arr(*[t.data_ptr() for t in taps_s])
    a_t = arr(*[t.data_ptr() for t in taps_t])
    a_d = arr(*[t.data_ptr() for t in dt]) if want_grads else None
    per = (ctypes.c_longlong * max(n, 1))(*[t[0].numel() for t in taps_s])
    losses = torch.empty(4, device=dev, dtype=torch.float32)
    ws = torch.empty(lib().pea_op_kd_loss_workspace_bytes(n, per, eps_s[0].numel(), B), device=dev, dtype=torch.uint8)
    check(lib().pea_op_kd_loss(n, a_s, a_t, a_d, per, ptr(eps_s), ptr(eps), ptr(eps_t), ptr(de), eps_s[0].numel(),
                               ptr(zh), B, feat_weight, int(nan_guard), grad_scale, ptr(losses), ptr(ws),
                               stream_ptr()))
    return losses, dt, de


def adamw_(w, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    check(lib().pea_op_adamw(ptr(w), ptr(g), ptr(m), ptr(v), w.numel(), lr, beta1, beta2, eps, weight_decay, step,
                             grad_scale, stream_ptr()))


# ---- inference denoise-loop glue (tests/test_sdxl_zh.py:376-406)
def cfg_combine(noise_pred2, guidance_scale, guidance_rescale=0.0):
    """`u, t = noise_pred.chunk(2); u + g * (t - u)` (:394-395) and, for guidance_rescale > 0, `rescale_noise_cfg`
    (:44-56).  noise_pred2: fp32 [2B, ...] on the GPU, unconditional half first."""
    assert noise_pred2.dtype == torch.float32 and noise_pred2.shape[0] % 2 == 0
    B = noise_pred2.shape[0] // 2
    x = noise_pred2.contiguous()
    out = torch.empty((B,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    ws = None
    if guidance_rescale > 0.0:
        ws = torch.empty(lib().pea_op_cfg_combine_workspace_bytes(B), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_cfg_combine(ptr(x), ptr(out), B, out[0].numel(), float(guidance_scale), float(guidance_rescale),
                                   ptr(ws), stream_ptr()))
    return out


# ---- self-attention guidance (Hong et al. 2023; pea_diffusion_amd/sag.py is the loop)
def attention_colsum_groups(B, heads, Sq, Skv):
    """G of `attention_colsum`: how many head groups its launch cuts the heads into (pea_op_attention_colsum_groups)"""
    g = int(lib().pea_op_attention_colsum_groups(int(B), int(heads), int(Sq), int(Skv)))
    if g < 1:
        check(g)
    return g


def attention_colsum(q, k, lse, heads, scale=None, q_prescaled=False, out=None):
    """Column sums of a softmax in one launch (pea_op_attention_colsum), head_dim 64, no V / O, probabilities fp32 throughout:
    part[b, g, key] = (1 / H) sum_{h in group g} sum_q exp(scale q_h . k_h - lse[b, h, q]).  q [B,Sq,H*64], k [B,Skv,>=H*64] bf16;
    lse fp32 [B,H,Sq] (natural log, as `attention_fwd(..., want_lse=True)` returns it).  out: a contiguous fp32 buffer of at least
    B*G*Skv elements.  -> fp32 [B, G, Skv] with G = attention_colsum_groups(B, heads, Sq, Skv); the column sum of the head-mean
    softmax is `part.sum(1)` in ascending g (what `sag_degrade` adds itself).  The same bits every run."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    if C != heads * 64:
        raise PeaError(f"attention_colsum: head_dim {C // max(heads, 1)} (the kernel is built for 64)")
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (B, heads, Sq) or not lse.is_contiguous()):
        raise PeaError(f"attention_colsum: lse {tuple(lse.shape)} {lse.dtype}, expected contiguous fp32 [{B}, {heads}, {Sq}]")
    scale = float(scale) if scale is not None else 64 ** -0.5
    G = attention_colsum_groups(B, heads, Sq, Skv)
    n = B * G * Skv
    if out is None:
        out = torch.empty(n, device=q.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < n or out.device != q.device:
        raise PeaError(f"attention_colsum: out {tuple(out.shape)} {out.dtype}, expected contiguous fp32 with at least {n} elements")
    check(lib().pea_op_attention_colsum(ptr(q), q.stride(1), ptr(k), k.stride(1), ptr(lse), ptr(out), B, heads, Sq, Skv, scale,
                                        int(q_prescaled), stream_ptr()))
    return out.view(-1)[:n].view(B, G, Skv)


def sag_degrade(latents, eps, part, map_hw, iy, ix, c_x, c_e, o_b, o_e):
    """Mask, blur and degraded model input of self-attention guidance in one launch (pea_op_sag_degrade).  latents, eps fp32
    [B,C,H,W]; part fp32 [B,G,h*w] (`attention_colsum` / `HipUNet.sag_colsum`), map_hw = (h, w); iy int32 [H], ix int32 [W]
    (`sag.nearest_tables`, on the device).  m = (part summed over g in ascending order) > 1 at (iy[y], ix[x]);
    x0 = c_x x + c_e eps; -> o_b (m ? gaussian9x9_reflect(x0) : x0) + o_e eps, fp32 [B,C,H,W]."""
    B, C, H, W = latents.shape
    h, w = int(map_hw[0]), int(map_hw[1])
    for t in (latents, eps, part):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise PeaError("sag_degrade: latents, eps and part are contiguous fp32 tensors")
    if eps.shape != latents.shape or part.dim() != 3 or part.shape[0] != B or part.shape[2] != h * w:
        raise PeaError(f"sag_degrade: eps {tuple(eps.shape)}, part {tuple(part.shape)} for latents {tuple(latents.shape)} and a {h} x {w} map")
    if iy.dtype != torch.int32 or ix.dtype != torch.int32 or iy.numel() != H or ix.numel() != W:
        raise PeaError(f"sag_degrade: index tables int32 [{H}] and [{W}]")
    out = torch.empty_like(latents)
    check(lib().pea_op_sag_degrade(ptr(latents), ptr(eps), ptr(part), part.shape[1], h, w, ptr(iy.contiguous()), ptr(ix.contiguous()),
                                   ptr(out), B, C, H, W, float(c_x), float(c_e), float(o_b), float(o_e), stream_ptr()))
    return out


def cfg_sag_combine(noise_pred, noise_pred_deg, guidance_scale, sag_scale, do_cfg=True):
    """The guidance combine of self-attention guidance (pea_op_cfg_sag_combine).  do_cfg: noise_pred fp32 [2B, ...],
    unconditional half first -> u + g (t - u) + s (u - d), at s = 0 the bits of `cfg_combine`.  Otherwise noise_pred [B, ...]
    -> e + s (e - d).  noise_pred_deg (d): fp32 [B, ...], the prediction on the degraded input."""
    x, d = noise_pred.contiguous(), noise_pred_deg.contiguous()
    B = d.shape[0]
    if x.dtype != torch.float32 or d.dtype != torch.float32 or x.shape[0] != (2 * B if do_cfg else B) or x.shape[1:] != d.shape[1:]:
        raise PeaError(f"cfg_sag_combine: noise_pred {tuple(x.shape)} {x.dtype}, degraded {tuple(d.shape)} {d.dtype}, do_cfg={do_cfg}")
    out = torch.empty_like(d)
    check(lib().pea_op_cfg_sag_combine(ptr(x), ptr(d), ptr(out), B, d[0].numel(), int(bool(do_cfg)), float(guidance_scale),
                                       float(sag_scale), stream_ptr()))
    return out


# ---- perturbed-attention / smoothed-energy guidance (Ahn et al. 2024; Hong 2024; pea_diffusion_amd/pag.py is the loop)
def query_blur_(qkv, grid, Mh, Mw, cols=None, col0=0):
    """In place (pea_op_query_blur): the columns [col0, col0 + cols) of the bf16 rows qkv [n, h*w, ld] read as n grids of
    h x w tokens and blurred per channel, Q~ = Mh . Q . Mw^T.  Mh fp32 [h, h], Mw fp32 [w, w] on the device
    (`pag.blur_matrix`).  cols: a multiple of 64 (default: all of ld); every other column keeps its bits.  -> qkv."""
    n, S, ld = qkv.shape
    h, w = int(grid[0]), int(grid[1])
    cols = ld - col0 if cols is None else int(cols)
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or S != h * w:
        raise PeaError(f"query_blur_: rows {tuple(qkv.shape)} {qkv.dtype}, expected contiguous bf16 [n, {h * w}, ld] for a {h} x {w} grid")
    for m, side in ((Mh, h), (Mw, w)):
        if m.dtype != torch.float32 or tuple(m.shape) != (side, side) or not m.is_contiguous() or m.device != qkv.device:
            raise PeaError(f"query_blur_: blur matrix {tuple(m.shape)} {m.dtype}, expected contiguous fp32 [{side}, {side}] on the device")
    check(lib().pea_op_query_blur(ptr(qkv), ld, int(col0), n, h, w, cols, ptr(Mh), ptr(Mw), stream_ptr()))
    return qkv


def attn_identity(v, out, cols, col0=0):
    """The identity attention O = V (pea_op_attn_identity): `cols` bf16 columns from column col0 of v [..., ldv] into the
    first `cols` columns of out [..., ldo], row by row; every other column of out keeps its bits.  -> out."""
    if v.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or not v.is_contiguous() or not out.is_contiguous():
        raise PeaError("attn_identity: v and out are contiguous bf16 tensors")
    rows = v.numel() // v.shape[-1]
    if out.numel() // out.shape[-1] != rows:
        raise PeaError(f"attn_identity: {rows} rows of v, {out.numel() // out.shape[-1]} of out")
    check(lib().pea_op_attn_identity(ptr(v), v.shape[-1], int(col0), ptr(out), out.shape[-1], rows, int(cols), stream_ptr()))
    return out


def cfg_pag_combine(noise_pred, guidance_scale, pag_scale, guidance_rescale=0.0, do_cfg=True):
    """The guidance combine with a perturbed third (pea_op_cfg_pag_combine).  do_cfg: noise_pred fp32 [3B, ...] =
    [uncond | text | perturbed] -> u + g (t - u) + s (t - p), then `rescale_noise_cfg` against t when guidance_rescale > 0;
    at s = 0 the bits of `cfg_combine` on the first 2B samples.  Otherwise noise_pred [2B, ...] = [text | perturbed]
    -> t + s (t - p)."""
    x = noise_pred.contiguous()
    k = 3 if do_cfg else 2
    if x.dtype != torch.float32 or x.shape[0] % k:
        raise PeaError(f"cfg_pag_combine: noise_pred {tuple(x.shape)} {x.dtype}, expected fp32 with a batch of {k} B (do_cfg={do_cfg})")
    B = x.shape[0] // k
    out = torch.empty((B,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    ws = None
    if do_cfg and guidance_rescale > 0.0:
        ws = torch.empty(lib().pea_op_cfg_combine_workspace_bytes(B), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_cfg_pag_combine(ptr(x), ptr(out), B, out[0].numel(), int(bool(do_cfg)), float(guidance_scale), float(pag_scale),
                                       float(guidance_rescale), ptr(ws), stream_ptr()))
    return out


# ---- semantic guidance (Brack et al. 2023; pea_diffusion_amd/sega.py is the loop)
def _sega_operands(op, eps, edit_scale, quantile, weight):
    """B, C, hw, K and the three host arrays of the SEGA entries, for eps fp32 [(2 + K) B, C, ...]"""
    K = len(edit_scale)
    if not (K >= 1 and len(quantile) == K and len(weight) == K):
        raise PeaError(f"{op}: {K} edit scales, {len(quantile)} quantiles, {len(weight)} weights (one each per concept, at least one)")
    if eps.dtype != torch.float32 or not eps.is_contiguous() or eps.dim() < 3 or eps.shape[0] % (2 + K):
        raise PeaError(f"{op}: noise_pred {tuple(eps.shape)} {eps.dtype}, expected contiguous fp32 [(2 + {K}) B, C, ...] "
                       "([uncond | text | edit_1 .. edit_K])")
    B, C = eps.shape[0] // (2 + K), eps.shape[1]
    arr = lambda v: (ctypes.c_float * K)(*[float(a) for a in v])
    return B, C, eps[0, 0].numel(), K, arr(edit_scale), arr(quantile), arr(weight)


def abs_diff_quantile(noise_pred, edit_scale, quantile, weight, want_bounds=False):
    """The per-group cut of semantic guidance in one launch (pea_op_abs_diff_quantile).  noise_pred fp32 [(2 + K) B, C, h, w] =
    [uncond | text | edit_1 .. edit_K]; edit_scale, quantile, weight: K numbers each.  -> thr fp32 [K, B, C] =
    `torch.quantile((s_c (e_c - u)).abs().flatten(2), q_c, dim=2)` (+inf for a concept of weight 0), and with want_bounds the
    two order statistics it interpolates, fp32 [K, B, C, 2]."""
    B, C, hw, K, s, q, w = _sega_operands("abs_diff_quantile", noise_pred, edit_scale, quantile, weight)
    thr = torch.empty(K, B, C, device=noise_pred.device, dtype=torch.float32)
    bounds = torch.empty(K, B, C, 2, device=noise_pred.device, dtype=torch.float32) if want_bounds else None
    check(lib().pea_op_abs_diff_quantile(ptr(noise_pred), ptr(thr), ptr(bounds), B, C, hw, K, s, q, w, stream_ptr()))
    return (thr, bounds) if want_bounds else thr


def sega_workspace(B, C, K, device):
    """the workspace `cfg_sega_combine` takes (pea_op_sega_workspace_bytes): allocate once before a loop"""
    return torch.empty(lib().pea_op_sega_workspace_bytes(int(B), int(C), int(K)), device=device, dtype=torch.uint8)


def cfg_sega_combine(noise_pred, momentum, guidance_scale, edit_scale, quantile, weight, warm, momentum_scale=0.1, momentum_beta=0.4,
                     workspace=None, out=None):
    """One step of semantic guidance in two launches (pea_op_cfg_sega_combine).  noise_pred fp32 [(2 + K) B, C, h, w] =
    [uncond | text | edit_1 .. edit_K]; momentum fp32 [B, C, h, w], updated IN PLACE; edit_scale (signed), quantile, weight,
    warm: K numbers each.  m_c = d_c where |d_c| >= its group's quantile else 0 with d_c = s_c (e_c - u);
    -> u + g (t - u) + (any warm ? sum_c warm_c w_c m_c + mu mom : 0), fp32 [B, C, h, w], and
    mom <- beta mom + (1 - beta) (sum_c w_c m_c + mu mom).  Every weight 0 and a zero momentum: the bits of `cfg_combine`."""
    B, C, hw, K, s, q, w = _sega_operands("cfg_sega_combine", noise_pred, edit_scale, quantile, weight)
    if len(warm) != K:
        raise PeaError(f"cfg_sega_combine: {len(warm)} warm flags for {K} concepts")
    shape = (B,) + tuple(noise_pred.shape[1:])
    for name, t in (("momentum", momentum), ("out", out)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != noise_pred.device):
            raise PeaError(f"cfg_sega_combine: {name} {tuple(t.shape)} {t.dtype}, expected contiguous fp32 {shape} on the device")
    if momentum is None:
        raise PeaError("cfg_sega_combine: the momentum buffer is missing")
    if out is None:
        out = torch.empty(shape, device=noise_pred.device, dtype=torch.float32)
    if workspace is None:
        workspace = sega_workspace(B, C, K, noise_pred.device)
    flags = (ctypes.c_int * K)(*[int(bool(a)) for a in warm])
    check(lib().pea_op_cfg_sega_combine(ptr(noise_pred), ptr(momentum), ptr(out), B, C, hw, K, float(guidance_scale), s, q, w, flags,
                                        float(momentum_scale), float(momentum_beta), ptr(workspace), stream_ptr()))
    return out


def dpm_update_(sample, eps, x0_prev, alpha_s, sigma_s, c_s, c_0, c_1):
    """In place: x0 = (sample - sigma_s*eps)/alpha_s; sample <- c_s*sample + c_0*x0 + c_1*x0_prev; x0_prev <- x0."""
    for t in (sample, eps, x0_prev):
        assert t.dtype == torch.float32 and t.is_contiguous()
    check(lib().pea_op_dpm_update(ptr(sample), ptr(eps), ptr(x0_prev), sample.numel(), float(alpha_s), float(sigma_s),
                                  float(c_s), float(c_0), float(c_1), stream_ptr()))
    return sample


def lcm_update_(sample, eps, noise, kx, ke, c_prev, c_noise, denoised=None):
    """In place, one LCMScheduler.step: d = kx*sample + ke*eps; sample <- c_prev*d + c_noise*noise (noise None: c_prev*d);
    `denoised` (optional, same shape) receives d."""
    for t in (sample, eps, noise, denoised):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == sample.numel())
    check(lib().pea_op_lcm_update(ptr(sample), ptr(eps), ptr(noise), ptr(denoised), sample.numel(), float(kx), float(ke),
                                  float(c_prev), float(c_noise), stream_ptr()))
    return sample


def euler_update_(sample, eps, noise, model_in, k_e, k_n, k_s, dup=1):
    """One Euler / Euler-ancestral step fused with the next model input (pea_op_euler_update): in place
    sample <- sample + k_e*eps (+ k_n*noise); model_in[d] <- sample * k_s for d < dup (model_in None: skipped).
    eps None is the entry form: sample is only read, model_in = sample * k_s."""
    n = sample.numel()
    for t in (sample, eps, noise):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    assert model_in is None or (model_in.dtype == torch.float32 and model_in.is_contiguous() and model_in.numel() == dup * n)
    check(lib().pea_op_euler_update(ptr(sample), ptr(eps), ptr(noise), ptr(model_in), n, int(dup), float(k_e), float(k_n),
                                    float(k_s), stream_ptr()))
    return sample


# ---- MultiDiffusion panoramas (Bar-Tal et al. 2023; pea_diffusion_amd/panorama.py is the loop)
def _view_slots(views, vb):
    if not 1 <= len(views) <= vb:
        raise PeaError(f"{len(views)} views for a chunk of {vb} slots (1..vb)")
    return (ctypes.c_int * (3 * len(views)))(*[int(v) for view in views for v in view])


def views_gather(canvas, views, vb, window, k_s=1.0, dup=1, wrap_x=False, out=None):
    """Canvas to UNet batch in one launch (pea_op_views_gather).  canvas fp32 [N,C,Hc,Wc]; views: the (n, y0, x0) of the chunk's
    real slots, at most vb; window = (h, w).  -> fp32 [dup * vb, C, h, w]: out[d * vb + s] = crop of slot s * k_s; the slots past
    len(views) repeat the last view."""
    N, C, Hc, Wc = canvas.shape
    h, w = int(window[0]), int(window[1])
    if canvas.dtype != torch.float32 or not canvas.is_contiguous():
        raise PeaError("views_gather: the canvas is a contiguous fp32 tensor")
    if out is None:
        out = torch.empty(int(dup) * int(vb), C, h, w, device=canvas.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != int(dup) * int(vb) * C * h * w or out.device != canvas.device:
        raise PeaError(f"views_gather: out {tuple(out.shape)} {out.dtype}, expected contiguous fp32 [{int(dup) * int(vb)}, {C}, {h}, {w}]")
    check(lib().pea_op_views_gather(ptr(canvas), ptr(out), _view_slots(views, vb), len(views), int(vb), int(dup), N, C, Hc, Wc, h, w,
                                    int(bool(wrap_x)), float(k_s), stream_ptr()))
    return out


def views_merge_(canvas, eps, views, wy, wx, total, dup=1, guidance_scale=0.0, factor=None, first=True, last=True, wrap_x=False):
    """UNet batch into the canvas in one launch, in place (pea_op_views_merge).  eps fp32 [dup * vb, C, h, w] ([uncond | text] for
    dup 2); views: the (n, y0, x0) of the chunk's real slots (the slots behind them are not read).  Each canvas element gets the
    sum, in ascending slot order, of wy[i] wx[j] e over the views that cover it, e = u + g (t - u) (`cfg_combine`'s expression) for
    dup 2 and eps for dup 1, times factor[s] (`cfg_rescale_factors`) when given.  first: the sum starts at 0 (and elements outside
    the chunk's views are set to 0), else at what the canvas holds; last: divided by total [N,Hc,Wc] in the same launch.
    wy [h], wx [w], total: fp32 on the device.  -> canvas."""
    N, C, Hc, Wc = canvas.shape
    h, w = eps.shape[-2:]
    vb = eps.shape[0] // int(dup)
    for t in (canvas, eps, wy, wx, total, factor):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != canvas.device):
            raise PeaError("views_merge_: canvas, eps, wy, wx, total and factor are contiguous fp32 tensors on one device")
    if eps.dim() != 4 or eps.shape[0] != vb * int(dup) or eps.shape[1] != C or wy.numel() != h or wx.numel() != w or total.numel() != N * Hc * Wc:
        raise PeaError(f"views_merge_: eps {tuple(eps.shape)}, wy {tuple(wy.shape)}, wx {tuple(wx.shape)}, total {tuple(total.shape)} for a "
                       f"canvas {tuple(canvas.shape)} and dup={dup}")
    if factor is not None and factor.numel() != vb:
        raise PeaError(f"views_merge_: factor {tuple(factor.shape)}, expected [{vb}]")
    check(lib().pea_op_views_merge(ptr(eps), ptr(canvas), _view_slots(views, vb), len(views), vb, int(dup), N, C, Hc, Wc, h, w,
                                   int(bool(wrap_x)), float(guidance_scale), ptr(factor), ptr(wy), ptr(wx), ptr(total), int(bool(first)),
                                   int(bool(last)), stream_ptr()))
    return canvas


def cfg_rescale_factors(noise_pred2, guidance_scale, guidance_rescale, out=None, workspace=None):
    """The per-sample factors of `rescale_noise_cfg` alone (pea_op_cfg_rescale_factors): noise_pred2 fp32 [2B, ...],
    unconditional half first -> fp32 [B], what `cfg_combine(..., guidance_rescale)` multiplies its result by."""
    x = noise_pred2
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] % 2:
        raise PeaError(f"cfg_rescale_factors: noise_pred {tuple(x.shape)} {x.dtype}, expected contiguous fp32 with a batch of 2 B")
    B = x.shape[0] // 2
    if out is None:
        out = torch.empty(B, device=x.device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty(lib().pea_op_cfg_combine_workspace_bytes(B), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_cfg_rescale_factors(ptr(x), B, x[0].numel(), float(guidance_scale), float(guidance_rescale), ptr(workspace),
                                           ptr(out), stream_ptr()))
    return out


def lora_compose(acc, down, up, scale, out=None):
    """out[M][Kf] = acc + scale * up[M][r] @ down[r][Kf], fp32 on the GPU (acc any shape with M leading; out may be acc)."""
    M, r = up.shape[0], down.shape[0]
    Kf = acc.numel() // M
    for t in (acc, down, up):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert up.numel() == M * r and down.numel() == r * Kf and acc.numel() == M * Kf
    if out is None:
        out = torch.empty_like(acc)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == acc.numel()
    check(lib().pea_op_lora_compose(ptr(acc), ptr(down), ptr(up), ptr(out), M, Kf, r, float(scale), stream_ptr()))
    return out


def clip_score(image_embeds, text_embeds, w=2.5, clamp=True):
    """CLIPScore (Hessel et al. 2021) per pair (pea_op_clip_score): w * max(cos(image_embeds[b], text_embeds[b]), 0), fp32
    [B,D] -> fp32 [B]; `w=1, clamp=False` is the plain cosine.  One wave per pair, fixed reduction order (bit-reproducible)."""
    assert image_embeds.shape == text_embeds.shape and image_embeds.dim() == 2
    a = image_embeds.detach().to(torch.float32).contiguous()
    t = text_embeds.detach().to(device=a.device, dtype=torch.float32).contiguous()
    out = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
    check(lib().pea_op_clip_score(ptr(a), ptr(t), ptr(out), a.shape[0], a.shape[1], float(w), int(bool(clamp)), stream_ptr()))
    return out


# ---- glue kernels (include/pea_hip.h, "Glue kernels between the families"): thin calls for the kernel-level parity tests.
# Where a kernel writes a strided or partial output, or accumulates, the caller hands over the (pre-filled) output buffer.
def _out(y, like=None, shape=None, dtype=BF):
    if y is not None:
        return y
    return torch.empty_like(like) if shape is None else torch.empty(*shape, device=like.device, dtype=dtype)


def add(a, b, y=None, n=None):
    y = _out(y, a)
    check(lib().pea_op_add(ptr(a), ptr(b), ptr(y), a.numel() if n is None else n, stream_ptr()))
    return y


def silu_fwd(x, y=None, n=None):
    y = _out(y, x)
    check(lib().pea_op_silu_fwd(ptr(x), ptr(y), x.numel() if n is None else n, stream_ptr()))
    return y


def gelu_fwd(x, y=None, n=None):
    y = _out(y, x)
    check(lib().pea_op_gelu_fwd(ptr(x), ptr(y), x.numel() if n is None else n, stream_ptr()))
    return y


def silu_bwd(x, dy, dx=None, accum=False, n=None):
    dx = _out(dx, x)
    check(lib().pea_op_silu_bwd(ptr(x), ptr(dy), ptr(dx), x.numel() if n is None else n, int(accum), stream_ptr()))
    return dx


def gelu_bwd(x, dy, dx=None, accum=False, n=None):
    dx = _out(dx, x)
    check(lib().pea_op_gelu_bwd(ptr(x), ptr(dy), ptr(dx), x.numel() if n is None else n, int(accum), stream_ptr()))
    return dx


def accum_(x, y, accum=True, n=None):
    check(lib().pea_op_accum(ptr(x), ptr(y), x.numel() if n is None else n, int(accum), stream_ptr()))
    return y


def sumpool2_(x, y, accum=False):
    """x [B,2H,2W,C] -> y [B,H,W,C] (+)= the 2 x 2 sums"""
    B, H, W, C = y.shape
    check(lib().pea_op_sumpool2(ptr(x), ptr(y), B, H, W, C, int(accum), stream_ptr()))
    return y


def geglu_bwd_il(hg, dy, dhg=None):
    dhg = _out(dhg, hg)
    check(lib().pea_op_geglu_bwd_il(ptr(hg), ptr(dy), ptr(dhg), dy.shape[0], dy.shape[1], stream_ptr()))
    return dhg


def select_rows_(c, u, mask, y, B, per, ystride=0):
    """mask: uint8 / bool [>= B] on the device (a slice selects the first row's byte)"""
    check(lib().pea_op_select_rows(ptr(c), ptr(u), ptr(mask), ptr(y), B, per, ystride, stream_ptr()))
    return y


def select_rows_bwd_(dy, mask, dc, du, B, per, dystride=0):
    check(lib().pea_op_select_rows_bwd(ptr(dy), ptr(mask), ptr(dc), ptr(du), B, per, dystride, stream_ptr()))
    return dc, du


def mean_tokens(x, y=None):
    B, L, C = x.shape
    y = _out(y, x, (B, C))
    check(lib().pea_op_mean_tokens(ptr(x), ptr(y), B, L, C, stream_ptr()))
    return y


def mean_tokens_bwd_(dy, dx, accum=False):
    B, L, C = dx.shape
    check(lib().pea_op_mean_tokens_bwd(ptr(dy), ptr(dx), B, L, C, int(accum), stream_ptr()))
    return dx


def colsum_(x, db, accum=False):
    R, C = x.shape
    check(lib().pea_op_colsum(ptr(x), ptr(db), R, C, int(accum), stream_ptr()))
    return db


def colsum_batched_(x, out, ldo=None):
    """x bf16 [B,HW,C] -> out fp32 [B][ldo] (columns [C, ldo) are left alone)"""
    B, HW, C = x.shape
    ws = torch.empty(lib().pea_op_colsum_batched_scratch_bytes(B, HW, C), device=x.device, dtype=torch.uint8)
    check(lib().pea_op_colsum_batched(ptr(x), ptr(out), B, HW, C, C if ldo is None else ldo, ptr(ws), stream_ptr()))
    return out


def copy2d_(x, ldx, y, ldy, rows, C, accum=False):
    check(lib().pea_op_copy2d(ptr(x), ldx, ptr(y), ldy, rows, C, int(accum), stream_ptr()))
    return y


def transpose_(x, y, R, C, ldy):
    """y[c * ldy + r] = x[r][c]; x bf16 or fp32, y bf16"""
    fn = lib().pea_op_transpose_f32_bf16 if x.dtype == torch.float32 else lib().pea_op_transpose_bf16
    check(fn(ptr(x), ptr(y), R, C, ldy, stream_ptr()))
    return y


def nhwc_to_nchw_f32(x, B, HW, C, d2s_hw=None, y=None):
    y = _out(y, x, (B, C, HW), torch.float32)
    dH, dW = d2s_hw or (0, 0)
    check(lib().pea_op_nhwc_to_nchw_f32(ptr(x), ptr(y), B, HW, C, dH, dW, stream_ptr()))
    return y


def nchw_f32_to_nhwc(x, B, HW, C, d2s_hw=None, y=None):
    y = _out(y, x, (B, HW, C), BF)
    dH, dW = d2s_hw or (0, 0)
    check(lib().pea_op_nchw_f32_to_nhwc(ptr(x), ptr(y), B, HW, C, dH, dW, stream_ptr()))
    return y


def pad_gather_(src, mode, d, dp, w, ldw, wt, ldwt, st_n, st_k):
    N_t, K_t = src.shape
    check(lib().pea_op_pad_gather(ptr(src), N_t, K_t, mode, d, dp, ptr(w), ldw, ptr(wt), ldwt, st_n, st_k, stream_ptr()))
    return w, wt


def pad_head_vec(src, heads, d, dp, dst=None):
    dst = _out(dst, src, (heads * dp,), torch.float32)
    check(lib().pea_op_pad_head_vec(ptr(src), ptr(dst), heads, d, dp, stream_ptr()))
    return dst


def permute_geglu_vec(src, dst=None):
    dst = _out(dst, src)
    check(lib().pea_op_permute_geglu_vec(ptr(src), ptr(dst), src.numel() // 2, stream_ptr()))
    return dst


def cast_i64_f32(x, y=None):
    y = _out(y, x, tuple(x.shape), torch.float32)
    check(lib().pea_op_cast_i64_f32(ptr(x), ptr(y), x.numel(), stream_ptr()))
    return y


def cast_f32_bf16(x, y=None):
    y = _out(y, x, tuple(x.shape), BF)
    check(lib().pea_op_cast_f32_bf16(ptr(x), ptr(y), x.numel(), stream_ptr()))
    return y


def cast_bf16_f32(x, y=None):
    y = _out(y, x, tuple(x.shape), torch.float32)
    check(lib().pea_op_cast_bf16_f32(ptr(x), ptr(y), x.numel(), stream_ptr()))
    return y


def fill_random_(p, seed, scale, offset=0.0, n=None):
    n = p.numel() if n is None else n
    if p.dtype == torch.float32:
        check(lib().pea_op_fill_random_f32(ptr(p), n, seed, float(scale), float(offset), stream_ptr()))
    else:
        check(lib().pea_op_fill_random_bf16(ptr(p), n, seed, float(scale), stream_ptr()))
    return p


def splitk_reduce_(part, nsplit, stride, out, ldo, M, N, accum=False):
    check(lib().pea_op_splitk_reduce(ptr(part), nsplit, stride, ptr(out), ldo, M, N, int(accum), stream_ptr()))
    return out


def rmsnorm_fwd_(x, gamma, y, R, C, eps=1e-6):
    check(lib().pea_op_rmsnorm_fwd(ptr(x), ptr(gamma), ptr(y), R, C, eps, stream_ptr()))
    return y


def layernorm_stats_(x, stats, R, C, eps=1e-5):
    check(lib().pea_op_layernorm_stats(ptr(x), ptr(stats), R, C, eps, stream_ptr()))
    return stats


def layernorm_fwd_(x, gamma, beta, y, stats, R, C, eps=1e-5):
    check(lib().pea_op_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(stats), R, C, eps, stream_ptr()))
    return y, stats


def layernorm_bwd_(x, dy, gamma, stats, dx, R, C, accum=False):
    check(lib().pea_op_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(stats), ptr(dx), None, None, R, C, int(accum), stream_ptr()))
    return dx


def softmax_rows_(s, rows, cols, ld, scale=1.0):
    check(lib().pea_op_softmax_rows(ptr(s), rows, cols, ld, float(scale), stream_ptr()))
    return s


def residual_import(src, dtype, B, C, HW, scale, dst=None):
    dst = _out(dst, src, (B, HW, C), BF)
    check(lib().pea_op_residual_import(ptr(src), dtype, ptr(dst), B, C, HW, float(scale), stream_ptr()))
    return dst


def vae_posterior(h, wq, bq, noise, scaling, want_moments=True, want_latents=True):
    B, C2 = h.shape[:2]
    HW = h[0, 0].numel()
    mom = torch.empty_like(h) if want_moments else None
    lat = torch.empty(B, C2 // 2, *h.shape[2:], device=h.device, dtype=torch.float32) if want_latents else None
    check(lib().pea_op_vae_posterior(ptr(h), ptr(wq), ptr(bq), ptr(noise), ptr(mom), ptr(lat), B, C2, HW, float(scaling), stream_ptr()))
    return mom, lat


def vae_post_quant(z, w, b, inv_scaling):
    out = torch.empty_like(z)
    check(lib().pea_op_vae_post_quant(ptr(z), ptr(w), ptr(b), ptr(out), z.shape[0], z.shape[1], z[0, 0].numel(), float(inv_scaling),
                                      stream_ptr()))
    return out


def embed_tokens(ids, tok, pos=None, type0=None):
    B, L = ids.shape
    vocab, width = tok.shape
    out = torch.empty(B, L, width, device=tok.device, dtype=BF)
    check(lib().pea_op_embed_tokens(ptr(ids), ptr(tok), ptr(pos), ptr(type0), ptr(out), B, L, width, vocab, stream_ptr()))
    return out


def t5_rel_bias_(rel, dist_bucket, bias, H, L, pitch):
    """rel fp32 [num_buckets][H], dist_bucket int32 [L], bias fp32 [H][L][pitch] (columns [L, pitch) left alone)"""
    check(lib().pea_op_t5_rel_bias(ptr(rel), ptr(dist_bucket), ptr(bias), H, L, pitch, rel.shape[0] // 2, stream_ptr()))
    return bias


def gather_eos(ids, x, eos_id):
    B, L, width = x.shape
    out = torch.empty(B, width, device=x.device, dtype=BF)
    check(lib().pea_op_gather_eos(ptr(ids), ptr(x), ptr(out), B, L, width, eos_id, stream_ptr()))
    return out


def kv_len(ids, pad_id):
    B, L = ids.shape
    out = torch.empty(B, device=ids.device, dtype=torch.int32)
    check(lib().pea_op_kv_len(ptr(ids), ptr(out), B, L, pad_id, stream_ptr()))
    return out


def kd_loss_tmap(taps_s, taps_t, eps_s, eps, eps_t, zh, tmap, feat_weight=0.1, nan_guard=False, grad_scale=1.0):
    """kd_loss over compacted teacher tensors: tmap int32 [B] on the device (row of sample b in taps_t / eps_t), or None"""
    n = len(taps_s)
    B = eps_s.shape[0]
    dt = [torch.empty_like(t) for t in taps_s]
    de = torch.empty_like(eps_s)
    arr = ctypes.c_void_p * max(n, 1)
    a_s, a_t, a_d = arr(*[t.data_ptr() for t in taps_s]), arr(*[t.data_ptr() for t in taps_t]), arr(*[t.data_ptr() for t in dt])
    per = (ctypes.c_longlong * max(n, 1))(*[t[0].numel() for t in taps_s])
    losses = torch.empty(4, device=eps_s.device, dtype=torch.float32)
    ws = torch.empty(lib().pea_op_kd_loss_workspace_bytes(n, per, eps_s[0].numel(), B), device=eps_s.device, dtype=torch.uint8)
    check(lib().pea_op_kd_loss_tmap(n, a_s, a_t, a_d, per, ptr(eps_s), ptr(eps), ptr(eps_t), ptr(de), eps_s[0].numel(), ptr(zh),
                                    ptr(tmap), B, feat_weight, int(nan_guard), grad_scale, ptr(losses), ptr(ws), stream_ptr()))
    return losses, dt, de
