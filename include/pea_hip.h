/* pea_hip.h -- C ABI of libpea_hip.so, the MI355X (gfx950) PEA-Diffusion training-step library.
 *
 * The reference (OPPO-Mente-Lab/PEA-Diffusion) is pure Python and defines no FFI; its plug-in
 * surfaces are three Python call signatures:
 *   - the adapter      `proj(x) -> (pooled, tokens)`           train_sdxl_zh.py:43-67, :383-384
 *   - the UNet call    `unet(x_t, t, ehs, added_cond_kwargs)`  train_sdxl_zh.py:397,415
 *   - the train step   `training_step(batch, i) -> {"loss"}`   train_sdxl_zh.py:305-449
 * Each entry point below cites the reference lines whose work it replaces.  Conventions:
 *   - every function returns 0 on success or a negative PEA_E_* code; pea_last_error() returns a
 *     thread-local message.  No exception crosses the boundary.
 *   - the caller owns all tensor memory: raw DEVICE pointers (e.g. torch `tensor.data_ptr()`),
 *     contiguous row-major.  Images cross the boundary as NCHW fp32; inside, activations are
 *     token-major ("NHWC") bf16.  `bf16` arguments are `void*` to 2-byte brain-float data.
 *   - all work is enqueued on the `stream` argument (a hipStream_t passed as void*; NULL = the
 *     default stream); nothing synchronises unless documented as blocking.
 *   - a context is driven by one host thread at a time.
 * There is NO CPU fallback: without a gfx950 device every compute entry point fails.
 */
#ifndef PEA_HIP_H
#define PEA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PEA_OK 0
#define PEA_E_INVALID (-1)
#define PEA_E_HIP (-2)
#define PEA_E_SHAPE (-3)
#define PEA_E_STATE (-4)
#define PEA_E_NOTFOUND (-5)
#define PEA_E_TIMEOUT (-6)

const char* pea_last_error(void);
int pea_version(void);
/* number of visible HIP devices (0 when none); never initialises a context on its own */
int pea_device_count(void);

/* ======================================================================== operator level ====
 * One entry point per hand-written kernel family; used by the parity tests and by callers that
 * want a single op.  act: 0 none, 1 GELU(erf), 2 SiLU, 3 quick-GELU x * sigmoid(1.702 x).      */

/* C[M][N] = act(alpha * A[M][K] . W[N][K]^T + bias[n] + rowvec[m / rows_per_batch][n]) + res[m][n]
 * (torch.nn.Linear / F.linear inside the UNet and the adapter, train_sdxl_zh.py:48-55,62-64).
 * A, W, rowvec, res, preact: bf16.  C: bf16, or fp32 when out_f32 (accum_f32: C += ...).
 * K % 64 == 0, N % 4 == 0.  NULL pointers switch the corresponding term off.                    */
int pea_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, float alpha,
                const float* bias, const void* rowvec, int ldrv, int rows_per_batch, int act, void* preact,
                int ldpre, const void* res, int ldres, int out_f32, int accum_f32, void* stream);

/* C = A . W^T + bias with columns n < qscale_cols multiplied by qscale (qscale_cols % 16 == 0): the fused Q|K|V projection
 * of an attention layer, whose Q block leaves multiplied by softmax_scale * log2(e) (diffusers Attention.to_q/to_k/to_v).   */
int pea_op_gemm_qscale(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const float* bias,
                       int qscale_cols, float qscale, void* stream);

/* The FF projection with GEGLU in its epilogue (diffusers GEGLU.forward: hidden, gate = proj(x).chunk(2); hidden *
 * gelu(gate); W rows interleaved (h_i, gate_i)):  y[m][n] = h * gelu(gate)  (bf16 [M][N/2]); stash (optional, bf16 [M][N],
 * rows < stash_rows when stash_rows > 0): stash_grad 0: the pre-activation pair (h, gate); 1: the pair the BACKWARD
 * multiplies by, (gelu(gate), h * gelu'(gate)) -- no weight gradients exist on this path, so nothing else reads it.  */
int pea_op_gemm_geglu(const void* A, int lda, const void* W, int ldw, const float* bias, void* y, void* stash, int M, int N,
                      int K, int stash_grad, int stash_rows, void* stream);

/* The data-gradient GEMM of the FF output projection with the GEGLU backward in its epilogue (diffusers GEGLU:
 * y = h * gelu(gate); train_sdxl_zh.py's student backward runs it in every transformer block):
 *   dy = A[M][K] . W[N][K]^T;  form 0: pre[m][2n] = h, pre[m][2n+1] = gate (the pre-activation stash of the forward);
 *   form 1: pre[m][2n] = gelu(gate), pre[m][2n+1] = h * gelu'(gate) (a stash_grad forward);
 *   C[m][2n] = dy * gelu(gate),  C[m][2n+1] = dy * h * gelu'(gate)      (C: bf16 [M][2N], ldc >= 2N)
 * dy itself is never stored.  K % 64 == 0, N % 16 == 0, ldc % 8 == 0, ldpre % 8 == 0.                              */
int pea_op_gemm_geglu_bwd(const void* A, int lda, const void* W, int ldw, const void* pre, int ldpre, void* C, int ldc,
                          int M, int N, int K, int form, void* stream);

/* LayerNorm folded into the Linear that consumes it (UNet transformer blocks: norm1 -> to_q|k|v, norm2 -> attn2.to_q,
 * norm3 -> ff.net.0.proj):  y = LN(x; gamma, beta, eps) . W^T + bias  computed as  rstd (x . W'^T - mean s) + t  with
 * W' = W . gamma, s[n] = sum_k W'[n][k], t[n] = sum_k beta[k] W[n][k] + bias[n] -- one statistics pass over x and one
 * GEMM on the un-normalised rows.  x bf16 [M][K]; W bf16 [N][K]; y bf16 [M][N]; geglu_y (optional) bf16 [M][N/2] =
 * h * gelu(gate) for interleaved (h_i, gate_i) weight rows (y then receives the pre-activation, may be NULL).
 * Caller-provided scratch: Wf bf16 [N][K], svec / tvec fp32 [N], stats fp32 [M][2].                      */
int pea_op_ln_linear(const void* x, const float* gamma, const float* beta, const void* W, const float* bias, void* y,
                     void* geglu_y, int M, int N, int K, float eps, void* Wf, float* svec, float* tvec, float* stats,
                     void* stream);

/* 3x3 convolution, padding 1, as implicit GEMM over an NHWC bf16 tensor x[B][Hs][Ws][Cin] with
 * packed weights w[Cout][(ky,kx,ci)] (see pea_op_pack_conv).  (ResnetBlock2D conv1/conv2,
 * Downsample2D, Upsample2D of the UNet called at train_sdxl_zh.py:397,415.)
 * stride 1|2; upsample2x: nearest-2x upsample folded into the gather; transposed2: zero-stuffed
 * input (data-gradient of a stride-2 conv).  Epilogue as pea_op_gemm.                            */
int pea_op_conv3x3(const void* x, const void* w, void* y, int B, int Hs, int Ws, int Cin, int Cout, int stride,
                   int upsample2x, int transposed2, const float* bias, const void* rowvec, int ldrv,
                   const void* res, void* stream);
/* torch conv weight [Co][Ci][3][3] fp32 -> bf16 packed; dgrad=1 gives the flipped/transposed
 * weights w'[ci][(2-ky,2-kx,co)] whose forward conv is the data gradient.                        */
int pea_op_pack_conv(const float* w, void* out, int Co, int Ci, int dgrad, void* stream);
/* The GEMM / conv forms that only the model tape fills (GemmP fields no entry above can set), one thin entry each:
 *   pea_op_gemm_geglu_tanh: pea_op_gemm_geglu with the gate's activation as an argument: geglu_tanh 0 = GELU(erf), 1 = gelu_new,
 *       0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))) (T5 v1.1 gated-gelu).  The gradient-form stash (stash_grad) exists for
 *       the erf gate only and is refused with geglu_tanh.
 *   pea_op_gemm_splitk: fp32 partial s (0 <= s < ksplit) = alpha * A[:, Ks] . W[:, Ks]^T over K-steps
 *       Ks = [s * per, min((s + 1) * per, K / 64)), per = ceil(K / 64 / ksplit), written [M][N] with rows ldc apart at
 *       part + s * split_stride (an empty range stores zeros); split_stride >= (M - 1) * ldc + N, split_stride % 4 == 0.
 *       pea_op_splitk_reduce adds the partials (the backward of the stacked cross-attention K|V projection).
 *   pea_op_conv3x3_ex: pea_op_conv3x3 on a plain source with ldw / ldc / ldres as arguments (Cout columns written into rows
 *       ldc >= Cout wide, the other columns left alone), `act` in the epilogue (0 none, 1 GELU(erf), 2 SiLU, 3 quick-GELU
 *       x * sigmoid(1.702 x)), Cin the STORED channel width of x (% 64; weights from pea_op_pack_conv_padded) and pad_off:
 *       0 = padding 1 on every side (Ho = ceil(Hs / stride)); 1 = F.pad(x, (0,1,0,1)) then stride 2 without padding, the VAE
 *       encoder's Downsample2D(padding=0): Ho = Hs / 2, Wo = Ws / 2, even sides only.
 *   pea_op_pack_conv_padded: pea_op_pack_conv(dgrad = 0) for an input stored Cip >= Ci channels wide: out bf16 [Co][9 Cip],
 *       zeros in the padding channels (ControlNet conditioning embedding).                                                  */
int pea_op_gemm_geglu_tanh(const void* A, int lda, const void* W, int ldw, const float* bias, void* y, void* stash, int M, int N,
                           int K, int stash_grad, int stash_rows, int geglu_tanh, void* stream);
int pea_op_gemm_splitk(const void* A, int lda, const void* W, int ldw, float* part, int ldc, long long split_stride, int M, int N,
                       int K, float alpha, int ksplit, void* stream);
int pea_op_conv3x3_ex(const void* x, const void* w, int ldw, void* y, int ldc, int B, int Hs, int Ws, int Cin, int Cout,
                      int stride, int pad_off, int act, const float* bias, const void* res, int ldres, void* stream);
int pea_op_pack_conv_padded(const float* w, void* out, int Co, int Ci, int Cip, void* stream);
/* conv3x3(interpolate(x, 2x nearest)) -- diffusers Upsample2D, the UNet's up_blocks[i].upsamplers[0] -- in its sub-pixel
 * form: per output parity (y&1, x&1) a 2 x 2 kernel of summed taps over the SOURCE (16 tap products per source pixel and
 * channel pair instead of the 36 of a 3 x 3 gather over the upsampled image).
 *   pea_op_pack_conv_subpixel: [Co][Ci][3][3] fp32 -> bf16 [4][Co][4 Ci] (dgrad = 0) or [Ci][16 Co] (dgrad = 1), 16 Co Ci elements
 *   pea_op_upconv_subpixel:    x NHWC [B][Hs][Ws][Cin] -> y depth-to-space [B][Hs][Ws][(y&1)*2+(x&1)][Cout]  (+ bias)
 *   pea_op_upconv_subpixel_dgrad: dy (that layout) -> dx NHWC [B][Hs][Ws][Cin] (+ res, may alias dx)                     */
int pea_op_pack_conv_subpixel(const float* w, void* out, int Co, int Ci, int dgrad, void* stream);
/* torch.cat([a, b], dim=1) on NHWC rows (unet_2d_blocks.py: the skip concatenation of every up-block resnet) and its backward
 * (da (+)= dy[:, :C1], db (+)= dy[:, C1:]; NULL = skip).  aH, aW != 0: a / da are stored depth-to-space at full resolution
 * aH x aW (an upsampler output in its sub-pixel form); the result rows are plain NHWC.                                   */
int pea_op_concat2(const void* a, int C1, const void* b, int C2, void* y, long long rows, int aH, int aW, void* stream);
int pea_op_split2(const void* dy, int C1, int C2, void* da, int accum_a, void* db, int accum_b, long long rows, int aH,
                  int aW, void* stream);
/* FreeU (diffusers 0.23 `apply_freeu`, `fourier_filter` with threshold 1) on the two operands of that concat, in two launches.
 * pea_op_freeu_coef: skip bf16 [B][H][W][C2] -> coef fp32 [B][7][C2], per channel map the sums S00 = sum v, C10 / S10 = sum v cos /
 * sin(2 pi y / H), C01 / S01 = sum v cos / sin(2 pi x / W), C11 / S11 = sum v cos / sin(2 pi y / H + 2 pi x / W), in that order.
 * Where one workgroup per (sample, 128 channels) would leave the chip empty the rows are split into slabs whose partial sums go
 * to `scratch` (pea_op_freeu_scratch_bytes device bytes; 0 = one slab, scratch may be NULL) and are added in slab order: no
 * atomics, the same bits on every run.
 * pea_op_concat2_freeu: y [B*H*W][C1 + C2] = ( bscale * a[:, :C1/2] | a[:, C1/2:] | skip filtered with scale s ), the filter
 * evaluated in fp32 from coef.  s == 1 and bscale == 1 are plain copies of their columns (s == 1 never reads coef; both: the bits
 * of pea_op_concat2).  aH, aW != 0: `a` is stored depth-to-space (aH == H, aW == W).  a may be b.
 * C1 / 2, C1 and C2 must be multiples of 8, H and W at least 2, s and bscale finite and positive (PEA_E_SHAPE otherwise). */
long long pea_op_freeu_scratch_bytes(int B, int H, int W, int C2);
int pea_op_freeu_coef(const void* skip, int B, int H, int W, int C2, float* coef, void* scratch, void* stream);
int pea_op_concat2_freeu(const void* a, int C1, const void* b, int C2, const float* coef, void* y, int B, int H, int W, float s,
                         float bscale, int aH, int aW, void* stream);
int pea_op_upconv_subpixel(const void* x, const void* w, void* y, int B, int Hs, int Ws, int Cin, int Cout,
                           const float* bias, void* stream);
int pea_op_upconv_subpixel_dgrad(const void* dy, const void* wt, void* dx, int B, int Hs, int Ws, int Cin, int Cout,
                                 const void* res, void* stream);
int pea_op_conv_in(const float* x_nchw, const float* w, const float* bias, void* y_nhwc, int B, int Cin, int H,
                   int W, int Cout, void* stream);
/* conv_in of an inpainting UNet (in_channels = 2 C + 1) without the per-step torch.cat of tests/test_sdxl_zh_inpaint.py
 * (`cat([cat([latents] * 2), mask, masked_image_latents], dim=1)`): input channel ci of image b is latents[b % latent_batch][ci]
 * (ci < C), mask[b % cond_batch][0] (ci == C), masked_latents[b % cond_batch][ci - C - 1] (ci > C); all fp32 NCHW, 16-byte
 * aligned, W % 4 == 0 (else PEA_E_SHAPE).  y: bf16 NHWC [B][H][W][Cout], equal bit for bit to pea_op_conv_in on the
 * concatenated [B][2C+1][H][W] tensor. */
int pea_op_conv_in_gather(const float* latents, const float* mask, const float* masked_latents, const float* w,
                          const float* bias, void* y_nhwc, int B, int C, int latent_batch, int cond_batch, int H, int W,
                          int Cout, void* stream);
int pea_op_conv_out(const void* x_nhwc, const float* w_packed, const float* bias, float* y_nchw, int B, int Cin,
                    int H, int W, int Cout, void* stream);
int pea_op_conv_out_dgrad(const float* dy_nchw, const float* w_packed, void* dx_nhwc, int B, int Cin, int H, int W,
                          int Cout, void* stream);
int pea_op_pack_conv_out(const float* w, float* out, int Co, int Ci, void* stream);

/* GroupNorm (+ optional SiLU) over x[B][HW][C] bf16; stats fp32 [B][groups][2]; scratch: device bytes from
 * pea_op_groupnorm_scratch_bytes (per-block partial sums: the reduction order is fixed, results are
 * bit-reproducible)                                                                               */
long long pea_op_groupnorm_scratch_bytes(int B, int HW, int C, int groups);
int pea_op_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, void* scratch,
                         int B, int HW, int C, int groups, float eps, int silu, void* stream);
int pea_op_groupnorm_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* stats,
                         void* dx, void* scratch, int B, int HW, int C, int groups, int silu, int accum,
                         void* stream);
/* LayerNorm over rows; stats fp32 [R][2]; dgamma/dbeta (fp32, accumulated) may be NULL */
int pea_op_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, int R, int C,
                         float eps, void* stream);
/* the same over fp32 rows with an fp32 result and no statistics (the image-prompt projection) */
int pea_op_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, int R, int C, float eps,
                             void* stream);
int pea_op_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* stats, void* dx,
                         float* dgamma, float* dbeta, int R, int C, int accum, void* stream);

/* softmax(scale Q K^T) V (diffusers AttnProcessor2_0 -> SDPA).  Q/K/V/O bf16 with row strides ld* (elements);
 * head h occupies columns [64*nd*h, 64*nd*(h+1)) where nd = ceil(head_dim / 64) in {1,2,3}; a head narrower than
 * 64*nd is zero padded (SD1.5: 40 -> 64, 80 -> 128, 160 -> 192) and `scale` stays head_dim^-0.5.  lse fp32 [B][H][Sq]. */
int pea_op_attention_fwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                         float* lse, int B, int H, int Sq, int Skv, float scale, int nd, void* stream);
/* ... on a Q that already carries scale * log2(e) (the product path: the Q|K|V / to_q projection applies the factor to its fp32
 * accumulator, pea_op_gemm_qscale, so nothing is rounded twice); `scale` is still the softmax scale */
int pea_op_attention_fwd_prescaled(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                   float* lse, int B, int H, int Sq, int Skv, float scale, int nd, void* stream);
/* text-encoder attention (head_dim 64, forward only): `causal` = key index <= query index (CLIP text model), kv_len =
 * device int[B] of valid key counts (BERT right padding) or NULL */
int pea_op_attention_fwd_masked(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                float* lse, int B, int H, int Sq, int Skv, float scale, int causal, const int* kv_len,
                                void* stream);
/* Everything launch_attention_fwd takes at head_dim 64 (what the text-encoder and merged-pass tapes ask of it), forward only:
 * q_prescaled as for pea_op_attention_fwd_prescaled, causal and kv_len as for pea_op_attention_fwd_masked (kv_len values in
 * 1 .. Skv), and `bias`: NULL, or an additive score bias (T5 relative positions) as the kernel reads it -- device fp32
 * [H][Sq][pitch] with pitch = 64 * ceil(Skv / 64), shared by the batch, 16-byte aligned, in the log2 domain (the natural-log
 * bias times log2(e)), added to the scaled score.  Columns Skv .. pitch of a row are read but never used: they must be
 * addressable, their values do not matter.  lse (may be NULL) fp32 [B][H][Sq], natural log, over the keys a row keeps. */
int pea_op_attention_fwd_text(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                              float* lse, int B, int H, int Sq, int Skv, float scale, int q_prescaled, int causal,
                              const int* kv_len, const float* bias, void* stream);
/* Decoupled cross-attention of an image prompt (IP-Adapter), forward only, head_dim 64:
 *   O = softmax(scale Q K^T) V + ip_scale * softmax(scale Q K2^T) V2
 * two separate softmaxes over the same Q, in ONE launch that writes O once.  1 <= Skv <= 128 text keys, 1 <= Skv2 <= 32 image
 * keys (K2 / V2 bf16 [B][Skv2][ldk2 / ldv2], ld* multiples of 8), any Sq >= 1.  q_prescaled: Q already carries scale * log2(e)
 * (the same factor serves both score products).  kv_len (device int[B] or NULL) masks text keys only; lse (may be NULL) is that
 * of the text softmax.  causal != 0 is refused, like every other shape outside the above, before any launch. */
int pea_op_attention_fwd_ip(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                            const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv, int Skv2,
                            float scale, float ip_scale, int q_prescaled, int causal, const int* kv_len, void* stream);
/* Several image prompts in one launch (two IP-Adapters, each with a weight and an optional region mask), forward only, head_dim 64:
 *   O[b,q,:] = softmax(scale q K^T) V + sum_j weight[j] * mask[j][b,q] * softmax(scale q K2_j^T) V2_j,       j < n_sets
 * 1 <= n_sets <= 4 sets of n_keys[j] >= 1 keys with sum n_keys <= 32, lying back to back in ONE K2 / V2 pair (bf16
 * [B][sum n_keys][ldk2 / ldv2], ld* as for pea_op_attention_fwd_ip): set j is rows off_j .. off_j + n_keys[j] of every sample, and
 * the boundaries need not be multiples of anything.  Every set has a softmax of its own (own maximum, own sum), like the text
 * keys.  mask[j]: NULL (a mask of 1) or device fp32 [Bm][Sq] with batch stride mask_stride[j] elements, 0 (one mask shared by
 * the batch) or >= Sq; any finite values (a bicubically reduced binary mask leaves [0, 1]); rows at or past Sq are never read.
 * The struct is host memory, read during the call.  kv_len, lse, q_prescaled, causal and the limits (1..128 text keys, any
 * Sq >= 1) are those of pea_op_attention_fwd_ip; every refusal is PEA_E_SHAPE before any launch.  One set without a mask runs
 * the kernel instance of pea_op_attention_fwd_ip (same bits); all weights 0 run the plain attention. */
typedef struct pea_attn_ip_sets {
  int n_sets;
  int n_keys[4];
  float weight[4];
  const float* mask[4];
  long long mask_stride[4];
} pea_attn_ip_sets;
int pea_op_attention_fwd_ipn(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                             const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv,
                             const pea_attn_ip_sets* sets, float scale, int q_prescaled, int causal, const int* kv_len, void* stream);
/* Few-query attention over the UNION of two key sets, forward only, head_dim 64 (nd must be 1):
 *   O = softmax(scale [Q K^T | Q K2^T]) [V ; V2]
 * ONE softmax (unlike pea_op_attention_fwd_ip), for 1 <= Sq <= 32 queries: the Perceiver Resampler of the IP-Adapter "plus" files,
 * whose 16 latents attend over the image rows and over themselves, with the two key / value sets left where their projections
 * wrote them.  Skv >= 1 without an upper limit; 0 <= Skv2 <= 32, and with 0 K2 / V2 are NULL (a plain few-query attention).
 * The key range, not the query range, is shared among the waves of a workgroup; their partial (max, sum, O) triples are merged
 * in a fixed order, so two runs give the same bits.  Batch strides Sq * ldq, Skv * ldk / ldv, Skv2 * ldk2 / ldv2; ldq / ldk /
 * ldv / ldk2 / ldv2 multiples of 8 and >= 64 H, ldo a multiple of 4 and >= 64 H; Q / K / V 16-byte, O 8-byte aligned.  Rows of
 * K / V behind a set's last key are never read.  lse (may be NULL) fp32 [B][H][Sq] over the union; q_prescaled as for
 * pea_op_attention_fwd_ip.  Anything else (Sq > 32, Skv2 > 32, nd != 1, one of K2 / V2 alone, Skv2 and K2 disagreeing, a bad
 * leading dimension) is refused with PEA_E_SHAPE before any launch. */
int pea_op_attention_fwd_fewq(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                              const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv, int Skv2,
                              float scale, int nd, int q_prescaled, void* stream);
/* dQ/dK/dV (dQ may be NULL; dK and dV together); delta: fp32 scratch [2][B][H][Sq] (row constants of the backward kernels); scratch: optional device
 * buffer of pea_op_attention_bwd_scratch_bytes(...) bytes enabling the query-split dK/dV form used when the
 * key count is small (cross-attention); NULL = single pass                                            */
long long pea_op_attention_bwd_scratch_bytes(int B, int H, int Sq, int Skv, int nd);
int pea_op_attention_bwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                         int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                         void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                         int accum_dq, int accum_dkv, int nd, void* scratch, void* stream);

/* the backward on a prescaled Q (see pea_op_attention_fwd_prescaled); dQ is the gradient w.r.t. the UNSCALED q, so the
 * projection's data-gradient GEMM needs no factor */
int pea_op_attention_bwd_prescaled(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                                   int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                                   void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                                   int accum_dq, int accum_dkv, int nd, void* scratch, void* stream);

/* pea_op_attention_bwd with the Q convention as an argument and per-sample key counts: kv_len = device int[B] or NULL, the
 * counts the forward ran with (O and lse are that forward's).  Keys >= kv_len[b] of sample b are padding: they take no part
 * in dQ, and their rows of dK / dV are written as zeros (left as they are by the accumulating form).  Values lie in
 * 1 .. Skv; a count of 0 (a sample without any key) is outside the contract.  head_dim 64 only with kv_len (nd = 1;
 * anything else is PEA_E_SHAPE before any launch).  There is no causal or biased backward: the text encoders are frozen. */
int pea_op_attention_bwd_masked(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                                int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                                void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                                int accum_dq, int accum_dkv, int nd, void* scratch, int q_prescaled, const int* kv_len,
                                void* stream);

int pea_op_geglu_fwd(const void* hg, void* y, long long rows, int inner, void* stream);
int pea_op_geglu_bwd(const void* hg, const void* dy, void* dhg, long long rows, int inner, void* stream);
int pea_op_sumpool2(const void* x, void* y, int B, int H, int W, int C, int accum, void* stream);
int pea_op_timestep_embed(const float* t, void* y, int n, int dim, void* stream);
/* DDPM add_noise (train_sdxl_zh.py:322); ac = alphas_cumprod fp32[1000] on device */
int pea_op_add_noise(const float* x0, const float* eps, const long long* t, const float* ac, float* xt, int B,
                     long long per, void* stream);
int pea_op_cast_f32_bf16(const float* x, void* y, long long n, void* stream);
int pea_op_cast_bf16_f32(const void* x, float* y, long long n, void* stream);

/* Inference denoise loop glue (tests/test_sdxl_zh.py:376-406).
 * cfg_combine: eps2 = fp32 [2B][per] (unconditional half first, :394); out[B][per] = u + g*(t-u) (:395), then when
 *   guidance_rescale > 0 `rescale_noise_cfg` (:44-56, unbiased per-sample std); workspace from *_workspace_bytes(B).
 * dpm_update: one DPMSolverMultistepScheduler.step (:406; diffusers 0.23 [ext], dpmsolver++ midpoint) with host-side
 *   coefficients: x0 = (sample - sigma_s*eps)/alpha_s; sample <- c_s*sample + c_0*x0 + c_1*x0_prev; x0_prev <- x0. */
/* inpainting inputs (tests/test_sdxl_zh_inpaint.py: VaeImageProcessor.preprocess, the masking of __call__, the nearest resize
 * of prepare_mask_latents): image fp32 [N][3][H][W] and mask [N][1][H][W] in [0, 1], H and W (pixels) multiples of 8 ->
 * init_image = 2 image - 1, masked_image = init_image * (mask < 0.5) (both [N][3][H][W]),
 * latent_mask = (mask >= 0.5)[:, :, ::8, ::8] ([N][1][H/8][W/8]).  Exact in fp32. */
int pea_op_inpaint_prepare(const float* image, const float* mask, int N, int H, int W, float* init_image, float* masked_image,
                           float* latent_mask, void* stream);
long long pea_op_cfg_combine_workspace_bytes(int B);
int pea_op_cfg_combine(const float* eps2, float* out, int B, long long per, float guidance_scale, float guidance_rescale,
                       void* workspace, void* stream);
int pea_op_dpm_update(float* sample, const float* eps, float* x0_prev, long long n, float alpha_s, float sigma_s,
                      float c_s, float c_0, float c_1, void* stream);
/* lcm_update: one LCMScheduler.step (tests/test_sdxl_zh_lcm.py:178; diffusers 0.23 [ext]: epsilon prediction, boundary scalings
 *   c_skip / c_out) with host-side coefficients folded to four scalars, fp32 [n], in place:
 *     denoised = kx * sample + ke * eps          kx = c_out / sqrt(a_t) + c_skip,  ke = -c_out * sqrt(1 - a_t) / sqrt(a_t)
 *     sample  <- c_prev * denoised + c_noise * noise        c_prev = sqrt(a_prev), c_noise = sqrt(1 - a_prev)
 *   noise NULL (the last step, c_prev = 1): the noise term is dropped.  denoised (diffusers' second output) may be NULL. */
int pea_op_lcm_update(float* sample, const float* eps, const float* noise, float* denoised, long long n, float kx, float ke,
                      float c_prev, float c_noise, void* stream);
/* euler_update: one EulerDiscreteScheduler / EulerAncestralDiscreteScheduler step (diffusers 0.23 [ext]: epsilon prediction,
 *   so the derivative (x - x0) / sigma is eps itself) fused with the NEXT step's scale_model_input and the CFG batch
 *   doubling, host-side coefficients folded to three scalars, fp32 [n]:
 *     x'        = sample + k_e * eps                  k_e = sigma_down - sigma   (Euler: sigma_down = sigma_next)
 *     x'       += k_n * noise                         k_n = sigma_up; noise NULL (Euler, or the last ancestral step): dropped
 *     sample   <- x'                                  in place
 *     model_in[d * n + i] <- x' * k_s  for d < dup    k_s = 1 / sqrt(sigma_next^2 + 1); dup 1 or 2 (2: the CFG-doubled batch)
 *   model_in NULL: only the sample is updated (the last step).  eps NULL is the entry form: sample is only read and
 *   model_in = sample * k_s (the first step's scale_model_input; noise must be NULL, model_in not).  model_in ([dup * n]) must
 *   not overlap sample.  16-byte accesses when every pointer (model_in + n included for dup 2) is 16-byte aligned, scalar
 *   otherwise, with identical results; no atomics: bit-reproducible. */
int pea_op_euler_update(float* sample, const float* eps, const float* noise, float* model_in, long long n, int dup, float k_e,
                        float k_n, float k_s, void* stream);

/* LoRA weight composition (`pipe.load_lora_weights(...)`, `pipe.fuse_lora()`, tests/test_sdxl_zh_lcm.py:181-182):
 *   out[m][k] = acc[m][k] + scale * sum_r up[m][r] * down[r][k]      all fp32 device, torch layouts, 1 <= rank <= 256
 * M = output features (Cout), Kf = numel / M (Cin, or Cin * 9 for a [Co][Ci][3][3] weight with `down [r][Ci][3][3]`).
 * acc may be out (several adapters accumulate into one matrix).  fp32 products in a fixed order: bit-reproducible. */
int pea_op_lora_compose(const float* acc, const float* down, const float* up, float* out, int M, int Kf, int rank, float scale,
                        void* stream);

/* Fused KD loss of train_sdxl_zh.py:399-441 (SD1.5: train_sd_zh.py:217-276, nan_guard=1).
 * taps_s/taps_t/dtaps: HOST arrays of ntaps device pointers (bf16, elementwise-paired layouts);
 * per: HOST array of per-sample element counts.  eps_*: fp32 [B][per_eps].  zh: int64 [B] device.
 * losses: fp32[4] device = (loss, train_loss, train_loss_logits, train_loss_features).
 * dtaps[k] / deps_s receive dL/d(student tap) / dL/d(eps_s) (may be NULL).
 * workspace: device scratch of pea_op_kd_loss_workspace_bytes(...) bytes (per-block partials).           */
long long pea_op_kd_loss_workspace_bytes(int ntaps, const long long* per, long long per_eps, int B);
int pea_op_kd_loss(int ntaps, const void* const* taps_s, const void* const* taps_t, void* const* dtaps,
                   const long long* per, const float* eps_s, const float* eps, const float* eps_t, float* deps_s,
                   long long per_eps, const long long* zh, int B, float feat_weight, int nan_guard,
                   float grad_scale, float* losses, void* workspace, void* stream);

/* touch `bytes` of a read-only buffer so it becomes resident in the Infinity Cache (side-stream prefetch) */
int pea_op_prefetch(const void* p, long long bytes, void* stream);

/* fused AdamW over a flat fp32 buffer (DeepSpeed FusedAdam(adam_w_mode=True), utils/model_utils.py:64-67) */
int pea_op_adamw(float* w, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float grad_scale, void* stream);

/* pea_op_kd_loss over COMPACTED teacher tensors: tmap = device int[B] (or NULL = pea_op_kd_loss), the row of student sample b
 * inside taps_t[] / eps_t; entries of samples with zh != 0 are not read (use -1).  A sample with KD weight and tmap[b] < 0 has
 * no teacher: its terms are NaN.  nan_guard inspects only samples with KD weight (masked samples are never read).           */
int pea_op_kd_loss_tmap(int ntaps, const void* const* taps_s, const void* const* taps_t, void* const* dtaps,
                        const long long* per, const float* eps_s, const float* eps, const float* eps_t, float* deps_s,
                        long long per_eps, const long long* zh, const int* tmap, int B, float feat_weight, int nan_guard,
                        float grad_scale, float* losses, void* workspace, void* stream);

/* ---- Glue kernels between the families above: one entry per launcher, used by the kernel-level parity tests.  bf16 tensors
 * are 16-byte aligned and move 8 elements per lane: flat sizes n, per-sample sizes and leading dimensions are multiples of 8
 * (PEA_E_SHAPE otherwise) unless stated.  accum != 0: the output is read and added to (fp32 sum, one rounding).
 *   add: y = a + b;  silu / gelu (erf): y = f(x), dx (+)= dy f'(x);  accum: y (+)= x
 *   geglu_bwd_il: the GEGLU backward on the interleaved stash of pea_op_gemm_geglu(stash_grad = 1): hg[r][2i] = gelu(gate_i),
 *     hg[r][2i+1] = h_i gelu'(gate_i); dhg[r][2i], [2i+1] = dy[r][i] * those; inner % 4 == 0
 *   select_rows: y[b] = mask[b] ? u[b] : c[b] for B rows of `per` elements (mask: one byte per row); ystride (0 = per, else >=
 *     per) = elements between consecutive rows of y, whose tails [per, ystride) are not written.  _bwd: dc[b] = mask[b] ? 0 :
 *     dy[b], du[b] = mask[b] ? dy[b] : 0, with dystride the row pitch of dy
 *   mean_tokens: y[b][c] = mean_l x[b][l][c] (any C);  _bwd: dx[b][l][c] (+)= dy[b][c] / L
 *   colsum: db[c] (+)= sum_r x[r][c], fp32, any C;  colsum_batched: out[b * ldo + c] = sum_p x[b][p][c] (C % 8 == 0, C <= 8192),
 *     scratch of pea_op_colsum_batched_scratch_bytes; fixed summation order, no atomics
 *   copy2d: y[r][0:C] (+)= x[r][0:C] with row pitches ldx / ldy (ldx = 0: one row broadcast)
 *   transpose_bf16 / _f32_bf16: y[c * ldy + r] = x[r * C + c], any R, C, ldy >= R
 *   nhwc_to_nchw_f32 / nchw_f32_to_nhwc: bf16 [B][HW][C] <-> fp32 [B][C][HW], any sizes; dH, dW != 0: the bf16 side is stored
 *     depth-to-space ([B][dH/2][dW/2][(y&1)*2+(x&1)][C], dH * dW == HW)
 *   pad_gather: torch Linear weight src fp32 [N_t][K_t] -> bf16 w[st_n][ldw] (and wt[st_k][ldwt] = its transpose, or NULL) with
 *     heads padded from d to dp: mode 0 plain, 1 rows (row = head * dp + j), 2 columns, 3 rows interleaved (h_i, gate_i)
 *   pad_head_vec: dst[h * dp + j] = j < d ? src[h * d + j] : 0;  permute_geglu_vec: dst[2i] = src[i], dst[2i+1] = src[inner + i]
 *   cast_i64_f32;  fill_random_*: uniform [-scale, scale) (+ offset), a function of (seed, index) alone
 *   splitk_reduce: out[m * ldo + n] (+)= sum_s part[s * stride + m * N + n], bf16 out; N, ldo, stride multiples of 4
 *   rmsnorm_fwd: y = x * rsqrt(mean(x^2) + eps) * gamma;  layernorm_stats: stats[r] = (mean, rstd); C % 8 == 0, C <= 4096
 *   softmax_rows: s[r][0:cols] = softmax(scale * s[r][0:cols]) in place, row pitch ld
 *   residual_import: src [B][C][HW] fp32 (dtype 0) / bf16 (1), or bf16 [B][HW][C] (2) -> dst bf16 [B][HW][C] * scale
 *   vae_posterior: moments = quant_conv(h) (1x1, C2 even, <= 8; NCHW fp32), latents = (mean + exp(0.5 clamp(logvar, -30, 20)) *
 *     noise) * scaling; noise NULL = the mean; moments or latents may be NULL
 *   vae_post_quant: out = post_quant_conv(z * inv_scaling), 1 <= C <= 8
 *   embed_tokens: out[b][l] = tok[clamp(ids[b][l], 0, vocab - 1)] (+ pos[l] (+ type0)); pos NULL: T5; type0 NULL: CLIP
 *   t5_rel_bias: bias[h][q * pitch + k] = rel[bucket(k - q)][h] * log2(e), bucket(d) = (d > 0 ? half_buckets : 0) +
 *     dist_bucket[|d|] (device int[L]); columns [L, pitch) are not written
 *   gather_eos: out[b] = x[b][first l with ids[b][l] == eos_id, else L - 1]; eos_id < 0: the first argmax of ids[b]
 *   kv_len: len[b] = (index of the last id != pad_id) + 1, at least 1                                                    */
int pea_op_add(const void* a, const void* b, void* y, long long n, void* stream);
int pea_op_silu_fwd(const void* x, void* y, long long n, void* stream);
int pea_op_silu_bwd(const void* x, const void* dy, void* dx, long long n, int accum, void* stream);
int pea_op_gelu_fwd(const void* x, void* y, long long n, void* stream);
int pea_op_gelu_bwd(const void* x, const void* dy, void* dx, long long n, int accum, void* stream);
int pea_op_accum(const void* x, void* y, long long n, int accum, void* stream);
int pea_op_geglu_bwd_il(const void* hg, const void* dy, void* dhg, long long rows, int inner, void* stream);
int pea_op_select_rows(const void* c, const void* u, const void* mask, void* y, int B, long long per, long long ystride,
                       void* stream);
int pea_op_select_rows_bwd(const void* dy, const void* mask, void* dc, void* du, int B, long long per, long long dystride,
                           void* stream);
int pea_op_mean_tokens(const void* x, void* y, int B, int L, int C, void* stream);
int pea_op_mean_tokens_bwd(const void* dy, void* dx, int B, int L, int C, int accum, void* stream);
int pea_op_colsum(const void* x, float* db, int R, int C, int accum, void* stream);
long long pea_op_colsum_batched_scratch_bytes(int B, int HW, int C);
int pea_op_colsum_batched(const void* x, float* out, int B, int HW, int C, int ldo, void* scratch, void* stream);
int pea_op_copy2d(const void* x, int ldx, void* y, int ldy, long long rows, int C, int accum, void* stream);
int pea_op_transpose_bf16(const void* x, void* y, int R, int C, int ldy, void* stream);
int pea_op_transpose_f32_bf16(const float* x, void* y, int R, int C, int ldy, void* stream);
int pea_op_nhwc_to_nchw_f32(const void* x, float* y, int B, int HW, int C, int dH, int dW, void* stream);
int pea_op_nchw_f32_to_nhwc(const float* x, void* y, int B, int HW, int C, int dH, int dW, void* stream);
int pea_op_pad_gather(const float* src, int N_t, int K_t, int mode, int d, int dp, void* w, int ldw, void* wt, int ldwt, int st_n,
                      int st_k, void* stream);
int pea_op_pad_head_vec(const float* src, float* dst, int heads, int d, int dp, void* stream);
int pea_op_permute_geglu_vec(const float* src, float* dst, int inner, void* stream);
int pea_op_cast_i64_f32(const long long* x, float* y, long long n, void* stream);
int pea_op_fill_random_bf16(void* p, long long n, unsigned long long seed, float scale, void* stream);
int pea_op_fill_random_f32(float* p, long long n, unsigned long long seed, float scale, float offset, void* stream);
int pea_op_splitk_reduce(const float* part, int nsplit, long long stride, void* out, int ldo, int M, int N, int accum, void* stream);
int pea_op_rmsnorm_fwd(const void* x, const float* gamma, void* y, int R, int C, float eps, void* stream);
int pea_op_layernorm_stats(const void* x, float* stats, int R, int C, float eps, void* stream);
int pea_op_softmax_rows(void* s, long long rows, int cols, int ld, float scale, void* stream);
int pea_op_residual_import(const void* src, int dtype, void* dst, int B, int C, long long HW, float scale, void* stream);
int pea_op_vae_posterior(const float* h, const float* wq, const float* bq, const float* noise, float* moments, float* latents, int B,
                         int C2, long long HW, float scaling, void* stream);
int pea_op_vae_post_quant(const float* z, const float* w, const float* b, float* out, int B, int C, long long HW, float inv_scaling,
                          void* stream);
int pea_op_embed_tokens(const long long* ids, const void* tok, const void* pos, const void* type0, void* out, int B, int L, int width,
                        int vocab, void* stream);
int pea_op_t5_rel_bias(const float* rel, const int* dist_bucket, float* bias, int H, int L, int pitch, int half_buckets, void* stream);
int pea_op_gather_eos(const long long* ids, const void* x, void* out, int B, int L, int width, long long eos_id, void* stream);
int pea_op_kv_len(const long long* ids, int* len, int B, int L, long long pad_id, void* stream);


/* ========================================================================== model level ====
 * The three plug-in surfaces of the reference, as opaque handles.                               */

/* UNet2DConditionModel config (diffusers 0.23 names; `heads` is what diffusers calls
 * `attention_head_dim` for SDXL).  Arrays are in DOWN-block order, n_levels entries used.        */
typedef struct pea_unet_config {
  int in_channels, out_channels;
  int n_levels;
  int block_out[4];
  int down_cross[4];          /* 1 = CrossAttnDownBlock2D, 0 = DownBlock2D */
  int up_cross[4];            /* 1 = CrossAttnUpBlock2D,   0 = UpBlock2D  (UP order) */
  int layers_per_block;
  int depth[4];               /* transformer_layers_per_block */
  int heads[4];               /* attention heads; channels / heads must be 64 */
  int cross_dim;
  int linear_proj;            /* use_linear_projection */
  int groups;
  float eps;
  int text_time;              /* addition_embed_type == "text_time" */
  int add_time_dim;
  int proj_in_dim;
  /* per-position transformer depths (diffusers >= 0.22 configs such as SSD-1B, loaded as a downstream UNet at
   * tests/test_sdxl_zh.py:449-454).  per_layer_depth = 0: the arrays below are ignored and filled from depth[]
   * (every attention of a level has depth[level], the mid block depth[n_levels - 1], the up path mirrors the down path). */
  int per_layer_depth;
  int depth_down[4][4];       /* transformer_layers_per_block[i][j], DOWN order, j < layers_per_block */
  int depth_up[4][4];         /* reverse_transformer_layers_per_block[i][j], UP order, j <= layers_per_block */
  int depth_mid;              /* mid block transformer layers; -1: mid_block_type == null (no mid block at all) */
} pea_unet_config;

/* Builds the static op tape for a fixed (batch B, latent H x W, context length L) and allocates
 * its activations (all kept resident: 288 GB HBM) -- replaces `UNet2DConditionModel.from_pretrained`
 * (train_sdxl_zh.py:138,151).  needs_grad=1 adds the reverse data-gradient tape (student);
 * own_weights=0 creates a context that must borrow weights via pea_unet_share_weights (the
 * reference loads teacher and student from the same checkpoint, train_sdxl_zh.py:138 vs :151).    */
/* flags: PEA_UNET_GRAD (backward support) | PEA_UNET_RESIDUAL_INPUTS (ControlNet residual inputs, inference only)
 * | PEA_UNET_INPAINT_INPUTS (inpainting UNet, inference only: refused with PEA_UNET_GRAD and unless
 * in_channels == 2 * out_channels + 1; enables pea_unet_set_inpaint_cond) */
#define PEA_UNET_GRAD 1
#define PEA_UNET_RESIDUAL_INPUTS 2
#define PEA_UNET_INPAINT_INPUTS 4
int pea_unet_create(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int own_weights,
                    void** out);
/* Host-only planning pass of pea_unet_create (no device needed, nothing allocated): builds the op tape for the same
 * arguments and reports its size -- ops, weight tensors, parameters (torch numel), and the bytes the weight / activation
 * / gradient arenas will take in HBM.  Use it to size a configuration against 288 GB before creating it.   */
int pea_unet_plan(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int* n_ops, int* n_weights,
                  long long* n_params, long long* weight_bytes, long long* act_bytes, long long* grad_bytes);
/* Guidance-embedded UNets (`time_cond_proj_dim` of fully distilled LCM checkpoints such as LCM-SDXL; the reference's loop
 * computes the input at tests/test_sdxl_zh_inpaint.py:721-745).  The layout of pea_unet_config is frozen, so the width travels
 * beside it: pea_unet_create_cond / pea_unet_plan_cond are pea_unet_create / pea_unet_plan with time_cond_proj_dim (0: none,
 * what the two plain entry points forward; otherwise a multiple of 64, the GEMM's K tile, else PEA_E_SHAPE).  The graph gains
 * the bias-free Linear `time_embedding.cond_proj.weight` [block_out[0]][time_cond_proj_dim], whose output is added to the
 * sinusoidal timestep projection in front of time_embedding.linear_1 (inference and PEA_UNET_GRAD contexts alike; the input
 * receives no gradient).  pea_unet_plan_cond also reports the attention census of pea_unet_plan_attention (either may be NULL).
 * pea_unet_plan_weight: numel / kind / dims (as pea_unet_weight_info) of the weight `name` on the planned graph, PEA_E_NOTFOUND
 * when the graph has none of that name.
 * pea_unet_set_timestep_cond: cond fp32 [B][time_cond_proj_dim] on the device (`timestep_cond` of the UNet call), copied into
 * the context and in effect for every following pea_unet_forward; NULL clears it.  Unset or cleared, the projection
 * contributes nothing (diffusers with timestep_cond=None) and eps equals that of a plain UNet with the same weights bit for
 * bit.  PEA_E_STATE on a context created without a time_cond_proj_dim. */
int pea_unet_create_cond(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim,
                         int own_weights, void** out);
int pea_unet_plan_cond(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim, int* n_ops,
                       int* n_weights, long long* n_params, long long* weight_bytes, long long* act_bytes,
                       long long* grad_bytes, int* n_attn, int* n_prescaled);
int pea_unet_plan_weight(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim,
                         const char* name, long long* numel, int* kind, int* d0, int* d1);
int pea_unet_set_timestep_cond(void* unet, const float* cond, void* stream);
/* ... and the scratch buffers the same context allocates beside those arenas on first use (GroupNorm partials, attention
 * row constants and dK/dV split partials, the FF d(pre-activation) buffer, split-K partials of the stacked K|V projection,
 * fp32 time-embedding gradients).  bwd_batch > 0: a merged-pass context that differentiates its leading bwd_batch samples. */
int pea_unet_plan_scratch(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int bwd_batch,
                          long long* scratch_bytes);
/* Attention ops on a graph (any handle of this library that owns an op tape: UNet, ControlNet, VAE, text encoder) and how
 * many of them are fed a Q the producing projection already multiplied by softmax_scale * log2(e) (the accurate path: one
 * rounding, from the fp32 accumulator).  An op outside that count runs the operator-level plain-Q path, which rounds the
 * scaled operand to bf16 once more.  pea_unet_plan_attention: the same census from the host-only planning pass. */
int pea_tape_attention_census(void* graph, int* n_attn, int* n_prescaled);
int pea_unet_plan_attention(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int* n_attn, int* n_prescaled);
int pea_graph_plan_attention(int graph, const pea_unet_config* cfg, int B, int H, int W, int L, int* n_attn,
                             int* n_prescaled);          /* graph: 1 VAE encoder, 2 ControlNet, 3 VAE decoder */
/* ControlNet extras of the UNet call (tests/test_sdxl_zh_controlnet.py:534-535): `down_block_additional_residuals`
 * (conv_in output, then every down-block resnet/attention output and downsampler output, in diffusers order) followed
 * by `mid_block_additional_residual` LAST.  ptrs: HOST array of n device pointers ([B,C,H,W]; NULL entry = zero);
 * dtype 0 fp32 NCHW, 1 bf16 NCHW, 2 bf16 NHWC; values are multiplied by `scale` (conditioning_scale) on import and
 * stay in effect for every following pea_unet_forward until set again. */
int pea_unet_num_residuals(void* unet);
int pea_unet_residual_info(void* unet, int i, int* C, int* H, int* W);
int pea_unet_set_residuals(void* unet, int n, const void* const* ptrs, int dtype, float scale, void* stream);
/* Inpainting condition (tests/test_sdxl_zh_inpaint.py: the per-step `cat([cat([latents] * 2), mask, masked_image_latents], dim=1)`):
 * mask fp32 [cond_batch][1][H][W], masked_latents fp32 [cond_batch][out_channels][H][W], copied into the context once per
 * generation.  From then on the `x` of pea_unet_forward is the latents alone, [latent_batch][out_channels][H][W], and conv_in
 * reads channel groups of image b from latents[b % latent_batch], mask / masked_latents[b % cond_batch] (CFG: both B / 2).
 * cond_batch and latent_batch must each divide B.  Needs PEA_UNET_INPAINT_INPUTS.  pea_unet_clear_inpaint_cond: `x` is the
 * plain [B][in_channels][H][W] again. */
int pea_unet_set_inpaint_cond(void* unet, const float* mask, const float* masked_latents, int cond_batch, int latent_batch,
                              void* stream);
int pea_unet_clear_inpaint_cond(void* unet);
/* FreeU (diffusers 0.23 `pipe.enable_freeu(s1, s2, b1, b2)`; training-free, no weights).  In front of every skip concatenation of
 * up block 0 (factors s1, b1) and up block 1 (s2, b2) the first half of the hidden state's channels is multiplied by b and the
 * skip tensor goes through `fourier_filter(skip, threshold=1, scale=s)`: pea_op_freeu_coef + pea_op_concat2_freeu instead of the
 * plain concat, everything else unchanged.  ControlNet residuals are in the skips by then, as in diffusers.  The feature taps
 * u0 / u1 keep their unscaled values.  A runtime switch of a UNet context (graph 0): PEA_E_STATE on a PEA_UNET_GRAD context
 * (an inference feature, no backward through it), PEA_E_INVALID for a factor that is not finite and positive, PEA_E_SHAPE where
 * up block 0 or 1 works on a map with H < 2 or W < 2.  The coefficient buffer is allocated by the first call and survives
 * pea_unet_release_activations.  pea_unet_clear_freeu: the plain concat launches again, bit for bit. */
int pea_unet_set_freeu(void* unet, float s1, float s2, float b1, float b2, void* stream);
int pea_unet_clear_freeu(void* unet);
/* Image prompt (IP-Adapter, `ip-adapter_sdxl_vit-h` and its kin): every cross-attention layer gets a second, independent
 * key / value projection `to_k_ip` / `to_v_ip` over n_tokens image tokens (1..32) and runs the decoupled attention of
 * pea_op_attention_fwd_ip.  The UNet's own weights do not change.
 * pea_unet_ip_plan (host only): cross-attention layers, width of the stacked to_k_ip | to_v_ip projection (that of the text K|V
 * stack) and its parameter count.  pea_unet_ip_create allocates that stack ([cols][cross_dim] bf16; column layout identical to
 * the text stack: pea_unet_stacked_layout(which = 0) with to_k / to_v read as to_k_ip / to_v_ip) and the image K|V buffer
 * [B * n_tokens][cols] bf16, both outside the activation arena (they survive pea_unet_release_activations).  Refused: contexts
 * with PEA_UNET_GRAD (there is no backward through the image branch), ControlNet handles, configs with padded heads (head_dim
 * != 64), a context length above 128.
 * pea_unet_ip_load_weight: key `<attn2 prefix>.to_k_ip.weight` / `.to_v_ip.weight`, fp32 device [C][cross_dim].
 * pea_unet_ip_set_tokens: fp32 device [B][n_tokens][cross_dim] -> ONE GEMM into the image K|V buffer, once per image; from then
 * on every pea_unet_forward of this context runs the decoupled attention, with the scale of pea_unet_ip_set_scale (default 1,
 * read at launch; 0 launches the plain attention) until pea_unet_ip_clear.  pea_unet_ip_destroy frees the state.
 * pea_unet_ip_export_kv (parity instrumentation): the image K|V buffer as fp32 [rows][cols]; out may be NULL (sizes only). */
int pea_unet_ip_plan(const pea_unet_config* cfg, int n_tokens, int* n_layers, int* cols, long long* n_params);
int pea_unet_ip_create(void* unet, int n_tokens);
int pea_unet_ip_load_weight(void* unet, const char* key, const float* src, long long numel, void* stream);
int pea_unet_ip_set_tokens(void* unet, const float* tokens, void* stream);
int pea_unet_ip_set_scale(void* unet, float scale);
int pea_unet_ip_clear(void* unet);
int pea_unet_ip_destroy(void* unet);
int pea_unet_ip_export_kv(void* unet, float* out, long long* rows, int* cols, void* stream);
/* Several image prompts at once (a style adapter plus a face adapter, each with a scale, optional per-block scales and an
 * optional region mask): up to four adapters ("sets") with n_tokens[j] image tokens each, sum n_tokens <= 32 -- all sets share
 * one packed image K|V buffer [B][sum n_tokens][cols], set j in rows off_j .. off_j + n_tokens[j] of every sample, and every
 * cross-attention layer runs ONE launch of pea_op_attention_fwd_ipn over it.  The functions above are the one-set case of the
 * same state: pea_unet_ip_create(u, n) == pea_unet_ip_create_sets(u, 1, &n), load_weight / set_tokens / set_scale address set 0,
 * pea_unet_ip_clear clears every set, pea_unet_ip_export_kv returns the whole packed buffer.
 * pea_unet_ip_load_weight_set / _set_tokens_set / _set_scale_set / _clear_set: as their namesakes, for set `set`; set_tokens
 * takes fp32 device [B][n_tokens[set]][cross_dim] and fills only that set's rows.
 * pea_unet_ip_set_layer_scales: host float[n_layers], one factor per cross-attention layer in the order an adapter file numbers
 * them (ip_adapter.layer_keys: down blocks, up blocks, mid block); NULL = 1 everywhere.  The weight of set j in layer l is
 * scale_j * layer_scale_j[l], read at launch.  A set that is not live or weighs 0 in a layer is dropped from that layer's launch;
 * with none left the plain attention runs, with one left (and no mask) the one-set launch, bit for bit.
 * pea_unet_ip_query_counts (host only): the distinct query counts of the context's cross-attention layers (SDXL at 1024^2:
 * 4096 and 1024); counts may be NULL (the number only).
 * pea_unet_ip_set_mask: device fp32 [Bm][Sq] (Bm 1 = shared by the batch, or B), copied; Sq must be one of those counts; any
 * finite values.  NULL removes the mask of that count (Sq 0: all of the set).  A set with a mask for some counts but not for all
 * makes pea_unet_forward return PEA_E_STATE before any launch, naming the missing count. */
int pea_unet_ip_create_sets(void* unet, int n_sets, const int* n_tokens);
int pea_unet_ip_load_weight_set(void* unet, int set, const char* key, const float* src, long long numel, void* stream);
int pea_unet_ip_set_tokens_set(void* unet, int set, const float* tokens, void* stream);
int pea_unet_ip_set_scale_set(void* unet, int set, float scale);
int pea_unet_ip_clear_set(void* unet, int set);
int pea_unet_ip_set_layer_scales(void* unet, int set, const float* scales, int n_layers);
int pea_unet_ip_query_counts(void* unet, int* counts, int cap, int* n);
int pea_unet_ip_set_mask(void* unet, int set, int Sq, const float* mask, int Bm, void* stream);
int pea_unet_destroy(void* unet);

/* ControlNet (`self.controlnet(control_model_input, t, encoder_hidden_states=..., controlnet_cond=image,
 * conditioning_scale=..., guess_mode=False, added_cond_kwargs=..., return_dict=False)`,
 * tests/test_sdxl_zh_controlnet.py:510-519; diffusers 0.23 ControlNetModel [ext]) on the same op tape: the UNet's
 * conditioning, conv_in, down blocks and mid block + `controlnet_cond_embedding.*`, `controlnet_down_blocks.*`,
 * `controlnet_mid_block.*` (diffusers keys; handle works with the pea_unet_* weight functions and destroy).
 * set_cond: conditioning image fp32 [B,3,8H,8W]; its embedding is computed here, once per generation (the image does
 *   not change over the denoise steps), and reused by every forward.
 * forward: same conditioning arguments as pea_unet_forward; results stay in the context as bf16 NHWC tensors
 *   (pea_controlnet_output: down residuals in diffusers order, mid LAST) -- hand them to
 *   pea_unet_set_residuals(unet, n, ptrs, 2, conditioning_scale, stream). */
int pea_controlnet_create(const pea_unet_config* cfg, int B, int H, int W, int L, void** out);
int pea_controlnet_set_cond(void* cn, const float* image, void* stream);
int pea_controlnet_forward(void* cn, const float* x, const float* t, const void* ehs, int ehs_dtype, const void* text,
                           int text_dtype, const float* time_ids, void* stream);
int pea_controlnet_num_outputs(void* cn);
int pea_controlnet_output(void* cn, int i, void** ptr, int* C, int* H, int* W);
int pea_controlnet_export_nchw(void* cn, int i, float* dst, void* stream);   /* fp32 [B,C,H,W] copy of output i */

/* Text encoders in front of the step, on the same op tape; handle works with the pea_unet_* weight
 * functions (HF transformers keys).  flavor 0 = CLIPTextModel[WithProjection] -- the teacher's CLIP-L and OpenCLIP-bigG
 * (train_sdxl_zh.py:147-150; encode_prompt :170-285 takes `hidden_states[-2]` of both and the pooled output of the
 * second): pre-LN, causal mask, final LayerNorm, pooled = final[EOS position] @ text_projection.  flavor 1 = BERT -- the
 * Chinese-CLIP text tower (train_sdxl_zh.py:103-107; `self.text_encoder.encode_text(batch["input_ids"])` :327-329 returns
 * the per-token states): post-LN, right-padding mask from pad id `eos_id`.  head_dim must be 64 (true for all three).
 * forward: ids int64 [B,L] device; hidden_index -1 = last state (CLIP: after the final LayerNorm), -2 = hidden_states[-2],
 * k >= 0 = hidden_states[k]; hidden_out fp32 [B,L,width] and / or pooled_out fp32 [B,proj_dim] (CLIP only).
 * flavor 2 = T5 encoder stack -- the mT5 student option (`T5EncoderModel.from_pretrained('mt5-xl')`, train_sdxl_zh.py:108-112;
 * `self.text_encoder.encoder(ids, attention_mask=ids.ne(pad))[0]` :337-345; HF keys `shared.weight`, `encoder.block.N.*`,
 * `encoder.final_layer_norm.weight`): token embedding only, pre-RMSNorm blocks, scores = q.k (unscaled) + bucketed
 * relative-position bias of block 0, right-padding mask from pad id `eos_id`, gated FF wo(gelu_new(wi_0 x) * wi_1 x);
 * `intermediate` = d_ff; inner attention width = heads * 64 (d_kv must be 64).  hidden_index -1 = after the final RMSNorm. */
typedef struct pea_text_config {
  int vocab, max_pos, width, heads, layers, intermediate;
  int act;          /* 1 GELU(erf), 3 quick-GELU */
  int flavor;       /* 0 CLIP, 1 BERT, 2 T5 encoder (mT5: RMSNorm, relative position bias, unscaled scores, gated gelu_new FF) */
  int proj_dim;     /* CLIP text_projection width, 0 = none */
  float eps;
  int pos_offset;   /* position row = token index + pos_offset: 2 for RoBERTa / XLM-R towers (mul_clip, alt_clip), else 0 */
  long long eos_id; /* CLIP: EOS id (< 0: argmax of the ids); BERT / T5: pad id */
  int rel_buckets;  /* T5: relative_attention_num_buckets (32) */
  int rel_max_dist; /* T5: relative_attention_max_distance (128) */
} pea_text_config;
int pea_text_create(const pea_text_config* cfg, int B, int L, void** out);
int pea_text_plan_attention(const pea_text_config* cfg, int B, int L, int* n_attn, int* n_prescaled);   /* see pea_tape_attention_census */
int pea_text_forward(void* enc, const long long* ids, int hidden_index, float* hidden_out, float* pooled_out, void* stream);
/* T5 flavour only: the additive attention bias the encoder uses, bias_out fp32 [heads][L][L] =
 * relative_attention_bias[bucket(k - q)][h] * log2(e) (HF T5Attention.compute_bias; the attention kernels work in the
 * log2 domain).  Diagnostic read-back for the bucket parity test. */
int pea_text_rel_bias(void* enc, float* bias_out, void* stream);

/* CLIP vision tower (HF transformers CLIPVisionModelWithProjection) on the same op tape, inference only: the image half of
 * the CLIP pairs whose text half pea_text_* runs, for image-text similarity (CLIPScore) of decoded samples.  Keys
 * `vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight}`, `vision_model.pre_layrnorm.*`
 * (spelling as HF), `vision_model.encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1, mlp.fc2}.*`,
 * `vision_model.post_layernorm.*`, `visual_projection.weight`; the handle works with pea_unet_num_weights / weight_info /
 * load_weight / init_random / memory / destroy.
 *   rows = patchify(pixels) [B*Np][3 P P], column (c, py, px) (zero-padded to a multiple of 64, the GEMM's K tile: 588 -> 640)
 *   x[b][0] = class_embedding + pos[0];  x[b][1+i] = rows[b][i] . patch_w^T + pos[1+i];  hidden_states[0] = pre_layrnorm(x)
 *   `layers` pre-LN blocks, unmasked attention over Np + 1 tokens, scale head_dim^-0.5, MLP activation `act`
 *   pooler_output = post_layernorm(h_N[:, 0]);  image_embeds = pooler_output . visual_projection^T
 * head_dim = width / heads must be 64 (ViT-B/32, B/16, L/14) or 80 (ViT-H/14; stored zero-padded to 128 like the SD1.5 UNet's
 * heads), else PEA_E_SHAPE; width and intermediate multiples of 64, proj_dim a multiple of 4.
 * pea_vision_plan: host only (no device needed): parameter total, tokens per image (Np + 1), attention ops (= layers).
 * pea_vision_forward: pixels fp32 [B,3,S,S] (already normalised: pea_op_preprocess), device.  hidden_index as pea_text_forward:
 * -1 = the last state BEFORE post_layernorm (HF `last_hidden_state`), -2 = hidden_states[-2], k >= 0 = hidden_states[k].
 * Outputs, each optional (NULL): hidden_out fp32 [B,Np+1,width], pooled_out fp32 [B,width] (`pooler_output`), embeds_out
 * fp32 [B,proj_dim] (`image_embeds`). */
typedef struct pea_vision_config {
  int image_size, patch_size, width, heads, layers, intermediate;
  int act;          /* 1 GELU(erf), 3 quick-GELU */
  int proj_dim;     /* visual_projection width */
  float eps;
} pea_vision_config;
int pea_vision_create(const pea_vision_config* cfg, int B, void** out);
int pea_vision_plan(const pea_vision_config* cfg, int B, long long* n_params, int* n_tokens, int* n_attn);
int pea_vision_forward(void* enc, const float* pixels, int hidden_index, float* hidden_out, float* pooled_out, float* embeds_out,
                       void* stream);
/* Perceiver Resampler of the IP-Adapter "plus" files (ip-adapter-plus_sdxl_vit-h, ip-adapter-plus-face_sdxl_vit-h, the SD1.5
 * plus files) on the same op tape, inference only: the image projection between the tower's hidden_states[-2] (pea_vision_forward,
 * hidden_index -2) and the image tokens pea_unet_ip_set_tokens takes.  Keys as the files hold them under `image_proj.`: `latents`
 * ([1][Nq][dim], stored [Nq][dim]), `proj_in.*`, `proj_out.*`, `norm_out.*`, `layers.L.0.{norm1,norm2}.*`, `layers.L.0.{to_q,
 * to_kv,to_out}.weight`, `layers.L.1.0.*` (LayerNorm), `layers.L.1.1.weight`, `layers.L.1.3.weight`; the handle works with
 * pea_unet_num_weights / weight_info / load_weight / init_random / memory / destroy.
 *   x = proj_in(hidden);  latents = `latents` repeated over the batch
 *   per layer:  q = to_q(norm2(latents));  k, v = to_kv([norm1(x) ; norm2(latents)])  -- S + Nq keys under ONE softmax, 1 / 8
 *               latents += to_out(softmax(q k^T / 8) v);  latents += ff.3(gelu(ff.1(ff.0(latents))))     (GELU: erf form)
 *   tokens = norm_out(proj_out(latents))
 * to_kv runs where its rows are -- over the B S image rows, and stacked under to_q over the B Nq latent rows -- and
 * pea_op_attention_fwd_fewq reads both key / value sets in place: no concatenation, no copy.  Heads are 64 wide (the only width
 * the published files use); embed_dim, dim, ff_inner multiples of 64, out_dim a multiple of 8, 1 <= n_queries <= 32, else
 * PEA_E_SHAPE.  SDXL plus (ViT-H): {1280, 1280, 20, 4, 16, 5120, 2048}, S = 257, 82 961 664 parameters.
 * pea_resampler_plan: host only (no device needed): parameter total, attention ops (= depth), of those fed a prescaled Q (= depth).
 * pea_resampler_plan_weight: host only: entry i of the weight table a handle of this configuration has (fields as
 * pea_unet_weight_info); PEA_E_NOTFOUND past its end.
 * pea_resampler_forward: hidden fp32 [B][S][embed_dim] -> tokens_out fp32 [B][n_queries][out_dim], both on the device. */
typedef struct pea_resampler_config {
  int embed_dim, dim, heads, depth, n_queries, ff_inner, out_dim;
  float eps;
} pea_resampler_config;
int pea_resampler_create(const pea_resampler_config* cfg, int B, int S, void** out);
int pea_resampler_plan(const pea_resampler_config* cfg, int B, int S, long long* n_params, int* n_attn, int* n_prescaled);
int pea_resampler_plan_weight(const pea_resampler_config* cfg, int B, int S, int i, char* name, int name_len, long long* numel,
                              int* kind, int* d0, int* d1);
int pea_resampler_forward(void* resampler, const float* hidden, float* tokens_out, void* stream);
/* Image preprocessing in front of the tower: images fp32 [B,3,H,W] -> v = clamp((x - lo) / (hi - lo), 0, 1), with `quantize`
 * round(v * 255) / 255 (what a saved 8-bit image holds) -> antialiased bicubic resample with the definition of
 * torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False) (separable Keys kernel a = -0.5, support
 * 2 max(scale, 1), per-output weights normalised to sum 1) -> centre crop -> (v - mean[c]) / std[c] -> out fp32 [B,3,size,size].
 * The caller supplies one tap table per axis, DEVICE buffers covering the `size` CROPPED output coordinates: coordinate i reads
 * source coordinates first[i] .. first[i] + count[i] - 1 with weights[i * taps + k] (zero past count[i]); and the tiling: one
 * workgroup produces tile_h x tile_w outputs (tile_w % 4 == 0) from a source window of at most win_h x win_w pixels (win_w % 4
 * == 0, its first column rounded down to a multiple of 4) staged in LDS: 4 (win_h win_w + win_h tile_w + tile_w x_taps +
 * tile_h y_taps) bytes <= 64 KiB, else PEA_E_SHAPE.  pea_diffusion_amd/vision.py builds both from (H, W, size) in float64. */
int pea_op_preprocess(const float* images, int B, int H, int W, float lo, float hi, int quantize, const int* y_first,
                      const int* y_count, const float* y_weights, int y_taps, const int* x_first, const int* x_count,
                      const float* x_weights, int x_taps, int size, int tile_h, int tile_w, int win_h, int win_w, float mean0,
                      float mean1, float mean2, float std0, float std1, float std2, float* out, void* stream);
/* pixels fp32 [B,3,S,S] -> rows bf16 [B*(S/P)^2][kpad] (the patch GEMM's A operand): column (c, py, px) = the conv weight
 * flattened, columns >= 3 P P zero; kpad >= 3 P P, a multiple of 8.  A gather and one rounding. */
int pea_op_patchify(const float* pixels, void* rows, int B, int S, int P, int kpad, void* stream);
/* CLIPScore (Hessel et al. 2021): out[b] = w * max(cos(image_embeds[b], text_embeds[b]), 0); clamp = 0 keeps negative cosines
 * (w = 1: the plain cosine).  fp32 [B,D] inputs, fp32 [B] output; norms floored at 1e-8 as torch.cosine_similarity does; one
 * wave per pair with a fixed reduction order: bit-reproducible run to run. */
int pea_op_clip_score(const float* image_embeds, const float* text_embeds, float* out, int B, int D, float w, int clamp,
                      void* stream);

/* VAE encoder (AutoencoderKL.encode, train_sdxl_zh.py:306-309; train_sd_zh.py:188-189) on the same op tape: cfg uses
 * in_channels (3), out_channels (2 * latent channels = 8), n_levels, block_out, layers_per_block, groups, eps.
 * The handle works with pea_unet_num_weights / weight_info / load_weight / init_random / memory / destroy (diffusers
 * keys `encoder.*`, `quant_conv.*`).  pea_vae_encode: pixels fp32 [B,3,H,W] -> moments = quant_conv(encoder(x))
 * fp32 [B,2L,h,w] (optional) and latents = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scaling fp32 [B,L,h,w]
 * (`.latent_dist.sample() * vae.config.scaling_factor`; noise NULL = `.mode()`). */
int pea_vae_encoder_create(const pea_unet_config* cfg, int B, int H, int W, void** out);
int pea_vae_latent_shape(void* vae, int* C, int* H, int* W);
int pea_vae_encode(void* vae, const float* pixels, const float* noise, float scaling, float* moments, float* latents,
                   void* stream);
/* VAE decoder (`image = self.vae.decode(latents / self.vae.config.scaling_factor, return_dict=False)[0]`,
 * tests/test_sdxl_zh.py:430): cfg.in_channels = latent channels, out_channels = image channels, block_out = the
 * AutoencoderKL block_out_channels; H x W = LATENT size; diffusers keys `decoder.*`, `post_quant_conv.*`.
 * latents fp32 [B,4,h,w] (multiplied by inv_scaling first) -> image fp32 [B,3,8h,8w]. */
int pea_vae_decoder_create(const pea_unet_config* cfg, int B, int H, int W, void** out);
int pea_vae_decode(void* vae, const float* latents, float inv_scaling, float* image, void* stream);
int pea_unet_num_weights(void* unet);
/* diffusers state-dict key + torch shape (d0,d1; conv adds [3][3]) of weight i; kind: 0 vector,
 * 1 linear [d0][d1] (1x1 convs included), 2 conv3x3 [d0][d1][3][3], 3 conv_in, 4 conv_out         */
int pea_unet_weight_info(void* unet, int i, char* name, int name_len, long long* numel, int* kind, int* d0, int* d1);
/* src: DEVICE fp32, torch layout, `numel` elements; converted to the internal bf16 layouts      */
int pea_unet_load_weight(void* unet, const char* name, const float* src, long long numel, void* stream);
/* pea_unet_load_weight of `base + sum_i scales[i] * ups[i] . downs[i]` (LoRA fusion): composed in fp32 (pea_op_lora_compose)
 * BEFORE the conversion to the internal bf16 layouts, so the fused weight is rounded once.  base: DEVICE fp32 [numel], torch
 * layout; downs / ups / ranks / scales: HOST arrays of n_adapters entries; downs[i]: DEVICE fp32 [ranks[i]][numel / d0],
 * ups[i]: DEVICE fp32 [d0][ranks[i]] (d0 of pea_unet_weight_info), scales[i] = lora_scale * alpha / rank.  Argument errors
 * (n_adapters < 1, a rank outside 1..256, null pointers), a vector weight, a numel that is not the weight's and a context
 * that borrows its weights are refused before any device work.                                       */
int pea_unet_load_weight_lora(void* unet, const char* name, const float* base, long long numel, int n_adapters,
                              const float* const* downs, const float* const* ups, const int* ranks, const float* scales,
                              void* stream);
/* random weights of this architecture (no checkpoints exist in the image)                        */
int pea_unet_init_random(void* unet, unsigned long long seed, void* stream);
int pea_unet_share_weights(void* dst, void* src);
/* unet(sample, t, encoder_hidden_states, added_cond_kwargs={text_embeds,time_ids})[0]
 * (train_sdxl_zh.py:397,415; tests/test_sdxl_zh.py:384-391).  x, eps_out: fp32 NCHW [B][4][H][W];
 * t: fp32 [B]; ehs: [B][L][cross_dim], text: [B][pooled], dtype 0 = fp32, 1 = bf16; time_ids fp32 [B][6]. */
int pea_unet_forward(void* unet, const float* x, const float* t, const void* ehs, int ehs_dtype, const void* text,
                     int text_dtype, const float* time_ids, float* eps_out, void* stream);
/* feature taps in the order of the reference's cast_hook (train_sdxl_zh.py:79-84): d0.., m, u0..  */
int pea_unet_num_taps(void* unet);
/* hook name of tap k: "d<i>" (down_blocks[i], the hidden state of its (hidden, res_samples) tuple), "m" (mid_block;
 * absent when the config has no mid block), "u<i>" (up_blocks[i])                                     */
int pea_unet_tap_name(void* unet, int k, char* name, int name_len);
/* shape of tap k and (optionally) its raw storage pointers.  A tap that is stored depth-to-space (pea_unet_tap_layout == 1)
 * hands out raw pointers only after pea_unet_tap_layout has been called on this context (PEA_E_STATE otherwise): the
 * shape alone does not reveal the storage order.                                                                   */
int pea_unet_tap_info(void* unet, int k, void** data, void** grad, int* B, int* H, int* W, int* C);
int pea_unet_tap_export_nchw(void* unet, int k, int grad, float* out, void* stream);
/* Storage layout behind pea_unet_tap_info's pointers: 0 = NHWC [B][H][W][C]; 1 = depth-to-space [B][H/2][W/2][(y&1)*2+(x&1)][C]
 * (the output of an upsampler conv in its sub-pixel form -- Upsample2D = interpolate(2x nearest) + conv, diffusers
 * resnet.py; reference call site: the u<i> hooks of train_sdxl_zh.py:79-84).  -1 = bad handle / index.  The NCHW export above
 * and the import below hide the layout; only callers that touch the raw pointers need it.                                  */
int pea_unet_tap_layout(void* unet, int k);
/* write a gradient seed for tap k (fp32 NCHW [B or bwd_batch][C][H][W]) into the tap's gradient buffer in its storage layout;
 * then pass bit k in pea_unet_backward's tap_seed_mask                                                                   */
int pea_unet_tap_import_grad_nchw(void* unet, int k, const float* src, void* stream);
/* reverse pass: d(loss)/d(eps) in `deps` (fp32 NCHW, may be NULL) plus tap gradient seeds already
 * written into the tap grad buffers for every k with bit k set in tap_seed_mask.  Results:
 * pea_unet_input_grads -> bf16 d(ehs) [B][L][cross], d(text_embeds) [B][pooled].                 */
int pea_unet_backward(void* unet, const float* deps, unsigned tap_seed_mask, void* stream);
int pea_unet_input_grads(void* unet, void** d_ehs, void** d_text);
/* resident bytes: weights; activations and gradients (allocated on the first forward / backward, 0 before) */
/* Parity instrumentation: gradients of the two STACKED projections after the last backward pass, per layer.  which 0: all
 * cross-attention to_k / to_v projections (one GEMM over encoder_hidden_states; diffusers Attention.to_k/to_v of every
 * BasicTransformerBlock under train_sdxl_zh.py:397): d(K|V) fp32 [rows][cols], rows = differentiated samples x context length;
 * which 1: all ResnetBlock2D.time_emb_proj layers (one GEMM over silu(emb)): fp32 [differentiated samples][cols].  out may be
 * NULL (sizes only; PEA_E_NOTFOUND for which 1 with a buffer on a graph whose time embedding receives no gradient, e.g. SD1.5).
 * pea_unet_stacked_layout: diffusers weight key and column block of member i; PEA_E_NOTFOUND past the end. */
int pea_unet_stacked_grad(void* unet, int which, float* out, long long* rows, int* cols, void* stream);
int pea_unet_stacked_layout(void* unet, int which, int i, char* name, int name_len, int* col_off, int* cols);
int pea_unet_memory(void* unet, long long* weight_bytes, long long* act_bytes, long long* grad_bytes, int* n_ops);
/* Free the activation / gradient arenas and scratch of a context (weights stay); the next forward allocates them again.
 * Pointers handed out by pea_unet_tap_info / pea_unet_input_grads become invalid.  Synchronises the device. */
int pea_unet_release_activations(void* unet);

/* The PEA adapter `MLP(in_dim, out_dim, hidden_dim, out_dim1, use_residual)` (train_sdxl_zh.py:43-67);
 * out_dim1 = 0 selects the SD1.5 variant (train_sd_zh.py:41-56).  Parameters live in ONE flat fp32
 * device buffer owned by the caller, in state_dict order (layernorm.weight, layernorm.bias,
 * projector.0.weight, projector.2.weight, projector.4.weight, fc.weight, fc.bias).               */
int pea_adapter_create(int in_dim, int out_dim, int hidden_dim, int out_dim1, int use_residual, void** out);
int pea_adapter_destroy(void* ad);
long long pea_adapter_num_params(void* ad);
int pea_adapter_bind(void* ad, float* flat_params);
int pea_adapter_prepare(void* ad, int batch, int L);     /* rows = batch * L */
int pea_adapter_sync(void* ad, void* stream);            /* refresh bf16 working copies after an update */
/* x1, x2 = proj(x): enc [batch][L][in] (dtype 0 fp32 / 1 bf16) -> pooled fp32 [batch][out] (may be NULL),
 * tokens fp32 [batch][L][out1]                                                                   */
int pea_adapter_forward(void* ad, const void* enc, int dtype, float* pooled, float* tokens, void* stream);
/* grads (flat fp32, same layout as the parameters) (+)= backward of the last forward             */
int pea_adapter_backward(void* ad, const float* d_pooled, const float* d_tokens, float* grads, int accumulate,
                         void* stream);

/* The fused KD training step (train_sdxl_zh.py:311-441 downstream of the frozen encoders).       */
int pea_trainer_create(void* adapter, void* student, void* teacher, float feat_weight, int nan_guard,
                       const float* alphas_cumprod, void** out);
int pea_trainer_destroy(void* tr);
/* latents/noise fp32 [B][4][H][W]; timesteps int64 [B]; enc/enc_uncond fp32 [B][L][in]; prompt_mask uint8 [B];
 * zh_or_not int64 [B]; teacher_ehs/teacher_neg fp32 [B][Lt][cross]; teacher_pooled fp32 [B][pooled] or NULL;
 * time_ids fp32 [B][6] or NULL.  grads: flat fp32 adapter gradients; losses fp32[4] device =
 * (loss, train_loss, train_loss_logits, train_loss_features).                                    */
int pea_train_step(void* tr, const float* latents, const float* noise, const long long* timesteps,
                   const float* enc, const float* enc_uncond, const unsigned char* prompt_mask,
                   const long long* zh_or_not, const float* teacher_ehs, const float* teacher_neg,
                   const float* teacher_pooled, const float* time_ids, float grad_scale, float* grads,
                   int accumulate, float* losses, void* stream);
/* options: "two_stream" (1 = teacher forward on a side HIP stream, default), "nan_guard", "merge_passes" (default 1:
 * when the teacher context shares the student's weights -- the reference default, train_sdxl_zh.py:138,151 -- and the
 * context lengths agree, both UNet forwards run as ONE pass over 2B samples and the backward differentiates the
 * first B; otherwise the two-stream path is used);
 * "live_teacher_mask" (dead-row elimination, opt-in, merged passes at B <= 30): bit i set = sample i's teacher row is
 * computed, -1 = all (default).  CONTRACT: bit i may only be cleared for a sample whose zh_or_not[i] != 0 (its KD weight
 * 1 - zh_or_not is zero, train_sdxl_zh.py:402-441).  The mask is host state and zh_or_not is device memory, so the library
 * cannot compare them before the step; a sample that carries KD weight without a teacher row makes the loss kernel emit
 * NaN for the losses and for that sample's gradient seeds (never another sample's row). */
int pea_trainer_set_option(void* tr, const char* name, int value);
/* the UNet context whose backward pass ran in the last step (the merged-pass context when the teacher is the student
 * checkpoint, else the student's): handle for pea_unet_stacked_grad.  Owned by the trainer. */
int pea_trainer_backward_context(void* trainer, void** unet);
int pea_trainer_get_option(void* trainer, const char* name);   /* also "merge_state": 0 undecided, 1 merged, -1 n/a; "kd_samples_hint" (set: profiling only -- samples with zh_or_not == 0, for the KD-loss kernel's byte count) */
/* pea_unet_release_activations on the trainer's student, teacher and merged-pass contexts.  The reference trains over
 * nine aspect-ratio buckets (utils/custom_dataset_sdxl.py:30, one bucket per batch): a caller keeps one trainer per
 * bucket -- all sharing one set of weights and one adapter -- and releases the least recently used when HBM runs short
 * (pea_diffusion_amd/train.py: BucketedTrainer). */
int pea_trainer_release_activations(void* trainer);
/* intermediate results of the last step (fp32 NCHW [B][4][H][W]): which 0 = x_t, 1 = eps_student, 2 = eps_teacher */
int pea_trainer_export(void* tr, int which, float* out, void* stream);

/* Data-parallel collective (replaces DeepSpeed ZeRO-1's gradient all-reduce + parameter
 * all-gather, train_sdxl_zh.sh:22,87 and utils/model_utils.py:57-67): one process per GPU, ONE RCCL all-reduce (sum, then
 * x 1/world) over the flat fp32 adapter gradient per step, on a dedicated HIP stream owned by the communicator.
 *   pea_comm_unique_id: rank 0 creates the 128-byte ncclUniqueId; the caller ships it to the other ranks (TCP store / file).
 *   pea_comm_init:      BLOCKING rendezvous (ncclCommInitRank) on the calling thread's current HIP device, bounded:
 *                       pea_comm_init_timeout waits at most `timeout_s` seconds (<= 0: forever) for all `world` ranks and
 *                       returns PEA_E_TIMEOUT past that (the reference's deadline is torch.distributed.run's rendezvous,
 *                       train_sdxl_zh.sh:108-113); the rendezvous thread cannot be cancelled, so after PEA_E_TIMEOUT the process
 *                       must exit (non-zero).  pea_comm_init = the same with PEA_COMM_TIMEOUT_S from the environment (600).
 *                       A process holds ONE trainer / communicator at a time: the RCCL binding and the profiler tables are
 *                       process-global.
 *   pea_allreduce_grads: asynchronous.  The comm stream first waits for everything enqueued on `compute_stream` so far
 *                        (the adapter wgrad), then all-reduces `grads` in place and scales by 1/world.
 *   pea_comm_join:      makes `stream` wait for the last all-reduce (call before the optimizer reads `grads`).
 *   pea_comm_last_ms:   BLOCKING; device time of the last all-reduce + scale in milliseconds.
 *   pea_comm_last_exposed_ms: BLOCKING; how long the first stream that joined the last all-reduce stood still for it
 *                       (0 when the collective had finished before the stream reached the join).
 *   pea_comm_broadcast: parameter broadcast from `root` (identical replicas at start), enqueued on `stream`.      */
int pea_comm_unique_id(void* out128);
int pea_comm_init(int rank, int world, const void* unique_id128, void** comm_out);
int pea_comm_init_timeout(int rank, int world, const void* unique_id128, double timeout_s, void** comm_out);
int pea_comm_destroy(void* comm);
int pea_comm_world(void* comm);
int pea_comm_rank(void* comm);
int pea_allreduce_grads(void* comm, float* grads, long long n, void* compute_stream);
int pea_comm_join(void* comm, void* stream);
int pea_comm_last_ms(void* comm, float* ms);
int pea_comm_last_exposed_ms(void* comm, float* ms);
int pea_comm_broadcast(void* comm, float* buf, long long n, int root, void* stream);

/* per-launch HIP-event timing by kernel family (bench.py roofline leg); families 0..7:
 * gemm<plain>, gemm<conv3x3>, attn_fwd, attn_bwd, groupnorm, layernorm, elementwise, kd_loss.
 * pea_prof_report synchronises the device.                                                       */
void pea_prof_enable(int on);
void pea_prof_reset(void);
const char* pea_prof_family_name(int fam);
/* CSV of every recorded launch: family, ms, flops, bytes, shape tags (GEMM: M,N,K,epilogue flags) */
int pea_prof_dump(const char* path);
int pea_prof_report(int fam, double* ms, double* flops, double* bytes, long long* launches);
/* Sustained MFMA ceiling of this device: v_mfma_f32_16x16x32_bf16 (shape32 = 1: 32x32x16) issued back to back from registers on
 * random operands, two waves per SIMD on every CU, launches back to back for `seconds` (<= 30; default 2); *tflops = the last
 * launch's FLOP/s from HIP events, *clock_mhz = its in-kernel clock (delta s_memtime / delta s_memrealtime x 100 MHz, median over
 * the workgroups).  Synchronises the stream.  bench.py reports it as roofline.sustained_peak beside the 2.5 PFLOP/s spec peak. */
int pea_probe_mfma_peak(double seconds, int shape32, double* tflops, double* clock_mhz, void* stream);

/* debugging aid for the parity tests: 1 = ds_read_b64_tr_b16 transpose reads (default), 0 = scalar gathers */
void pea_debug_set_attn_tr(int v);
/* A/B aid: 1 = dQ and dK/dV workgroups of an attention backward in ONE launch (default), 0 = two launches */
void pea_debug_set_attn_fused_bwd(int v);
/* 0: cross-attention backward (<= 128 keys, head_dim 64) on the general kernels instead of the one-pass kernel (A/B) */
void pea_debug_set_attn_xattn(int v);
/* which one-pass cross-attention backward kernel (A/B, parity tests): 0 = the round-3 kernel for every key count; 2 = the
 * specialised-wave kernel (33..96 keys, 7 products); 1 or 3 = the newest that applies (default): the five-product kernel for
 * 33..80 keys, the specialised-wave kernel for 81..96 */
void pea_debug_set_xattn_bwd_v2(int v);
/* A/B aid: 1 = GEGLU backward inside the FF output projection's dgrad GEMM (default), 0 = its own kernel */
void pea_debug_set_geglu_bwd_fused(int v);
/* benchmark aid: force GEMM tile variant (>= 0) or restore the shape-based choice (-1) */
void pea_debug_set_gemm_variant(int v);
/* Test aid, needs no device: which kernel instantiation launch_gemm launches for a problem.  Returns the launcher's enumerator:
 * a variant id of the table (18 .. 41), 100 + id for the fused GEGLU-backward kernels (127, 128, 131), 200 + id for the
 * folded-LayerNorm kernels (224, 225, 227, 228, 231).  mode: 0 GEMM, 1 conv gather; rows_per_batch: rows per sample of the row
 * vector (<= 0: M); cus: CUs the launch may occupy (PEA_CU_LIMIT halves it); forced: a pinned variant id or -1.
 * features: 1 residual, 2 row vector, 4 fp32 output, 8 activation, 16 pre-activation stash (with GEGLU: C takes the stash,
 * without the bit a GEGLU problem has no C), 32 GEGLU output, 64 fused GEGLU backward, 128 folded-LayerNorm statistics,
 * 256 column scale, 512 split-K, 1024 pointers 16-byte aligned and row strides multiples of 8 (else 4-byte / multiples of 4).
 * M <= 0: the N-th entry of the enumerator list instead (-1 past its end). */
int pea_debug_gemm_dispatch(int M, int N, int K, int mode, int rows_per_batch, int features, int cus, int forced);
/* Test aid, needs no device: what launch_attention_fwd / _bwd / _fwd_fewq launch for a problem (shape checks included).
 * q[14] = { direction (0 forward, 1 backward, 2 few-query forward), B, H, Sq, Skv, nd, features, Skv2, image key sets, bit j: set j
 * has a mask, then the four switches or -1 for the process's own: pea_debug_set_xattn_bwd_v2, _attn_tr, _attn_xattn,
 * _attn_fused_bwd }.  features: 1 causal, 2 per-sample key counts, 4 score bias, 8 prescaled Q, 16 a second key set (K2 / V2 with
 * Skv2 keys, shared evenly among the sets), 32 every set weight 0, 64 / 128 / 256 dQ / dK / dV wanted, 512 split scratch passed,
 * 1024 gradients accumulate.  Returns PEA_OK and out[0] = launches (<= 3), out[1] = query-range splits, then per launch 7 ints at
 * out[2 + 7 i]: enumerator, grid x / y / z, dynamic LDS bytes, two scalar arguments (units per workgroup; or dQ and dK/dV blocks
 * per head of the fused backward); or the error code of a refused problem (pea_last_error has the text).  out holds 23 ints.
 * Enumerators: 0 + 4 f + (KB - 1) xattn_fwd_kernel<KB> (f: 0 plain, 1 one image key set, 2 several); 12 + 6 MODE + 3 TR + (ND - 1)
 * attn_q_kernel (MODE 1: dQ); 24 its masked instance; 25 + 3 TR + (ND - 1) attn_dkv_kernel; 31 + 3 TR + (ND - 1)
 * attn_bwd_fused_kernel; 37 + (KB - 1) xattn_bwd_kernel; 41 / 45 + 2 (KB - 2) + PRE xattn_bwd2_kernel / xattn_bwd3_kernel;
 * 49 attn_fewq_kernel; 50 attn_delta_kernel; 51 attn_dkv_reduce_kernel.  direction outside 0..2: the q[1]-th enumerator (-1 past the end). */
int pea_debug_attn_dispatch(const int* q, int* out);
/* timing-only probes of the loader/consumer GEMM (results are wrong while set): 1 no DMA, 2 no barriers, 4 no ds_reads */
void pea_debug_set_gemm_debug(int v);
/* experiment aid (scripts/chain_probe.py): arms the NEXT GEMM / conv launch with a prefetch target -- its DMA waves touch
 * [p, p + bytes) behind their last K-step (the product's tapes set the next launch's weight matrix themselves: GemmP::pf_ptr) */
void pea_debug_set_gemm_prefetch(const void* p, long long bytes);

/* ---- regional text prompts ("regional prompter" / "attention couple"): every region of the picture its own text prompt.
 * pea_op_attention_fwd_regions: O[b][q] = sum_r w[b][r][q] softmax(scale Q K_r^T) V_r, r < R, in ONE launch, forward only, head_dim
 * 64.  K / V: bf16 [B][R * Lr][ldk / ldv], region r in rows r Lr .. (r + 1) Lr of every sample -- what a context of R prompts of Lr
 * tokens leaves in a K|V projection.  1 <= R <= 4, 1 <= Lr <= 96, any Sq >= 1.  w: device fp32 [Bw][R][Sq], Bw 1 (shared by the
 * batch) or B; any finite values, NOT normalised by the kernel (pea_diffusion_amd/regional.py: region_weights makes them sum to
 * 1 per query).  Every region has a softmax of its own (own maximum, own sum).  A region whose weight is 0 on all 32 queries of
 * a wave is skipped by that wave (contribution exactly zero); one-hot weights on region r give the bits of pea_op_attention_fwd
 * on that region's rows; queries whose weights are all 0 come out as zeros.  No atomics: the same bits every run.  ld* and
 * alignment as for pea_op_attention_fwd_ip (multiples of 8 holding every head, ldo a multiple of 4; Q / K / V 16-byte, O 8-byte
 * aligned).  Every refusal is PEA_E_SHAPE before any launch. */
int pea_op_attention_fwd_regions(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                                 int Sq, int R, int Lr, const float* w, int Bw, float scale, int q_prescaled, void* stream);
/* The same in a UNet context (graph 0, inference) whose context length is L = R * Lr: while regions are set, every cross-attention
 * layer runs ONE launch of pea_op_attention_fwd_regions over its columns of the stacked K|V projection, with the weights of its own
 * query count.  pea_unet_set_prompt_regions sets the weights of ONE query count (device fp32 [Bw][R][Sq], copied into a buffer
 * outside the arenas; Sq one of pea_unet_ip_query_counts); R must be the same in every call until pea_unet_clear_prompt_regions.
 * A forward then needs weights for every count of pea_unet_ip_query_counts, L % R == 0 and L / R <= 96 (PEA_E_STATE / PEA_E_SHAPE
 * before the first launch).  PEA_E_STATE: a PEA_UNET_GRAD context, live image prompts (pea_unet_ip_set_tokens), per-sample context
 * lengths.  After pea_unet_clear_prompt_regions a forward gives the bits it gave before.  The tape, the plans and the arenas do
 * not change; pooled embeds and time ids stay the caller's. */
int pea_unet_set_prompt_regions(void* unet, int R, int Sq, const float* w, int Bw, void* stream);
int pea_unet_clear_prompt_regions(void* unet);
/* Test aid, needs no device: what pea_op_attention_fwd_regions launches (shape checks included).  q[8] = { B, H, Sq, R, Lr, nd,
 * ldk (<= 0: 64 H, like every other leading dimension), Bw (<= 0: 1) }.  Returns PEA_OK and out[6] = { KB (the instantiation
 * xattn_regions_fwd_kernel<KB>), grid x / y / z, dynamic LDS bytes, 128-query units per workgroup }, or the error code of a
 * refused problem.  LDS = R KB 2 4096 + 4 4096 + 4 4096 bytes (keys and values, the O images, the Q images). */
int pea_debug_attn_regions_dispatch(const int* q, int* out);

/* ---- cross-attention heat maps ("DAAM", diffusion attentive attribution maps): where in the picture each prompt token acts.
 * pea_op_attention_maps: maps[b][key][q] (op)= (1 / H) sum_h softmax_key(scale Q[b, q, h, :] . K[b, key, h, :]) in ONE launch, head_dim
 * 64, no V / O / lse.  maps: device fp32 [B][Skv][Sq], so one key's map is one contiguous image of the layer's latent grid.
 * 1 <= Skv <= 128, any Sq >= 1.  (op) is a store, or with accumulate != 0 a += done by the one thread that owns the element
 * (load, one fp32 add, store; no atomics).  q_prescaled: Q arrives multiplied by scale * log2(e), as for pea_op_attention_fwd.
 * kv_len: NULL or device int [B], 1 <= kv_len[b] <= Skv; the maps of keys at or past it are exact zeros (with accumulate: + 0).
 * The probabilities are never rounded to bf16: exp2 and the normalisation are fp32.  Sum over heads in a fixed order (wave w of
 * the workgroup's eight takes heads w, w + 8, ... in ascending order; the eight partial sums are added in wave order,
 * (((w0 + w1) + w2) + ...) + w7, then x 1 / H): the same bits every run.  ldq / ldk multiples of 8 holding every head, Q / K 16-byte aligned.  Every refusal is PEA_E_SHAPE
 * before any launch. */
int pea_op_attention_maps(const void* Q, int ldq, const void* K, int ldk, float* maps, int B, int H, int Sq, int Skv, float scale,
                          int q_prescaled, const int* kv_len, int accumulate, void* stream);
/* The same in a UNet context (graph 0, inference): while enabled, every selected cross-attention layer is followed by ONE launch of
 * pea_op_attention_maps (accumulate = 1) over its own Q and its columns of the stacked K|V projection, into the accumulator of its
 * query count: fp32 [B][L][Sq], one per count of pea_unet_ip_query_counts, zeroed, outside the arenas
 * (pea_unet_release_activations keeps them).  layer_on: NULL (every cross-attention layer) or n_layers floats in the order of the
 * IP-Adapter files' layers (pea_unet_ip_set_layer_scales), non-zero = capture.  The ordinary attention launch, the tape, the plans
 * and the arenas do not change: a forward gives the bits it gives without capture.  With image prompts the maps are those of the
 * text softmax (the decoupled attention's text term does not depend on the image keys); per-sample context lengths mask as in
 * the layer.  Refused: a PEA_UNET_GRAD context (PEA_E_STATE), any other graph than a UNet (PEA_E_INVALID), padded heads or a
 * context longer than 128 rows (PEA_E_SHAPE); a forward with prompt regions set while capture is on (PEA_E_STATE).
 * pea_unet_reset_attention_maps zeroes the accumulators (on `stream`) and their counters; pea_unet_disable_attention_maps
 * synchronises the device and frees them.  pea_unet_attention_maps: the accumulator of one query count and how many
 * layer-forwards have been added to it since the last reset -- a host counter of launches issued, so a forward replayed from a
 * captured graph is not counted.  Enable before a denoising loop and read after it: the sums then run over layers and steps. */
int pea_unet_enable_attention_maps(void* unet, const float* layer_on, int n_layers);
int pea_unet_reset_attention_maps(void* unet, void* stream);
int pea_unet_disable_attention_maps(void* unet);
int pea_unet_attention_maps(void* unet, int Sq, float** maps, long long* n_accumulated);
/* Test aid, needs no device: what pea_op_attention_maps launches (shape checks included).  q[8] = { B, H, Sq, Skv, nd, ldq (<= 0:
 * 64 H), ldk (<= 0: 64 H), flags (1: kv_len, 2: accumulate, 4: q_prescaled) }.  Returns PEA_OK and out[6] = { KB (the instantiation
 * xattn_maps_kernel<KB>, ceil(Skv / 32)), grid x / y / z, dynamic LDS bytes, 32-query units per workgroup }, or the error code of a
 * refused problem.  grid = ceil(Sq / 32) x B x 1, workgroups of 512 threads; LDS = 8 waves x (KB + 1) x 4096 bytes. */
int pea_debug_attn_maps_dispatch(const int* q, int* out);

/* ---- prompt-to-prompt editing (Hertz et al.): keep the picture, change one word.  A batch holds N prompts denoised from the same
 * initial latents; sample b with src[b] = s >= 0 is edited with the unedited sample s as its source (src[b] < 0, or src[b] = b,
 * a sample that is its own source: not edited).
 * pea_op_attention_fwd_edit, ONE launch over the whole batch, forward only, head_dim 64, 1 <= Skv <= 96, any Sq >= 1, B <= 32:
 *   edited b:    P0 = softmax(scale Q[s] K[s]^T), P1 = softmax(scale Q[b] K[b]^T), each with its own maximum and sum,
 *                A[q][j] = c[b][j] sum_k P0[q][k] Mt[b][j][k] + d[b][j] P1[q][j],  O[b] = A V[b]   (no renormalisation)
 *   unedited b:  O[b] = softmax(scale Q[b] K[b]^T) V[b], the bits of pea_op_attention_fwd; no table row of that sample is read.
 * src: HOST int[B], validated before any launch and passed in the kernel arguments.  Mt: device bf16 [B][Skv][ldm], the transposed
 * token mapper (row j the target key, column k the source key; ldm a multiple of 8, >= Skv; columns at or past Skv are ignored).
 * c, d: device fp32 [B][Skv].  The mixture is formed in fp32 and rounded to bf16 once; c = 0, d = 1 on a sample gives that sample
 * the bits of the plain kernel (Sq >= 128: below, pea_op_attention_fwd is another kernel, which then writes the unedited samples).
 * No atomics: the same bits every run.  ld* and alignment as for pea_op_attention_fwd_regions; Mt 16-byte aligned.  PEA_E_SHAPE
 * before any launch: src[b] >= B, a source that is itself edited, B > 32, Skv > 96, a leading dimension that is no multiple of 8,
 * an empty problem, a null table while any sample is edited.  PEA_E_INVALID: null src. */
int pea_op_attention_fwd_edit(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                              int Sq, int Skv, const int* src, const void* Mt, int ldm, const float* c, const float* d, float scale,
                              int q_prescaled, void* stream);
/* The same in a UNet context (graph 0, inference), a runtime state like regions and maps: the tape, the plans and the arenas do not
 * change.  pea_unet_set_prompt_edit: src host int[B]; Mt device bf16 [B][L][L] (ldm = L rounded up to 8 is made inside); cd device
 * fp32 [T][2][B][L], c then d for every one of T steps; all copied into buffers outside the arenas (cd also to the host, so the
 * launch choice per step reads no device memory).  pea_unet_set_prompt_edit_step sets the current step, a host int: nothing is
 * transferred inside a denoising loop.  While set, every cross-attention layer runs pea_op_attention_fwd_edit at a step that has
 * any c != 0 or d != 1 on an edited sample, and the plain launch otherwise; every self-attention layer with at most
 * self_max_tokens queries, while step < self_until, runs its ordinary launch and then ONE more plain launch per edited sample
 * (B = 1: Q and K of the source, V and O of the sample), O[b] = softmax(scale Q[s] K[s]^T) V[b].  A forward refuses
 * (PEA_E_STATE / PEA_E_SHAPE, before the first launch): a PEA_UNET_GRAD context, live image prompts, prompt regions, attention-map
 * capture, per-sample context lengths, L > 96, head_dim other than 64 in the cross-attention, a step outside 0..T-1.  After
 * pea_unet_clear_prompt_edit a forward gives the bits it gave before. */
int pea_unet_set_prompt_edit(void* unet, const int* src, const void* Mt, const float* cd, int T, int self_until, int self_max_tokens,
                             void* stream);
int pea_unet_set_prompt_edit_step(void* unet, int step);
int pea_unet_clear_prompt_edit(void* unet);
/* Test aid, needs no device: what pea_op_attention_fwd_edit launches (shape checks included).  q[40] = { B, H, Sq, Skv, nd, ldk
 * (<= 0: 64 H, like every other leading dimension), ldm (<= 0: Skv rounded up to 8), flags (bit 0: null tables), src[0..31] }.
 * Returns PEA_OK and out[8] = { KB (the instantiation xattn_edit_fwd_kernel<KB>), grid x / y / z, dynamic LDS bytes, 128-query
 * units per workgroup of an unedited sample, 1 if the plain launch runs first and the kernel writes the edited samples only, units
 * per workgroup of an edited sample }, or the error code of a refused problem.  The grid is 1-D: H x ceil(units / units per
 * workgroup) workgroups per sample with the count of its kind, the edited samples' first; y = z = 1.  LDS = 3 KB 4096 + KB 32 (KB 64 + 16) + KB 256 + 4 4096 + 8 4096 bytes (own keys, values, the source's keys; the
 * mapper; c and d; the O images; the Q images of both samples). */
int pea_debug_attn_edit_dispatch(const int* q, int* out);

/* ---- StyleAligned generation (Hertz et al. 2023, "Style Aligned Image Generation via Shared Attention"): a batch of N prompts
 * denoised together keeps one style.  Sample b with ref[b] = r >= 0 is a TARGET of the reference r, a plain sample of the same batch
 * (ref[b] < 0, or ref[b] = b, a sample that is its own reference: plain).  Everything below is per head, head_dim 64; a
 * restatement from the paper and the authors' public code (unpinned).
 * pea_op_attn_adain_coef: the AdaIN coefficients.  Q [B][S][ldq], K [B][S][ldk] bf16, C = 64 H columns each.  Over the S tokens of a
 * sample, per channel, mu(X) the mean and sigma(X) = sqrt(var_unbiased(X) + eps); for a target b with reference r and X in {Q, K}
 *   a = sigma(X[r]) / sigma(X[b]),  s = mu(X[r]) - a mu(X[b])          (AdaIN: X' = a o X + s)
 * coef fp32 [B][4][C] = (a_q, s_q, a_k, s_k); a pair switched off (adain_queries / adain_keys = 0) is (1, 0); rows of plain samples
 * are not written.  eps = 1e-5, and (scale log2 e)^2 1e-5 for a q_prescaled Q, whose statistics are those of q times scale log2 e.
 * Sums of (x - x[row 0]) and its square in fp32, split over token slabs whose partials (scratch: pea_op_attn_adain_scratch_bytes,
 * always needed while there is a target) are added in slab order: no atomics, the same bits every run.  PEA_E_SHAPE before any
 * launch: B > 32, S < 2 while any sample is a target, ref[b] >= B, a reference that is itself a target, a leading dimension that is
 * no multiple of 8, an empty problem, a null operand.  PEA_E_INVALID: null ref.  ref: HOST int[B]. */
long long pea_op_attn_adain_scratch_bytes(int B, int H, int S);
int pea_op_attn_adain_coef(const void* Q, int ldq, const void* K, int ldk, int B, int H, int S, const int* ref, float scale,
                           int q_prescaled, int adain_queries, int adain_keys, float* coef, void* scratch, void* stream);
/* pea_op_attention_fwd_shared, ONE launch over the whole batch, forward only, no lse, head_dim 64, Sq == Skv = S, B <= 32:
 *   target b:  q' = a_q o q + s_q;  own scores  scale (q' o a_k) . K[b][j] + scale q' . s_k   ( = scale q' . (a_k o K[b][j] + s_k) ),
 *              reference scores  shared_score_scale scale q' . K[r][j] + shared_score_shift,
 *              O[b] = softmax over the 2 S scores . [V[b]; V[r]]
 *   plain b:   O[b] = softmax(scale Q[b] K[b]^T) V[b], the bits of pea_op_attention_fwd; no coef row of that sample is read.
 * K is never rewritten and nothing is concatenated: the own segment runs a second resident Q fragment set against the untouched K
 * tiles with one constant per query in the accumulator operand, the reference's K and V are read in place.  coef: device fp32
 * [B][4][64 H] from pea_op_attn_adain_coef, 16-byte aligned; null is accepted while no sample is a target.  ref: HOST int[B],
 * validated before any launch and passed in the kernel arguments.  The workgroups of the targets, which run twice the key tiles,
 * are dispatched first.  No atomics: the same bits every run.  ld* in elements, Q / K / V / O 16-byte aligned.  PEA_E_SHAPE before any
 * launch: S < 2 while any sample is a target, Sq != Skv, nd != 1, B > 32, ref[b] >= B, a reference that is itself a target, a
 * leading dimension that is no multiple of 8, null coef while any sample is a target, an empty problem.  PEA_E_INVALID: null ref. */
int pea_op_attention_fwd_shared(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                                int Sq, int Skv, const int* ref, const float* coef, float scale, int q_prescaled,
                                float shared_score_scale, float shared_score_shift, int nd, void* stream);
/* The same in a UNet context (graph 0, inference), a runtime state like regions, maps and edits: the tape, the plans and the arenas
 * do not change.  ref: host int[B] as above.  layer_on: one switch per SELF-attention layer in the order a forward runs them (down
 * blocks, mid block, up blocks), non-zero = shared; null (n_layers ignored) = every layer; n_layers must equal
 * pea_unet_num_self_attention_layers otherwise.  While set, every switched-on self-attention layer runs pea_op_attn_adain_coef over
 * its Q and K columns and then pea_op_attention_fwd_shared instead of its plain launch; the coefficient buffer [B][4][widest layer]
 * and the scratch are allocated here, once, outside the arenas.  Refused (PEA_E_STATE / PEA_E_SHAPE; by a forward too, before its
 * first launch): a PEA_UNET_GRAD context, live prompt editing (whose self-attention rule rewrites the same outputs), B > 32, a
 * self-attention layer whose head_dim is not 64 or that has fewer than 2 tokens.  Image prompts, regions, heat maps, FreeU and
 * ControlNet residuals combine freely: they never see a self-attention launch.  Not a UNet handle, null ref: PEA_E_INVALID.  After
 * pea_unet_clear_style_aligned a forward gives the bits it gave before. */
int pea_unet_set_style_aligned(void* unet, const int* ref, const float* layer_on, int n_layers, int adain_queries, int adain_keys,
                               float shared_score_scale, float shared_score_shift, void* stream);
int pea_unet_clear_style_aligned(void* unet);
int pea_unet_num_self_attention_layers(void* unet);      /* a count, or a negative error code */
/* Test aid, needs no device: what pea_op_attention_fwd_shared launches (shape checks included).  q[39] = { B, H, Sq, Skv, nd, ldk
 * (<= 0: 64 H, like every other leading dimension), flags (bit 0: null coef), ref[0..31] }.  Returns PEA_OK and out[8] = { grid x /
 * y / z, dynamic LDS bytes, workgroups of target samples, workgroups of plain samples, 1 if the plain launch runs first and the
 * kernel's grid holds the targets only, number of target samples }, or the error code of a refused problem.  The grid is 1-D: H x
 * ceil(S / 128) workgroups per sample, the targets' first; y = z = 1.  LDS = 2 stages x (K tile + V tile) x 8192 bytes. */
int pea_debug_attn_shared_dispatch(const int* q, int* out);

/* ---- self-attention guidance (Hong et al. 2023, "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance"): a
 * second guidance term from the model's own self-attention, no training, no weights.  A restatement from the paper and the public
 * pipelines (unpinned).
 * pea_op_attention_colsum: the probability mass each key receives from all queries, head_dim 64, ONE launch, no V / O:
 *   part[b][g][k] = (1 / H) sum_{h in group g} sum_q exp(scale Q[b, q, h, :] . K[b, k, h, :] - lse[b][h][q])
 * Q [B][Sq][ldq], K [B][Skv][ldk] bf16 holding all H heads; lse device fp32 [B][H][Sq], natural log, as pea_op_attention_fwd writes
 * it; part device fp32 [B][G][Skv], G = pea_op_attention_colsum_groups(B, H, Sq, Skv) groups of consecutive heads (a positive
 * count, or PEA_E_SHAPE for an empty problem).  The column sum of the head-mean softmax is part[b][0][k] + part[b][1][k] + ... in
 * ascending g, which the consumer adds (pea_op_sag_degrade does): no reduce launch, no atomics.  q_prescaled: Q arrives multiplied
 * by scale * log2(e); otherwise that factor multiplies the fp32 score, and no bf16 operand is rounded a second time.  The
 * probabilities stay fp32.  Keys on the lane: a workgroup is 128 keys of one (sample, head group) and streams the Q tiles of its
 * heads; sums run over a lane's queries, then tiles, then heads in ascending order, then the two halves of the wave: the same bits
 * every run.  Query rows at or past Sq and key rows at or past Skv of an over-allocated buffer are never used.  Any Sq >= 1, Skv >= 1;
 * B <= 65535 (grid z), H <= 65535; ldq / ldk multiples of 8 holding every head, Q / K 16-byte aligned; one sample's Q or K below
 * 2 GiB.  Every refusal is PEA_E_SHAPE before any launch: an empty problem, a null operand, a null lse, a leading dimension that is
 * no multiple of 8. */
int pea_op_attention_colsum_groups(int B, int H, int Sq, int Skv);
int pea_op_attention_colsum(const void* Q, int ldq, const void* K, int ldk, const float* lse, float* part, int B, int H, int Sq, int Skv,
                            float scale, int q_prescaled, void* stream);
/* Test aid, needs no device: what pea_op_attention_colsum launches (shape checks included).  q[8] = { B, H, Sq, Skv, nd, ldq (<= 0:
 * 64 H), ldk (<= 0: 64 H), flags (1: q_prescaled, 2: null lse) }.  Returns PEA_OK and out[6] = { G, grid x / y / z, dynamic LDS
 * bytes, heads per group }, or the error code of a refused problem.  grid = ceil(Skv / 128) x G x B, workgroups of 256 threads;
 * LDS = 2 stages x 4 x (8192-byte Q tile + 256 bytes of row constants).  G: the fewest groups that give 512 workgroups, at most H, made
 * even: heads per group = ceil(H / that), G = ceil(H / heads per group). */
int pea_debug_attn_colsum_dispatch(const int* q, int* out);
/* pea_op_sag_degrade: mask, blur and degraded model input in ONE launch.  latents, eps, out: fp32 [B][C][H][W]; part: fp32
 * [B][G][map_h map_w] from pea_op_attention_colsum (any G >= 1); iy int[H], ix int[W] device tables: latent row / column -> map row /
 * column (nearest: min(floor(dst * (float)in / out), in - 1), built on the host).
 *   A = part[b][0][k] + part[b][1][k] + ...  (ascending g, fp32),  m = A > 1.0f at k = iy[y] map_w + ix[x], shared by every channel
 *   x0 = c_x x + c_e eps;  x0_blur: 9 x 9 Gaussian of x0, taps exp(-i^2 / 2) / sum, separable (rows, then columns), reflect padding of
 *   4 without edge repeat;  out = o_b (m ? x0_blur : x0) + o_e eps
 * Where m is false the result is o_b (c_x x + c_e eps) + o_e eps evaluated in that order, every product and sum rounded once.
 * PEA_E_SHAPE before any launch: H < 5 or W < 5, G < 1, a null operand, an empty problem. */
int pea_op_sag_degrade(const float* latents, const float* eps, const float* part, int G, int map_h, int map_w, const int* iy,
                       const int* ix, float* out, int B, int C, int H, int W, float c_x, float c_e, float o_b, float o_e, void* stream);
/* pea_op_cfg_sag_combine: cfg != 0: eps fp32 [2B][per] (unconditional half first), out[B][per] = u + g (t - u) + s (u - eps_deg);
 * sag_scale = 0 gives the bits of pea_op_cfg_combine at guidance_rescale 0.  cfg == 0: eps [B][per], out = eps + s (eps - eps_deg).
 * eps_deg fp32 [B][per]: the prediction on the degraded input. */
int pea_op_cfg_sag_combine(const float* eps, const float* eps_deg, float* out, int B, long long per, int cfg, float guidance_scale,
                           float sag_scale, void* stream);
/* The capture in a UNet context (graph 0, inference), a runtime state like regions, maps, edits and StyleAligned: the tape, the plans
 * and the arenas do not change.  layer: an index into the self-attention layers in the order of pea_unet_num_self_attention_layers.
 * While enabled, that layer's ordinary launch is handed an lse buffer of the state's own (fp32 [B][H][S], outside the arenas) and is
 * followed by ONE pea_op_attention_colsum over samples first_sample .. first_sample + n_samples - 1; the ordinary launch, its
 * dispatch decision and its O do not change: a forward gives the bits it gives without capture.  pea_unet_sag_colsum: the
 * partials of the last forward, device fp32 [n_samples][G][S], with G and S.  Refused (PEA_E_STATE / PEA_E_SHAPE; by a forward too,
 * before its first launch): a PEA_UNET_GRAD context, a layer whose head_dim is not 64, live prompt editing, StyleAligned switched
 * on for that same layer (both rewrite or replace that launch), a layer or sample range outside the context.  Image prompts,
 * regions, heat maps, FreeU, ControlNet residuals and inpainting combine freely.  pea_unet_disable_sag synchronises the device
 * and frees the buffers; after it a forward gives the bits it gave before. */
int pea_unet_enable_sag(void* unet, int layer, int first_sample, int n_samples);
int pea_unet_disable_sag(void* unet);
int pea_unet_sag_colsum(void* unet, float** part, int* G, int* S);

/* ---- perturbed-attention guidance (Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance") and
 * smoothed-energy guidance (Hong 2024, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of
 * Attention"): one more sample per prompt rides in the SAME UNet call, last in the batch, and in chosen self-attention layers its
 * attention is perturbed; s (eps_text - eps_perturbed) is added to the guidance.  Restatements from the papers and the authors'
 * public code (unpinned).
 * pea_op_query_blur: Q bf16 rows [n][h * w] of pitch ld, the C columns from col0 (C % 64 == 0, col0 % 8 == 0) read as n grids of
 * h x w tokens and blurred per channel IN PLACE: Q~ = Mh . Q . Mw^T with dense device fp32 Mh [h][h], Mw [w][w] (pag.blur_matrix
 * folds taps, size clamp, reflect padding and the infinite-sigma mean into them).  One launch; a workgroup owns 8 channels of one
 * sample and holds their whole grid in LDS as fp32, both passes accumulate in fp32 and only the store rounds.  Columns outside
 * [col0, col0 + C) and rows outside the n samples are not touched.  h, w <= 64 (pea_op_query_blur_lds_bytes(h, w): the LDS the
 * launch takes, 133120 of 163840 bytes at 64 x 64, or PEA_E_SHAPE for a grid it cannot hold): larger grids are refused, not
 * served by another path.  PEA_E_SHAPE before any launch: a null operand, C % 64 != 0, a pitch or offset that is no multiple of 8
 * or does not hold the columns, n > 65535.
 * pea_op_attn_identity: the identity "attention" O = V: rows x C bf16 from V (pitch ldv, from column col0) to O (pitch ldo),
 * 16 bytes per lane (the pitched copy the tape's concats use).
 * pea_op_cfg_pag_combine: cfg != 0: eps fp32 [3B][per] = [u | t | p], out[B][per] = u + g (t - u) + s (t - p), then, when
 * guidance_rescale > 0, rescale_noise_cfg against t as pea_op_cfg_combine does it (its reduction, its workspace:
 * pea_op_cfg_combine_workspace_bytes(B)); s = 0 gives pea_op_cfg_combine's bits on the first 2B samples at any rescale.  cfg == 0:
 * eps [2B][per] = [t | p], out = t + s (t - p); guidance_rescale is not applied. */
int pea_op_query_blur(void* Q, int ld, int col0, int n, int h, int w, int C, const float* Mh, const float* Mw, void* stream);
int pea_op_query_blur_lds_bytes(int h, int w);
int pea_op_attn_identity(const void* V, int ldv, int col0, void* O, int ldo, long long rows, int C, void* stream);
int pea_op_cfg_pag_combine(const float* eps, float* out, int B, long long per, int cfg, float guidance_scale, float pag_scale,
                           float guidance_rescale, void* workspace, void* stream);
/* The perturbation in a UNet context (graph 0, inference), a runtime state like the others: the tape, the plans and the arenas do
 * not change.  The samples first_sample .. B - 1 are the perturbed ones (a non-empty suffix that leaves plain samples in front).
 * layer_on: null = every self-attention layer, else n_layers switches in the order of pea_unet_num_self_attention_layers.  mode 1
 * (identity, PAG): in a switched-on layer O[b] = V[b] for the perturbed samples -- the ordinary launch runs over the plain
 * samples alone and ONE pitched copy follows.  mode 2 (query blur, SEG): ONE pea_op_query_blur over the perturbed samples' Q
 * columns, in place, then the ordinary launch over all samples; the grids come as n_grids (<= 16) sides grid_h[i] x grid_w[i]
 * and `tables`, HOST fp32: per grid Mh [h][h] then Mw [w][w], back to back; every switched-on layer's query count needs its grid
 * (a forward without refuses).  The plain samples keep the bits they have without the feature.  Refused (PEA_E_STATE /
 * PEA_E_SHAPE; by a forward too, before its first launch): a PEA_UNET_GRAD context, a switched-on layer whose head_dim is not
 * 64, an empty or whole-batch suffix, live prompt editing (in both orders), StyleAligned switched on for a perturbed layer,
 * self-attention guidance capturing one.  Image prompts, regions, heat maps, FreeU and ControlNet residuals combine freely.
 * pea_unet_clear_attn_perturb frees the tables; after it a forward gives the bits it gave before. */
int pea_unet_set_attn_perturb(void* unet, int mode, int first_sample, const float* layer_on, int n_layers, int n_grids,
                              const int* grid_h, const int* grid_w, const float* tables, void* stream);
int pea_unet_clear_attn_perturb(void* unet);

/* ---- MultiDiffusion panoramas (Bar-Tal et al. 2023, "MultiDiffusion: Fusing Diffusion Paths for Controlled Image Generation"; the
 * weights of Mixture of Diffusers, Jimenez 2023): a canvas fp32 [N][C][Hc][Wc] larger than the context's window h x w is denoised
 * through overlapping window-sized VIEWS with the unchanged fixed-shape UNet, reconciled in the overlaps at every step.  A restatement
 * from the paper (unpinned).  A view is (n, y0, x0): image n, rows y0 .. y0 + h - 1, columns (x0 + j) mod Wc for
 * j < w; without wrap_x x0 + w <= Wc, with it 0 <= x0 < Wc and a view may straddle the seam; no wrap in y.  Both ops work on a CHUNK,
 * the vb <= 16 view slots of one UNet call, n_valid of them real: `slots` is a HOST array int [n_valid][3] = (n, y0, x0), copied into
 * the kernel arguments -- no device table, no host-to-device copy.  One launch each, every element read once, no atomics: the same
 * bits every run.  16-byte accesses when w, Wc and every x0 are multiples of 4 and the pointers 16-byte aligned (a wrapped view
 * included), one element per thread otherwise, with identical results.
 * pea_op_views_gather: model_in fp32 [dup][vb][C][h][w], model_in[d][s] = crop of slot s * k_s for d < dup (dup 2: the CFG-doubled
 *   batch); a slot past n_valid repeats the last valid slot (the UNet never reads uninitialised memory; its output there is ignored).
 * pea_op_views_merge: eps fp32 [dup][vb][C][h][w] into the canvas, gather-style: a thread owns canvas elements and walks the valid
 *   slots in ascending order.  Per covering slot e = u + g (t - u) for dup 2 (the expression of pea_op_cfg_combine, unconditional
 *   half first), eps itself for dup 1; times factor[s] when `factor` (device fp32 [vb], pea_op_cfg_rescale_factors) is given;
 *   acc += wy[i] wx[j] e with device fp32 tables wy [h], wx [w].  `first`: acc starts at 0 and every canvas element is stored (0 where
 *   no slot of the chunk covers it); otherwise acc starts at what the canvas holds and elements outside the chunk's views are not
 *   touched.  `last`: every element is then divided by total[n][Y][X] (device fp32 [N][Hc][Wc], the summed weights of ALL covering
 *   views) in the same launch, in place.  C, h, w, Hc, Wc are free: the same entry merges decoded pixel tiles (C 3, dup 1).
 * pea_op_cfg_rescale_factors: factor[b] = phi std(t_b) / std(cfg_b) + 1 - phi of rescale_noise_cfg for eps2 = [u | t] fp32 [2B][per]:
 *   the reduction and factor launches of pea_op_cfg_combine without its apply pass (the same bits as its factors); workspace of
 *   pea_op_cfg_combine_workspace_bytes(B), factor device fp32 [B].
 * PEA_E_SHAPE before any HIP call: a null operand, vb outside 1..16, n_valid outside 1..vb, dup outside 1..2, a window larger than
 * the canvas, a view outside the canvas without wrap_x, x0 >= Wc with it, n outside 0..N-1, factor given with dup 1. */
int pea_op_views_gather(const float* canvas, float* model_in, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc,
                        int Wc, int h, int w, int wrap_x, float k_s, void* stream);
int pea_op_views_merge(const float* eps, float* canvas, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc, int Wc,
                       int h, int w, int wrap_x, float guidance_scale, const float* factor, const float* wy, const float* wx,
                       const float* total, int first, int last, void* stream);
int pea_op_cfg_rescale_factors(const float* eps2, int B, long long per, float guidance_scale, float guidance_rescale, void* workspace,
                               float* factor, void* stream);

/* ---- semantic guidance (Brack et al. 2023, "SEGA: Instructing Text-to-Image Models using Semantic Guidance"): K <= 8 edit concepts
 * ride in the SAME UNet call behind the CFG pair, eps fp32 [(2 + K) B][C][hw] = [u | t | e_1 .. e_K]; each concept's scaled
 * difference d_c = s_c (e_c - u) (s_c signed: a reversed edit is a negative scale) is kept only in its upper tail, per GROUP = one
 * (concept, sample, channel) of hw positions: m_c = d_c where |d_c| >= thr_c else 0, thr_c = torch.quantile(|d_c|, q_c) with linear
 * interpolation: r = q (hw - 1) in fp32, k = floor(r), thr = lerp(v[k], v[min(k + 1, hw - 1)], r - k) over the ascending values v.
 * A restatement from the paper and diffusers' semantic pipeline (unpinned).  edit_scale, quantile, weight and
 * warm are HOST arrays of K entries, read at call time and copied into the kernel arguments.  A concept of weight 0 (cooled down) is
 * not computed and its samples are not read.
 * pea_op_abs_diff_quantile: thr fp32 [K][B][C]; bounds (may be null) fp32 [K][B][C][2] = the two order statistics.  One launch, one
 *   workgroup of 1024 threads per group: the group is read once into registers (16 values a thread, so hw <= 16384) and v[k] found by
 *   an exact radix select over the 32-bit pattern of |d| (four 256-bin histograms in LDS; no sort, no global atomics, no scratch);
 *   ties are exact: v[k + 1] is v[k] again when more than k + 1 values are <= v[k], else the smallest value above.  thr and bounds
 *   of a cooled concept are +inf.  hw is free (no multiple of 4 or 64 needed).
 * pea_op_cfg_sega_combine: the whole step in two launches (the select into `workspace`, pea_op_sega_workspace_bytes(B, C, K), then one
 *   elementwise pass; the select is skipped when every concept is cooled):
 *     E_all = sum_c w_c m_c (ascending c), E_warm = sum_c warm_c w_c m_c, used = E_all + mu mom,
 *     out [B][C][hw] = u + g (t - u) + (any warm_c ? E_warm + mu mom : 0),   mom <- beta mom + (1 - beta) used   (fp32 [B][C][hw], in place).
 *   The pass recomputes d_c with the select's two operations, so the cut sees the ranked values; u + g (t - u) is
 *   pea_op_cfg_combine's expression: with every concept cooled and a zero momentum, its bits on [u | t].  The same bits every run.
 *   Non-finite eps: unspecified.
 * PEA_E_SHAPE before any device work: a null operand, B < 1, C < 1, hw outside 2..16384, K outside 1..8, a quantile outside [0, 1),
 * a negative weight, momentum_beta outside [0, 1], a missing workspace. */
long long pea_op_sega_workspace_bytes(int B, int C, int K);
int pea_op_abs_diff_quantile(const float* eps, float* thr, float* bounds, int B, int C, int hw, int K, const float* edit_scale,
                             const float* quantile, const float* weight, void* stream);
int pea_op_cfg_sega_combine(const float* eps, float* momentum, float* out, int B, int C, int hw, int K, float guidance_scale,
                            const float* edit_scale, const float* quantile, const float* weight, const int* warm, float momentum_scale,
                            float momentum_beta, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEA_HIP_H */
