// C-ABI, operator level: thin argument marshalling onto the kernel launchers (include/pea_hip.h).
#include <stdarg.h>
#include <string.h>

#include "../../include/pea_hip.h"
#include "pea_kernels.h"

static thread_local char g_err[512] = "";
void pea_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static bf16* g_zero_page = nullptr;
int pea_zero_page(const bf16** out) {
  if (!g_zero_page) {
    HIPCHK(hipMalloc((void**)&g_zero_page, 256));
    HIPCHK(hipMemset(g_zero_page, 0, 256));
  }
  *out = g_zero_page;
  return PEA_OK;
}

// what every attention entry point starts from: a zeroed P -- AttnP, or a feature's struct with the operands it shares with
// AttnP (pea_kernels.h: attn_feature_p) -- with Q / K / V / O, lse, the shape, the scale, nd and the Q convention set
template <class P = AttnP>
static P attn_operands(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O, int ldo,
                       const float* lse, int B, int H, int Sq, int Skv, float scale, int nd, int q_prescaled = 0) {
  AttnP p;
  memset(&p, 0, sizeof(p));
  p.Q = (const bf16*)Q; p.K = (const bf16*)K; p.V = (const bf16*)V; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
  p.O = (bf16*)O; p.ldo = ldo; p.lse = (float*)lse; p.B = B; p.H = H; p.Sq = Sq; p.Skv = Skv; p.scale = scale; p.nd = nd;
  p.q_prescaled = q_prescaled;
  return attn_feature_p<P>(p);
}
// bodies of the attention operators with the Q convention as a PARAMETER (the entry points below pass 0 or 1): nothing
// process-wide is written around a call, so concurrent callers (ctypes releases the GIL) cannot see each other's mode
static int attention_fwd_impl(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                              float* lse, int B, int H, int Sq, int Skv, float scale, int nd, int q_prescaled, void* stream) {
  return launch_attention_fwd(attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, nd, q_prescaled), (hipStream_t)stream);
}
static int attention_bwd_impl(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                              int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                              void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                              int accum_dq, int accum_dkv, int nd, void* scratch, int q_prescaled, const int* kv_len,
                              void* stream) {
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, nd);
  p.dO = (const bf16*)dO; p.lddo = lddo; p.delta = delta;
  p.dQ = (bf16*)dQ; p.lddq = lddq; p.dK = (bf16*)dK; p.lddk = lddk; p.dV = (bf16*)dV; p.lddv = lddv;
  p.accum_dq = accum_dq; p.accum_dkv = accum_dkv; p.dkv_part = (float*)scratch;
  p.q_prescaled = q_prescaled; p.kv_len = kv_len;
  return launch_attention_bwd(p, (hipStream_t)stream);
}

extern "C" {

const char* pea_last_error(void) { return g_err; }
int pea_version(void) { return 100; }
int pea_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pea_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, float alpha,
                const float* bias, const void* rowvec, int ldrv, int rows_per_batch, int act, void* preact,
                int ldpre, const void* res, int ldres, int out_f32, int accum_f32, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.mode = 0;
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.alpha = alpha; p.bias = bias;
  p.rowvec = (const bf16*)rowvec; p.ldrv = ldrv; p.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1;
  p.act = act; p.preact = (bf16*)preact; p.ldpre = ldpre; p.res = (const bf16*)res; p.ldres = ldres;
  p.out_f32 = out_f32; p.accum_f32 = accum_f32;
  return launch_gemm(p, (hipStream_t)stream);
}

int pea_op_gemm_qscale(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const float* bias,
                       int qscale_cols, float qscale, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.alpha = 1.f; p.bias = bias; p.rows_per_batch = 1;
  p.qscale_cols = qscale_cols; p.qscale = qscale;
  return launch_gemm(p, (hipStream_t)stream);
}

int pea_op_gemm_geglu_bwd(const void* A, int lda, const void* W, int ldw, const void* pre, int ldpre, void* C, int ldc,
                          int M, int N, int K, int form, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.alpha = 1.f; p.rows_per_batch = 1;
  p.gbwd_pre = (const bf16*)pre; p.ldgp = ldpre; p.gbwd_form = form;
  return launch_gemm(p, (hipStream_t)stream);
}

int pea_op_gemm_geglu(const void* A, int lda, const void* W, int ldw, const float* bias, void* y, void* stash, int M, int N,
                      int K, int stash_grad, int stash_rows, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K; p.alpha = 1.f; p.rows_per_batch = 1;
  p.geglu_y = (bf16*)y; p.ldy = N / 2; p.C = stash; p.ldc = N; p.stash_grad = stash_grad; p.stash_rows = stash_rows;
  return launch_gemm(p, (hipStream_t)stream);
}

// pea_op_gemm_geglu with the gate's activation as an argument (GemmP::geglu_tanh: the T5 v1.1 gated gelu_new)
int pea_op_gemm_geglu_tanh(const void* A, int lda, const void* W, int ldw, const float* bias, void* y, void* stash, int M, int N,
                           int K, int stash_grad, int stash_rows, int geglu_tanh, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.bias = bias;
  p.M = M; p.N = N; p.K = K; p.alpha = 1.f; p.rows_per_batch = 1;
  p.geglu_y = (bf16*)y; p.ldy = N / 2; p.C = stash; p.ldc = N; p.stash_grad = stash_grad; p.stash_rows = stash_rows;
  p.geglu_tanh = geglu_tanh ? 1 : 0;
  return launch_gemm(p, (hipStream_t)stream);
}

// split-K (the tape's stacked K|V projection backward): fp32 partial s = alpha * A[:, K range s] . W[:, K range s]^T at
// part + s * split_stride, rows ldc apart; pea_op_splitk_reduce adds them
int pea_op_gemm_splitk(const void* A, int lda, const void* W, int ldw, float* part, int ldc, long long split_stride, int M, int N,
                       int K, float alpha, int ksplit, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)A; p.lda = lda; p.W = (const bf16*)W; p.ldw = ldw; p.C = part; p.ldc = ldc;
  SHAPECHK(ksplit >= 2, "gemm_splitk: ksplit=%d (at least two splits)", ksplit);
  p.M = M; p.N = N; p.K = K; p.alpha = alpha; p.rows_per_batch = 1; p.out_f32 = 1;
  p.ksplit = ksplit; p.split_stride = split_stride;
  return launch_gemm(p, (hipStream_t)stream);
}

int pea_op_ln_linear(const void* x, const float* gamma, const float* beta, const void* W, const float* bias, void* y,
                     void* geglu_y, int M, int N, int K, float eps, void* Wf, float* svec, float* tvec, float* stats,
                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_layernorm_stats((const bf16*)x, stats, M, K, eps, st);
  if (rc) return rc;
  rc = launch_ln_fold((const bf16*)W, K, gamma, beta, bias, (bf16*)Wf, svec, tvec, N, K, st);
  if (rc) return rc;
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.A = (const bf16*)x; p.lda = K; p.W = (const bf16*)Wf; p.ldw = K; p.M = M; p.N = N; p.K = K; p.alpha = 1.f;
  p.bias = tvec; p.rows_per_batch = 1; p.ln_stats = stats; p.ln_s = svec;
  if (geglu_y) { p.geglu_y = (bf16*)geglu_y; p.ldy = N / 2; p.C = y; p.ldc = N; }
  else { p.C = y; p.ldc = N; }
  return launch_gemm(p, st);
}

int pea_op_conv3x3(const void* x, const void* w, void* y, int B, int Hs, int Ws, int Cin, int Cout, int stride,
                   int upsample2x, int transposed2, const float* bias, const void* rowvec, int ldrv,
                   const void* res, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.mode = 1;
  p.A = (const bf16*)x; p.W = (const bf16*)w; p.ldw = 9 * Cin; p.C = y; p.ldc = Cout;
  p.Hs = Hs; p.Ws = Ws; p.Cin = Cin;
  p.shift = (upsample2x || transposed2) ? 1 : 0;
  p.parity = transposed2 ? 1 : 0;
  p.stride = stride;
  const int Hv = Hs << p.shift, Wv = Ws << p.shift;
  p.Ho = stride == 2 ? (Hv + 1) / 2 : Hv;
  p.Wo = stride == 2 ? (Wv + 1) / 2 : Wv;
  p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = 9 * Cin; p.alpha = 1.f; p.bias = bias;
  p.rowvec = (const bf16*)rowvec; p.ldrv = ldrv; p.rows_per_batch = p.Ho * p.Wo;
  p.res = (const bf16*)res; p.ldres = Cout;
  int rc = pea_zero_page(&p.zeros);
  if (rc) return rc;
  return launch_gemm(p, (hipStream_t)stream);
}

// The conv forms the tape's OP_CONV3 fills beyond pea_op_conv3x3: pad_off (the VAE encoder's Downsample2D(padding=0):
// F.pad (0,1,0,1), then stride 2), an activation in the epilogue, Cin as the STORED width of x (zero-padded channels,
// w = pea_op_pack_conv_padded), ldw / ldc / ldres as arguments (Cout columns written into rows ldc wide)
int pea_op_conv3x3_ex(const void* x, const void* w, int ldw, void* y, int ldc, int B, int Hs, int Ws, int Cin, int Cout,
                      int stride, int pad_off, int act, const float* bias, const void* res, int ldres, void* stream) {
  SHAPECHK(B > 0 && Hs > 0 && Ws > 0 && (stride == 1 || stride == 2) && (pad_off == 0 || pad_off == 1) && act >= 0 && act <= 3,
           "conv3x3_ex: B=%d Hs=%d Ws=%d stride=%d pad_off=%d act=%d", B, Hs, Ws, stride, pad_off, act);
  SHAPECHK(!pad_off || (stride == 2 && Hs % 2 == 0 && Ws % 2 == 0),
           "conv3x3_ex: pad_off is the stride-2 downsampler's (0,1,0,1) padding on even sides (stride=%d Hs=%d Ws=%d)", stride, Hs, Ws);
  SHAPECHK(ldc >= Cout && ldw >= 9 * Cin && (!res || ldres >= Cout), "conv3x3_ex: ldc=%d ldres=%d vs Cout=%d, ldw=%d vs 9*Cin=%d",
           ldc, ldres, Cout, ldw, 9 * Cin);
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.mode = 1;
  p.A = (const bf16*)x; p.W = (const bf16*)w; p.ldw = ldw; p.C = y; p.ldc = ldc;
  p.Hs = Hs; p.Ws = Ws; p.Cin = Cin; p.stride = stride; p.pad_off = pad_off;
  p.Ho = stride == 2 ? (pad_off ? Hs / 2 : (Hs + 1) / 2) : Hs;
  p.Wo = stride == 2 ? (pad_off ? Ws / 2 : (Ws + 1) / 2) : Ws;
  p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = 9 * Cin; p.alpha = 1.f; p.bias = bias; p.act = act;
  p.rows_per_batch = p.Ho * p.Wo;
  p.res = (const bf16*)res; p.ldres = ldres;
  int rc = pea_zero_page(&p.zeros);
  if (rc) return rc;
  return launch_gemm(p, (hipStream_t)stream);
}

// conv3x3(nearest_2x(x)) in its sub-pixel form (elementwise.hip: pack_conv_subpix_kernel; the tape's OP_CONV3 p1 == 2):
// x [B][Hs][Ws][Cin] -> y depth-to-space [B][Hs][Ws][4][Cout];  w = pea_op_pack_conv_subpixel(dgrad = 0)
int pea_op_upconv_subpixel(const void* x, const void* w, void* y, int B, int Hs, int Ws, int Cin, int Cout,
                           const float* bias, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.mode = 1; p.A = (const bf16*)x; p.ldw = 4 * Cin; p.ldc = 4 * Cout;
  p.Hs = Hs; p.Ws = Ws; p.Cin = Cin; p.Ho = Hs; p.Wo = Ws; p.stride = 1; p.kside = 2;
  p.M = B * Hs * Ws; p.N = Cout; p.K = 4 * Cin; p.alpha = 1.f; p.bias = bias; p.rows_per_batch = Hs * Ws;
  int rc = pea_zero_page(&p.zeros);
  if (rc) return rc;
  for (int pl = 0; pl < 4; ++pl) {
    p.W = (const bf16*)w + (size_t)pl * Cout * 4 * Cin;
    p.C = (bf16*)y + (size_t)pl * Cout;
    p.pad_off = pl >> 1; p.pad_dx = (pl & 1) - (pl >> 1);
    rc = launch_gemm(p, (hipStream_t)stream);
    if (rc) return rc;
  }
  return PEA_OK;
}
// its data gradient: dy depth-to-space [B][Hs][Ws][4][Cout] -> dx [B][Hs][Ws][Cin] (+ res);  wt = pea_op_pack_conv_subpixel(dgrad = 1)
int pea_op_upconv_subpixel_dgrad(const void* dy, const void* wt, void* dx, int B, int Hs, int Ws, int Cin, int Cout,
                                 const void* res, void* stream) {
  GemmP p;
  memset(&p, 0, sizeof(p));
  p.mode = 1; p.A = (const bf16*)dy; p.W = (const bf16*)wt; p.ldw = 16 * Cout; p.C = dx; p.ldc = Cin;
  p.Hs = Hs; p.Ws = Ws; p.Cin = Cout; p.pix = 4 * Cout; p.kside = 4; p.Ho = Hs; p.Wo = Ws; p.stride = 1; p.pad_off = 1;
  p.M = B * Hs * Ws; p.N = Cin; p.K = 16 * Cout; p.alpha = 1.f; p.rows_per_batch = Hs * Ws;
  p.res = (const bf16*)res; p.ldres = Cin;
  int rc = pea_zero_page(&p.zeros);
  if (rc) return rc;
  return launch_gemm(p, (hipStream_t)stream);
}
// channel concat / its backward; aH, aW != 0: the FIRST operand is stored depth-to-space at full resolution aH x aW
int pea_op_concat2(const void* a, int C1, const void* b, int C2, void* y, long long rows, int aH, int aW, void* stream) {
  return launch_concat2((const bf16*)a, C1, (const bf16*)b, C2, (bf16*)y, rows, (hipStream_t)stream, aH, aW);
}
int pea_op_split2(const void* dy, int C1, int C2, void* da, int accum_a, void* db, int accum_b, long long rows, int aH,
                  int aW, void* stream) {
  return launch_split2((const bf16*)dy, C1, C2, (bf16*)da, accum_a, (bf16*)db, accum_b, rows, (hipStream_t)stream, aH, aW);
}
// FreeU on the operands of an up-path concat (elementwise.hip: freeu_coef_kernel, concat2_freeu_kernel)
long long pea_op_freeu_scratch_bytes(int B, int H, int W, int C2) { return (long long)freeu_scratch_bytes(B, H, W, C2); }
int pea_op_freeu_coef(const void* skip, int B, int H, int W, int C2, float* coef, void* scratch, void* stream) {
  return launch_freeu_coef((const bf16*)skip, B, H, W, C2, coef, (float*)scratch, (hipStream_t)stream);
}
int pea_op_concat2_freeu(const void* a, int C1, const void* b, int C2, const float* coef, void* y, int B, int H, int W, float s,
                         float bscale, int aH, int aW, void* stream) {
  return launch_concat2_freeu((const bf16*)a, C1, (const bf16*)b, C2, coef, (bf16*)y, B, H, W, s, bscale, (hipStream_t)stream, aH, aW);
}
int pea_op_pack_conv_subpixel(const float* w, void* out, int Co, int Ci, int dgrad, void* stream) {
  return launch_pack_conv_subpix(w, (bf16*)out, Co, Ci, dgrad, (hipStream_t)stream);
}

int pea_op_pack_conv(const float* w, void* out, int Co, int Ci, int dgrad, void* stream) {
  return dgrad ? launch_pack_conv_dgrad(w, (bf16*)out, Co, Ci, (hipStream_t)stream)
               : launch_pack_conv_fwd(w, (bf16*)out, Co, Ci, (hipStream_t)stream);
}
// forward pack for an input stored Cip >= Ci channels wide: out [Co][9 Cip], the padding channels' weights zero
int pea_op_pack_conv_padded(const float* w, void* out, int Co, int Ci, int Cip, void* stream) {
  SHAPECHK(Co > 0 && Ci > 0 && Cip >= Ci, "pack_conv_padded: Co=%d Ci=%d stored as %d", Co, Ci, Cip);
  return launch_pack_conv_fwd(w, (bf16*)out, Co, Ci, (hipStream_t)stream, Cip);
}
int pea_op_pack_conv_out(const float* w, float* out, int Co, int Ci, void* stream) {
  return launch_pack_conv_out(w, out, Co, Ci, (hipStream_t)stream);
}
int pea_op_conv_in(const float* x, const float* w, const float* bias, void* y, int B, int Cin, int H, int W,
                   int Cout, void* stream) {
  return launch_conv_in(x, w, bias, (bf16*)y, B, Cin, H, W, Cout, (hipStream_t)stream);
}
int pea_op_conv_in_gather(const float* latents, const float* mask, const float* masked_latents, const float* w,
                          const float* bias, void* y, int B, int C, int latent_batch, int cond_batch, int H, int W, int Cout,
                          void* stream) {
  if (!w || !bias || !y) { pea_set_error("pea_op_conv_in_gather: null pointer"); return PEA_E_INVALID; }
  return launch_conv_in_gather(latents, mask, masked_latents, w, bias, (bf16*)y, B, C, latent_batch, cond_batch, H, W, Cout,
                               (hipStream_t)stream);
}
int pea_op_conv_out(const void* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W,
                    int Cout, void* stream) {
  return launch_conv_out((const bf16*)x, w, bias, y, B, Cin, H, W, Cout, (hipStream_t)stream);
}
int pea_op_conv_out_dgrad(const float* dy, const float* w, void* dx, int B, int Cin, int H, int W, int Cout,
                          void* stream) {
  return launch_conv_out_dgrad(dy, w, (bf16*)dx, B, Cin, H, W, Cout, (hipStream_t)stream);
}

int pea_op_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, void* scratch,
                         int B, int HW, int C, int groups, float eps, int silu, void* stream) {
  return launch_groupnorm_fwd((const bf16*)x, gamma, beta, (bf16*)y, stats, (double*)scratch, B, HW, C, groups, eps,
                              silu, (hipStream_t)stream);
}
int pea_op_groupnorm_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* stats,
                         void* dx, void* scratch, int B, int HW, int C, int groups, int silu, int accum,
                         void* stream) {
  return launch_groupnorm_bwd((const bf16*)x, (const bf16*)dy, gamma, beta, stats, (bf16*)dx, (double*)scratch, B, HW,
                              C, groups, silu, accum ? (const bf16*)dx : nullptr, (hipStream_t)stream);
}
int pea_op_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, int R, int C,
                         float eps, void* stream) {
  return launch_layernorm_fwd((const bf16*)x, gamma, beta, (bf16*)y, stats, R, C, eps, (hipStream_t)stream);
}
int pea_op_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* stats, void* dx,
                         float* dgamma, float* dbeta, int R, int C, int accum, void* stream) {
  return launch_layernorm_bwd((const bf16*)x, (const bf16*)dy, gamma, stats, (bf16*)dx, dgamma, dbeta, R, C,
                              accum ? (const bf16*)dx : nullptr, (hipStream_t)stream);
}

int pea_op_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, int R, int C, float eps,
                             void* stream) {
  return launch_layernorm_fwd_f32(x, gamma, beta, y, R, C, eps, (hipStream_t)stream);
}

int pea_op_attention_fwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                         float* lse, int B, int H, int Sq, int Skv, float scale, int nd, void* stream) {
  return attention_fwd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, nd, 0, stream);
}
/* the same two operators on a Q that already carries scale * log2(e) (what the model's Q|K|V / to_q projections hand over:
 * pea_op_gemm_qscale); `scale` is still the softmax scale: dQ comes back as the gradient w.r.t. the UNSCALED q */
int pea_op_attention_fwd_prescaled(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                   float* lse, int B, int H, int Sq, int Skv, float scale, int nd, void* stream) {
  return attention_fwd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, nd, 1, stream);
}
int pea_op_attention_fwd_masked(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                float* lse, int B, int H, int Sq, int Skv, float scale, int causal, const int* kv_len,
                                void* stream) {
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, 1);
  p.causal = causal; p.kv_len = kv_len;
  return launch_attention_fwd(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_text(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                              float* lse, int B, int H, int Sq, int Skv, float scale, int q_prescaled, int causal,
                              const int* kv_len, const float* bias, void* stream) {
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, 1);
  p.q_prescaled = q_prescaled; p.causal = causal; p.kv_len = kv_len; p.bias = bias;
  return launch_attention_fwd(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_ip(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                            const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv, int Skv2,
                            float scale, float ip_scale, int q_prescaled, int causal, const int* kv_len, void* stream) {
  SHAPECHK(K2 && V2 && Skv2 >= 1, "pea_op_attention_fwd_ip: no image keys (Skv2=%d)", Skv2);
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, 1);
  p.q_prescaled = q_prescaled; p.causal = causal; p.kv_len = kv_len;
  p.K2 = (const bf16*)K2; p.V2 = (const bf16*)V2; p.ldk2 = ldk2; p.ldv2 = ldv2; p.Skv2 = Skv2; p.scale2 = ip_scale;
  return launch_attention_fwd(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_ipn(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                             const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv,
                             const pea_attn_ip_sets* sets, float scale, int q_prescaled, int causal, const int* kv_len, void* stream) {
  SHAPECHK(sets && K2 && V2, "pea_op_attention_fwd_ipn: no image keys");
  SHAPECHK(sets->n_sets >= 1 && sets->n_sets <= 4, "pea_op_attention_fwd_ipn: 1..4 image key sets (n_sets=%d)", sets->n_sets);
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, 1);
  p.q_prescaled = q_prescaled; p.causal = causal; p.kv_len = kv_len;
  p.K2 = (const bf16*)K2; p.V2 = (const bf16*)V2; p.ldk2 = ldk2; p.ldv2 = ldv2;
  p.nset = sets->n_sets;
  int total = 0;
  for (int j = 0; j < p.nset; ++j) {
    SHAPECHK(sets->n_keys[j] >= 1 && sets->n_keys[j] <= 32, "pea_op_attention_fwd_ipn: image key set %d holds %d keys (1..32)", j, sets->n_keys[j]);
    total += sets->n_keys[j];
    p.set_end[j] = total; p.set_w[j] = sets->weight[j]; p.set_mask[j] = sets->mask[j]; p.set_mstride[j] = sets->mask_stride[j];
  }
  SHAPECHK(total <= 32, "pea_op_attention_fwd_ipn: the image key sets hold %d keys together, at most 32", total);
  p.Skv2 = total;
  return launch_attention_fwd(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_regions(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                                 int Sq, int R, int Lr, const float* w, int Bw, float scale, int q_prescaled, void* stream) {
  AttnRegionsP p = attn_operands<AttnRegionsP>(Q, ldq, K, ldk, V, ldv, O, ldo, nullptr, B, H, Sq, 0, scale, 1, q_prescaled);
  p.R = R; p.Lr = Lr; p.w = w; p.Bw = Bw;
  return launch_attention_fwd_regions(p, (hipStream_t)stream);
}
int pea_op_attention_maps(const void* Q, int ldq, const void* K, int ldk, float* maps, int B, int H, int Sq, int Skv, float scale,
                          int q_prescaled, const int* kv_len, int accumulate, void* stream) {
  AttnMapsP p = attn_operands<AttnMapsP>(Q, ldq, K, ldk, nullptr, 0, nullptr, 0, nullptr, B, H, Sq, Skv, scale, 1, q_prescaled);
  p.maps = maps; p.kv_len = kv_len; p.accumulate = accumulate;
  return launch_attention_maps(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_edit(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                              int Sq, int Skv, const int* src, const void* Mt, int ldm, const float* c, const float* d, float scale,
                              int q_prescaled, void* stream) {
  if (!src) { pea_set_error("pea_op_attention_fwd_edit: null src (a host int[B]; negative entries for unedited samples)"); return PEA_E_INVALID; }
  AttnEditP p = attn_operands<AttnEditP>(Q, ldq, K, ldk, V, ldv, O, ldo, nullptr, B, H, Sq, Skv, scale, 1, q_prescaled);
  p.Mt = (const bf16*)Mt; p.ldm = ldm; p.c = c; p.d = d;
  for (int b = 0; b < 32; ++b) p.src[b] = b < B ? src[b] : -1;      // (B > 32 is refused by the launcher)
  return launch_attention_fwd_edit(p, (hipStream_t)stream);
}
// StyleAligned shared self-attention (attention.hip: attn_adain_part_kernel / attn_adain_coef_kernel, attn_shared_kernel)
long long pea_op_attn_adain_scratch_bytes(int B, int H, int S) { return (long long)attn_adain_scratch_bytes(B, H, S); }
int pea_op_attn_adain_coef(const void* Q, int ldq, const void* K, int ldk, int B, int H, int S, const int* ref, float scale,
                           int q_prescaled, int adain_queries, int adain_keys, float* coef, void* scratch, void* stream) {
  if (!ref) { pea_set_error("pea_op_attn_adain_coef: null ref (a host int[B]; negative entries for plain samples)"); return PEA_E_INVALID; }
  return launch_attn_adain_coef((const bf16*)Q, ldq, (const bf16*)K, ldk, B, H, S, ref, scale, q_prescaled, adain_queries, adain_keys,
                                coef, (float*)scratch, (hipStream_t)stream);
}
int pea_op_attention_fwd_shared(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H,
                                int Sq, int Skv, const int* ref, const float* coef, float scale, int q_prescaled,
                                float shared_score_scale, float shared_score_shift, int nd, void* stream) {
  if (!ref) { pea_set_error("pea_op_attention_fwd_shared: null ref (a host int[B]; negative entries for plain samples)"); return PEA_E_INVALID; }
  AttnSharedP p = attn_operands<AttnSharedP>(Q, ldq, K, ldk, V, ldv, O, ldo, nullptr, B, H, Sq, Skv, scale, nd, q_prescaled);
  p.coef = coef; p.share_scale = shared_score_scale; p.share_shift = shared_score_shift;
  for (int b = 0; b < 32; ++b) p.ref[b] = b < B ? ref[b] : -1;      // (B > 32 is refused by the launcher)
  return launch_attention_fwd_shared(p, (hipStream_t)stream);
}
int pea_op_attention_fwd_fewq(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* K2, int ldk2,
                              const void* V2, int ldv2, void* O, int ldo, float* lse, int B, int H, int Sq, int Skv, int Skv2,
                              float scale, int nd, int q_prescaled, void* stream) {
  AttnP p = attn_operands(Q, ldq, K, ldk, V, ldv, O, ldo, lse, B, H, Sq, Skv, scale, nd);
  p.q_prescaled = q_prescaled;
  p.K2 = (const bf16*)K2; p.V2 = (const bf16*)V2; p.ldk2 = ldk2; p.ldv2 = ldv2; p.Skv2 = Skv2;
  return launch_attention_fwd_fewq(p, (hipStream_t)stream);
}
int pea_op_attention_bwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                         int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                         void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                         int accum_dq, int accum_dkv, int nd, void* scratch, void* stream) {
  return attention_bwd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse, delta, dQ, lddq, dK, lddk, dV, lddv, B, H, Sq, Skv,
                            scale, accum_dq, accum_dkv, nd, scratch, 0, nullptr, stream);
}
int pea_op_attention_bwd_prescaled(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                                   int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                                   void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                                   int accum_dq, int accum_dkv, int nd, void* scratch, void* stream) {
  return attention_bwd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse, delta, dQ, lddq, dK, lddk, dV, lddv, B, H, Sq, Skv,
                            scale, accum_dq, accum_dkv, nd, scratch, 1, nullptr, stream);
}
int pea_op_attention_bwd_masked(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* O,
                                int ldo, const void* dO, int lddo, const float* lse, float* delta, void* dQ, int lddq,
                                void* dK, int lddk, void* dV, int lddv, int B, int H, int Sq, int Skv, float scale,
                                int accum_dq, int accum_dkv, int nd, void* scratch, int q_prescaled, const int* kv_len,
                                void* stream) {
  return attention_bwd_impl(Q, ldq, K, ldk, V, ldv, O, ldo, dO, lddo, lse, delta, dQ, lddq, dK, lddk, dV, lddv, B, H, Sq, Skv,
                            scale, accum_dq, accum_dkv, nd, scratch, q_prescaled, kv_len, stream);
}

int pea_op_geglu_fwd(const void* hg, void* y, long long rows, int inner, void* stream) {
  return launch_geglu_fwd((const bf16*)hg, (bf16*)y, rows, inner, (hipStream_t)stream);
}
int pea_op_geglu_bwd(const void* hg, const void* dy, void* dhg, long long rows, int inner, void* stream) {
  return launch_geglu_bwd((const bf16*)hg, (const bf16*)dy, (bf16*)dhg, rows, inner, (hipStream_t)stream);
}
int pea_op_sumpool2(const void* x, void* y, int B, int H, int W, int C, int accum, void* stream) {
  return launch_sumpool2((const bf16*)x, (bf16*)y, B, H, W, C, accum, (hipStream_t)stream);
}
int pea_op_timestep_embed(const float* t, void* y, int n, int dim, void* stream) {
  return launch_timestep_embed(t, (bf16*)y, n, dim, (hipStream_t)stream);
}
int pea_op_add_noise(const float* x0, const float* eps, const long long* t, const float* ac, float* xt, int B,
                     long long per, void* stream) {
  return launch_add_noise(x0, eps, t, ac, xt, B, per, (hipStream_t)stream);
}
int pea_op_cast_f32_bf16(const float* x, void* y, long long n, void* stream) {
  return launch_cast_f32_bf16(x, (bf16*)y, n, (hipStream_t)stream);
}
int pea_op_cast_bf16_f32(const void* x, float* y, long long n, void* stream) {
  return launch_cast_bf16_f32((const bf16*)x, y, n, (hipStream_t)stream);
}

// tmap: optional device int[B], the row of student sample b inside COMPACTED teacher tensors (KdLossP::tmap), null = row b
int pea_op_kd_loss_tmap(int ntaps, const void* const* taps_s, const void* const* taps_t, void* const* dtaps,
                        const long long* per, const float* eps_s, const float* eps, const float* eps_t, float* deps_s,
                        long long per_eps, const long long* zh, const int* tmap, int B, float feat_weight, int nan_guard,
                        float grad_scale, float* losses, void* workspace, void* stream) {
  if (ntaps < 0 || ntaps > PEA_MAX_TAPS) {
    pea_set_error("kd_loss: ntaps=%d out of range", ntaps);
    return PEA_E_SHAPE;
  }
  KdLossP p;
  memset(&p, 0, sizeof(p));
  p.kd_samples_hint = -1;
  p.ntaps = ntaps;
  for (int k = 0; k < ntaps; ++k) {
    p.fs[k] = (const bf16*)taps_s[k];
    p.ft[k] = (const bf16*)taps_t[k];
    p.dfs[k] = dtaps ? (bf16*)dtaps[k] : nullptr;
    p.per[k] = per[k];
  }
  p.eps_s = eps_s; p.eps = eps; p.eps_t = eps_t; p.deps_s = deps_s; p.per_eps = per_eps; p.zh = zh; p.B = B;
  p.feat_weight = feat_weight; p.nan_guard = nan_guard; p.grad_scale = grad_scale; p.losses = losses;
  p.partial = (float*)workspace; p.tmap = tmap;
  return launch_kd_loss(p, (hipStream_t)stream);
}
int pea_op_kd_loss(int ntaps, const void* const* taps_s, const void* const* taps_t, void* const* dtaps,
                   const long long* per, const float* eps_s, const float* eps, const float* eps_t, float* deps_s,
                   long long per_eps, const long long* zh, int B, float feat_weight, int nan_guard,
                   float grad_scale, float* losses, void* workspace, void* stream) {
  return pea_op_kd_loss_tmap(ntaps, taps_s, taps_t, dtaps, per, eps_s, eps, eps_t, deps_s, per_eps, zh, nullptr, B, feat_weight,
                             nan_guard, grad_scale, losses, workspace, stream);
}

long long pea_op_attention_bwd_scratch_bytes(int B, int H, int Sq, int Skv, int nd) {
  return (long long)attention_bwd_scratch_bytes(B, H, Sq, Skv, nd);
}
long long pea_op_groupnorm_scratch_bytes(int B, int HW, int C, int groups) {
  return (long long)groupnorm_scratch_bytes(B, HW, C, groups);
}
long long pea_op_kd_loss_workspace_bytes(int ntaps, const long long* per, long long per_eps, int B) {
  return (long long)kd_loss_workspace_bytes(ntaps, per, per_eps, B);
}

int pea_op_prefetch(const void* p, long long bytes, void* stream) {
  return launch_prefetch(p, bytes, nullptr, (hipStream_t)stream);
}

int pea_op_adamw(float* w, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                 float eps, float weight_decay, int step, float grad_scale, void* stream) {
  return launch_adamw(w, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, (hipStream_t)stream);
}

// ---- inference denoise-loop glue (sampler.hip)
long long pea_op_cfg_combine_workspace_bytes(int B) { return (long long)cfg_combine_workspace_bytes(B); }
int pea_op_cfg_combine(const float* eps2, float* out, int B, long long per, float guidance_scale, float guidance_rescale,
                       void* workspace, void* stream) {
  if (!eps2 || !out) { pea_set_error("pea_op_cfg_combine: null pointer"); return PEA_E_INVALID; }
  return launch_cfg_combine(eps2, out, B, per, guidance_scale, guidance_rescale, workspace, (hipStream_t)stream);
}
int pea_op_dpm_update(float* sample, const float* eps, float* x0_prev, long long n, float alpha_s, float sigma_s,
                      float c_s, float c_0, float c_1, void* stream) {
  if (!sample || !eps || !x0_prev) { pea_set_error("pea_op_dpm_update: null pointer"); return PEA_E_INVALID; }
  return launch_dpm_update(sample, eps, x0_prev, n, alpha_s, sigma_s, c_s, c_0, c_1, (hipStream_t)stream);
}
int pea_op_lcm_update(float* sample, const float* eps, const float* noise, float* denoised, long long n, float kx, float ke,
                      float c_prev, float c_noise, void* stream) {
  return launch_lcm_update(sample, eps, noise, denoised, n, kx, ke, c_prev, c_noise, (hipStream_t)stream);
}
int pea_op_euler_update(float* sample, const float* eps, const float* noise, float* model_in, long long n, int dup, float k_e,
                        float k_n, float k_s, void* stream) {
  return launch_euler_update(sample, eps, noise, model_in, n, dup, k_e, k_n, k_s, (hipStream_t)stream);
}
// ---- MultiDiffusion panoramas (sampler.hip: view gather, overlap merge, the per-view rescale factors)
int pea_op_views_gather(const float* canvas, float* model_in, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc,
                        int Wc, int h, int w, int wrap_x, float k_s, void* stream) {
  return launch_views_gather(canvas, model_in, slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap_x, k_s, (hipStream_t)stream);
}
int pea_op_views_merge(const float* eps, float* canvas, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc, int Wc,
                       int h, int w, int wrap_x, float guidance_scale, const float* factor, const float* wy, const float* wx,
                       const float* total, int first, int last, void* stream) {
  return launch_views_merge(eps, canvas, slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap_x, guidance_scale, factor, wy, wx, total,
                            first, last, (hipStream_t)stream);
}
int pea_op_cfg_rescale_factors(const float* eps2, int B, long long per, float guidance_scale, float guidance_rescale, void* workspace,
                               float* factor, void* stream) {
  return launch_cfg_rescale_factors(eps2, B, per, guidance_scale, guidance_rescale, workspace, factor, (hipStream_t)stream);
}
// ---- self-attention guidance (attention.hip: the column sums; sampler.hip: degrade and combine)
int pea_op_attention_colsum_groups(int B, int H, int Sq, int Skv) { return attention_colsum_groups(B, H, Sq, Skv); }
int pea_op_attention_colsum(const void* Q, int ldq, const void* K, int ldk, const float* lse, float* part, int B, int H, int Sq, int Skv,
                            float scale, int q_prescaled, void* stream) {
  AttnColsumP p = attn_operands<AttnColsumP>(Q, ldq, K, ldk, nullptr, 0, nullptr, 0, nullptr, B, H, Sq, Skv, scale, 1, q_prescaled);
  p.lse = lse; p.part = part;
  return launch_attention_colsum(p, (hipStream_t)stream);
}
int pea_op_sag_degrade(const float* latents, const float* eps, const float* part, int G, int map_h, int map_w, const int* iy,
                       const int* ix, float* out, int B, int C, int H, int W, float c_x, float c_e, float o_b, float o_e, void* stream) {
  return launch_sag_degrade(latents, eps, part, G, map_h, map_w, iy, ix, out, B, C, H, W, c_x, c_e, o_b, o_e, (hipStream_t)stream);
}
int pea_op_cfg_sag_combine(const float* eps, const float* eps_deg, float* out, int B, long long per, int cfg, float guidance_scale,
                           float sag_scale, void* stream) {
  return launch_cfg_sag_combine(eps, eps_deg, out, B, per, cfg, guidance_scale, sag_scale, (hipStream_t)stream);
}
// ---- perturbed-attention / smoothed-energy guidance (elementwise.hip: the query blur and the pitched copy; sampler.hip: the combine)
int pea_op_query_blur(void* Q, int ld, int col0, int n, int h, int w, int C, const float* Mh, const float* Mw, void* stream) {
  SHAPECHK(Q, "query_blur: null operand");
  SHAPECHK(col0 >= 0 && col0 % 8 == 0 && C > 0 && col0 <= ld - C, "query_blur: columns %d .. %d of rows of %d (an offset that is a multiple of 8, inside the row)",
           col0, col0 + C - 1, ld);
  return launch_query_blur((bf16*)Q + col0, ld, n, h, w, C, Mh, Mw, (hipStream_t)stream);
}
int pea_op_query_blur_lds_bytes(int h, int w) {
  return h > 0 && w > 0 && h <= QUERY_BLUR_MAX_SIDE && w <= QUERY_BLUR_MAX_SIDE ? (int)query_blur_lds_bytes(h, w) : PEA_E_SHAPE;
}
int pea_op_attn_identity(const void* V, int ldv, int col0, void* O, int ldo, long long rows, int C, void* stream) {
  SHAPECHK(V && O, "attn_identity: null operand");
  SHAPECHK(rows > 0 && C > 0 && C % 8 == 0 && col0 >= 0 && col0 % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && col0 <= ldv - C && ldo >= C,
           "attn_identity: %lld rows, columns %d .. %d of %d -> %d of %d (multiples of 8, inside the rows)", rows, col0, col0 + C - 1, ldv, C, ldo);
  SHAPECHK((((uintptr_t)V | (uintptr_t)O) & 15) == 0, "attn_identity: V and O are 16-byte aligned");
  return launch_copy2d((const bf16*)V + col0, ldv, (bf16*)O, ldo, rows, C, 0, (hipStream_t)stream);
}
int pea_op_cfg_pag_combine(const float* eps, float* out, int B, long long per, int cfg, float guidance_scale, float pag_scale,
                           float guidance_rescale, void* workspace, void* stream) {
  return launch_cfg_pag_combine(eps, out, B, per, cfg, guidance_scale, pag_scale, guidance_rescale, workspace, (hipStream_t)stream);
}
// ---- semantic guidance (sega.hip: the per-group quantile select and the masked combine)
long long pea_op_sega_workspace_bytes(int B, int C, int K) { return (long long)sega_workspace_bytes(B, C, K); }
int pea_op_abs_diff_quantile(const float* eps, float* thr, float* bounds, int B, int C, int hw, int K, const float* edit_scale,
                             const float* quantile, const float* weight, void* stream) {
  return launch_abs_diff_quantile(eps, thr, bounds, B, C, hw, K, edit_scale, quantile, weight, (hipStream_t)stream);
}
int pea_op_cfg_sega_combine(const float* eps, float* momentum, float* out, int B, int C, int hw, int K, float guidance_scale,
                            const float* edit_scale, const float* quantile, const float* weight, const int* warm, float momentum_scale,
                            float momentum_beta, void* workspace, void* stream) {
  return launch_cfg_sega_combine(eps, momentum, out, B, C, hw, K, guidance_scale, edit_scale, quantile, weight, warm, momentum_scale,
                                 momentum_beta, workspace, (hipStream_t)stream);
}
// ---- LoRA weight composition (lora.hip)
int pea_op_lora_compose(const float* acc, const float* down, const float* up, float* out, int M, int Kf, int rank, float scale,
                        void* stream) {
  return launch_lora_compose(acc, down, up, out, M, Kf, rank, scale, (hipStream_t)stream);
}
int pea_op_inpaint_prepare(const float* image, const float* mask, int N, int H, int W, float* init_image, float* masked_image,
                           float* latent_mask, void* stream) {
  if (!image || !mask || !init_image || !masked_image || !latent_mask) {
    pea_set_error("pea_op_inpaint_prepare: null pointer");
    return PEA_E_INVALID;
  }
  return launch_inpaint_prepare(image, mask, N, H, W, init_image, masked_image, latent_mask, (hipStream_t)stream);
}

// ---- the glue kernels between the families above (elementwise.hip, norm.hip, sampler.hip, gemm.hip, kdloss.hip), one
// entry per launcher: a cast and a forward each, for the kernel-level parity tests (tests/test_glue_ops_gpu.py)
int pea_op_add(const void* a, const void* b, void* y, long long n, void* stream) {
  return launch_add((const bf16*)a, (const bf16*)b, (bf16*)y, n, (hipStream_t)stream);
}
int pea_op_silu_fwd(const void* x, void* y, long long n, void* stream) {
  return launch_silu_fwd((const bf16*)x, (bf16*)y, n, (hipStream_t)stream);
}
int pea_op_silu_bwd(const void* x, const void* dy, void* dx, long long n, int accum, void* stream) {
  return launch_silu_bwd((const bf16*)x, (const bf16*)dy, (bf16*)dx, n, accum, (hipStream_t)stream);
}
int pea_op_gelu_fwd(const void* x, void* y, long long n, void* stream) {
  return launch_gelu_fwd((const bf16*)x, (bf16*)y, n, (hipStream_t)stream);
}
int pea_op_gelu_bwd(const void* x, const void* dy, void* dx, long long n, int accum, void* stream) {
  return launch_gelu_bwd((const bf16*)x, (const bf16*)dy, (bf16*)dx, n, accum, (hipStream_t)stream);
}
int pea_op_accum(const void* x, void* y, long long n, int accum, void* stream) {
  return launch_accum((const bf16*)x, (bf16*)y, n, accum, (hipStream_t)stream);
}
int pea_op_geglu_bwd_il(const void* hg, const void* dy, void* dhg, long long rows, int inner, void* stream) {
  return launch_geglu_bwd_il((const bf16*)hg, (const bf16*)dy, (bf16*)dhg, rows, inner, (hipStream_t)stream);
}
int pea_op_select_rows(const void* c, const void* u, const void* mask, void* y, int B, long long per, long long ystride,
                       void* stream) {
  return launch_select_rows((const bf16*)c, (const bf16*)u, (const unsigned char*)mask, (bf16*)y, B, per, (hipStream_t)stream, ystride);
}
int pea_op_select_rows_bwd(const void* dy, const void* mask, void* dc, void* du, int B, long long per, long long dystride,
                           void* stream) {
  return launch_select_rows_bwd((const bf16*)dy, (const unsigned char*)mask, (bf16*)dc, (bf16*)du, B, per, (hipStream_t)stream, dystride);
}
int pea_op_mean_tokens(const void* x, void* y, int B, int L, int C, void* stream) {
  return launch_mean_tokens((const bf16*)x, (bf16*)y, B, L, C, (hipStream_t)stream);
}
int pea_op_mean_tokens_bwd(const void* dy, void* dx, int B, int L, int C, int accum, void* stream) {
  return launch_mean_tokens_bwd((const bf16*)dy, (bf16*)dx, B, L, C, accum, (hipStream_t)stream);
}
int pea_op_colsum(const void* x, float* db, int R, int C, int accum, void* stream) {
  return launch_colsum((const bf16*)x, db, R, C, accum, (hipStream_t)stream);
}
long long pea_op_colsum_batched_scratch_bytes(int B, int HW, int C) { return (long long)colsum_batched_scratch_bytes(B, HW, C); }
int pea_op_colsum_batched(const void* x, float* out, int B, int HW, int C, int ldo, void* scratch, void* stream) {
  return launch_colsum_batched((const bf16*)x, out, B, HW, C, ldo, (float*)scratch, (hipStream_t)stream);
}
int pea_op_copy2d(const void* x, int ldx, void* y, int ldy, long long rows, int C, int accum, void* stream) {
  return launch_copy2d((const bf16*)x, ldx, (bf16*)y, ldy, rows, C, accum, (hipStream_t)stream);
}
int pea_op_transpose_bf16(const void* x, void* y, int R, int C, int ldy, void* stream) {
  return launch_transpose_bf16((const bf16*)x, (bf16*)y, R, C, ldy, (hipStream_t)stream);
}
int pea_op_transpose_f32_bf16(const float* x, void* y, int R, int C, int ldy, void* stream) {
  return launch_transpose_f32_bf16(x, (bf16*)y, R, C, ldy, (hipStream_t)stream);
}
int pea_op_nhwc_to_nchw_f32(const void* x, float* y, int B, int HW, int C, int dH, int dW, void* stream) {
  return launch_nhwc_to_nchw_f32((const bf16*)x, y, B, HW, C, (hipStream_t)stream, dH, dW);
}
int pea_op_nchw_f32_to_nhwc(const float* x, void* y, int B, int HW, int C, int dH, int dW, void* stream) {
  return launch_nchw_f32_to_nhwc(x, (bf16*)y, B, HW, C, (hipStream_t)stream, dH, dW);
}
int pea_op_pad_gather(const float* src, int N_t, int K_t, int mode, int d, int dp, void* w, int ldw, void* wt, int ldwt, int st_n,
                      int st_k, void* stream) {
  return launch_pad_gather(src, N_t, K_t, mode, d, dp, (bf16*)w, ldw, (bf16*)wt, ldwt, st_n, st_k, (hipStream_t)stream);
}
int pea_op_pad_head_vec(const float* src, float* dst, int heads, int d, int dp, void* stream) {
  return launch_pad_head_vec(src, dst, heads, d, dp, (hipStream_t)stream);
}
int pea_op_permute_geglu_vec(const float* src, float* dst, int inner, void* stream) {
  return launch_permute_geglu_vec(src, dst, inner, (hipStream_t)stream);
}
int pea_op_cast_i64_f32(const long long* x, float* y, long long n, void* stream) {
  return launch_cast_i64_f32(x, y, n, (hipStream_t)stream);
}
int pea_op_fill_random_bf16(void* p, long long n, unsigned long long seed, float scale, void* stream) {
  return launch_fill_random_bf16((bf16*)p, n, seed, scale, (hipStream_t)stream);
}
int pea_op_fill_random_f32(float* p, long long n, unsigned long long seed, float scale, float offset, void* stream) {
  return launch_fill_random_f32(p, n, seed, scale, offset, (hipStream_t)stream);
}
int pea_op_splitk_reduce(const float* part, int nsplit, long long stride, void* out, int ldo, int M, int N, int accum, void* stream) {
  return launch_splitk_reduce(part, nsplit, stride, (bf16*)out, ldo, M, N, accum, (hipStream_t)stream);
}
int pea_op_rmsnorm_fwd(const void* x, const float* gamma, void* y, int R, int C, float eps, void* stream) {
  return launch_rmsnorm_fwd((const bf16*)x, gamma, (bf16*)y, R, C, eps, (hipStream_t)stream);
}
int pea_op_layernorm_stats(const void* x, float* stats, int R, int C, float eps, void* stream) {
  return launch_layernorm_stats((const bf16*)x, stats, R, C, eps, (hipStream_t)stream);
}
int pea_op_softmax_rows(void* s, long long rows, int cols, int ld, float scale, void* stream) {
  return launch_softmax_rows((bf16*)s, rows, cols, ld, scale, (hipStream_t)stream);
}
int pea_op_residual_import(const void* src, int dtype, void* dst, int B, int C, long long HW, float scale, void* stream) {
  return launch_residual_import(src, dtype, (bf16*)dst, B, C, HW, scale, (hipStream_t)stream);
}
int pea_op_vae_posterior(const float* h, const float* wq, const float* bq, const float* noise, float* moments, float* latents, int B,
                         int C2, long long HW, float scaling, void* stream) {
  return launch_vae_posterior(h, wq, bq, noise, moments, latents, B, C2, HW, scaling, (hipStream_t)stream);
}
int pea_op_vae_post_quant(const float* z, const float* w, const float* b, float* out, int B, int C, long long HW, float inv_scaling,
                          void* stream) {
  return launch_vae_post_quant(z, w, b, out, B, C, HW, inv_scaling, (hipStream_t)stream);
}
int pea_op_embed_tokens(const long long* ids, const void* tok, const void* pos, const void* type0, void* out, int B, int L, int width,
                        int vocab, void* stream) {
  return launch_embed_tokens(ids, (const bf16*)tok, (const bf16*)pos, (const bf16*)type0, (bf16*)out, B, L, width, vocab, (hipStream_t)stream);
}
int pea_op_t5_rel_bias(const float* rel, const int* dist_bucket, float* bias, int H, int L, int pitch, int half_buckets, void* stream) {
  return launch_t5_rel_bias(rel, dist_bucket, bias, H, L, pitch, half_buckets, (hipStream_t)stream);
}
int pea_op_gather_eos(const long long* ids, const void* x, void* out, int B, int L, int width, long long eos_id, void* stream) {
  return launch_gather_eos(ids, (const bf16*)x, (bf16*)out, B, L, width, eos_id, (hipStream_t)stream);
}
int pea_op_kv_len(const long long* ids, int* len, int B, int L, long long pad_id, void* stream) {
  return launch_kv_len(ids, len, B, L, pad_id, (hipStream_t)stream);
}

}  // extern "C"
