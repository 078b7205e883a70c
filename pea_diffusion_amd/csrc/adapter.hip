// The PEA adapter: MLP of train_sdxl_zh.py:43-67 (SD1.5: train_sd_zh.py:41-56): LayerNorm -> 3 x (Linear, no bias)
// with GELU(erf) between -> { GELU -> Linear+bias = tokens ; mean over tokens = pooled }.
// Forward GEMMs use the fused GELU epilogue (pre-activation stashed for the backward);
// backward = dgrad (transposed bf16 copies) + wgrad (fp32 accumulation into the flat grad buffer).
#include <algorithm>

#include "model.h"

Adapter::~Adapter() {
  if (arena) (void)hipFree(arena);
}

int Adapter::prepare(int B2_, int L_) {
  SHAPECHK(in_dim % 64 == 0 && hidden % 64 == 0 && out_dim % 64 == 0 && (out1 == 0 || out1 % 64 == 0),
           "adapter: dims must be multiples of 64 (in=%d hidden=%d out=%d out1=%d)", in_dim, hidden, out_dim, out1);
  SHAPECHK(!use_residual || in_dim == out_dim, "adapter: use_residual needs in_dim == out_dim");
  B2 = B2_; L = L_; R = B2 * L; Rpad = (R + 63) / 64 * 64;
  off_lnw = 0; off_lnb = in_dim; off_w0 = off_lnb + in_dim; off_w1 = off_w0 + (long long)hidden * in_dim;
  off_w2 = off_w1 + (long long)hidden * hidden; off_fcw = off_w2 + (long long)out_dim * hidden;
  off_fcb = off_fcw + (long long)out1 * out_dim; nparam = off_fcb + out1;
  if (arena) { (void)hipFree(arena); arena = nullptr; }
  size_t off = 0;
  std::vector<std::pair<bf16**, size_t>> req;
  auto want = [&](bf16** p, size_t elems) { req.push_back({p, off}); off += al256(elems * 2); };
  const size_t mx = (size_t)std::max(std::max(in_dim, hidden), std::max(out_dim, std::max(out1, 64)));
  want(&w0, (size_t)hidden * in_dim); want(&w1, (size_t)hidden * hidden); want(&w2, (size_t)out_dim * hidden);
  want(&wfc, (size_t)out1 * out_dim + 64);
  want(&w0t, (size_t)hidden * in_dim); want(&w1t, (size_t)hidden * hidden); want(&w2t, (size_t)out_dim * hidden);
  want(&wfct, (size_t)out1 * out_dim + 64);
  want(&x, (size_t)R * in_dim); want(&xn, (size_t)R * in_dim);
  want(&z0, (size_t)R * hidden); want(&a0, (size_t)R * hidden); want(&z1, (size_t)R * hidden); want(&a1, (size_t)R * hidden);
  want(&z2, (size_t)R * out_dim); want(&a2, (size_t)R * out_dim); want(&tok, (size_t)R * (out1 ? out1 : 64));
  want(&pooled, (size_t)B2 * out_dim);
  want(&dtok, (size_t)R * (out1 ? out1 : 64)); want(&da2, (size_t)R * out_dim); want(&dz2, (size_t)R * out_dim);
  want(&da1, (size_t)R * hidden); want(&dz1, (size_t)R * hidden); want(&da0, (size_t)R * hidden);
  want(&dz0, (size_t)R * hidden); want(&dxn, (size_t)R * in_dim); want(&dpool, (size_t)B2 * out_dim);
  want(&tA, mx * Rpad); want(&tB, mx * Rpad);
  const size_t stats_off = off;
  off += al256((size_t)R * 2 * 4);
  HIPCHK(hipMalloc((void**)&arena, off));
  HIPCHK(hipMemset(arena, 0, off));
  for (auto& r : req) *r.first = (bf16*)(arena + r.second);
  ln_stats = (float*)(arena + stats_off);
  return PEA_OK;
}

int Adapter::sync_weights(hipStream_t s) {
  SHAPECHK(params != nullptr, "adapter: parameter buffer not set");
  RC(launch_cast_f32_bf16(params + off_w0, w0, (long long)hidden * in_dim, s));
  RC(launch_cast_f32_bf16(params + off_w1, w1, (long long)hidden * hidden, s));
  RC(launch_cast_f32_bf16(params + off_w2, w2, (long long)out_dim * hidden, s));
  RC(launch_transpose_f32_bf16(params + off_w0, w0t, hidden, in_dim, hidden, s));
  RC(launch_transpose_f32_bf16(params + off_w1, w1t, hidden, hidden, hidden, s));
  RC(launch_transpose_f32_bf16(params + off_w2, w2t, out_dim, hidden, out_dim, s));
  if (out1) {
    RC(launch_cast_f32_bf16(params + off_fcw, wfc, (long long)out1 * out_dim, s));
    RC(launch_transpose_f32_bf16(params + off_fcw, wfct, out1, out_dim, out1, s));
  }
  return PEA_OK;
}

static int agemm(const bf16* A, int lda, const bf16* W, int ldw, void* C, int ldc, int M, int N, int K, int act,
                 bf16* pre, const float* bias, int out_f32, int accum, hipStream_t s) {
  GemmP p; fill_gemm(p);
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.act = act;
  p.preact = pre; p.ldpre = N; p.bias = bias; p.out_f32 = out_f32; p.accum_f32 = accum;
  return launch_gemm(p, s);
}

int Adapter::forward(const void* enc, const void* enc2, int dtype, hipStream_t s) {
  SHAPECHK(arena && params, "adapter: prepare()/bind() first");
  // enc2 == nullptr: enc holds all R rows; otherwise enc / enc2 hold R/2 rows each (cond | uncond)
  const long long n1 = (enc2 ? (long long)(R / 2) : (long long)R) * in_dim;
  if (dtype == 0) RC(launch_cast_f32_bf16((const float*)enc, x, n1, s));
  else HIPCHK(hipMemcpyAsync(x, enc, (size_t)n1 * 2, hipMemcpyDeviceToDevice, s));
  if (enc2) {
    if (dtype == 0) RC(launch_cast_f32_bf16((const float*)enc2, x + n1, n1, s));
    else HIPCHK(hipMemcpyAsync(x + n1, enc2, (size_t)n1 * 2, hipMemcpyDeviceToDevice, s));
  }
  RC(launch_layernorm_fwd(x, params + off_lnw, params + off_lnb, xn, ln_stats, R, in_dim, 1e-5f, s));
  RC(agemm(xn, in_dim, w0, in_dim, a0, hidden, R, hidden, in_dim, 1, z0, nullptr, 0, 0, s));
  RC(agemm(a0, hidden, w1, hidden, a1, hidden, R, hidden, hidden, 1, z1, nullptr, 0, 0, s));
  if (out1) {
    RC(agemm(a1, hidden, w2, hidden, a2, out_dim, R, out_dim, hidden, 1, z2, nullptr, 0, 0, s));
    RC(agemm(a2, out_dim, wfc, out_dim, tok, out1, R, out1, out_dim, 0, nullptr, params + off_fcb, 0, 0, s));
    if (use_residual) {
      RC(launch_add(z2, x, dz2, (long long)R * out_dim, s));   // dz2 is free during the forward pass
      RC(launch_mean_tokens(dz2, pooled, B2, L, out_dim, s));
    } else {
      RC(launch_mean_tokens(z2, pooled, B2, L, out_dim, s));
    }
  } else {
    RC(agemm(a1, hidden, w2, hidden, z2, out_dim, R, out_dim, hidden, 0, nullptr, nullptr, 0, 0, s));
  }
  return PEA_OK;
}

// dW[N][K] (+)= dZ[R][N]^T . X[R][K]  via transposed operands (contraction padded to Rpad with zeros)
static int wgrad(Adapter& a, const bf16* dZ, int N, const bf16* X, int K, float* dW, int accum, hipStream_t s) {
  RC(launch_transpose_bf16(dZ, a.tA, a.R, N, a.Rpad, s));
  RC(launch_transpose_bf16(X, a.tB, a.R, K, a.Rpad, s));
  return agemm(a.tA, a.Rpad, a.tB, a.Rpad, dW, K, N, K, a.Rpad, 0, nullptr, nullptr, 1, accum, s);
}

int Adapter::backward(float* g, int accumulate, hipStream_t s) {
  // inputs: dtok [R][out1] (SD1.5: dz2 [R][out]) and dpool [B2][out] already filled by the caller
  if (!accumulate) HIPCHK(hipMemsetAsync(g, 0, nparam * 4, s));
  if (out1) {
    RC(agemm(dtok, out1, wfct, out1, da2, out_dim, R, out_dim, out1, 0, nullptr, nullptr, 0, 0, s));
    RC(wgrad(*this, dtok, out1, a2, out_dim, g + off_fcw, 1, s));
    RC(launch_colsum(dtok, g + off_fcb, R, out1, 1, s));
    RC(launch_gelu_bwd(z2, da2, dz2, (long long)R * out_dim, 0, s));
    RC(launch_mean_tokens_bwd(dpool, dz2, B2, L, out_dim, 1, s));
  }
  RC(agemm(dz2, out_dim, w2t, out_dim, da1, hidden, R, hidden, out_dim, 0, nullptr, nullptr, 0, 0, s));
  RC(wgrad(*this, dz2, out_dim, a1, hidden, g + off_w2, 1, s));
  RC(launch_gelu_bwd(z1, da1, dz1, (long long)R * hidden, 0, s));
  RC(agemm(dz1, hidden, w1t, hidden, da0, hidden, R, hidden, hidden, 0, nullptr, nullptr, 0, 0, s));
  RC(wgrad(*this, dz1, hidden, a0, hidden, g + off_w1, 1, s));
  RC(launch_gelu_bwd(z0, da0, dz0, (long long)R * hidden, 0, s));
  RC(agemm(dz0, hidden, w0t, hidden, dxn, in_dim, R, in_dim, hidden, 0, nullptr, nullptr, 0, 0, s));
  RC(wgrad(*this, dz0, hidden, xn, in_dim, g + off_w0, 1, s));
  RC(launch_layernorm_bwd(x, dxn, params + off_lnw, ln_stats, nullptr /*no input gradient needed*/, g + off_lnw, g + off_lnb, R,
                          in_dim, 0, s));
  return PEA_OK;
}
