// Inference denoise-loop glue of tests/test_sdxl_zh.py:376-406: classifier-free-guidance combine (+ the std rescale of
// rescale_noise_cfg, :44-56) and the DPM-Solver++ (2M) latent update.  fp32 NCHW latents; HBM-bound elementwise and
// fixed-order reductions (bit-reproducible).  The schedule's scalar coefficients are computed on the host.
#include "pea_kernels.h"

#define SM_LOOP(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)
static inline int sm_grid(long long n) { long long g = (n + 255) / 256; return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g)); }

// eps2 = [uncond (B samples) | text (B samples)]; out = u + g * (t - u)
__global__ void cfg_combine_kernel(const float* __restrict__ eps2, float* __restrict__ out, long long n, float g) {
  SM_LOOP(i, n) {
    const float u = eps2[i], t = eps2[n + i];
    out[i] = u + g * (t - u);
  }
}

#define CFG_NBLK 64
// The guided prediction of element i: u + g (t - u); PAG (perturbed-attention / smoothed-energy guidance): eps holds a third run of
// samples p behind t, and sg (t - p) is added -- at sg = 0 the first form's bits.
template <bool PAG>
__device__ __forceinline__ float cfg_guided(const float* __restrict__ eps, long long n, long long i, float uv, float tv, float g, float sg) {
  const float c = uv + g * (tv - uv);
  if constexpr (PAG) return sg != 0.f ? c + sg * (tv - eps[2 * n + i]) : c;
  return c;
}
// per (sample, block): sums of t, t^2, c, c^2 in double, fixed order inside the block
template <bool PAG>
__global__ __launch_bounds__(256) void cfg_stats_kernel(const float* __restrict__ eps2, long long n, long long per,
                                                        float g, float sg, double* __restrict__ part) {
  const int b = blockIdx.y;
  const float* u = eps2 + (long long)b * per;
  const float* t = eps2 + n + (long long)b * per;
  double s[4] = {0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)CFG_NBLK * 256) {
    const float uv = u[i], tv = t[i];
    const float c = cfg_guided<PAG>(eps2, n, (long long)b * per + i, uv, tv, g, sg);
    s[0] += tv; s[1] += (double)tv * tv; s[2] += c; s[3] += (double)c * c;
  }
  __shared__ double red[4][256];
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x < 4) part[((long long)b * CFG_NBLK + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
}
// factor[b] = phi * std_text / std_cfg + (1 - phi)   (torch.std: unbiased)
__global__ void cfg_factor_kernel(const double* __restrict__ part, float* __restrict__ factor, int B, long long per,
                                  float phi) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s[4] = {0, 0, 0, 0};
  for (int k = 0; k < CFG_NBLK; ++k)
    for (int j = 0; j < 4; ++j) s[j] += part[((long long)b * CFG_NBLK + k) * 4 + j];
  const double nn = (double)per;
  const double vt = (s[1] - s[0] * s[0] / nn) / (nn - 1.0), vc = (s[3] - s[2] * s[2] / nn) / (nn - 1.0);
  factor[b] = (float)((double)phi * sqrt(vt / vc) + (1.0 - (double)phi));
}
template <bool PAG>
__global__ void cfg_apply_kernel(const float* __restrict__ eps2, float* __restrict__ out, long long n, long long per,
                                 float g, float sg, const float* __restrict__ factor) {
  SM_LOOP(i, n) {
    const float u = eps2[i], t = eps2[n + i];
    out[i] = cfg_guided<PAG>(eps2, n, i, u, t, g, sg) * factor[i / per];
  }
}

size_t cfg_combine_workspace_bytes(int B) { return (size_t)B * CFG_NBLK * 4 * sizeof(double) + (size_t)B * sizeof(float); }

int launch_cfg_combine(const float* eps2, float* out, int B, long long per, float g, float rescale, void* ws,
                       hipStream_t s) {
  SHAPECHK(B > 0 && per > 1, "cfg_combine: B=%d per=%lld", B, per);
  const long long n = (long long)B * per;
  if (rescale <= 0.f) {
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(sm_grid(n)), dim3(256), 0, s, eps2, out, n, g);
  } else {
    SHAPECHK(ws != nullptr, "cfg_combine: guidance_rescale needs the workspace");
    double* part = (double*)ws;
    float* factor = (float*)(part + (size_t)B * CFG_NBLK * 4);
    hipLaunchKernelGGL(cfg_stats_kernel<false>, dim3(CFG_NBLK, B), dim3(256), 0, s, eps2, n, per, g, 0.f, part);
    hipLaunchKernelGGL(cfg_factor_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, part, factor, B, per, rescale);
    hipLaunchKernelGGL(cfg_apply_kernel<false>, dim3(sm_grid(n)), dim3(256), 0, s, eps2, out, n, per, g, 0.f, factor);
  }
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// Perturbed-attention / smoothed-energy guidance (Ahn et al. 2024; Hong 2024): the perturbed samples p ride in the same batch behind
// the text samples.  cfg: eps = [u | t | p] (B samples each), out = u + g (t - u) + sg (t - p), then rescale_noise_cfg against t when
// rescale > 0 -- cfg_combine's kernels with the third term, its reduction and its workspace; sg = 0 gives its bits on [u | t].
// Otherwise eps = [t | p], out = t + sg (t - p), and no rescale (it is defined against the CFG result).
__global__ void pag_combine_kernel(const float* __restrict__ eps, float* __restrict__ out, long long n, int cfg, float g, float sg) {
  SM_LOOP(i, n) {
    const float a = eps[i], b = eps[n + i];
    out[i] = cfg ? cfg_guided<true>(eps, n, i, a, b, g, sg) : (sg != 0.f ? a + sg * (a - b) : a);
  }
}
int launch_cfg_pag_combine(const float* eps, float* out, int B, long long per, int cfg, float g, float sg, float rescale, void* ws,
                           hipStream_t s) {
  SHAPECHK(eps && out, "cfg_pag_combine: null operand");
  SHAPECHK(B > 0 && per > 1, "cfg_pag_combine: B=%d per=%lld", B, per);
  const long long n = (long long)B * per;
  if (!cfg || rescale <= 0.f) {
    hipLaunchKernelGGL(pag_combine_kernel, dim3(sm_grid(n)), dim3(256), 0, s, eps, out, n, cfg != 0, g, sg);
  } else {
    SHAPECHK(ws != nullptr, "cfg_pag_combine: guidance_rescale needs the workspace (pea_op_cfg_combine_workspace_bytes)");
    double* part = (double*)ws;
    float* factor = (float*)(part + (size_t)B * CFG_NBLK * 4);
    hipLaunchKernelGGL(cfg_stats_kernel<true>, dim3(CFG_NBLK, B), dim3(256), 0, s, eps, n, per, g, sg, part);
    hipLaunchKernelGGL(cfg_factor_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, part, factor, B, per, rescale);
    hipLaunchKernelGGL(cfg_apply_kernel<true>, dim3(sm_grid(n)), dim3(256), 0, s, eps, out, n, per, g, sg, factor);
  }
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// x0 = (sample - sigma_s * eps) / alpha_s;  sample <- c_s * sample + c_0 * x0 + c_1 * x0_prev;  x0_prev <- x0
__global__ void dpm_update_kernel(float* __restrict__ sample, const float* __restrict__ eps, float* __restrict__ x0_prev,
                                  long long n, float inv_alpha, float sigma, float cs, float c0, float c1) {
  SM_LOOP(i, n) {
    const float x = sample[i];
    const float x0 = (x - sigma * eps[i]) * inv_alpha;
    float y = cs * x + c0 * x0;
    if (c1 != 0.f) y += c1 * x0_prev[i];
    sample[i] = y;
    x0_prev[i] = x0;
  }
}
int launch_dpm_update(float* sample, const float* eps, float* x0_prev, long long n, float alpha_s, float sigma_s,
                      float c_s, float c_0, float c_1, hipStream_t s) {
  SHAPECHK(n > 0 && alpha_s > 0.f, "dpm_update: n=%lld alpha=%g", n, alpha_s);
  hipLaunchKernelGGL(dpm_update_kernel, dim3(sm_grid(n)), dim3(256), 0, s, sample, eps, x0_prev, n, 1.0f / alpha_s,
                     sigma_s, c_s, c_0, c_1);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// LCMScheduler.step (tests/test_sdxl_zh_lcm.py:178; diffusers 0.23 [ext]) with the host's float64 scalars folded to four:
//   denoised = c_out * (x - sqrt(1 - a_t) eps) / sqrt(a_t) + c_skip * x = kx * x + ke * eps
//   sample  <- c_prev * denoised + c_noise * noise          (noise NULL, the last step: c_prev * denoised)
// The vector part covers [0, 4 n4) with 16-byte accesses, the scalar part the rest (everything when n4 == 0).
__global__ void lcm_update_kernel(float* __restrict__ sample, const float* __restrict__ eps, const float* __restrict__ noise,
                                  float* __restrict__ denoised, long long n, long long n4, float kx, float ke, float c_prev,
                                  float c_noise) {
  SM_LOOP(i, n4) {
    const f32x4 x = ((const f32x4*)sample)[i], e = ((const f32x4*)eps)[i];
    f32x4 d, y;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = fmaf(kx, x[j], ke * e[j]); y[j] = c_prev * d[j]; }
    if (noise) {
      const f32x4 z = ((const f32x4*)noise)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = fmaf(c_noise, z[j], y[j]);
    }
    ((f32x4*)sample)[i] = y;
    if (denoised) ((f32x4*)denoised)[i] = d;
  }
  SM_LOOP(t, n - 4 * n4) {
    const long long i = 4 * n4 + t;
    const float d = fmaf(kx, sample[i], ke * eps[i]);       // explicit fmaf: both parts round alike whatever hipcc contracts
    float y = c_prev * d;
    if (noise) y = fmaf(c_noise, noise[i], y);
    sample[i] = y;
    if (denoised) denoised[i] = d;
  }
}
int launch_lcm_update(float* sample, const float* eps, const float* noise, float* denoised, long long n, float kx, float ke,
                      float c_prev, float c_noise, hipStream_t s) {
  SHAPECHK(n > 0, "lcm_update: n=%lld", n);
  if (!sample || !eps) {
    pea_set_error("lcm_update: null pointer");
    return PEA_E_INVALID;
  }
  const bool vec = (((uintptr_t)sample | (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)denoised) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  hipLaunchKernelGGL(lcm_update_kernel, dim3(sm_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, s, sample, eps, noise, denoised, n,
                     n4, kx, ke, c_prev, c_noise);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// EulerDiscreteScheduler / EulerAncestralDiscreteScheduler step (diffusers 0.23 [ext]; epsilon prediction, so the derivative
// (x - x0) / sigma IS eps) fused with the NEXT step's scale_model_input and the CFG batch doubling:
//   x' = sample + k_e * eps (+ k_n * noise);  sample <- x';  model_in[d * n + i] <- x' * k_s  for d < dup
// eps NULL is the entry form (sample is only read: model_in = sample * k_s).  The vector part covers [0, 4 n4) with 16-byte
// accesses, the scalar part the rest (everything when n4 == 0); explicit fmaf so that both parts round alike.
__global__ void euler_update_kernel(float* __restrict__ sample, const float* __restrict__ eps, const float* __restrict__ noise,
                                    float* __restrict__ model_in, long long n, long long n4, int dup, float k_e, float k_n,
                                    float k_s) {
  SM_LOOP(i, n4) {
    f32x4 x = ((const f32x4*)sample)[i];
    if (eps) {
      const f32x4 e = ((const f32x4*)eps)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = fmaf(k_e, e[j], x[j]);
      if (noise) {
        const f32x4 z = ((const f32x4*)noise)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = fmaf(k_n, z[j], x[j]);
      }
      ((f32x4*)sample)[i] = x;
    }
    if (model_in) {
      f32x4 m;
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = x[j] * k_s;
      ((f32x4*)model_in)[i] = m;
      if (dup == 2) ((f32x4*)(model_in + n))[i] = m;
    }
  }
  SM_LOOP(t, n - 4 * n4) {
    const long long i = 4 * n4 + t;
    float x = sample[i];
    if (eps) {
      x = fmaf(k_e, eps[i], x);
      if (noise) x = fmaf(k_n, noise[i], x);
      sample[i] = x;
    }
    if (model_in) {
      const float m = x * k_s;
      model_in[i] = m;
      if (dup == 2) model_in[n + i] = m;
    }
  }
}
int launch_euler_update(float* sample, const float* eps, const float* noise, float* model_in, long long n, int dup, float k_e,
                        float k_n, float k_s, hipStream_t s) {
  SHAPECHK(n > 0 && (dup == 1 || dup == 2), "euler_update: n=%lld dup=%d (1 or 2)", n, dup);
  if (!sample) {
    pea_set_error("euler_update: null sample");
    return PEA_E_INVALID;
  }
  if (!eps && (noise || !model_in)) {
    pea_set_error("euler_update: without eps (the entry form) model_in is the only output and there is no noise term");
    return PEA_E_INVALID;
  }
  // the second copy of a doubled model input starts at model_in + n: one more pointer that has to be 16-byte aligned
  const uintptr_t second = (model_in && dup == 2) ? (uintptr_t)(model_in + n) : 0;
  const bool vec = (((uintptr_t)sample | (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)model_in | second) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  hipLaunchKernelGGL(euler_update_kernel, dim3(sm_grid(vec ? (n + 3) / 4 : n)), dim3(256), 0, s, sample, eps, noise, model_in, n,
                     n4, dup, k_e, k_n, k_s);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// Self-attention guidance (Hong et al. 2023), steps 2 and 3 of a denoising step in ONE launch: the mask from the column sums of a
// self-attention layer, the data prediction, its 9 x 9 Gaussian blur, the select, and the degraded model input.
//   A[b][k] = part[b][0][k] + part[b][1][k] + ...   (ascending g, plain fp32 adds),   m = A[b][iy[y] * mw + ix[x]] > 1.0f
//   x0 = c_x x + c_e eps;  x0_blur = reflect-padded separable blur of x0 (taps exp(-i^2 / 2) / sum, i = -4..4; rows, then columns)
//   out = o_b (m ? x0_blur : x0) + o_e eps
// A workgroup is one 32 x 32 tile of one (sample, channel): x0 over the tile and its 4-pixel halo goes into LDS (reflect indexing
// of the source pixel: F.pad(mode="reflect"), no edge repeat), the row pass writes 40 x 32 sums, the column pass reads nine of them.
// Contraction is off in here: where the mask is false the result is the written formula, each product and sum rounded once.
#define SAG_T 32
#define SAG_R 4
struct SagTaps { float w[SAG_R + 1]; };                  // w[|i|], symmetric
__device__ __forceinline__ int sag_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);               // (only pixels of a ragged tile that are never stored get here out of range)
}
__global__ __launch_bounds__(256) void sag_degrade_kernel(const float* __restrict__ lat, const float* __restrict__ eps,
                                                          const float* __restrict__ part, int G, int mhw, int mw,
                                                          const int* __restrict__ iy, const int* __restrict__ ix,
                                                          float* __restrict__ out, int C, int H, int W, int tiles_x, float c_x,
                                                          float c_e, float o_b, float o_e, SagTaps taps) {
#pragma clang fp contract(off)
  constexpr int E = SAG_T + 2 * SAG_R;
  __shared__ float x0s[E][E + 1];
  __shared__ float rows[E][SAG_T + 1];
  const int b = blockIdx.z, ch = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * SAG_T, tx0 = (blockIdx.x % tiles_x) * SAG_T;
  const long long plane = ((long long)b * C + ch) * H * W;
  for (int i = threadIdx.x; i < E * E; i += 256) {
    const int ly = i / E, lx = i - ly * E;
    const long long src = plane + (long long)sag_reflect(ty0 - SAG_R + ly, H) * W + sag_reflect(tx0 - SAG_R + lx, W);
    const float a = c_x * lat[src], e = c_e * eps[src];
    x0s[ly][lx] = a + e;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < E * SAG_T; i += 256) {
    const int ly = i / SAG_T, lx = i - ly * SAG_T;
    float s = taps.w[SAG_R] * x0s[ly][lx];
#pragma unroll
    for (int k = 1; k <= 2 * SAG_R; ++k) {
      const float v = taps.w[k < SAG_R ? SAG_R - k : k - SAG_R] * x0s[ly][lx + k];
      s = s + v;
    }
    rows[ly][lx] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SAG_T * SAG_T; i += 256) {
    const int ly = i / SAG_T, lx = i - ly * SAG_T;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    const int my = min(max(iy[y], 0), mhw / mw - 1), mx = min(max(ix[x], 0), mw - 1);   // (a table entry off the map reads its edge)
    const float* pk = part + (long long)b * G * mhw + my * mw + mx;
    float A = pk[0];
    for (int g = 1; g < G; ++g) A = A + pk[(long long)g * mhw];
    float v = x0s[ly + SAG_R][lx + SAG_R];
    if (A > 1.0f) {
      float s = taps.w[SAG_R] * rows[ly][lx];
#pragma unroll
      for (int k = 1; k <= 2 * SAG_R; ++k) {
        const float u = taps.w[k < SAG_R ? SAG_R - k : k - SAG_R] * rows[ly + k][lx];
        s = s + u;
      }
      v = s;
    }
    const long long o = plane + (long long)y * W + x;
    const float a = o_b * v, e = o_e * eps[o];
    out[o] = a + e;
  }
}
int launch_sag_degrade(const float* latents, const float* eps, const float* part, int G, int mh, int mw, const int* iy, const int* ix,
                       float* out, int B, int C, int H, int W, float c_x, float c_e, float o_b, float o_e, hipStream_t s) {
  SHAPECHK(latents && eps && part && iy && ix && out, "sag_degrade: null operand");
  SHAPECHK(G >= 1, "sag_degrade: G=%d partial column sums (at least 1)", G);
  SHAPECHK(B > 0 && B <= 65535 && C > 0 && C <= 65535 && mh > 0 && mw > 0, "sag_degrade: B=%d C=%d, a %d x %d map (B, C <= 65535)", B, C, mh, mw);
  SHAPECHK(H >= SAG_R + 1 && W >= SAG_R + 1, "sag_degrade: a %d x %d latent; reflect padding of %d needs at least %d x %d", H, W, SAG_R, SAG_R + 1, SAG_R + 1);
  SHAPECHK((long long)mh * mw < (1ll << 30) && (long long)H * W < (1ll << 30), "sag_degrade: map or latent too large");
  SagTaps taps;
  double w[SAG_R + 1], sum = 0.0;
  for (int i = 0; i <= SAG_R; ++i) { w[i] = exp(-0.5 * i * i); sum += (i ? 2.0 : 1.0) * w[i]; }
  for (int i = 0; i <= SAG_R; ++i) taps.w[i] = (float)(w[i] / sum);
  const int tx = cdiv(W, SAG_T), ty = cdiv(H, SAG_T);
  hipLaunchKernelGGL(sag_degrade_kernel, dim3(tx * ty, C, B), dim3(256), 0, s, latents, eps, part, G, mh * mw, mw, iy, ix, out, C, H, W,
                     tx, c_x, c_e, o_b, o_e, taps);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// Self-attention guidance, step 5.  cfg: eps = [uncond (B samples) | text (B samples)], out = u + g (t - u) + s (u - d), the first
// two terms as cfg_combine_kernel writes them (s = 0: its bits); otherwise eps holds B samples, out = e + s (e - d).
__global__ void cfg_sag_combine_kernel(const float* __restrict__ eps, const float* __restrict__ deg, float* __restrict__ out,
                                       long long n, int cfg, float g, float sg) {
  SM_LOOP(i, n) {
    const float u = eps[i];
    float base = u;
    if (cfg) {
      const float t = eps[n + i];
      base = u + g * (t - u);
    }
    out[i] = sg != 0.f ? base + sg * (u - deg[i]) : base;
  }
}
int launch_cfg_sag_combine(const float* eps, const float* eps_deg, float* out, int B, long long per, int cfg, float g, float sag,
                           hipStream_t s) {
  SHAPECHK(eps && eps_deg && out, "cfg_sag_combine: null operand");
  SHAPECHK(B > 0 && per > 0, "cfg_sag_combine: B=%d per=%lld", B, per);
  const long long n = (long long)B * per;
  hipLaunchKernelGGL(cfg_sag_combine_kernel, dim3(sm_grid(n)), dim3(256), 0, s, eps, eps_deg, out, n, cfg != 0, g, sag);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// MultiDiffusion panoramas (Bar-Tal et al. 2023): the canvas [N][C][Hc][Wc] is denoised through window-sized views with the
// fixed-shape UNet; these two kernels move a CHUNK -- the vb view slots of one UNet call -- between canvas and batch.  A slot is
// (n, y0, x0): image n, rows y0 .. y0 + h - 1, columns (x0 + j) mod Wc.  The slot table travels by value in the kernel arguments.
// Each kernel is instantiated for 4 consecutive columns per thread (16-byte accesses: w, Wc and every x0 multiples of 4, which also
// keeps a group of 4 on one side of the wrap seam, and 16-byte aligned pointers) and for 1; the arithmetic per element is the same.
#define VIEWS_MAX 16
struct ViewSlots { int n[VIEWS_MAX], y0[VIEWS_MAX], x0[VIEWS_MAX]; };
template <int V> struct ViewsVec { typedef float type; };
template <> struct ViewsVec<4> { typedef f32x4 type; };

// model_in[d][s][c][i][j] = canvas[n_s][c][y0_s + i][(x0_s + j) mod Wc] * k_s for d < dup; a slot past n_valid repeats the last valid one
template <int V>
__global__ __launch_bounds__(256) void views_gather_kernel(const float* __restrict__ canvas, float* __restrict__ model_in, ViewSlots sl,
                                                           int n_valid, int dup, int C, int h, int w, int Hc, int Wc, float k_s,
                                                           long long total, long long half) {
  typedef typename ViewsVec<V>::type vec;
  const int wv = w / V;
  SM_LOOP(idx, total) {                                  // idx = (((s * C + c) * h + i) * w + j) / V
    const int jq = (int)(idx % wv);
    long long r = idx / wv;
    const int i = (int)(r % h);
    r /= h;
    const int c = (int)(r % C), s = min((int)(r / C), n_valid - 1);
    int X = sl.x0[s] + jq * V;
    X = X >= Wc ? X - Wc : X;
    const long long src = (((long long)sl.n[s] * C + c) * Hc + sl.y0[s] + i) * Wc + X;
    vec m = *(const vec*)(canvas + src);
    m = m * k_s;
    *(vec*)(model_in + idx * V) = m;
    if (dup == 2) *(vec*)(model_in + half + idx * V) = m;
  }
}

static int views_check(const char* op, const void* a, const void* b, const int* slots, int n_valid, int vb, int dup, int N, int C,
                       int Hc, int Wc, int h, int w, int wrap_x, ViewSlots* sl, bool* x0_by4) {
  SHAPECHK(a && b && slots, "%s: null operand", op);
  SHAPECHK(vb >= 1 && vb <= VIEWS_MAX, "%s: vb=%d view slots (1..%d)", op, vb, VIEWS_MAX);
  SHAPECHK(n_valid >= 1 && n_valid <= vb, "%s: n_valid=%d of vb=%d slots (1..vb)", op, n_valid, vb);
  SHAPECHK(dup == 1 || dup == 2, "%s: dup=%d (1 or 2)", op, dup);
  SHAPECHK(N > 0 && C > 0 && h > 0 && w > 0, "%s: N=%d C=%d, a %d x %d window", op, N, C, h, w);
  SHAPECHK(h <= Hc && w <= Wc, "%s: a %d x %d window on a %d x %d canvas (the window is larger)", op, h, w, Hc, Wc);
  SHAPECHK((long long)vb * C * h * w < (1ll << 31) && (long long)Hc * Wc < (1ll << 31), "%s: chunk or canvas plane too large", op);
  *x0_by4 = true;
  for (int s = 0; s < n_valid; ++s) {
    const int n = slots[3 * s], y0 = slots[3 * s + 1], x0 = slots[3 * s + 2];
    SHAPECHK(n >= 0 && n < N, "%s: slot %d names image n=%d of %d", op, s, n, N);
    SHAPECHK(y0 >= 0 && y0 <= Hc - h, "%s: slot %d: rows %d .. %d outside the %d rows of the canvas (no wrap in y)", op, s, y0, y0 + h - 1, Hc);
    if (wrap_x) SHAPECHK(x0 >= 0 && x0 < Wc, "%s: slot %d: x0=%d outside 0 .. %d (wrap_x)", op, s, x0, Wc - 1);
    else SHAPECHK(x0 >= 0 && x0 <= Wc - w, "%s: slot %d: columns %d .. %d outside the %d columns of the canvas (no wrap_x)", op, s, x0, x0 + w - 1, Wc);
    sl->n[s] = n; sl->y0[s] = y0; sl->x0[s] = x0;
    *x0_by4 = *x0_by4 && x0 % 4 == 0;
  }
  for (int s = n_valid; s < VIEWS_MAX; ++s) { sl->n[s] = sl->n[n_valid - 1]; sl->y0[s] = sl->y0[n_valid - 1]; sl->x0[s] = sl->x0[n_valid - 1]; }
  return PEA_OK;
}

int launch_views_gather(const float* canvas, float* model_in, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc,
                        int Wc, int h, int w, int wrap_x, float k_s, hipStream_t s) {
  ViewSlots sl;
  bool by4;
  const int rc = views_check("views_gather", canvas, model_in, slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap_x, &sl, &by4);
  if (rc != PEA_OK) return rc;
  const long long half = (long long)vb * C * h * w;
  const bool vec = by4 && w % 4 == 0 && Wc % 4 == 0 && (((uintptr_t)canvas | (uintptr_t)model_in) & 15) == 0;
  if (vec) hipLaunchKernelGGL(views_gather_kernel<4>, dim3(sm_grid(half / 4)), dim3(256), 0, s, canvas, model_in, sl, n_valid, dup, C, h, w, Hc, Wc, k_s, half / 4, half);
  else hipLaunchKernelGGL(views_gather_kernel<1>, dim3(sm_grid(half)), dim3(256), 0, s, canvas, model_in, sl, n_valid, dup, C, h, w, Hc, Wc, k_s, half, half);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// The overlap merge, gather-style: a thread owns V consecutive canvas elements of one row and walks the valid slots in ascending
// order, so no two threads write one address and the sum has one order.  Per covering slot, at window position (i, j):
//   e = dup == 2 ? u + g (t - u) (cfg_guided<false>, the expression of cfg_combine) : eps;   e *= factor[s] when factor is given
//   acc = fmaf(wy[i] * wx[j], e, acc)
// acc starts at 0 (first) or at what the canvas holds; `last` divides by T[n][Y][X] in the same launch.  An element that no slot of the
// chunk covers is written only by `first` (0) or `last` (the division): in a middle chunk it keeps its partial sum untouched.
template <int V>
__global__ __launch_bounds__(256) void views_merge_kernel(const float* __restrict__ eps, float* __restrict__ canvas,
                                                          const float* __restrict__ factor, const float* __restrict__ wy,
                                                          const float* __restrict__ wx, const float* __restrict__ T, ViewSlots sl,
                                                          int n_valid, int dup, int C, int h, int w, int Hc, int Wc, float g, int first,
                                                          int last, long long total, long long half) {
  typedef typename ViewsVec<V>::type vec;
  const int wcv = Wc / V;
  SM_LOOP(idx, total) {                                  // idx = (((n * C + c) * Hc + Y) * Wc + X) / V
    const int X = (int)(idx % wcv) * V;
    long long r = idx / wcv;
    const int Y = (int)(r % Hc);
    r /= Hc;
    const int c = (int)(r % C), n = (int)(r / C);
    float acc[V];
    if (first) {
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = 0.f;
    } else {
      const vec a = *(const vec*)(canvas + idx * V);
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = ((const float*)&a)[k];
    }
    bool write = first || last;
    for (int s = 0; s < n_valid; ++s) {
      const int i = Y - sl.y0[s];
      int j = X - sl.x0[s];
      j = j < 0 ? j + Wc : j;                            // a wrapped view's columns behind the seam; without wrap x0 + w <= Wc and j stays >= w
      if (sl.n[s] != n || (unsigned)i >= (unsigned)h || (unsigned)j >= (unsigned)w) continue;
      const long long e = (((long long)s * C + c) * h + i) * w + j;
      const vec uv = *(const vec*)(eps + e);
      vec tv = uv;
      if (dup == 2) tv = *(const vec*)(eps + half + e);
      const float f = factor ? factor[s] : 1.f, wyi = wy[i];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float u = ((const float*)&uv)[k];
        float v = dup == 2 ? cfg_guided<false>(eps, half, e + k, u, ((const float*)&tv)[k], g, 0.f) : u;
        if (factor) v = v * f;
        acc[k] = fmaf(wyi * wx[j + k], v, acc[k]);
      }
      write = true;
    }
    if (!write) continue;
    vec o;
    if (last) {
      const vec t = *(const vec*)(T + ((long long)n * Hc + Y) * Wc + X);
#pragma unroll
      for (int k = 0; k < V; ++k) ((float*)&o)[k] = acc[k] / ((const float*)&t)[k];
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) ((float*)&o)[k] = acc[k];
    }
    *(vec*)(canvas + idx * V) = o;
  }
}

int launch_views_merge(const float* eps, float* canvas, const int* slots, int n_valid, int vb, int dup, int N, int C, int Hc, int Wc,
                       int h, int w, int wrap_x, float g, const float* factor, const float* wy, const float* wx, const float* total,
                       int first, int last, hipStream_t s) {
  ViewSlots sl;
  bool by4;
  const int rc = views_check("views_merge", eps, canvas, slots, n_valid, vb, dup, N, C, Hc, Wc, h, w, wrap_x, &sl, &by4);
  if (rc != PEA_OK) return rc;
  SHAPECHK(wy && wx && total, "views_merge: null operand (wy, wx and the weight total)");
  SHAPECHK(!(factor && dup == 1), "views_merge: per-slot rescale factors belong to the guided form (dup=2), not to dup=1");
  const long long half = (long long)vb * C * h * w, n = (long long)N * C * Hc * Wc;
  const bool vec = by4 && w % 4 == 0 && Wc % 4 == 0 && (((uintptr_t)eps | (uintptr_t)canvas | (uintptr_t)total) & 15) == 0;
  if (vec) hipLaunchKernelGGL(views_merge_kernel<4>, dim3(sm_grid(n / 4)), dim3(256), 0, s, eps, canvas, factor, wy, wx, total, sl, n_valid, dup, C, h, w, Hc, Wc, g, first != 0, last != 0, n / 4, half);
  else hipLaunchKernelGGL(views_merge_kernel<1>, dim3(sm_grid(n)), dim3(256), 0, s, eps, canvas, factor, wy, wx, total, sl, n_valid, dup, C, h, w, Hc, Wc, g, first != 0, last != 0, n, half);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// The per-view rescale_noise_cfg factors of a chunk laid out as [u | t] with B = vb: cfg_combine's reduction and factor kernels
// without its apply pass (the merge multiplies).  ws: cfg_combine_workspace_bytes(B); factor: fp32 [B].
int launch_cfg_rescale_factors(const float* eps2, int B, long long per, float g, float rescale, void* ws, float* factor, hipStream_t s) {
  SHAPECHK(eps2 && ws && factor, "cfg_rescale_factors: null operand");
  SHAPECHK(B > 0 && per > 1, "cfg_rescale_factors: B=%d per=%lld", B, per);
  double* part = (double*)ws;
  hipLaunchKernelGGL(cfg_stats_kernel<false>, dim3(CFG_NBLK, B), dim3(256), 0, s, eps2, (long long)B * per, per, g, 0.f, part);
  hipLaunchKernelGGL(cfg_factor_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, part, factor, B, per, rescale);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// Inpainting inputs (tests/test_sdxl_zh_inpaint.py: VaeImageProcessor.preprocess of image and mask, the masking of __call__ and
// the nearest-mode resize of prepare_mask_latents): per pixel of image [N][3][H][W] and mask [N][1][H][W], both in [0, 1],
//   init = 2 image - 1,  masked = init * (mask < 0.5),  latent_mask[n][0][y/8][x/8] = (mask >= 0.5) at y % 8 == x % 8 == 0.
// The multiply by the 0 / 1 keep factor is literal (a negative init gives -0, as in torch); every result is exact in fp32.
__global__ void inpaint_prepare_kernel(const float* __restrict__ image, const float* __restrict__ mask,
                                       float* __restrict__ init, float* __restrict__ masked, float* __restrict__ lmask,
                                       int H, int W, long long n) {
  const long long HW = (long long)H * W;
  SM_LOOP(i, n) {                                 // i = pixel of the mask, n = N * H * W
    const long long b = i / HW, p = i - b * HW;
    const float m = mask[i];
    const float keep = m >= 0.5f ? 0.f : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long j = (b * 3 + c) * HW + p;
      const float v = 2.f * image[j] - 1.f;
      init[j] = v;
      masked[j] = v * keep;
    }
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    if (((y | x) & 7) == 0) lmask[(b * (H / 8) + y / 8) * (W / 8) + x / 8] = 1.f - keep;
  }
}
int launch_inpaint_prepare(const float* image, const float* mask, int N, int H, int W, float* init, float* masked,
                           float* lmask, hipStream_t s) {
  SHAPECHK(N > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "inpaint_prepare: N=%d, image %dx%d must be multiples of 8", N,
           H, W);
  const long long n = (long long)N * H * W;
  hipLaunchKernelGGL(inpaint_prepare_kernel, dim3(sm_grid(n)), dim3(256), 0, s, image, mask, init, masked, lmask, H, W, n);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ControlNet residual hand-over: [B][C][HW] (fp32 or bf16) -> [B][HW][C] bf16, scaled
template <typename T>
__global__ void nchw_to_nhwc_scaled_kernel(const T* __restrict__ x, bf16* __restrict__ y, int C, long long HW,
                                           long long n, float scale) {
  SM_LOOP(i, n) {
    const int c = (int)(i % C);
    const long long r = i / C;
    const long long p = r % HW, b = r / HW;
    y[i] = (bf16)((float)x[(b * C + c) * HW + p] * scale);
  }
}
__global__ void scale_copy_bf16_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long long n, float scale) {
  SM_LOOP(i, n) y[i] = (bf16)((float)x[i] * scale);
}
int launch_residual_import(const void* src, int dtype, bf16* dst, int B, int C, long long HW, float scale,
                           hipStream_t s) {
  const long long n = (long long)B * C * HW;
  if (dtype == 0) hipLaunchKernelGGL(nchw_to_nhwc_scaled_kernel<float>, dim3(sm_grid(n)), dim3(256), 0, s, (const float*)src, dst, C, HW, n, scale);
  else if (dtype == 1) hipLaunchKernelGGL(nchw_to_nhwc_scaled_kernel<bf16>, dim3(sm_grid(n)), dim3(256), 0, s, (const bf16*)src, dst, C, HW, n, scale);
  else if (dtype == 2) hipLaunchKernelGGL(scale_copy_bf16_kernel, dim3(sm_grid(n)), dim3(256), 0, s, (const bf16*)src, dst, n, scale);
  else SHAPECHK(false, "residual import: dtype %d (0 fp32 NCHW, 1 bf16 NCHW, 2 bf16 NHWC)", dtype);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ---- VAE encoder tail (train_sdxl_zh.py:306-309): moments = quant_conv(h) (1x1, C2 = 2*latent channels <= 8);
// mean, logvar = chunk(moments); logvar clamped to [-30, 20]; latents = (mean + exp(0.5 logvar) * noise) * scaling
// (diffusers 0.23 DiagonalGaussianDistribution [ext]).  NCHW fp32; one thread per pixel.
__global__ void vae_posterior_kernel(const float* __restrict__ h, const float* __restrict__ wq,
                                     const float* __restrict__ bq, const float* __restrict__ noise,
                                     float* __restrict__ moments, float* __restrict__ latents, int B, int C2,
                                     long long HW, float scaling) {
  SM_LOOP(i, (long long)B * HW) {
    const long long b = i / HW, p = i - b * HW;
    float in[8], m[8];
    for (int c = 0; c < C2; ++c) in[c] = h[(b * C2 + c) * HW + p];
    for (int o = 0; o < C2; ++o) {
      float a = bq[o];
      for (int c = 0; c < C2; ++c) a += wq[o * C2 + c] * in[c];
      m[o] = a;
      if (moments) moments[(b * C2 + o) * HW + p] = a;
    }
    const int L = C2 / 2;
    if (latents)
      for (int c = 0; c < L; ++c) {
        const float lv = fminf(fmaxf(m[L + c], -30.f), 20.f);
        const float nz = noise ? noise[(b * L + c) * HW + p] : 0.f;
        latents[(b * L + c) * HW + p] = (m[c] + __expf(0.5f * lv) * nz) * scaling;
      }
  }
}
int launch_vae_posterior(const float* h, const float* wq, const float* bq, const float* noise, float* moments,
                         float* latents, int B, int C2, long long HW, float scaling, hipStream_t s) {
  SHAPECHK(C2 >= 2 && C2 <= 8 && C2 % 2 == 0, "vae posterior: %d moment channels", C2);
  hipLaunchKernelGGL(vae_posterior_kernel, dim3(sm_grid((long long)B * HW)), dim3(256), 0, s, h, wq, bq, noise, moments,
                     latents, B, C2, HW, scaling);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ---- row softmax of a materialised score matrix (VAE mid-block attention: ONE head of width 512 over H*W tokens,
// outside the flash kernel's head widths): s[r][:] = softmax(scale * s[r][:]) in place, bf16 storage, fp32 math.
// One workgroup per row; the row is read twice (max+sum pass with online rescale, then the write pass).
__global__ __launch_bounds__(256) void softmax_rows_kernel(bf16* __restrict__ s, int cols, int ld, float scale) {
  bf16* row = s + (long long)blockIdx.x * ld;
  const float k = scale * 1.4426950408889634f;
  float m = -INFINITY, l = 0.f;
  for (int c = threadIdx.x * 8; c < cols; c += 256 * 8) {
    const bf16x8 v = *(const bf16x8*)(row + c);
    float mx = m;
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, (float)v[j] * k);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += __builtin_amdgcn_exp2f((float)v[j] * k - mx);
    l = l * __builtin_amdgcn_exp2f(m - mx) + acc;
    m = mx;
  }
  __shared__ float sm[4], sl[4];
  const float wm = wave_max(m);
  l *= (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - wm);
  const float wl = wave_sum(l);
  if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = wm; sl[threadIdx.x >> 6] = wl; }
  __syncthreads();
  const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float Lsum = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) Lsum += sl[w] * __builtin_amdgcn_exp2f(sm[w] - M);
  const float inv = 1.0f / Lsum;
  for (int c = threadIdx.x * 8; c < cols; c += 256 * 8) {
    bf16x8 v = *(const bf16x8*)(row + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16)(__builtin_amdgcn_exp2f((float)v[j] * k - M) * inv);
    *(bf16x8*)(row + c) = v;
  }
}
int launch_softmax_rows(bf16* s, long long rows, int cols, int ld, float scale, hipStream_t st) {
  SHAPECHK(cols % 8 == 0 && ld % 8 == 0 && rows > 0, "softmax_rows: cols=%d ld=%d", cols, ld);
  PROF_BEGIN(6, 0.0, 6.0 * rows * (double)cols, st);
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, s, cols, ld, scale);
  PROF_END(st);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ---- VAE decode head: z' = post_quant_conv(latents * inv_scaling)  (1x1 conv over <= 8 channels), NCHW fp32
__global__ void vae_post_quant_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                      const float* __restrict__ b, float* __restrict__ out, int B, int C, long long HW,
                                      float inv_scaling) {
  SM_LOOP(i, (long long)B * HW) {
    const long long bb = i / HW, p = i - bb * HW;
    float in[8];
    for (int c = 0; c < C; ++c) in[c] = z[(bb * C + c) * HW + p] * inv_scaling;
    for (int o = 0; o < C; ++o) {
      float a = b[o];
      for (int c = 0; c < C; ++c) a += w[o * C + c] * in[c];
      out[(bb * C + o) * HW + p] = a;
    }
  }
}
int launch_vae_post_quant(const float* z, const float* w, const float* b, float* out, int B, int C, long long HW,
                          float inv_scaling, hipStream_t s) {
  SHAPECHK(C >= 1 && C <= 8, "vae post_quant: %d latent channels", C);
  hipLaunchKernelGGL(vae_post_quant_kernel, dim3(sm_grid((long long)B * HW)), dim3(256), 0, s, z, w, b, out, B, C, HW,
                     inv_scaling);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
