// Image side of the CLIP pairs (adapter evaluation): what sits between HipVAEDecoder's pixels and a CLIPScore.
//   preprocess_kernel   [0,1] map + clamp (+ 8-bit grid) -> antialiased bicubic resample (the definition of
//                       torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False): separable Keys
//                       kernel a = -0.5, support 2 max(scale, 1), per-output weights normalised) -> centre crop -> (x - mean) / std.
//                       The per-coordinate tap tables come from the host (float64, pea_diffusion_amd/vision.py) with the crop
//                       folded in; a workgroup stages the source window of its output tile in LDS, runs the horizontal pass
//                       into LDS and the vertical pass out (~19 taps per axis at 1024 -> 224: the separable form does 1/20 of
//                       the tap products of the direct one).
//   patchify_kernel     normalised pixels -> bf16 patch rows in the GEMM's A layout (K zero-padded to the K tile)
//   vision_embed_kernel class row + position add + pre_layrnorm in one pass over [B][Np + 1][width]
//   clip_score_kernel   w * max(cos(image, text), 0), one wave per pair, fixed-order fp32 reduction (bit-reproducible)
// and the C ABI of the vision tower (Tape::build_vision, graph.hip).  No atomics anywhere; explicit fmaf as in sampler.hip.
#include <stdio.h>
#include <string.h>

#include "../../include/pea_hip.h"
#include "model.h"

#define VS_LOOP(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)
static inline int vs_grid(long long n) { long long g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }
static inline bool aligned16(const void* p) { return ((unsigned long long)p & 15) == 0; }

// ============================================================================ resample + crop + normalise
#define PP_MAX_LDS (64 * 1024)
static size_t preprocess_lds_bytes(const PreprocessP& p) {
  return sizeof(float) * ((size_t)p.win_h * p.win_w + (size_t)p.win_h * p.tile_w + (size_t)p.tile_w * p.x.taps + (size_t)p.tile_h * p.y.taps);
}

__device__ __forceinline__ float pp_map(float v, float lo, float range, int quantize) {
  v = (v - lo) / range;                              // the reference's operations in its order: with `quantize` a value one ulp
  v = fminf(fmaxf(v, 0.f), 1.f);                     // off a rounding boundary would land on the neighbouring 8-bit level
  if (quantize) v = rintf(v * 255.f) / 255.f;        // (round half to even, as torch.round)
  return v;
}

// grid (tiles_x, tiles_y, B * 3), 256 threads.  LDS: src[win_h][win_w] | tmp[win_h][tile_w] | wx[tile_w][x.taps] | wy[tile_h][y.taps]
__global__ __launch_bounds__(256) void preprocess_kernel(PreprocessP p) {
  extern __shared__ __attribute__((aligned(16))) float pp_lds[];
  float* src = pp_lds;
  float* tmp = src + (size_t)p.win_h * p.win_w;
  float* wx = tmp + (size_t)p.win_h * p.tile_w;
  float* wy = wx + (size_t)p.tile_w * p.x.taps;
  const int tid = threadIdx.x;
  const int plane = blockIdx.z, ch = plane % 3;
  const int i0 = blockIdx.y * p.tile_h, j0 = blockIdx.x * p.tile_w;
  const int ni = min(p.tile_h, p.size - i0), nj = min(p.tile_w, p.size - j0);
  // source window of this tile: the hull of its rows' / columns' tap ranges, clamped to the image and to the LDS capacity the
  // host sized from the same tables (a capacity that is too small would give wrong pixels, never an access outside the buffers)
  int y0 = p.H, y1 = 0, x0 = p.W, x1 = 0;
  for (int i = 0; i < ni; ++i) {
    const int f = p.y.first[i0 + i], c = min(p.y.count[i0 + i], p.y.taps);
    y0 = min(y0, f); y1 = max(y1, f + c);
  }
  for (int j = 0; j < nj; ++j) {
    const int f = p.x.first[j0 + j], c = min(p.x.count[j0 + j], p.x.taps);
    x0 = min(x0, f); x1 = max(x1, f + c);
  }
  y0 = max(y0, 0); y1 = min(y1, p.H); x0 = max(x0, 0) & ~3; x1 = min(x1, p.W);
  const int wh = max(0, min(y1 - y0, p.win_h));
  const int ww = max(0, min((x1 - x0 + 3) & ~3, p.win_w));
  // ---- stage the tap weights and the (mapped, clamped, quantised) source window
  for (int t = tid; t < nj * p.x.taps; t += 256) wx[t] = p.x.w[(long long)j0 * p.x.taps + t];
  for (int t = tid; t < ni * p.y.taps; t += 256) wy[t] = p.y.w[(long long)i0 * p.y.taps + t];
  const float* ip = p.img + (long long)plane * p.H * p.W;
  const bool vec_in = (p.W & 3) == 0 && (((unsigned long long)p.img) & 15) == 0;
  const int wg = ww >> 2;
  for (int t = tid; t < wh * wg; t += 256) {
    const int r = t / wg, g = t - r * wg;
    const int gx = x0 + 4 * g;
    const float* rowp = ip + (long long)(y0 + r) * p.W;
    f32x4 v;
    if (vec_in && gx + 3 < p.W) v = *(const f32x4*)(rowp + gx);
    else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = gx + k < p.W ? rowp[gx + k] : p.lo;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = pp_map(v[k], p.lo, p.range, p.quantize);
    *(f32x4*)(src + (size_t)r * p.win_w + 4 * g) = v;
  }
  __syncthreads();
  // ---- horizontal pass: tmp[r][j] = sum_k wx[j][k] * src[r][first_x[j] - x0 + k]
  for (int t = tid; t < wh * nj; t += 256) {
    const int r = t / nj, j = t - r * nj;
    const int f = p.x.first[j0 + j] - x0, c = min(p.x.count[j0 + j], p.x.taps);
    const float* sr = src + (size_t)r * p.win_w;
    const float* wr = wx + j * p.x.taps;
    float acc = 0.f;
    for (int k = 0; k < c; ++k) {
      const int sx = f + k;
      if (sx >= 0 && sx < ww) acc = fmaf(wr[k], sr[sx], acc);
    }
    tmp[(size_t)r * p.tile_w + j] = acc;
  }
  __syncthreads();
  // ---- vertical pass, four output columns per thread; (x - mean) / std; 16-byte stores where the row allows them
  const int q = p.tile_w >> 2;
  const float mean = p.mean[ch], istd = p.istd[ch];
  const bool vec_out = (p.size & 3) == 0 && (((unsigned long long)p.out) & 15) == 0;
  for (int t = tid; t < ni * q; t += 256) {
    const int i = t / q, j4 = (t - i * q) * 4;
    if (j4 >= nj) continue;
    const int f = p.y.first[i0 + i] - y0, c = min(p.y.count[i0 + i], p.y.taps);
    const float* wr = wy + i * p.y.taps;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < c; ++k) {
      const int sy = f + k;
      if (sy < 0 || sy >= wh) continue;
      const f32x4 tv = *(const f32x4*)(tmp + (size_t)sy * p.tile_w + j4);
      const float w = wr[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, tv[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = (acc[e] - mean) * istd;
    float* op = p.out + ((long long)plane * p.size + (i0 + i)) * p.size + j0 + j4;
    if (vec_out && j4 + 3 < nj) *(f32x4*)op = acc;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j4 + e < nj) op[e] = acc[e];
    }
  }
}

int launch_preprocess(const PreprocessP& p, hipStream_t s) {
  SHAPECHK(p.B > 0 && p.H > 0 && p.W > 0 && p.size > 0, "preprocess: B=%d image %dx%d size=%d", p.B, p.H, p.W, p.size);
  SHAPECHK(p.img && p.out && p.y.first && p.y.count && p.y.w && p.x.first && p.x.count && p.x.w, "preprocess: null buffer");
  SHAPECHK(p.y.taps > 0 && p.x.taps > 0, "preprocess: empty tap table");
  SHAPECHK(p.tile_h > 0 && p.tile_w > 0 && p.tile_w % 4 == 0 && p.tile_h <= 64 && p.tile_w <= 64 && p.win_h > 0 && p.win_w > 0 && p.win_w % 4 == 0,
           "preprocess: tile %dx%d window %dx%d (tile_w and window width multiples of 4)", p.tile_h, p.tile_w, p.win_h, p.win_w);
  SHAPECHK(p.range != 0.f, "preprocess: empty value range");
  SHAPECHK((long long)p.B * 3 <= 65535, "preprocess: batch %d", p.B);
  const size_t lds = preprocess_lds_bytes(p);
  SHAPECHK(lds <= PP_MAX_LDS, "preprocess: a %dx%d tile with a %dx%d source window needs %zu bytes of LDS (limit %d)", p.tile_h, p.tile_w,
           p.win_h, p.win_w, lds, PP_MAX_LDS);
  const dim3 grid(cdiv(p.size, p.tile_w), cdiv(p.size, p.tile_h), p.B * 3);
  hipLaunchKernelGGL(preprocess_kernel, grid, dim3(256), lds, s, p);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ============================================================================ patchify
// one thread per 8 output columns (one 16-byte store); the fp32 sources are runs of P pixels, read as scalars
__global__ void patchify_kernel(const float* __restrict__ px, bf16* __restrict__ rows, long long nrows, int S, int P, int G, int K,
                                int kpad) {
  const int ck = kpad >> 3, PP = P * P;
  VS_LOOP(i, nrows * ck) {
    const long long r = i / ck;
    const int c8 = (int)(i - r * ck) * 8;
    const long long b = r / (G * G);
    const int pi = (int)(r - b * (G * G)), gy = pi / G, gx = pi - gy * G;
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int col = c8 + k;
      float v = 0.f;
      if (col < K) {
        const int c = col / PP, rem = col - c * PP, py = rem / P, pxx = rem - py * P;
        v = px[((b * 3 + c) * S + gy * P + py) * S + gx * P + pxx];
      }
      o[k] = (bf16)v;
    }
    *(bf16x8*)(rows + r * kpad + c8) = o;
  }
}
int launch_patchify(const float* pixels, bf16* rows, int B, int S, int P, int kpad, hipStream_t s) {
  SHAPECHK(pixels && rows, "patchify: null buffer");
  SHAPECHK(B > 0 && P > 0 && S >= P && S % P == 0, "patchify: B=%d image %d patch %d", B, S, P);
  const int G = S / P, K = 3 * P * P;
  SHAPECHK(kpad >= K && kpad % 8 == 0, "patchify: row width %d for %d patch values (>= and a multiple of 8)", kpad, K);
  const long long nrows = (long long)B * G * G;
  hipLaunchKernelGGL(patchify_kernel, dim3(vs_grid(nrows * (kpad / 8))), dim3(256), 0, s, pixels, rows, nrows, S, P, G, K, kpad);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ============================================================================ embedding assemble + pre-LayerNorm
// one wave per token row, the row held in registers (width <= 4096: 8 chunks of 64 lanes x 8 values); fp32 statistics
// (mean, then the centred second moment), bf16 storage
#define VE_CHUNKS 8
__global__ __launch_bounds__(256) void vision_embed_kernel(const bf16* __restrict__ pe, const float* __restrict__ cls,
                                                           const bf16* __restrict__ pos, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, bf16* __restrict__ y, long long rows,
                                                           int L, int width, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                        // wave-uniform
  const long long b = row / L;
  const int t = (int)(row - b * L);
  const bf16* pr = pos + (long long)t * width;
  const bf16* xr = t ? pe + (b * (L - 1) + (t - 1)) * width : nullptr;
  float v[VE_CHUNKS][8];
  float sum = 0.f;
#pragma unroll
  for (int it = 0; it < VE_CHUNKS; ++it) {
    const int c0 = it * 512 + lane * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[it][k] = 0.f;
    if (c0 < width) {
      const bf16x8 pv = *(const bf16x8*)(pr + c0);
      if (xr) {
        const bf16x8 xv = *(const bf16x8*)(xr + c0);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[it][k] = (float)xv[k] + (float)pv[k];
      } else {
        const f32x4 c_lo = *(const f32x4*)(cls + c0), c_hi = *(const f32x4*)(cls + c0 + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[it][k] = c_lo[k] + (float)pv[k]; v[it][4 + k] = c_hi[k] + (float)pv[4 + k]; }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) sum += v[it][k];
    }
  }
  const float mean = wave_sum(sum) / (float)width;
  float sq = 0.f;
#pragma unroll
  for (int it = 0; it < VE_CHUNKS; ++it) {
    if (it * 512 + lane * 8 < width) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { const float d = v[it][k] - mean; sq = fmaf(d, d, sq); }
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)width + eps);
  bf16* yr = y + row * width;
#pragma unroll
  for (int it = 0; it < VE_CHUNKS; ++it) {
    const int c0 = it * 512 + lane * 8;
    if (c0 < width) {
      const f32x4 g_lo = *(const f32x4*)(gamma + c0), g_hi = *(const f32x4*)(gamma + c0 + 4);
      const f32x4 b_lo = *(const f32x4*)(beta + c0), b_hi = *(const f32x4*)(beta + c0 + 4);
      bf16x8 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = (bf16)fmaf((v[it][k] - mean) * rstd, g_lo[k], b_lo[k]);
        o[4 + k] = (bf16)fmaf((v[it][4 + k] - mean) * rstd, g_hi[k], b_hi[k]);
      }
      *(bf16x8*)(yr + c0) = o;
    }
  }
}
int launch_vision_embed(const bf16* pe, const float* cls, const bf16* pos, const float* gamma, const float* beta, bf16* y, int B,
                        int L, int width, float eps, hipStream_t s) {
  SHAPECHK(B > 0 && L >= 2 && width > 0 && width % 8 == 0 && width <= 512 * VE_CHUNKS, "vision_embed: B=%d L=%d width=%d", B, L, width);
  SHAPECHK(aligned16(pe) && aligned16(cls) && aligned16(pos) && aligned16(gamma) && aligned16(beta) && aligned16(y),
           "vision_embed: 16-byte aligned buffers");
  const long long rows = (long long)B * L;
  hipLaunchKernelGGL(vision_embed_kernel, dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, s, pe, cls, pos, gamma, beta, y, rows, L,
                     width, eps);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

__global__ void pad_head_vec_kernel(const float* __restrict__ src, float* __restrict__ dst, int heads, int d, int dp) {
  VS_LOOP(i, (long long)heads * dp) {
    const int h = (int)(i / dp), j = (int)(i - (long long)h * dp);
    dst[i] = j < d ? src[h * d + j] : 0.f;
  }
}
int launch_pad_head_vec(const float* src, float* dst, int heads, int d, int dp, hipStream_t s) {
  SHAPECHK(heads > 0 && d > 0 && dp >= d, "pad_head_vec: heads=%d d=%d dp=%d", heads, d, dp);
  hipLaunchKernelGGL(pad_head_vec_kernel, dim3(vs_grid((long long)heads * dp)), dim3(256), 0, s, src, dst, heads, d, dp);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ============================================================================ CLIPScore
// One wave per (image, text) pair: each lane walks the row with stride 64 (16-byte pieces, then a scalar tail), the three sums
// meet in the butterfly of pea_common.h -- the same order every run.  Norms are floored at 1e-8 as in torch.cosine_similarity.
__global__ __launch_bounds__(64) void clip_score_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                        float* __restrict__ out, int D, int D4, float w, int clamp) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* a = img + (long long)b * D;
  const float* t = txt + (long long)b * D;
  float sd = 0.f, sa = 0.f, st = 0.f;
  for (int i = lane; i < D4; i += 64) {
    const f32x4 x = ((const f32x4*)a)[i], y = ((const f32x4*)t)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) { sd = fmaf(x[k], y[k], sd); sa = fmaf(x[k], x[k], sa); st = fmaf(y[k], y[k], st); }
  }
  for (int i = 4 * D4 + lane; i < D; i += 64) {
    const float x = a[i], y = t[i];
    sd = fmaf(x, y, sd); sa = fmaf(x, x, sa); st = fmaf(y, y, st);
  }
  sd = wave_sum(sd); sa = wave_sum(sa); st = wave_sum(st);
  if (lane == 0) {
    float c = sd / (fmaxf(sqrtf(sa), 1e-8f) * fmaxf(sqrtf(st), 1e-8f));
    if (clamp) c = fmaxf(c, 0.f);
    out[b] = w * c;
  }
}
int launch_clip_score(const float* img, const float* txt, float* out, int B, int D, float w, int clamp, hipStream_t s) {
  SHAPECHK(B > 0 && D > 0, "clip_score: B=%d D=%d", B, D);
  SHAPECHK(img && txt && out, "clip_score: null buffer");
  const int D4 = (D % 4 == 0 && aligned16(img) && aligned16(txt)) ? D / 4 : 0;     // every row 16-byte aligned
  hipLaunchKernelGGL(clip_score_kernel, dim3(B), dim3(64), 0, s, img, txt, out, D, D4, w, clamp);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ============================================================================ C ABI
static_assert(sizeof(pea_vision_config) == sizeof(PeaVisionCfg), "vision config struct mismatch");
static_assert(sizeof(pea_resampler_config) == sizeof(PeaResamplerCfg), "resampler config struct mismatch");
#define VNOTNULL(p, what)                        \
  do {                                           \
    if (!(p)) {                                  \
      pea_set_error("%s: null argument", what);  \
      return PEA_E_INVALID;                      \
    }                                            \
  } while (0)

static void vision_setup(Tape& u, const pea_vision_config* cfg, int B) {
  memset(&u.cfg, 0, sizeof(PeaUnetCfg));
  memcpy(&u.vcfg, cfg, sizeof(PeaVisionCfg));
  const int G = (cfg->patch_size > 0 && cfg->image_size > 0) ? cfg->image_size / cfg->patch_size : 0;
  u.graph = 5;
  u.B = B; u.H = G; u.W = G; u.L = G * G + 1; u.needs_grad = false; u.owns_weights = true;
}

extern "C" {

int pea_vision_create(const pea_vision_config* cfg, int B, void** out) {
  VNOTNULL(cfg, "pea_vision_create");
  VNOTNULL(out, "pea_vision_create");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    pea_set_error("pea_vision_create: no HIP device (there is no CPU fallback)");
    return PEA_E_HIP;
  }
  Tape* u = new Tape();
  vision_setup(*u, cfg, B);
  int rc = u->build();
  if (rc == PEA_OK) rc = u->alloc();
  if (rc != PEA_OK) {
    delete u;
    return rc;
  }
  *out = u;
  return PEA_OK;
}

int pea_vision_plan(const pea_vision_config* cfg, int B, long long* n_params, int* n_tokens, int* n_attn) {
  VNOTNULL(cfg, "pea_vision_plan");
  Tape u;
  vision_setup(u, cfg, B);
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  long long np = 0;
  for (const WSlot& s : u.slots) np += s.numel;
  if (n_params) *n_params = np;
  if (n_tokens) *n_tokens = u.L;
  if (n_attn) *n_attn = u.n_attn;
  return PEA_OK;
}

int pea_vision_forward(void* h, const float* pixels, int hidden_index, float* hidden_out, float* pooled_out, float* embeds_out,
                       void* stream) {
  VNOTNULL(h, "pea_vision_forward");
  VNOTNULL(pixels, "pea_vision_forward");
  Tape* u = (Tape*)h;
  if (u->graph != 5) { pea_set_error("pea_vision_forward: not a vision-tower handle"); return PEA_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  std::string miss;
  if (!u->all_loaded(&miss)) {
    pea_set_error("vision tower: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  const int nh = (int)u->hidden.size();
  int th = u->t_final;
  if (hidden_out && hidden_index != -1) {
    const int k = hidden_index < 0 ? nh + hidden_index : hidden_index;
    if (k < 0 || k >= nh) { pea_set_error("pea_vision_forward: hidden_index %d out of range (%d states)", hidden_index, nh); return PEA_E_INVALID; }
    th = u->hidden[k];
  }
  int rc = u->ensure_acts();
  if (rc != PEA_OK) return rc;
  const Tn& rows = u->tn[u->t_vrows];
  rc = launch_patchify(pixels, rows.d, u->B, u->vcfg.image_size, u->vcfg.patch_size, rows.cols, s);
  if (rc != PEA_OK) return rc;
  rc = u->exec_ops(0, u->ops.size(), false, s);
  if (rc != PEA_OK) return rc;
  const struct { float* dst; int t; } outs[3] = {{hidden_out, th}, {pooled_out, u->t_vpool}, {embeds_out, u->t_pooled}};
  for (const auto& o : outs) {
    if (!o.dst) continue;
    const Tn& t = u->tn[o.t];
    rc = launch_cast_bf16_f32(t.d, o.dst, t.rows * t.cols, s);
    if (rc != PEA_OK) return rc;
  }
  return PEA_OK;
}

// ---- Perceiver Resampler of the IP-Adapter "plus" files (Tape::build_resampler): the tower's hidden_states[-2] -> image tokens
static void resampler_setup(Tape& u, const pea_resampler_config* cfg, int B, int S) {
  memset(&u.cfg, 0, sizeof(PeaUnetCfg));
  memcpy(&u.rcfg, cfg, sizeof(PeaResamplerCfg));
  u.graph = 6;
  u.B = B; u.H = 1; u.W = S; u.L = S; u.needs_grad = false; u.owns_weights = true;
}

int pea_resampler_create(const pea_resampler_config* cfg, int B, int S, void** out) {
  VNOTNULL(cfg, "pea_resampler_create");
  VNOTNULL(out, "pea_resampler_create");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    pea_set_error("pea_resampler_create: no HIP device (there is no CPU fallback)");
    return PEA_E_HIP;
  }
  Tape* u = new Tape();
  resampler_setup(*u, cfg, B, S);
  int rc = u->build();
  if (rc == PEA_OK) rc = u->alloc();
  if (rc != PEA_OK) {
    delete u;
    return rc;
  }
  *out = u;
  return PEA_OK;
}

int pea_resampler_plan(const pea_resampler_config* cfg, int B, int S, long long* n_params, int* n_attn, int* n_prescaled) {
  VNOTNULL(cfg, "pea_resampler_plan");
  Tape u;
  resampler_setup(u, cfg, B, S);
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  long long np = 0;
  for (const WSlot& s : u.slots) np += s.numel;
  if (n_params) *n_params = np;
  if (n_attn) *n_attn = u.n_attn;
  if (n_prescaled) *n_prescaled = u.n_attn_pre;
  return PEA_OK;
}

/* weight i of the table a handle for this configuration would have, host only: what pea_unet_weight_info says about a handle */
int pea_resampler_plan_weight(const pea_resampler_config* cfg, int B, int S, int i, char* name, int name_len, long long* numel,
                              int* kind, int* d0, int* d1) {
  VNOTNULL(cfg, "pea_resampler_plan_weight");
  Tape u;
  resampler_setup(u, cfg, B, S);
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  if (i < 0 || i >= (int)u.slots.size()) {
    pea_set_error("pea_resampler_plan_weight: index %d of %d weights", i, (int)u.slots.size());
    return PEA_E_NOTFOUND;
  }
  const WSlot& w = u.slots[i];
  if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s", w.name.c_str());
  if (numel) *numel = w.numel;
  if (kind) *kind = w.kind;
  if (d0) *d0 = w.d0;
  if (d1) *d1 = w.d1;
  return PEA_OK;
}

int pea_resampler_forward(void* h, const float* hidden, float* tokens_out, void* stream) {
  VNOTNULL(h, "pea_resampler_forward");
  VNOTNULL(hidden, "pea_resampler_forward");
  VNOTNULL(tokens_out, "pea_resampler_forward");
  Tape* u = (Tape*)h;
  if (u->graph != 6) { pea_set_error("pea_resampler_forward: not a resampler handle"); return PEA_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  std::string miss;
  if (!u->all_loaded(&miss)) {
    pea_set_error("resampler: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  int rc = u->ensure_acts();
  if (rc != PEA_OK) return rc;
  // the two inputs of the tape: the tower's states in bf16, and the `latents` rows once per sample (source row stride 0)
  const Tn &in = u->tn[u->t_rs_in], &lat = u->tn[u->t_rs_lat];
  rc = launch_cast_f32_bf16(hidden, in.d, in.rows * in.cols, s);
  if (rc != PEA_OK) return rc;
  const int per = u->rcfg.n_queries * lat.cols;
  rc = launch_copy2d(u->slots[u->w_rs_lat].w, 0, lat.d, per, u->B, per, 0, s);
  if (rc != PEA_OK) return rc;
  rc = u->exec_ops(0, u->ops.size(), false, s);
  if (rc != PEA_OK) return rc;
  const Tn& t = u->tn[u->t_final];
  return launch_cast_bf16_f32(t.d, tokens_out, t.rows * t.cols, s);
}

int pea_op_preprocess(const float* images, int B, int H, int W, float lo, float hi, int quantize, const int* y_first,
                      const int* y_count, const float* y_weights, int y_taps, const int* x_first, const int* x_count,
                      const float* x_weights, int x_taps, int size, int tile_h, int tile_w, int win_h, int win_w, float mean0,
                      float mean1, float mean2, float std0, float std1, float std2, float* out, void* stream) {
  PreprocessP p;
  memset(&p, 0, sizeof(p));
  if (!(std0 > 0.f && std1 > 0.f && std2 > 0.f)) { pea_set_error("pea_op_preprocess: std must be positive"); return PEA_E_INVALID; }
  p.img = images; p.B = B; p.H = H; p.W = W; p.lo = lo; p.range = hi - lo; p.quantize = quantize;
  p.y.first = y_first; p.y.count = y_count; p.y.w = y_weights; p.y.taps = y_taps;
  p.x.first = x_first; p.x.count = x_count; p.x.w = x_weights; p.x.taps = x_taps;
  p.size = size; p.tile_h = tile_h; p.tile_w = tile_w; p.win_h = win_h; p.win_w = win_w;
  p.mean[0] = mean0; p.mean[1] = mean1; p.mean[2] = mean2;
  p.istd[0] = 1.0f / std0; p.istd[1] = 1.0f / std1; p.istd[2] = 1.0f / std2;
  p.out = out;
  return launch_preprocess(p, (hipStream_t)stream);
}

int pea_op_patchify(const float* pixels, void* rows, int B, int S, int P, int kpad, void* stream) {
  return launch_patchify(pixels, (bf16*)rows, B, S, P, kpad, (hipStream_t)stream);
}

int pea_op_clip_score(const float* image_embeds, const float* text_embeds, float* out, int B, int D, float w, int clamp,
                      void* stream) {
  return launch_clip_score(image_embeds, text_embeds, out, B, D, w, clamp, (hipStream_t)stream);
}

}  // extern "C"
