// Semantic guidance (Brack et al. 2023, "SEGA: Instructing Text-to-Image Models using Semantic Guidance"): K edit concepts ride in
// the UNet batch behind [uncond | text]; eps = fp32 [(2 + K) B][C][hw] = [u | t | e_1 .. e_K].  Per concept c, sample b, channel ch
// (a GROUP of hw values)
//   d = s_c * (e_c - u)                    one subtraction, one multiplication: the select and the apply pass see the same bits
//   thr = quantile_q( |d| ) over the group, torch.quantile's linear interpolation between the order statistics v[k], v[k + 1]
//   m = |d| >= thr ? d : 0
// and then E_all = sum_c w_c m_c, E_warm = sum_c warm_c w_c m_c, used = E_all + mu mom,
//   out = u + g (t - u) + (any warm ? E_warm + mu mom : 0),  mom <- beta mom + (1 - beta) used.
// Two launches: an exact radix select per group (no sort, no global atomics, no scratch copy: the group lives in registers), and
// one elementwise pass over [B][C][hw].  Integer counting and fixed-order sums: the same bits every run.
#include "pea_kernels.h"

#define SEGA_MAX_K 8
#define SEGA_THREADS 1024
#define SEGA_NPT 16                                       // values per thread: 1024 x 16 = 16384 = the largest group
#define SEGA_MAX_HW (SEGA_THREADS * SEGA_NPT)

struct SegaConcepts {
  float scale[SEGA_MAX_K], weight[SEGA_MAX_K], frac[SEGA_MAX_K];   // s_c, w_c, the interpolation weight r - floor(r)
  int rank[SEGA_MAX_K], warm[SEGA_MAX_K];                          // k = floor(q (hw - 1)); warm_c
};

// Non-negative floats order as their bit patterns, so the k-th smallest |d| is found digit by digit on the 32-bit pattern, most
// significant byte first: a 256-bin histogram of the values that still match the prefix, a scan by the first wave, four rounds.
// UNet outputs are bf16-rounded, so one byte value often holds most of a wave: up to SEGA_LEADER_ROUNDS times the lanes that share
// the first active lane's digit are counted by a ballot and added by that lane alone, the rest add one by one.
#define SEGA_LEADER_ROUNDS 4
__global__ __launch_bounds__(SEGA_THREADS) void sega_select_kernel(const float* __restrict__ eps, float* __restrict__ thr,
                                                                   float* __restrict__ bounds, int B, int C, int hw, SegaConcepts P) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_digit, sh_rank, sh_below, sh_equal;
  __shared__ unsigned sh_min[SEGA_THREADS / 64];
  const int grp = blockIdx.x;                              // (c * B + b) * C + ch
  const int c = grp / (B * C), bch = grp - c * (B * C);
  const int tid = threadIdx.x, lane = tid & 63;
  if (P.weight[c] == 0.f) {                                // cooled down: nothing is ranked, nothing passes the cut
    if (tid == 0) {
      thr[grp] = __builtin_inff();
      if (bounds) { bounds[2 * grp] = __builtin_inff(); bounds[2 * grp + 1] = __builtin_inff(); }
    }
    return;
  }
  const float* u = eps + (long long)bch * hw;
  const float* e = eps + ((long long)(2 + c) * B * C + bch) * hw;
  const float s = P.scale[c];
  unsigned v[SEGA_NPT];
#pragma unroll
  for (int j = 0; j < SEGA_NPT; ++j) {
    const int i = j * SEGA_THREADS + tid;
    v[j] = 0xffffffffu;                                    // past the group: above every |d| pattern, never ranked
    if (i < hw) v[j] = __float_as_uint(s * (e[i] - u[i])) & 0x7fffffffu;
  }
  const int npt = (hw + SEGA_THREADS - 1) / SEGA_THREADS;
  if (tid == 0) { sh_rank = (unsigned)P.rank[c]; sh_below = 0; }
  unsigned prefix = 0, pmask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SEGA_NPT; ++j) {
      if (j < npt) {                                       // uniform
        bool act = j * SEGA_THREADS + tid < hw && (v[j] & pmask) == prefix;
        const unsigned digit = (v[j] >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < SEGA_LEADER_ROUNDS; ++r) {
          const unsigned long long am = __ballot(act);
          if (am == 0) break;                              // uniform
          const int leader = __ffsll((long long)am) - 1;
          const unsigned d0 = (unsigned)__shfl((int)digit, leader);   // (measured faster than v_readlane here: EXPERIMENTS f16)
          const bool same = act && digit == d0;
          const unsigned long long sm = __ballot(same);
          if (lane == leader) atomicAdd(&hist[d0], (unsigned)__popcll(sm));
          act = act && !same;
        }
        if (act) atomicAdd(&hist[digit], 1u);
      }
    }
    __syncthreads();
    if (tid < 64) {                                        // the digit whose bin holds rank sh_rank among the matching values
      const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const unsigned sum = h0 + h1 + h2 + h3;
      unsigned inc = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, o);
        if (lane >= o) inc += t;
      }
      const unsigned exc = inc - sum, k = sh_rank;
      if (k >= exc && k < inc) {                           // one lane
        unsigned below = exc, d = 4 * lane, eq = h0;
        if (k >= below + h0) { below += h0; d += 1; eq = h1;
          if (k >= below + h1) { below += h1; d += 1; eq = h2;
            if (k >= below + h2) { below += h2; d += 1; eq = h3; } } }
        sh_digit = d; sh_rank = k - below; sh_below += below; sh_equal = eq;
      }
    }
    __syncthreads();
    prefix |= sh_digit << shift;
    pmask |= 255u << shift;
  }
  // prefix = the pattern of v[k]; sh_below values lie under it and sh_equal on it.  v[k + 1] is v[k] again when more than k + 1 values
  // are <= v[k], else the smallest value above it.
  unsigned above = 0xffffffffu;
#pragma unroll
  for (int j = 0; j < SEGA_NPT; ++j)
    if (v[j] > prefix && j * SEGA_THREADS + tid < hw) above = min(above, v[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) above = min(above, (unsigned)__shfl_xor((int)above, o));
  if (lane == 0) sh_min[tid >> 6] = above;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < SEGA_THREADS / 64; ++w) above = min(above, sh_min[w]);
    const unsigned k = (unsigned)P.rank[c], le = sh_below + sh_equal;
    const unsigned hi = (k + 1 >= (unsigned)hw || le > k + 1 || above == 0xffffffffu) ? prefix : above;
    const float a = __uint_as_float(prefix), b = __uint_as_float(hi), w = P.frac[c];
    thr[grp] = w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w);          // torch's lerp
    if (bounds) { bounds[2 * grp] = a; bounds[2 * grp + 1] = b; }
  }
}

// The elementwise pass.  V elements per thread (V = 4: hw % 4 == 0, so a vector never straddles two groups).
template <int V> struct SegaVec { typedef float type; };
template <> struct SegaVec<4> { typedef f32x4 type; };
template <int V>
__global__ __launch_bounds__(256) void sega_apply_kernel(const float* __restrict__ eps, float* __restrict__ mom, float* __restrict__ out,
                                                         const float* __restrict__ thr, long long n, int hw, int K, float g, float mu,
                                                         float beta, int any_warm, SegaConcepts P) {
  typedef typename SegaVec<V>::type vec;
  const long long nv = n / V;
  const int groups = (int)(n / hw);                        // B * C
  for (long long iv = (long long)blockIdx.x * blockDim.x + threadIdx.x; iv < nv; iv += (long long)gridDim.x * blockDim.x) {
    const long long i = iv * V;
    const int grp = (int)(i / hw);
    const vec uv = *(const vec*)(eps + i), tv = *(const vec*)(eps + n + i), mv = *(const vec*)(mom + i);
    float all[V], warm[V];
#pragma unroll
    for (int x = 0; x < V; ++x) all[x] = warm[x] = 0.f;
    for (int c = 0; c < K; ++c) {
      const float w = P.weight[c];
      if (w == 0.f) continue;                              // cooled down: its samples are not read
      const float s = P.scale[c], cut = thr[c * groups + grp];
      const vec ev = *(const vec*)(eps + (long long)(2 + c) * n + i);
#pragma unroll
      for (int x = 0; x < V; ++x) {
        const float d = s * (((const float*)&ev)[x] - ((const float*)&uv)[x]);
        const float m = w * (fabsf(d) >= cut ? d : 0.f);
        all[x] += m;
        if (P.warm[c]) warm[x] += m;
      }
    }
    vec ov, nm;
#pragma unroll
    for (int x = 0; x < V; ++x) {
      const float u = ((const float*)&uv)[x], t = ((const float*)&tv)[x], m0 = ((const float*)&mv)[x];
      const float cfg = u + g * (t - u);                   // cfg_combine_kernel's expression: its bits when nothing is added
      const float carried = mu * m0;
      ((float*)&ov)[x] = any_warm ? cfg + (warm[x] + carried) : cfg;
      ((float*)&nm)[x] = beta * m0 + (1.f - beta) * (all[x] + carried);
    }
    *(vec*)(out + i) = ov;
    *(vec*)(mom + i) = nm;
  }
}

size_t sega_workspace_bytes(int B, int C, int K) {
  return B > 0 && C > 0 && K > 0 ? (size_t)K * B * C * sizeof(float) : 0;
}

// the checks both entries share, and the by-value concept table: rank and weight of torch.quantile, r = q (hw - 1) in fp32
static int sega_concepts(const char* op, int B, int C, int hw, int K, const float* edit_scale, const float* quantile,
                         const float* weight, const int* warm, SegaConcepts* P) {
  SHAPECHK(B >= 1 && C >= 1, "%s: B=%d C=%d (both >= 1)", op, B, C);
  SHAPECHK(hw >= 2 && hw <= SEGA_MAX_HW, "%s: groups of hw=%d positions (2 .. %d: a group lives in one workgroup's registers)", op, hw,
           SEGA_MAX_HW);
  SHAPECHK(K >= 1 && K <= SEGA_MAX_K, "%s: K=%d edit concepts (1 .. %d)", op, K, SEGA_MAX_K);
  SHAPECHK((long long)K * B * C < (1ll << 31), "%s: too many groups (K=%d B=%d C=%d)", op, K, B, C);
  SHAPECHK(edit_scale && quantile && weight, "%s: null operand (the per-concept host arrays)", op);
  *P = SegaConcepts();
  for (int c = 0; c < K; ++c) {
    SHAPECHK(quantile[c] >= 0.f && quantile[c] < 1.f, "%s: concept %d: quantile %g outside [0, 1)", op, c, (double)quantile[c]);
    SHAPECHK(weight[c] >= 0.f, "%s: concept %d: negative weight %g", op, c, (double)weight[c]);
    volatile float r = quantile[c] * (float)(hw - 1);      // one fp32 product, as torch rounds it
    int k = (int)floorf(r);
    k = k > hw - 1 ? hw - 1 : k;
    P->scale[c] = edit_scale[c]; P->weight[c] = weight[c];
    P->rank[c] = k; P->frac[c] = r - (float)k;
    P->warm[c] = warm ? (warm[c] != 0) : 0;
  }
  return PEA_OK;
}

int launch_abs_diff_quantile(const float* eps, float* thr, float* bounds, int B, int C, int hw, int K, const float* edit_scale,
                             const float* quantile, const float* weight, hipStream_t s) {
  SHAPECHK(eps && thr, "abs_diff_quantile: null operand");
  SegaConcepts P;
  const int rc = sega_concepts("abs_diff_quantile", B, C, hw, K, edit_scale, quantile, weight, nullptr, &P);
  if (rc != PEA_OK) return rc;
  hipLaunchKernelGGL(sega_select_kernel, dim3(K * B * C), dim3(SEGA_THREADS), 0, s, eps, thr, bounds, B, C, hw, P);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

int launch_cfg_sega_combine(const float* eps, float* momentum, float* out, int B, int C, int hw, int K, float g, const float* edit_scale,
                            const float* quantile, const float* weight, const int* warm, float mu, float beta, void* ws,
                            hipStream_t s) {
  SHAPECHK(eps && momentum && out && warm, "cfg_sega_combine: null operand");
  SegaConcepts P;
  const int rc = sega_concepts("cfg_sega_combine", B, C, hw, K, edit_scale, quantile, weight, warm, &P);
  if (rc != PEA_OK) return rc;
  SHAPECHK(beta >= 0.f && beta <= 1.f, "cfg_sega_combine: momentum_beta %g outside [0, 1]", (double)beta);
  SHAPECHK(ws != nullptr, "cfg_sega_combine: needs the workspace (pea_op_sega_workspace_bytes)");
  float* thr = (float*)ws;
  int any_warm = 0, any_live = 0;
  for (int c = 0; c < K; ++c) { any_warm |= P.warm[c]; any_live |= P.weight[c] != 0.f; }
  if (any_live) hipLaunchKernelGGL(sega_select_kernel, dim3(K * B * C), dim3(SEGA_THREADS), 0, s, eps, thr, (float*)nullptr, B, C, hw, P);
  const long long n = (long long)B * C * hw;
  const bool vec = hw % 4 == 0 && (((uintptr_t)eps | (uintptr_t)momentum | (uintptr_t)out) & 15) == 0;
  if (vec) {
    const long long blocks = (n / 4 + 255) / 256;
    hipLaunchKernelGGL(sega_apply_kernel<4>, dim3((int)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, eps, momentum, out, thr, n, hw, K, g,
                       mu, beta, any_warm, P);
  } else {
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(sega_apply_kernel<1>, dim3((int)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, eps, momentum, out, thr, n, hw, K, g,
                       mu, beta, any_warm, P);
  }
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
