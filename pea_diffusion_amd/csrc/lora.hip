// LoRA weight composition (diffusers `pipe.load_lora_weights(...)` / `pipe.fuse_lora()`, tests/test_sdxl_zh_lcm.py:181-182):
//   out[m][k] = acc[m][k] + scale * sum_r up[m][r] * down[r][k]        all fp32, torch layouts
// m < M (output features / Cout), k < Kf (Cin, or Cin * 9 in the [Co][Ci][3][3] order: a conv LoRA `down [r][Ci][3][3]`,
// `up [Co][r][1][1]` is the same product), 1 <= rank <= 256.  It runs on the fp32 weight BEFORE the bf16 packers
// (Tape::load_weight_lora), so a fused weight is rounded once, like any loaded weight.
//
// The kernel moves 4 (2 M Kf + r (M + Kf)) bytes for 2 M Kf r FLOP: 16 FLOP per byte at rank 64, more than the fp32 VALU
// sustains beside the loads, so the product runs on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32 operands, a
// k-ordered fmaf chain per element, no atomics, no split over r -- two runs are bit-identical).  Orientation: the MFMA's row
// index is the k axis and its column index (the lane) is m, so a lane ends up with 4 consecutive k per register quad and the
// acc read / out write are 16-byte accesses on the k axis.
#include "pea_kernels.h"

#define LORA_TK 128                    // block tile on the k axis
#define LORA_TM 64                     // ... on the m axis
#define LORA_RC 32                     // ranks staged in LDS per pass
#define LORA_UP_PITCH (LORA_TM + 1)    // odd pitch: the transposing LDS writes of the `up` panel hit 32 different banks

// 4 waves: wave w computes k in [64 (w & 1), +64) x m in [32 (w >> 1), +32) of the block tile as two 32 x 32 MFMA tiles.
// VEC: Kf % 4 == 0 and 16-byte aligned acc / down / out (then a 4-wide group never straddles the end of a row).
// acc may alias out (every element is read and written by the same lane); down / up never do.
template <bool VEC>
__global__ __launch_bounds__(256) void lora_compose_kernel(const float* acc, const float* __restrict__ down,
                                                           const float* __restrict__ up, float* out, int M, int Kf,
                                                           int rank, float scale) {
  __shared__ __attribute__((aligned(16))) float down_s[LORA_RC][LORA_TK];
  __shared__ float up_s[LORA_RC][LORA_UP_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int k0 = blockIdx.x * LORA_TK, m0 = blockIdx.y * LORA_TM;
  const int kw = (wave & 1) * 64, mw = (wave >> 1) * 32;
  f32x16 c[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) c[t][v] = 0.f;

  for (int r0 = 0; r0 < rank; r0 += LORA_RC) {
    if (r0) __syncthreads();
    // down[r0 .. r0+32)[k0 .. k0+128) -> down_s, zeros past rank / Kf
#pragma unroll
    for (int i = 0; i < LORA_RC * LORA_TK / 4 / 256; ++i) {
      const int q = tid + i * 256;
      const int rr = q >> 5, kq = (q & 31) * 4;
      const int r = r0 + rr, k = k0 + kq;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rank) {
        const float* p = down + (size_t)r * Kf + k;
        if (VEC) {
          if (k < Kf) v = *(const f32x4*)p;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k + j < Kf) v[j] = p[j];
        }
      }
      *(f32x4*)&down_s[rr][kq] = v;
    }
    // up[m0 .. m0+64)[r0 .. r0+32) -> up_s[r][m] (transposed), zeros past M / rank
#pragma unroll
    for (int i = 0; i < LORA_RC * LORA_TM / 256; ++i) {
      const int rr = tid & 31, mm = (tid >> 5) + 8 * i;
      const int r = r0 + rr, m = m0 + mm;
      up_s[rr][mm] = (r < rank && m < M) ? up[(size_t)m * rank + r] : 0.f;
    }
    __syncthreads();
    // lane (l31, h) feeds A[row = k][kk = h] = down[r + h][k] and B[kk = h][col = m] = up[m][r + h]; a zero-filled rank adds
    // fma(0, 0, c) = c, so an odd rank needs no special step
    const int rn = rank - r0 < LORA_RC ? rank - r0 : LORA_RC;
    for (int rr = 0; rr < rn; rr += 2) {
      const float b = up_s[rr + h][mw + l31];
      const float a0 = down_s[rr + h][kw + l31], a1 = down_s[rr + h][kw + 32 + l31];
      c[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, c[0], 0, 0, 0);
      c[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, c[1], 0, 0, 0);
    }
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int m = m0 + mw + l31;
  if (m >= M) return;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = k0 + kw + t * 32 + 8 * g + 4 * h;
      const size_t o = (size_t)m * Kf + k;
      if (VEC) {
        if (k < Kf) {
          f32x4 a = *(const f32x4*)(acc + o);
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = fmaf(scale, c[t][4 * g + j], a[j]);
          *(f32x4*)(out + o) = a;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < Kf) out[o + j] = fmaf(scale, c[t][4 * g + j], acc[o + j]);
      }
    }
}

int launch_lora_compose(const float* acc, const float* down, const float* up, float* out, int M, int Kf, int rank,
                        float scale, hipStream_t s) {
  SHAPECHK(M > 0 && Kf > 0 && (long long)M <= 65535ll * LORA_TM, "lora_compose: M=%d Kf=%d", M, Kf);
  SHAPECHK(rank >= 1 && rank <= 256, "lora_compose: rank=%d (1..256)", rank);
  if (!acc || !down || !up || !out) {
    pea_set_error("lora_compose: null pointer");
    return PEA_E_INVALID;
  }
  const dim3 grid(cdiv(Kf, LORA_TK), cdiv(M, LORA_TM));
  const bool vec = Kf % 4 == 0 && (((uintptr_t)acc | (uintptr_t)down | (uintptr_t)out) & 15) == 0;
  PROF_BEGIN(6, 2.0 * M * (double)Kf * rank, 4.0 * (2.0 * M * (double)Kf + (double)rank * (M + Kf)), s);
  if (vec) hipLaunchKernelGGL(lora_compose_kernel<true>, grid, dim3(256), 0, s, acc, down, up, out, M, Kf, rank, scale);
  else hipLaunchKernelGGL(lora_compose_kernel<false>, grid, dim3(256), 0, s, acc, down, up, out, M, Kf, rank, scale);
  PROF_END(s);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
