// bf16 MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (MI355X).
//
// Replaces the cuBLAS/cuDNN calls that diffusers' UNet2DConditionModel triggers from
// train_sdxl_zh.py:397,415 (Linear layers, ResBlock conv3x3, up/down-sample convs) and
// the adapter Linears of train_sdxl_zh.py:48-55.
//
// Structure: BM x BN x 64 block tiles (128x160, 256x160, 128x128, 256x128, 64x160) of v_mfma_f32_16x16x32_bf16; both
// operands K-contiguous ("NT"), staged global->LDS with global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave
// instruction) by dedicated loader waves into an S-stage ring; the LDS image is linear, the XOR swizzle
// (chunk ^ ((row>>1)&7)) is applied to the SOURCE address and to the ds_read_b128 address, which makes the fragment
// reads of 128-byte rows bank-conflict free.  The MFMA is issued with weights as the A operand and activations as
// the B operand, so each lane ends with 4 consecutive output columns of one output row -> packed bf16 stores and
// vector bias/residual loads.  gemm_lc_kernel: one tile per workgroup; gemm_lcp_kernel: persistent, one workgroup
// per CU walking its tiles (XCD-aware order, 8 M-tiles grouped per N-tile so the tiles resident on one XCD share
// operand panels).  DESIGN.md section 4 has the measured variant table and what was tried and dropped.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "pea_kernels.h"

#define BK 64
// The fragment reads of the 64-row-wave-tile K-loops are interleaved with the MFMAs (mfma_half_interleaved: persistent kernel and
// K-split consumers; the one-tile-per-workgroup kernel keeps its burst -- profiles/EXPERIMENTS.md has both A/Bs):
constexpr int GEMM_ILV_M = 1;        // MFMAs between two interleaved ds_reads
constexpr int GEMM_ILV_HEAD = 4;     // MFMAs in front of the first interleaved ds_read

__device__ __forceinline__ int swz_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Timing probes of the persistent kernel (scripts/gemm_loop_probe.py; results are wrong while one is set) exist only in a
// build with -DPEA_GEMM_PROBES (make probes): merely carrying the runtime tests changes the register allocation of the
// 256x160 kernel from 164 registers without spills to 168 with 120 bytes of scratch in the tile transition.
#ifdef PEA_GEMM_PROBES
#define PEA_PROBE(bit) (p.debug & (bit))
#else
#define PEA_PROBE(bit) false
#endif

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- epilogue shared by both kernels.  acc[ni][mi][4g+j] = D[n = 8g + 4h + j][m = lane&31]
// Next-op weight prefetch (GemmP::pf_ptr): called by a DMA wave behind its last K-step -- nothing of the ring is waited for any
// more, so the loads' place in the in-order vmcnt queue cannot hold up a stage.  `slot` of `nslots` (DMA waves of the whole grid)
// takes the 8 KiB chunks slot, slot + nslots, ...: one global_load_dword per chunk, lane l touching line l (a line is fetched
// whole whatever part of it is asked for).  The loads are inline assembly (invisible to hipcc's waitcnt pass), so their
// destination must stay reserved until they have returned: ONE register, an in/out operand of every load and consumed behind
// the final wait -- as a fresh "=v" output per load the allocator reused it for the next iteration's address while the previous
// load was still in flight (a returning load then overwrote an address: memory access fault in the step).
__device__ __forceinline__ unsigned dma_prefetch_issue(const GemmP& p, int slot, int nslots, int lane) {
  unsigned sink = 0;
  if (!p.pf_ptr) return sink;
  const char* const base = (const char*)p.pf_ptr;
  const long long nchunk = (p.pf_bytes + 8191) >> 13;
  for (long long c = slot; c < nchunk; c += nslots) {
    const long long off = (c << 13) + lane * 128;
    if (off < p.pf_bytes) asm volatile("global_load_dword %0, %1, off" : "+v"(sink) : "v"(base + off) : "memory");
  }
  return sink;
}
__device__ __forceinline__ void dma_prefetch_wait(unsigned sink) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" ::"v"(sink));
}
__device__ __forceinline__ void dma_prefetch_next(const GemmP& p, int slot, int nslots, int lane) {
  dma_prefetch_wait(dma_prefetch_issue(p, slot, nslots, lane));
}

template <int MI, int NI>
__device__ __forceinline__ void gemm_epilogue(const GemmP& p, f32x16 (&acc)[NI][MI], int m_base, int n_base, int frow,
                                              int fh) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m_base + mi * 32 + frow;
    if (m >= p.M) continue;
    const int bidx = p.rowvec ? m / p.rows_per_batch : 0;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n_base + ni * 32 + 8 * g + 4 * fh;
        if (n >= p.N) continue;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[ni][mi][4 * g + j] * p.alpha;
        if (p.bias) {
          const f32x4 b = *(const f32x4*)(p.bias + n);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += b[j];
        }
        if (p.rowvec) {
          const bf16x4 rv = *(const bf16x4*)(p.rowvec + (long long)bidx * p.ldrv + n);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += (float)rv[j];
        }
        if (n < p.qscale_cols) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= p.qscale;
        }
        if (p.geglu_y) {            // v = (h_a, gate_a, h_b, gate_b) after bias
          bf16x2 y;
          if (p.stash_grad) {       // stash (gelu(gate), h * gelu'(gate)): what the backward multiplies d y by
            float ga, gb, da, db;
            gelu_val_grad(v[1], ga, da);
            gelu_val_grad(v[3], gb, db);
            y[0] = (bf16)(v[0] * ga);
            y[1] = (bf16)(v[2] * gb);
            v[1] = v[0] * da; v[0] = ga; v[3] = v[2] * db; v[2] = gb;
          } else {
            y[0] = (bf16)(v[0] * (p.geglu_tanh ? gelu_tanh(v[1]) : gelu_erf(v[1])));
            y[1] = (bf16)(v[2] * (p.geglu_tanh ? gelu_tanh(v[3]) : gelu_erf(v[3])));
          }
          *(bf16x2*)(p.geglu_y + (long long)m * p.ldy + (n >> 1)) = y;
          if (!p.C || (p.stash_rows > 0 && m >= p.stash_rows)) continue;
        }
        if (p.preact) {
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
          *(bf16x4*)(p.preact + (long long)m * p.ldpre + n) = o;
        }
        if (p.act == 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
        } else if (p.act == 2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = siluf_(v[j]);
        } else if (p.act == 3) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = v[j] * sigmoidf_(1.702f * v[j]);
        }
        if (p.res) {
          const bf16x4 rr = *(const bf16x4*)(p.res + (long long)m * p.ldres + n);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += (float)rr[j];
        }
        if (p.out_f32) {
          float* cp = (float*)p.C + (long long)m * p.ldc + n;
          f32x4 o;
          if (p.accum_f32) {
            o = *(const f32x4*)cp;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += v[j];
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = v[j];
          }
          *(f32x4*)cp = o;
        } else {
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
          *(bf16x4*)((bf16*)p.C + (long long)m * p.ldc + n) = o;
        }
      }
    }
  }
}

// ---- epilogue for the 16x16x32 accumulator layout: acc[nt][mt][j] = D[n = 4*(lane>>4) + j][m = lane&15]
template <int MT, int NT, int M0 = 0, int M1 = MT, bool PRELOAD_RES = false>
__device__ __forceinline__ void gemm_epilogue16(const GemmP& p, f32x4 (&acc)[NT][MT], int m_base, int n_base, int r16,
                                                int q4) {
  // PRELOAD_RES (one-tile-per-workgroup kernel, where the K-loop's fragment registers are dead by now): the residual
  // tile first -- all of its 8-byte quads are requested before any arithmetic, so the tile pays ONE global-load latency
  // instead of one per (mt, nt) group.  The persistent kernel keeps the next tile's fragments live and has no room.
  bf16x4 resq[PRELOAD_RES ? NT : 1][PRELOAD_RES ? MT : 1];
  if (PRELOAD_RES && p.res) {
#pragma unroll
    for (int mt = M0; mt < M1; ++mt) {
      const int m = min(m_base + mt * 16 + r16, p.M - 1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = min(n_base + nt * 16 + 4 * q4, p.N - 4);
        resq[nt][mt] = *(const bf16x4*)(p.res + (long long)m * p.ldres + n);
      }
    }
  }
  // everything of the epilogue except the final store of C; false: nothing to store (GEGLU without the stash)
  auto value = [&](int mt, int nt, int m, int bidx, float (&v)[4]) -> bool {
    const int n = n_base + nt * 16 + 4 * q4;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[nt][mt][j] * p.alpha;
    if (p.bias) {
      const f32x4 b = *(const f32x4*)(p.bias + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += b[j];
    }
    if (p.rowvec) {
      const bf16x4 rv = *(const bf16x4*)(p.rowvec + (long long)bidx * p.ldrv + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += (float)rv[j];
    }
    if (n < p.qscale_cols) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= p.qscale;
    }
    if (p.geglu_y) {            // v = (h_a, gate_a, h_b, gate_b) after bias
      bf16x2 y;
      if (p.stash_grad) {       // stash (gelu(gate), h * gelu'(gate)): what the backward multiplies d y by
        float ga, gb, da, db;
        gelu_val_grad(v[1], ga, da);
        gelu_val_grad(v[3], gb, db);
        y[0] = (bf16)(v[0] * ga);
        y[1] = (bf16)(v[2] * gb);
        v[1] = v[0] * da; v[0] = ga; v[3] = v[2] * db; v[2] = gb;
      } else {
        y[0] = (bf16)(v[0] * (p.geglu_tanh ? gelu_tanh(v[1]) : gelu_erf(v[1])));
        y[1] = (bf16)(v[2] * (p.geglu_tanh ? gelu_tanh(v[3]) : gelu_erf(v[3])));
      }
      *(bf16x2*)(p.geglu_y + (long long)m * p.ldy + (n >> 1)) = y;
      if (!p.C || (p.stash_rows > 0 && m >= p.stash_rows)) return false;
    }
    if (p.preact) {
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
      *(bf16x4*)(p.preact + (long long)m * p.ldpre + n) = o;
    }
    if (p.act == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
    } else if (p.act == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = siluf_(v[j]);
    } else if (p.act == 3) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] * sigmoidf_(1.702f * v[j]);
    }
    if (p.res) {
      bf16x4 rr;
      if constexpr (PRELOAD_RES) rr = resq[nt][mt];
      else rr = *(const bf16x4*)(p.res + (long long)m * p.ldres + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += (float)rr[j];
    }
    return true;
  };
  const bool pairs_ok = !p.out_f32 && !(p.geglu_y && !p.C) && (p.ldc % 8 == 0) && (((unsigned long long)p.C & 15) == 0);
#pragma unroll
  for (int mt = M0; mt < M1; ++mt) {
    const int m = m_base + mt * 16 + r16;
    if (m >= p.M) continue;      // depends on r16 only: the four q4 lanes of a row leave together (swap partners)
    const int bidx = p.rowvec ? m / p.rows_per_batch : 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      // Two adjacent n-tiles fully inside N: exchange 8-byte quads between the q4 lane rows (v_permlane16_swap) so
      // every lane stores 16 contiguous bytes and a row's 64 bytes of the pair leave in ONE instruction -- half
      // the cache lines touched per stored byte (the store tail of a tile is issue-bound, not bandwidth-bound).
      if ((nt & 1) == 0 && nt + 1 < NT && pairs_ok && n_base + (nt + 2) * 16 <= p.N) {
        float v0[4], v1[4];
        const bool st = value(mt, nt, m, bidx, v0);
        value(mt, nt + 1, m, bidx, v1);
        if (!st) continue;                    // GEGLU row without a stash (depends on the row only: partners agree)
        union { bf16x4 h; unsigned u[2]; } a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a.h[j] = (bf16)v0[j]; b.h[j] = (bf16)v1[j]; }
        const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
        // row q4 now holds: {lo[0], hi[0]} = quad of lane row (q4 & ~1) and {lo[1], hi[1]} = quad of lane row (q4 | 1),
        // both of n-tile nt + (q4 & 1)
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        const u32x4 o = {lo[0], hi[0], lo[1], hi[1]};
        const int n = n_base + (nt + (q4 & 1)) * 16 + 8 * (q4 >> 1);
        *(u32x4*)((bf16*)p.C + (long long)m * p.ldc + n) = o;
        continue;
      }
      if ((nt & 1) == 1 && pairs_ok && n_base + (nt + 1) * 16 <= p.N) continue;   // stored with its left neighbour
      const int n = n_base + nt * 16 + 4 * q4;
      if (n >= p.N) continue;
      float v[4];
      if (!value(mt, nt, m, bidx, v)) continue;
      if (p.out_f32) {
        float* cp = (float*)p.C + (long long)m * p.ldc + n;
        f32x4 o;
        if (p.accum_f32) {
          o = *(const f32x4*)cp;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] += v[j];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = v[j];
        }
        *(f32x4*)cp = o;
      } else {
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
        *(bf16x4*)((bf16*)p.C + (long long)m * p.ldc + n) = o;
      }
    }
  }
}

// Batched-load epilogue for the 16x16x32 accumulator layout (bf16 output; alpha, bias, per-sample row vector, residual,
// fused GEGLU with its pre-activation stash).  The generic epilogue above walks the tile quad by quad -- load bias, load
// residual, wait, convert, store -- and on this hardware vmcnt counts stores as well as loads, in issue order: every quad's
// wait also waits for the store of the quad before it, so a tile's 20 quads per lane pay 20 dependent round trips while
// both MFMA waves of the SIMD stand still (the tile transition measured 27-36 % of a K = 640..1280 launch,
// profiles/r01_gemm_epi_probe.log).  Here every load of the wave tile is issued first (bias + row vector: NT quads,
// residual: MT x NT quads), then the arithmetic runs and all stores leave back to back: one load latency per tile.
// Preconditions (launch_gemm sets p.epi_fast): !out_f32, act == 0, no preact, ldc % 8 == 0, C 16-byte aligned,
// N % 16 == 0, and for a row vector rows_per_batch % (rows of a wave tile) == 0 (one batch sample per wave tile).
// LNF (own kernel instantiations, so the common kernels keep their register allocation): the A operand is the
// UN-normalised input of a LayerNorm folded into this GEMM -- W holds W' = W . gamma, p.bias holds t, and
//   value = rstd[m] * (acc - mean[m] * s[n]) + t[n]        (p.ln_stats = [M][2] (mean, rstd), p.ln_s = s[N]);
// such GEMMs have no residual and no row vector (QKV, attn2.to_q, FF projection with GEGLU).
// EK: 0 = common form, 1 = LNF, 2 = the fused GEGLU backward (p.gbwd_pre; own instantiations for the same reason)
// (The stores were once hidden from hipcc's s_waitcnt bookkeeping as inline assembly, and once write-through: both A/Bs are in
// profiles/EXPERIMENTS.md.  What keeps the loads' waits out of the next tile's K-loop are the empty asm uses below.)
typedef __attribute__((ext_vector_type(4))) unsigned epi_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned epi_u32x2;
// "this loaded value has been consumed": an empty asm use.  Placed behind every predicated region of the epilogue for the loads
// whose real uses sit inside it, so that on the path that skips the region (all lanes of the wave past M: s_cbranch_execz) the
// load is still waited for -- otherwise hipcc carries it as pending into the next tile's K-loop (see above).  No instruction.
template <typename T>
__device__ __forceinline__ void epi_consumed(const T& v) { asm volatile("" :: "v"(v)); }
__device__ __forceinline__ void epi_store16(void* ptr, epi_u32x4 v) { *(epi_u32x4*)ptr = v; }
__device__ __forceinline__ void epi_store8(void* ptr, epi_u32x2 v) { *(epi_u32x2*)ptr = v; }
__device__ __forceinline__ void epi_store4(void* ptr, unsigned v) { *(unsigned*)ptr = v; }
template <int MT, int NT, int EK = 0>
__device__ __forceinline__ void gemm_epilogue16_fast(const GemmP& p, f32x4 (&acc)[NT][MT], int m_base, int n_base, int r16,
                                                     int q4) {
  constexpr bool LNF = EK == 1;
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  // ---- loads: bias (+ row vector) per n-tile
  f32x4 bq[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bq[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (p.bias) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bq[nt] = *(const f32x4*)(p.bias + min(n_base + nt * 16 + 4 * q4, p.N - 4));
  }
  bf16x4 rvq[NT];
  if (!LNF && p.rowvec) {
    const int bidx = min(m_base, p.M - 1) / p.rows_per_batch;          // uniform over the wave tile (precondition)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      rvq[nt] = *(const bf16x4*)(p.rowvec + (long long)bidx * p.ldrv + min(n_base + nt * 16 + 4 * q4, p.N - 4));
  }
  if (!LNF && p.rowvec) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[nt][j] += (float)rvq[nt][j];
  }
  const bool has_res = !LNF && p.res != nullptr;
  // per-n-tile factors (wave-uniform -> scalar registers): alpha, times qscale for the n-tiles left of qscale_cols; the bias
  // (+ row vector) quads take the same factor here, once per tile, so the per-value arithmetic stays ONE fma
  float al[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const float f = (n_base + nt * 16 < p.qscale_cols) ? p.qscale : 1.f;
    al[nt] = p.alpha * f;
    if (p.qscale_cols > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[nt][j] *= f;
    }
  }
  // folded LayerNorm: per row (c1, c2) = (rstd, -rstd * mean); v = c1 * acc + (c2 * s[n] + t[n])
  f32x4 sq[LNF ? NT : 1];
  float2 st[LNF ? MT : 1];
  if constexpr (LNF) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) sq[nt] = *(const f32x4*)(p.ln_s + min(n_base + nt * 16 + 4 * q4, p.N - 4));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) st[mt] = *(const float2*)(p.ln_stats + 2 * (long long)min(m_base + mt * 16 + r16, p.M - 1));
    __builtin_amdgcn_sched_barrier(0);
  }
  auto val = [&](int nt, int mt, int j) -> float {
    if constexpr (LNF) return (st[mt].y * (acc[nt][mt][j] - st[mt].x * sq[nt][j])) * al[nt] + bq[nt][j];
    else return acc[nt][mt][j] * al[nt] + bq[nt][j];
  };
  if (p.geglu_y) {
    // v = (h_a, gate_a, h_b, gate_b) after bias: y = h * gelu(gate) -> geglu_y[m][n / 2]; the pre-activation goes to C
    // for the rows that will be differentiated (stash_rows) -- none for a teacher / inference pass (C == null)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + mt * 16 + r16;
      if (m >= p.M) continue;                                          // r16 only: swap partners leave together
      const bool stash = p.C && !(p.stash_rows > 0 && m >= p.stash_rows);
      bf16* yrow = p.geglu_y + (long long)m * p.ldy;
      bf16* crow = (bf16*)p.C + (long long)m * p.ldc;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bool paired = (nt & 1) == 0 && nt + 1 < NT && n_base + (nt + 2) * 16 <= p.N;
        if ((nt & 1) == 1 && n_base + (nt + 1) * 16 <= p.N) continue;                 // done with its left neighbour
        if (n_base + nt * 16 >= p.N) continue;
        float v0[4], v1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v0[j] = val(nt, mt, j);
        union { bf16x2 h; unsigned u; } y0, y1;
        // y = h * gelu(gate); with stash_grad the stashed pair becomes (gelu(gate), h * gelu'(gate)) -- the two factors the
        // backward multiplies d y by (one erf for both; only for rows that are stashed)
        auto geglu2 = [&](float (&v)[4], bf16x2& y) {
          if (stash && p.stash_grad) {
            float ga, gb, da, db;
            gelu_val_grad(v[1], ga, da);
            gelu_val_grad(v[3], gb, db);
            y[0] = (bf16)(v[0] * ga);
            y[1] = (bf16)(v[2] * gb);
            v[1] = v[0] * da; v[0] = ga; v[3] = v[2] * db; v[2] = gb;
          } else {
            y[0] = (bf16)(v[0] * gelu_erf(v[1]));
            y[1] = (bf16)(v[2] * gelu_erf(v[3]));
          }
        };
        geglu2(v0, y0.h);
        if (paired) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v1[j] = val(nt + 1, mt, j);
          geglu2(v1, y1.h);
          // lane row q4 receives the words of lane rows (q4 & ~1) and (q4 | 1) of n-tile nt + (q4 & 1): 8 contiguous bytes
          const auto w = __builtin_amdgcn_permlane16_swap(y0.u, y1.u, false, false);
          const u32x2 o = {w[0], w[1]};
          epi_store8(yrow + ((n_base + (nt + (q4 & 1)) * 16) >> 1) + 4 * (q4 >> 1), o);
          if (stash) {
            union { bf16x4 h; unsigned u[2]; } a, b;
#pragma unroll
            for (int j = 0; j < 4; ++j) { a.h[j] = (bf16)v0[j]; b.h[j] = (bf16)v1[j]; }
            const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
            const u32x4 oc = {lo[0], hi[0], lo[1], hi[1]};
            epi_store16(crow + n_base + (nt + (q4 & 1)) * 16 + 8 * (q4 >> 1), oc);
          }
        } else {
          epi_store4(yrow + ((n_base + nt * 16 + 4 * q4) >> 1), y0.u);
          if (stash) {
            union { bf16x4 h; u32x2 u; } oc;
#pragma unroll
            for (int j = 0; j < 4; ++j) oc.h[j] = (bf16)v0[j];
            epi_store8(crow + n_base + nt * 16 + 4 * q4, oc.u);
          }
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) epi_consumed(bq[nt]);
    return;
  }
  if constexpr (EK == 2) {
    {
      // GEGLU backward in the epilogue of the FF output projection's dgrad: a lane's 4 columns n..n+3 of d y meet the 4 stashed
      // (h, gate) pairs at columns 2n..2n+7 (one 16-byte load) and leave as 4 (dh, dgate) pairs (one 16-byte store; the four
      // lanes of a row cover 64 contiguous bytes).  Pairs one 16-row block ahead, as the residual quads below.
      // (one buffer: two -- the next 16-row block's pairs in flight under this block's arithmetic -- cost the 256 x 160 persistent
      // instantiation 16 spilled registers, among them loop invariants it then reloaded from scratch in every K-step)
      bf16x8 pq[NT];
      auto load_pre = [&](int mt) {
        const long long mo = (long long)min(m_base + mt * 16 + r16, p.M - 1) * p.ldgp;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) pq[nt] = *(const bf16x8*)(p.gbwd_pre + mo + 2 * min(n_base + nt * 16 + 4 * q4, p.N - 4));
      };
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        load_pre(mt);
        __builtin_amdgcn_sched_barrier(0);
        const int m = m_base + mt * 16 + r16;
        bf16* crow = (bf16*)p.C + (long long)min(m, p.M - 1) * p.ldc;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int n = n_base + nt * 16 + 4 * q4;
          bf16x8 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float dh, dg;
            if (p.gbwd_form) {        // the stash holds (gelu(gate), h * gelu'(gate)): two multiplies
              const float d = val(nt, mt, j);
              dh = d * (float)pq[nt][2 * j];
              dg = d * (float)pq[nt][2 * j + 1];
            } else {
              geglu_pair_bwd((float)pq[nt][2 * j], (float)pq[nt][2 * j + 1], val(nt, mt, j), dh, dg);
            }
            o[2 * j] = (bf16)dh;
            o[2 * j + 1] = (bf16)dg;
          }
          if (m < p.M && n < p.N) *(bf16x8*)(crow + 2 * n) = o;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    }
  }
  // Residual one 16-row block ahead of the arithmetic (two register buffers): the loads of block mt + 1 are issued before
  // the stores of block mt, so the wait for them leaves those stores in flight; holding the whole tile's residual
  // (MT x NT x 8 bytes per lane) beside the accumulators would not fit the 168-register budget of three waves per SIMD.
  // res may alias C: a block's values are read before its own stores are issued and blocks do not overlap.
  // The residual is read in the STORE layout -- 16 bytes per lane at the lane's final columns, a row's four lanes covering
  // 64 contiguous bytes -- and added after the lane exchange, on fp32 values (one rounding, as before): as 8-byte quads in
  // the accumulator layout a 256 x 160 tile's residual took 20 load instructions per wave and 11.4 k cycles of a CU's load
  // path when every CU reads its tile at once, in the 16-byte form 12 instructions and 7.6 k (profiles/r03_mem_patterns.log).
  // nv = the wave tile's n-tiles inside N (a prefix; N % 16 == 0): pairs (0,1), (2,3), ... and, for odd nv, one single tile.
  const int nv = max(0, min(NT, (p.N - n_base) >> 4));                  // wave-uniform
  auto body = [&](auto has_res_t) {
    constexpr bool HR = decltype(has_res_t)::value;
    constexpr int NP = (NT + 1) / 2;
    // ALL residual pieces of the wave tile are requested before the first store (48 registers; the fragment registers are
    // free by now).  gfx950 counts loads and stores in one vmcnt and they complete out of order with respect to each other, so
    // a wait for a load while stores are pending is a wait for vmcnt(0): with the pieces one 16-row block ahead of the
    // arithmetic (round 2) every block's stores were waited out -- three store round trips in series per tile epilogue.
    bf16x8 rp[HR ? MT : 1][HR ? NP : 1];
    bf16x4 rs[HR ? MT : 1];
    if constexpr (HR) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const long long mo = (long long)min(m_base + mt * 16 + r16, p.M - 1) * p.ldres;
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr)
          if (2 * pr + 1 < nv) rp[mt][pr] = *(const bf16x8*)(p.res + mo + n_base + (2 * pr + (q4 & 1)) * 16 + 8 * (q4 >> 1));
        if (nv & 1) rs[mt] = *(const bf16x4*)(p.res + mo + n_base + (nv - 1) * 16 + 4 * q4);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + mt * 16 + r16;
      if (m < p.M) {                                                   // r16 only: swap partners agree
        bf16* crow = (bf16*)p.C + (long long)m * p.ldc;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt >= nv) continue;
          const bool paired = (nt & 1) == 0 && nt + 1 < nv;
          if ((nt & 1) == 1) continue;                                 // an odd tile inside N is stored with its left neighbour
          if (paired) {
            if constexpr (HR) {
              // exchange the fp32 values: element j of lane rows (q4 & ~1) and (q4 | 1) of n-tile nt + (q4 & 1) -> this lane's 8 columns
              // (inline assembly: with fp32 operands bit-cast in and out of __builtin_amdgcn_permlane16_swap, hipcc 7.2 folds the
              // second result onto the first -- scripts/ubench/swap_test.hip; the s_nops are the swap's VALU-write hazard)
              float lo[4], hi[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                lo[j] = val(nt, mt, j);
                hi[j] = val(nt + 1 < NT ? nt + 1 : nt, mt, j);
                asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo[j]), "+v"(hi[j]));
              }
              const bf16x8 r8 = rp[mt][nt >> 1];
              union { bf16x8 h; u32x4 u; } o;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                o.h[j] = (bf16)(lo[j] + (float)r8[j]);
                o.h[4 + j] = (bf16)(hi[j] + (float)r8[4 + j]);
              }
              epi_store16(crow + n_base + (nt + (q4 & 1)) * 16 + 8 * (q4 >> 1), o.u);
            } else {
              union { bf16x4 h; unsigned u[2]; } a, b;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                a.h[j] = (bf16)val(nt, mt, j);
                b.h[j] = (bf16)val(nt + 1 < NT ? nt + 1 : nt, mt, j);
              }
              const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
              const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
              const u32x4 o = {lo[0], hi[0], lo[1], hi[1]};
              epi_store16(crow + n_base + (nt + (q4 & 1)) * 16 + 8 * (q4 >> 1), o);
            }
          } else {                                                     // the single last tile of an odd nv
            union { bf16x4 h; u32x2 u; } o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float v = val(nt, mt, j);
              if constexpr (HR) v += (float)rs[mt][j];
              o.h[j] = (bf16)v;
            }
            epi_store8(crow + n_base + nt * 16 + 4 * q4, o.u);
          }
        }
      }
      if constexpr (HR) {
#pragma unroll
        for (int pr = 0; pr < NT / 2; ++pr) epi_consumed(rp[mt][pr]);
        epi_consumed(rs[mt]);
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) epi_consumed(bq[nt]);
  };
  if (has_res) body(std::true_type{});
  else body(std::false_type{});
}

// Folded-LayerNorm epilogue (LN(x) W^T = rstd (x W'^T - mean s) + t with W' = gamma * W, s = rowsum(W'), t = W beta + bias):
//   value = c1[m] * acc + (c2[m] * s[n] + t[n]),  c1 = rstd, c2 = -rstd * mean   (p.ln_stats = [M][2] (mean, rstd), p.ln_s = s, p.bias = t)
// N-tile PAIRS outermost, 16-row blocks inside: only one pair's (s, t) quads and the row constants are live beside the
// accumulators (the generic epilogue, 16-row blocks outermost, held s and t of the whole wave tile and spilled 27 registers in
// the 256 x 160 persistent kernel: 104 against 76 us on M8192 N3840 K1280).  Handles what the three folded Linears need: the
// column scale (Q prescale), GEGLU with the stash forms, plain bf16 output; no residual / row vector.
template <int MT, int NT>
__device__ __forceinline__ void gemm_epilogue16_lnf(const GemmP& p, f32x4 (&acc)[NT][MT], int m_base, int n_base, int r16, int q4) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  float c1[MT], c2[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const float2 st = *(const float2*)(p.ln_stats + 2 * (long long)min(m_base + mt * 16 + r16, p.M - 1));
    c1[mt] = st.y;
    c2[mt] = -st.y * st.x;
  }
  const int nv = max(0, min(NT, (p.N - n_base) >> 4));                  // n-tiles of the wave tile inside N (N % 16 == 0)
#pragma unroll
  for (int pr = 0; pr < (NT + 1) / 2; ++pr) {
    const int nt0 = 2 * pr, nt1 = 2 * pr + 1;
    if (nt0 >= nv) continue;
    const bool paired = nt1 < NT && nt1 < nv;
    const int na = min(n_base + nt0 * 16 + 4 * q4, p.N - 4), nb = min(n_base + (nt1 < NT ? nt1 : nt0) * 16 + 4 * q4, p.N - 4);
    f32x4 sa = *(const f32x4*)(p.ln_s + na), ta = *(const f32x4*)(p.bias + na);
    f32x4 sb = sa, tb = ta;
    if (paired) { sb = *(const f32x4*)(p.ln_s + nb); tb = *(const f32x4*)(p.bias + nb); }
    const float fa = (n_base + nt0 * 16 < p.qscale_cols) ? p.qscale : 1.f, fb = (n_base + nt1 * 16 < p.qscale_cols) ? p.qscale : 1.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + mt * 16 + r16;
      if (m >= p.M) continue;                                           // r16 only: swap partners agree
      float v0[4], v1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = fmaf(c1[mt], acc[nt0][mt][j], fmaf(c2[mt], sa[j], ta[j])) * fa;
        v1[j] = fmaf(c1[mt], acc[nt1 < NT ? nt1 : nt0][mt][j], fmaf(c2[mt], sb[j], tb[j])) * fb;
      }
      if (p.geglu_y) {
        const bool stash = p.C && !(p.stash_rows > 0 && m >= p.stash_rows);
        bf16* yrow = p.geglu_y + (long long)m * p.ldy;
        bf16* crow = (bf16*)p.C + (long long)m * p.ldc;
        union { bf16x2 h; unsigned u; } y0, y1;
        auto geglu2 = [&](float (&v)[4], bf16x2& y) {
          if (stash && p.stash_grad) {
            float ga, gb, da, db;
            gelu_val_grad(v[1], ga, da);
            gelu_val_grad(v[3], gb, db);
            y[0] = (bf16)(v[0] * ga);
            y[1] = (bf16)(v[2] * gb);
            v[1] = v[0] * da; v[0] = ga; v[3] = v[2] * db; v[2] = gb;
          } else {
            y[0] = (bf16)(v[0] * gelu_erf(v[1]));
            y[1] = (bf16)(v[2] * gelu_erf(v[3]));
          }
        };
        geglu2(v0, y0.h);
        if (paired) {
          geglu2(v1, y1.h);
          const auto w = __builtin_amdgcn_permlane16_swap(y0.u, y1.u, false, false);
          const u32x2 o = {w[0], w[1]};
          *(u32x2*)(yrow + ((n_base + (nt0 + (q4 & 1)) * 16) >> 1) + 4 * (q4 >> 1)) = o;
          if (stash) {
            union { bf16x4 h; unsigned u[2]; } a, b;
#pragma unroll
            for (int j = 0; j < 4; ++j) { a.h[j] = (bf16)v0[j]; b.h[j] = (bf16)v1[j]; }
            const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
            const u32x4 oc = {lo[0], hi[0], lo[1], hi[1]};
            *(u32x4*)(crow + n_base + (nt0 + (q4 & 1)) * 16 + 8 * (q4 >> 1)) = oc;
          }
        } else {
          *(bf16x2*)(yrow + ((n_base + nt0 * 16 + 4 * q4) >> 1)) = y0.h;
          if (stash) {
            bf16x4 oc;
#pragma unroll
            for (int j = 0; j < 4; ++j) oc[j] = (bf16)v0[j];
            *(bf16x4*)(crow + n_base + nt0 * 16 + 4 * q4) = oc;
          }
        }
        continue;
      }
      bf16* crow = (bf16*)p.C + (long long)m * p.ldc;
      if (paired) {
        union { bf16x4 h; unsigned u[2]; } a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a.h[j] = (bf16)v0[j]; b.h[j] = (bf16)v1[j]; }
        const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
        const u32x4 o = {lo[0], hi[0], lo[1], hi[1]};
        *(u32x4*)(crow + n_base + (nt0 + (q4 & 1)) * 16 + 8 * (q4 >> 1)) = o;
      } else {
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16)v0[j];
        *(bf16x4*)(crow + n_base + nt0 * 16 + 4 * q4) = o;
      }
    }
  }
}

// lean slice epilogue for the deferred form: alpha, optional bias, bf16 output (ldc % 8 == 0, C 16-byte aligned: the
// launcher's rule); few live values, so it can sit inside the K-loop
template <int MT, int NT, int M0, int M1>
__device__ __forceinline__ void gemm_epilogue16_lean(const GemmP& p, f32x4 (&acc)[NT][MT], int m_base, int n_base,
                                                     int r16, int q4) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  auto quad = [&](int mt, int nt) -> bf16x4 {
    const int n = min(n_base + nt * 16 + 4 * q4, p.N - 4);
    f32x4 b0 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) b0 = *(const f32x4*)(p.bias + n);
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (bf16)(acc[nt][mt][j] * p.alpha + b0[j]);
    return o;
  };
#pragma unroll
  for (int mt = M0; mt < M1; ++mt) {
    const int m = m_base + mt * 16 + r16;
    if (m >= p.M) continue;               // depends on r16 only: the four q4 lanes of a row leave together
    bf16* crow = (bf16*)p.C + (long long)m * p.ldc;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if ((nt & 1) == 0 && nt + 1 < NT && n_base + (nt + 2) * 16 <= p.N) {      // both n-tiles inside N: 16-byte stores
        union { bf16x4 h; unsigned u[2]; } a, b;
        a.h = quad(mt, nt);
        b.h = quad(mt, nt + 1);
        const auto lo = __builtin_amdgcn_permlane16_swap(a.u[0], b.u[0], false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(a.u[1], b.u[1], false, false);
        const u32x4 o = {lo[0], hi[0], lo[1], hi[1]};
        *(u32x4*)(crow + n_base + (nt + (q4 & 1)) * 16 + 8 * (q4 >> 1)) = o;
        continue;
      }
      if ((nt & 1) == 1 && n_base + (nt + 1) * 16 <= p.N) continue;              // stored with its left neighbour
      const int n = n_base + nt * 16 + 4 * q4;
      if (n >= p.N) continue;
      *(bf16x4*)(crow + n) = quad(mt, nt);
    }
  }
}

// Conv gather (mode 1): elements per source pixel, and tap -> (window offset, channel-block offset).
//   kside 0 / 3: 3 x 3 window, tap = ky * 3 + kx
//   kside 2:     2 x 2 window, tap = ky * 2 + kx      (one output parity of an upsample-folded conv in its sub-pixel form)
//   kside 4:     16 taps = 4 parity blocks x 2 x 2 over a depth-to-space source [B][Hs][Ws][4][Cin] (pix = 4 Cin): block pl = (py, px)
//                reads the window shifted by (-py, -px) at channel offset pl * Cin -- the data gradient of the sub-pixel form
__device__ __forceinline__ int conv_pix(const GemmP& p) { return p.pix ? p.pix : p.Cin; }
__device__ __forceinline__ void conv_tap(const GemmP& p, int tap, int& ky, int& kx, int& cblk) {
  cblk = 0;
  if (p.kside == 2) { ky = tap >> 1; kx = tap & 1; }
  else if (p.kside == 4) { const int pl = tap >> 2; ky = ((tap >> 1) & 1) - (pl >> 1); kx = (tap & 1) - (pl & 1); cblk = pl * p.Cin; }
  else { ky = tap / 3; kx = tap - ky * 3; }
}

#ifdef __HIP_DEVICE_COMPILE__                     // (the host pass has no buffer-resource type)
// Buffer resource of one row-tile's A operand.  The resource starts at the tile's first row (plain GEMM) or at the first
// sample the tile touches (conv gather), so the per-lane 32-bit offsets only span one tile / a couple of samples and the
// operand itself may be any size (the SDXL VAE decoder's [4][1024][1024][256] activations are 2^31 bytes).  num_records
// never exceeds 0x7f000000, the offset the conv gather uses for "halo: return zeros"; launch_gemm checks that a tile's
// own span stays below it.  org = the row / sample the offsets are relative to.
template <int MODE, int BM>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const GemmP& p, int bm, int& org) {
  long long first, left;
  if (MODE == 0) {
    org = __builtin_amdgcn_readfirstlane(bm * BM);
    first = (long long)org * p.lda;
    left = (long long)(p.M - org) * p.lda;
  } else {
    const int hw = p.Ho * p.Wo;
    const long long sample = (long long)p.Hs * p.Ws * conv_pix(p);
    org = __builtin_amdgcn_readfirstlane((bm * BM) / hw);
    first = org * sample;
    left = (p.M / hw - org) * sample;
  }
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + first), 0, (int)min(left * 2, 0x7f000000LL), 0x00020000);
}
#endif

// ---- one k32 half of a 64-row-wave-tile K-step: all MT x NT MFMAs, their issue order pinned so that the MT + NT ds_reads the
// caller has just requested (the other half's fragments) go out one per GEMM_ILV_M MFMAs behind the first GEMM_ILV_HEAD, instead
// of one burst behind the first n-tile: the 8 consumer waves of a CU run in lockstep between barriers, so a burst is 72 KB hitting
// the LDS at once while no wave issues an MFMA.  Whole step (round 4, alternating processes on one box): 104.38 / 103.99 ms ->
// 103.68 / 103.55 (M = 1, HEAD = 4), 104.04 / 103.65 (M = 2, HEAD = 2).  The caller brackets reads + this with sched_barrier(0).
template <int MT, int NT>
__device__ __forceinline__ void mfma_half_interleaved(f32x4 (&acc)[NT][MT], const bf16x8 (&wf)[NT], const bf16x8 (&af)[MT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], af[mt], acc[nt][mt], 0, 0, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, GEMM_ILV_HEAD, 0);
#pragma unroll
  for (int i = 0; i < MT + NT; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, GEMM_ILV_M, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, MT * NT, 0);
}
// ------------------------------------------------------------------------------------------------
// Loader / consumer kernel.  WM x WN consumer waves run ONLY ds_reads + MFMAs (register double-buffered
// fragments as above); LW extra loader waves run ONLY the LDS-DMA stream (address arithmetic + pieces), so
// the MFMA waves never spend issue slots on staging and each SIMD interleaves one wave of each kind.
// One s_barrier per K-step is shared by both roles:
//   loader  t: wait "tile t+1 landed" (counted vmcnt) -> barrier_t -> refill the slot of tile t with tile t+S
//   consumer t: sub-steps 0..2 of tile t, lgkmcnt(0) -> barrier_t -> prefetch (t+1, 0), sub-step 3 of tile t
// After barrier_t every consumer has issued and retired all reads of tile t's LDS slot, so the ring runs S
// tiles ahead (all S slots in flight).
// KSW: INTRA-WORKGROUP K SPLIT (one-round launches with a long K on the 128 x 160 tile).  The eight consumer waves of the plain
// form own 32 x 80 each and read 14 fragments per 20 MFMAs -- the fragment reads are the largest adder on top of the bare MFMA
// stream there (profiles/r05_gemm_loop_probe_oneround.log: 64 -> 80 us on K = 10240).  With KSW the wave grid is WM x WN x 2: wave
// (wr, wc, wk) owns a (BM / WM) x (BN / WN) = 64 x 80 tile like the 256 x 160 kernel's waves (9 reads per 20 MFMAs) but only the
// k32 half wk of every K-step; behind the loop the two halves of a tile swap half of their accumulators through the (free) ring
// and each wave finishes 32 x 80 -- the same epilogue, the same stores as the plain form.  fp32 sum of the two halves in the
// order (half 0) + (half 1) on both sides: deterministic.
template <int MODE, int BM, int BN, int WM, int WN, int LW, int S, bool PROBE16 = false, bool M16 = false, int MINW = 1,
          bool LNF = false, bool KSW = false>
__global__ __launch_bounds__((WM * WN * (KSW ? 2 : 1) + LW) * 64, MINW) void gemm_lc_kernel(const bf16* pl_A, const bf16* pl_W, int pl_lda, int pl_ldw, int pl_M,
                                                                           int pl_N, int pl_K, int pl_ksplit, int pl_debug, const GemmP p_in) {
  // Kernarg preload (-mllvm -amdgpu-kernarg-preload-count): the leading SCALAR parameters arrive in SGPRs with the wave, so the
  // DMA waves' way to their first LDS-DMA issue (tile index, buffer resources, per-lane offsets) does not start with a scalar-load
  // round trip to the 552-byte GemmP in the kernarg segment (a by-value struct is never preloaded); everything else is read from
  // the struct as before.  The local copy costs nothing: its fields are loaded where they are used.
  GemmP p = p_in;
  p.A = pl_A; p.W = pl_W; p.lda = pl_lda; p.ldw = pl_ldw; p.M = pl_M; p.N = pl_N; p.K = pl_K; p.ksplit = pl_ksplit; p.debug = pl_debug;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWC = WM * WN * (KSW ? 2 : 1);
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int A_BYTES = BM * 128;
  constexpr int PA = BM / 8 / LW, PB = BN / 8 / LW;
  constexpr int PP = PA + PB;
  constexpr int MI = BM / WM / 32, NI = BN / WN / 32;
  static_assert(BM % (8 * LW) == 0 && BN % (8 * LW) == 0, "tile / loader split");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int nwg = nbm * nbn;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  constexpr int GROUP = BM >= 256 ? 4 : 8;      // m-tiles sharing an n-tile column in the tile order: the tiles an XCD works on at a time
                                                // touch GROUP A panels and 32 / GROUP W panels; 4 balances 256-row A against 160-row W panels
  const int per_group = GROUP * nbn;
  const int gid = bid / per_group;
  const int first_m = gid * GROUP;
  const int gsize = min(nbm - first_m, GROUP);
  const int bm = first_m + (bid % per_group) % gsize;
  const int bn = (bid % per_group) / gsize;
  // split-K (p.ksplit > 1): blockIdx.y owns K-steps [kt0, kt0 + nt) and writes its fp32 partial tile to
  // C + blockIdx.y * split_stride; launch_splitk_reduce adds the partials in order
  int nt = p.K / BK, kt0 = 0;
  if (p.ksplit > 1) {
    const int per = (nt + p.ksplit - 1) / p.ksplit;
    kt0 = blockIdx.y * per;
    nt = min(per, nt - kt0);
    if (nt < 0) nt = 0;
  }
  const int kb0 = kt0 * BK;

  if (wave >= NWC) {
    // ============================== loader waves
    const int lw = wave - NWC;
    const int lrow = lane >> 3, cpos = lane & 7;
#ifdef __HIP_DEVICE_COMPILE__
    // buffer form of the LDS-DMA, as in gemm_lcp_kernel: no vector instruction per K-step in the DMA waves
    int org;
    const __amdgpu_buffer_rsrc_t rsrc_a = tile_rsrc<MODE, BM>(p, bm, org);
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, 0x7fffffff, 0x00020000);
    int a_off[PA], a_iy0[PA], a_ix0[PA], w_off[PB];
#pragma unroll
    for (int j = 0; j < PA; ++j) {
      const int r = (lw * PA + j) * 8 + lrow;
      const int chunk = cpos ^ ((r >> 1) & 7);
      int gm = bm * BM + r;
      gm = gm < p.M ? gm : p.M - 1;
      if (MODE == 0) {
        a_off[j] = ((gm - org) * p.lda + chunk * 8) * 2;
        a_iy0[j] = a_ix0[j] = 0;
      } else {
        const int hw = p.Ho * p.Wo;
        const int b = gm / hw;
        const int rem = gm - b * hw;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        a_iy0[j] = oy * p.stride - 1 + p.pad_off;
        a_ix0[j] = ox * p.stride - 1 + p.pad_off + p.pad_dx;
        a_off[j] = ((b - org) * p.Hs * p.Ws * conv_pix(p) + chunk * 8) * 2;
      }
    }
#pragma unroll
    for (int j = 0; j < PB; ++j) {
      const int r = (lw * PB + j) * 8 + lrow;
      const int chunk = cpos ^ ((r >> 1) & 7);
      int gn = bn * BN + r;
      gn = gn < p.N ? gn : p.N - 1;
      w_off[j] = (gn * p.ldw + chunk * 8) * 2;
    }
    const int Hv = p.Hs << p.shift, Wv = p.Ws << p.shift;
    int tap_off[PA];
    int tap_cur = -1;
    auto issue = [&](int st, int k0) {
      char* base = smem + st * STAGE;
      int c0 = 0;
      if (MODE == 1) {
        const int tap = k0 / p.Cin;
        c0 = k0 - tap * p.Cin;
        if (tap != tap_cur) {
          tap_cur = tap;
          int ky, kx, cblk;
          conv_tap(p, tap, ky, kx, cblk);
          const int pix = conv_pix(p);
#pragma unroll
          for (int j = 0; j < PA; ++j) {
            const int iy = a_iy0[j] + ky, ix = a_ix0[j] + kx;
            bool ok = ((unsigned)iy < (unsigned)Hv) && ((unsigned)ix < (unsigned)Wv);
            if (p.parity) ok = ok && (((iy | ix) & 1) == 0);
            const int sy = iy >> p.shift, sx = ix >> p.shift;
            tap_off[j] = ok ? a_off[j] + ((sy * p.Ws + sx) * pix + cblk) * 2 : 0x7f000000;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        if (MODE == 0)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, PEA_LDS(base + (lw * PA + j) * 1024), 16, a_off[j], k0 * 2, 0, 0);
        else
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, PEA_LDS(base + (lw * PA + j) * 1024), 16, tap_off[j], c0 * 2, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, PEA_LDS(base + A_BYTES + (lw * PB + j) * 1024), 16, w_off[j], k0 * 2, 0, 0);
    };
#else
    auto issue = [](int, int) {};
#endif
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (i < nt) issue(i, kb0 + i * BK);
    if (nt >= S) wait_vmcnt<(S - 1) * PP>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                              // prologue barrier: tile 0 landed
    int cur = 0;
    for (int t = 0; t + 1 < nt; ++t) {
      // tile t+1 must have landed; tiles t+2 .. t+S-1 may stay in flight (tile t+S is issued after the barrier)
      if (t + S - 1 < nt) wait_vmcnt<(S - 2) * PP>();
      else wait_vmcnt<0>();
      if (!(p.debug & 2)) __builtin_amdgcn_s_barrier();        // barrier_t
      if (t + S < nt && !(p.debug & 1)) issue(cur, kb0 + (t + S) * BK);
      cur = cur + 1 == S ? 0 : cur + 1;
    }
    const unsigned pf_sink = dma_prefetch_issue(p, (blockIdx.y * gridDim.x + blockIdx.x) * LW + lw, gridDim.x * gridDim.y * LW, lane);
    if constexpr (KSW) {                                       // the consumers' accumulator exchange: two workgroup barriers
      __builtin_amdgcn_s_barrier();                            // (the prefetch loads are in flight across them)
      __builtin_amdgcn_s_barrier();
    }
    dma_prefetch_wait(pf_sink);
    return;
  }

  // ================================ consumer waves
  if constexpr (KSW) {
    constexpr int MT = BM / WM / 16, NT = BN / WN / 16, MH = MT / 2;
    static_assert(MT % 2 == 0 && M16 && !LNF, "K-split consumers: even row-fragment count, 16x16x32 form");
    const int wk = wave / (WM * WN), w4 = wave % (WM * WN);
    const int wr = w4 / WN, wc = w4 % WN;
    const int r16 = lane & 15, q4 = lane >> 4;
    const int a_row0 = wr * (BM / WM) + r16, w_row0 = wc * (BN / WN) + r16;
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 af[2][MT], wf[2][NT];
    // this wave's k32 half of a stage: chunks 4 wk .. 4 wk + 3; rows 16 apart share the swizzle term, so TWO per-lane offsets
    // + compile-time multiples of 2048 address all nine fragments
    const int a_off = swz_off(a_row0, 4 * wk + q4), w_off = A_BYTES + swz_off(w_row0, 4 * wk + q4);
    auto load_frags = [&](int which, const char* tile) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[which][mt] = *(const bf16x8*)(tile + a_off + mt * 2048);
#pragma unroll
      for (int n_ = 0; n_ < NT; ++n_) wf[which][n_] = *(const bf16x8*)(tile + w_off + n_ * 2048);
    };
    __builtin_amdgcn_s_barrier();                              // prologue barrier
    load_frags(0, smem);
    int cur = 0;
    // one K-step: wait for its fragments, barrier_t (K-step t + 1 landed, slot t free), request K-step t + 1's fragments into the
    // OTHER register set interleaved with this step's MFMAs.  Two steps per loop iteration in straight-line code (nt is even:
    // launch_gemm only takes this form then) -- a register set picked by the parity of a loop counter made hipcc shuffle and
    // spill fragments inside the loop.  Behind the last K-step the read is a harmless one of a stale slot.
    auto kstep = [&](auto set_c, int t) {
      constexpr int P = decltype(set_c)::value;
      const int nxt = cur + 1 == S ? 0 : cur + 1;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (t + 1 < nt) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      load_frags(P ^ 1, smem + nxt * STAGE);
      mfma_half_interleaved<MT, NT>(acc, wf[P], af[P]);
      __builtin_amdgcn_sched_barrier(0);
      cur = nxt;
    };
    for (int t = 0; t < nt; t += 2) {
      kstep(std::integral_constant<int, 0>{}, t);
      kstep(std::integral_constant<int, 1>{}, t + 1);
    }
    // ---- accumulator exchange through the ring (every wave is past its last fragment read behind the first barrier).  The half
    // a wave hands over / keeps is a compile-time index on either side of a wave-uniform branch (a runtime index into the
    // accumulator array would go through scratch).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    char* const mine = smem + (size_t)wave * (MH * NT * 1024) + lane * 16;
    const char* const theirs = smem + (size_t)(wk == 0 ? wave + WM * WN : wave - WM * WN) * (MH * NT * 1024) + lane * 16;
    f32x4 fin[NT][MH];
    auto xchg = [&](auto give_c, auto keep_c) {
      constexpr int G0 = decltype(give_c)::value, K0 = decltype(keep_c)::value;
#pragma unroll
      for (int j = 0; j < MH; ++j)
#pragma unroll
        for (int n_ = 0; n_ < NT; ++n_) *(f32x4*)(mine + (j * NT + n_) * 1024) = acc[n_][G0 + j];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
#pragma unroll
      for (int j = 0; j < MH; ++j)
#pragma unroll
        for (int n_ = 0; n_ < NT; ++n_) {
          const f32x4 o = *(const f32x4*)(theirs + (j * NT + n_) * 1024);
          const f32x4 a = acc[n_][K0 + j];
          // (half 0) + (half 1) on both sides: the same bits whichever wave finishes these rows
          if constexpr (K0 == 0) fin[n_][j] = (f32x4){a[0] + o[0], a[1] + o[1], a[2] + o[2], a[3] + o[3]};
          else fin[n_][j] = (f32x4){o[0] + a[0], o[1] + a[1], o[2] + a[2], o[3] + a[3]};
        }
    };
    if (wk == 0) xchg(std::integral_constant<int, MH>{}, std::integral_constant<int, 0>{});
    else xchg(std::integral_constant<int, 0>{}, std::integral_constant<int, MH>{});
    const int keep0 = wk == 0 ? 0 : MH;
    gemm_epilogue16_fast<MH, NT>(p, fin, bm * BM + wr * (BM / WM) + keep0 * 16, bn * BN + wc * (BN / WN), r16, q4);
    return;
  }
  if constexpr (M16) {
    // 16x16x32 MFMAs (sustain a higher clock than 32x32x16 on this chip) with a (BM/WM) x (BN/WN) wave tile built
    // from 16-row fragments: e.g. 2 x 2 waves of 64 x 80 on the 128 x 160 tile -> 9 fragment reads per 20 MFMAs
    // instead of 12, the fragment ds_reads being the main in-loop loss of the 32x32 form.
    constexpr int MT = BM / WM / 16, NT = BN / WN / 16;
    const int wr = wave / WN, wc = wave % WN;
    const int r16 = lane & 15, q4 = lane >> 4;
    const int a_row0 = wr * (BM / WM) + r16, w_row0 = wc * (BN / WN) + r16;
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 af[2][MT], wf[2][NT];
    auto load_frags = [&](int which, const char* tile, int s2) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[which][mt] = *(const bf16x8*)(tile + swz_off(a_row0 + mt * 16, 4 * s2 + q4));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        wf[which][nt] = *(const bf16x8*)(tile + A_BYTES + swz_off(w_row0 + nt * 16, 4 * s2 + q4));
    };
    __builtin_amdgcn_s_barrier();                              // prologue barrier
    load_frags(0, smem, 0);
    int cur = 0;
    for (int t = 0; t < nt; ++t) {
      const char* tile = smem + cur * STAGE;
      const int nxt = cur + 1 == S ? 0 : cur + 1;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bool late_frags = false;
        if (s2 == 1) {
          if (t + 1 < nt) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                      // barrier_t
            late_frags = true;                                 // K-step t+1's first fragments: behind this half's first MFMAs (see gemm_lcp_kernel)
          }
        } else if (MT < 4) {
          load_frags(1, tile, 1);                              // (32-row wave tiles: hipcc's own placement measures better)
        }
#pragma unroll
        for (int nt_ = 0; nt_ < NT; ++nt_) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[nt_][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s2][nt_], af[s2][mt], acc[nt_][mt], 0, 0, 0);
          if (nt_ == 0 && (s2 == 1 || MT >= 4)) {             // the other half's fragments behind this half's first MFMAs
            __builtin_amdgcn_sched_barrier(0);
            if (s2 == 0) load_frags(1, tile, 1);
            else if (late_frags) load_frags(0, smem + nxt * STAGE, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      cur = nxt;
    }
    if constexpr (LNF) {
      gemm_epilogue16_lnf<MT, NT>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16, q4);
      return;
    }
    if (p.epi_fast) {
      gemm_epilogue16_fast<MT, NT>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16, q4);
      return;
    }
    GemmP q = p;
    if (p.ksplit > 1) q.C = (float*)p.C + (long long)blockIdx.y * p.split_stride;
    gemm_epilogue16<MT, NT, 0, MT, true>(q, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16, q4);
    return;
  }
  const int wr = wave / WN, wc = wave % WN;
  const int frow = lane & 31, fh = lane >> 5;
  const int a_row0 = wr * (BM / WM) + frow, w_row0 = wc * (BN / WN) + frow;
  f32x16 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  bf16x8 af[2][MI], wf[2][NI];
  auto load_frags = [&](int which, const char* tile, int s) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) af[which][mi] = *(const bf16x8*)(tile + swz_off(a_row0 + mi * 32, 2 * s + fh));
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
      wf[which][ni] = *(const bf16x8*)(tile + A_BYTES + swz_off(w_row0 + ni * 32, 2 * s + fh));
  };
  __builtin_amdgcn_s_barrier();                                // prologue barrier
  load_frags(0, smem, 0);
  int cur = 0;
  for (int t = 0; t < nt; ++t) {
    const char* tile = smem + cur * STAGE;
    const int nxt = cur + 1 == S ? 0 : cur + 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (s == 3) {
        if (t + 1 < nt) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (!(p.debug & 2)) __builtin_amdgcn_s_barrier();    // barrier_t
          if (!(p.debug & 4)) load_frags(0, smem + nxt * STAGE, 0);
        }
      } else {
        if (!(p.debug & 4)) load_frags((s + 1) & 1, tile, s + 1);
      }
      if constexpr (PROBE16) {    // timing probe: same FLOPs as 16x16x32 MFMAs (2 per 32x32x16), results meaningless
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            f32x4 q0 = {acc[ni][mi][0], acc[ni][mi][1], acc[ni][mi][2], acc[ni][mi][3]};
            f32x4 q1 = {acc[ni][mi][4], acc[ni][mi][5], acc[ni][mi][6], acc[ni][mi][7]};
            q0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s & 1][ni], af[s & 1][mi], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s & 1][ni], af[s & 1][mi], q1, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[ni][mi][j] = q0[j]; acc[ni][mi][4 + j] = q1[j]; }
          }
      } else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s & 1][ni], af[s & 1][mi], acc[ni][mi], 0, 0, 0);
      }
    }
    cur = nxt;
  }
  if (p.ksplit > 1) {
    GemmP q = p;
    q.C = (float*)p.C + (long long)blockIdx.y * p.split_stride;
    gemm_epilogue<MI, NI>(q, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), frow, fh);
    return;
  }
  gemm_epilogue<MI, NI>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), frow, fh);
}

template <int MODE, int BM, int BN, int WM, int WN, int LW, int S, bool PROBE16 = false, bool M16 = false, int MINW = 1,
          bool LNF = false, bool KSW = false>
static int launch_lc(const GemmP& p, hipStream_t stream) {
  constexpr int lds = S * (BM + BN) * 128;
  static_assert(lds <= 160 * 1024, "LDS budget");
  static_assert(!KSW || WM * WN * 2 * (BM / WM / 32) * (BN / WN / 16) * 1024 <= lds, "K-split exchange fits the ring");
  static bool attr_set = false;
  if (!attr_set) {
    HIPCHK(hipFuncSetAttribute((const void*)gemm_lc_kernel<MODE, BM, BN, WM, WN, LW, S, PROBE16, M16, MINW, LNF, KSW>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_set = true;
  }
  SHAPECHK(!KSW || (p.epi_fast && p.ksplit <= 1), "gemm: the K-split form needs the batched-load epilogue");
  const int grid = cdiv(p.M, BM) * cdiv(p.N, BN);
  hipLaunchKernelGGL((gemm_lc_kernel<MODE, BM, BN, WM, WN, LW, S, PROBE16, M16, MINW, LNF, KSW>),
                     dim3(grid, p.ksplit > 1 ? p.ksplit : 1), dim3((WM * WN * (KSW ? 2 : 1) + LW) * 64), lds, stream, p.A, p.W, p.lda, p.ldw,
                     p.M, p.N, p.K, p.ksplit, p.debug, p);
  return PEA_OK;
}

// ------------------------------------------------------------------------------------------------
// PERSISTENT loader / consumer kernel (16x16x32 MFMAs).  One block per CU walks its share of the output tiles;
// the K-steps of consecutive tiles form ONE stream through the LDS ring, so while the consumer waves run the
// epilogue of tile i the DMA waves already have the first S K-steps of tile i+1 in flight / landed -- the per-tile
// prologue (address setup + HBM/L2 latency of the first stages) and the block relaunch disappear for every tile
// but the first.  With K = 640 .. 1280 that fixed cost was 35-55 % of a tile (scripts/gemm_ksweep.py).
// Tile order: XCD x owns a contiguous range of (grouped) tile ids, its CUs take them round-robin, so the CUs
// of an XCD work on neighbouring tiles at any time (shared A rows / W columns in that XCD's L2).
// SW > 0: STAGED EPILOGUE.  The MFMA waves only convert a finished tile to bf16 (alpha / bias / row vector /
// activation / GEGLU applied) and drop it into an LDS staging image; SW extra "store waves" move it to HBM in
// 16-byte row-contiguous pieces, a slice after every K-step barrier of the NEXT tile.  Without this every CU
// bursts its tile at the same moment and the MFMA waves sit in the store-issue queue: 27-36 % of a K = 640..1280
// launch (scripts/gemm_epi_probe.py).  Only for bf16 outputs without residual / pre-activation stash.
// DF = 1: DEFERRED EPILOGUE.  A finished tile's accumulators are parked in a second register set and written out
// in 16-row slices at the head of the next tile's K-steps; the two MFMA waves that share a SIMD take turns (even /
// odd K-steps), so while one converts and stores a slice the other keeps the matrix pipe busy -- the tile
// transition, 27-36 % of a K = 640..1280 launch when every wave stops for its epilogue at once
// (scripts/gemm_epi_probe.py), disappears behind the main loop.
// FASTONLY: only the batched-load epilogue is compiled in (the 256-row tiles: with both epilogues in one kernel the
// register allocator spills around the tile transition); launch_gemm sends other epilogues to a 128-row variant.
// OCC = 2: TWO workgroups per CU (each with its own ring in at most half of the LDS, registers capped for three waves
// per SIMD): the two run out of phase, so one's tile transition / DMA wait is the other's main loop.
template <int MODE, int BM, int BN, int WM, int WN, int LW, int S, int SW = 0, int DF = 0, int EPI = 0, int OCC = 1>
__global__ __launch_bounds__((WM * WN + LW + SW) * 64, (OCC == 2 ? 3 : 1)) void gemm_lcp_kernel(const GemmP p) {
  // (no preloaded leading scalars here: measured no gain on the multi-tile launches, and the 256 x 160 instantiation's epilogue
  // spills 16 instead of 8 registers with them)
  constexpr bool FASTONLY = EPI != 0;     // EPI 1: batched-load epilogue only; 2: the same with the folded LayerNorm; 3: with the fused GEGLU backward
  constexpr int PITCH = BN * 2 + 16;                            // staging row pitch: conflict-free 8-byte writes
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NWC = WM * WN;
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int A_BYTES = BM * 128;
  constexpr int PA = BM / 8 / LW, PB = BN / 8 / LW;
  constexpr int PP = PA + PB;
  static_assert(BM % (8 * LW) == 0 && BN % (8 * LW) == 0, "tile / loader split");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int nwg = nbm * nbn;
  const int nblk = gridDim.x;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int nbx = (nblk - xcd + 7) >> 3;                        // blocks living on this XCD
  const int tq = nwg >> 3, tr = nwg & 7;
  const int cnt_x = tq + (xcd < tr ? 1 : 0);                    // tiles owned by this XCD
  const int start_x = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
  const int my_n = idx < cnt_x ? (cnt_x - idx + nbx - 1) / nbx : 0;
  const int nt = p.K / BK;
  const int G = my_n * nt;                                      // K-steps of this block, all tiles
  if (G == 0) return;
  constexpr int GROUP = BM >= 256 ? 4 : 8;      // m-tiles sharing an n-tile column in the tile order: the tiles an XCD works on at a time
                                                // touch GROUP A panels and 32 / GROUP W panels; 4 balances 256-row A against 160-row W panels
  const int per_group = GROUP * nbn;
  auto tile_of = [&](int i, int& bm, int& bn) {
    const int bid = start_x + idx + i * nbx;
    const int gid = bid / per_group;
    const int first_m = gid * GROUP;
    const int gsize = min(nbm - first_m, GROUP);
    const int rem = bid - gid * per_group;
    bm = first_m + rem % gsize;
    bn = rem / gsize;
  };

  char* const stg = smem + S * STAGE;                          // [BM][PITCH] bf16 staging image (SW > 0)
  if (SW > 0 && wave >= NWC + LW) {
    // ============================== store waves
    const int sw = wave - NWC - LW;
    const bool gg = p.geglu_y != nullptr;
    const int cpr = (gg ? BN / 2 : BN) / 8;                     // 16-byte chunks per staged row
    const int NP = (BM * cpr + SW * 64 - 1) / (SW * 64);        // passes of SW*64 chunks per tile
    bf16* const dst = gg ? p.geglu_y : (bf16*)p.C;
    const int ldd = gg ? p.ldy : p.ldc;
    const int Nout = gg ? p.N / 2 : p.N;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    auto drain = [&](int ti, int pb, int pe) {
      int bm, bn;
      tile_of(ti, bm, bn);
      const int n0 = bn * (gg ? BN / 2 : BN);
      for (int ps = pb; ps < pe; ++ps) {
        const int c = (ps * SW + sw) * 64 + lane;
        const int row = c / cpr, col = c - row * cpr;
        const int gm = bm * BM + row, gn = n0 + col * 8;
        if (row < BM && gm < p.M && gn < Nout && !(p.debug & 32)) {
          const u32x4 v = *(const u32x4*)(stg + row * PITCH + col * 16);
          *(u32x4*)(dst + (long long)gm * ldd + gn) = v;
        }
      }
    };
    __builtin_amdgcn_s_barrier();                              // prologue barrier
    int ti = 0, t = 0;
    for (int g = 0; g < G; ++g) {                              // SW > 0: every K-step has its barrier, the last one too
      __builtin_amdgcn_s_barrier();                            // barrier_g
      // tile ti-1 was staged before the barrier of this tile's first K-step; spread its NP passes over K-steps
      // 0 .. nt-2 (the MFMA waves overwrite the image after barrier nt-1, which this wave reaches only when its
      // reads of the last slice have returned)
      if (ti > 0 && t < nt - 1) drain(ti - 1, t * NP / (nt - 1), (t + 1) * NP / (nt - 1));
      if (++t == nt) { t = 0; ++ti; }
    }
    __builtin_amdgcn_s_barrier();                              // final barrier: the last tile is staged
    drain(my_n - 1, 0, NP);
    return;
  }
  if (wave >= NWC) {
    // ============================== loader waves
    // DMA waves issue ahead of the MFMA waves: +0.3..1.0 % on every shape (scripts/gemm_prio_probe.py; bit 64 of the debug
    // word = the old equal priorities for an A/B)
    if (!(p.debug & 64)) __builtin_amdgcn_s_setprio(3);
    const int lw = wave - NWC;
    const int lrow = lane >> 3, cpos = lane & 7;
#ifdef __HIP_DEVICE_COMPILE__           // (the host pass has no buffer-resource type; it only needs the stubs)
    // Buffer form of the LDS-DMA (buffer_load_dwordx4 ... offen lds): a per-lane 32-bit byte offset + a scalar offset
    // instead of a 64-bit address per lane -- half the address registers handed to the memory pipe per piece, and for the
    // plain GEMM no vector instruction at all per K-step (the K offset is the scalar one).  Reads past num_records return
    // zeros, which is what the conv gather wants for its halo and zero-stuffed taps.
    __amdgpu_buffer_rsrc_t rsrc_a;
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, 0x7fffffff, 0x00020000);
    int a_off[PA], a_iy0[PA], a_ix0[PA], w_off[PB];
    auto setup = [&](int ti) {
      int bm, bn, org;
      tile_of(ti, bm, bn);
      rsrc_a = tile_rsrc<MODE, BM>(p, bm, org);
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        const int r = (lw * PA + j) * 8 + lrow;
        const int chunk = cpos ^ ((r >> 1) & 7);
        int gm = bm * BM + r;
        gm = gm < p.M ? gm : p.M - 1;
        if (MODE == 0) {
          a_off[j] = ((gm - org) * p.lda + chunk * 8) * 2;
          a_iy0[j] = a_ix0[j] = 0;
        } else {
          const int hw = p.Ho * p.Wo;
          const int b = gm / hw;
          const int rem = gm - b * hw;
          const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
          a_iy0[j] = oy * p.stride - 1 + p.pad_off;
          a_ix0[j] = ox * p.stride - 1 + p.pad_off + p.pad_dx;
          a_off[j] = ((b - org) * p.Hs * p.Ws * conv_pix(p) + chunk * 8) * 2;
        }
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const int r = (lw * PB + j) * 8 + lrow;
        const int chunk = cpos ^ ((r >> 1) & 7);
        int gn = bn * BN + r;
        gn = gn < p.N ? gn : p.N - 1;
        w_off[j] = (gn * p.ldw + chunk * 8) * 2;
      }
    };
    const int Hv = p.Hs << p.shift, Wv = p.Ws << p.shift;
    int tap_off[PA];                    // conv: per-lane byte offset of the current tap's pixel (or out of range), refreshed
    int tap_cur = -1;                   // only when the K-step enters a new tap; the channel offset rides in the scalar offset
    auto issue = [&](int st, int k0) {
      char* base = smem + st * STAGE;
      int c0 = 0;
      if (MODE == 1) {
        const int tap = k0 / p.Cin;
        c0 = k0 - tap * p.Cin;
        if (tap != tap_cur) {
          tap_cur = tap;
          int ky, kx, cblk;
          conv_tap(p, tap, ky, kx, cblk);
          const int pix = conv_pix(p);
#pragma unroll
          for (int j = 0; j < PA; ++j) {
            const int iy = a_iy0[j] + ky, ix = a_ix0[j] + kx;
            bool ok = ((unsigned)iy < (unsigned)Hv) && ((unsigned)ix < (unsigned)Wv);
            if (p.parity) ok = ok && (((iy | ix) & 1) == 0);
            const int sy = iy >> p.shift, sx = ix >> p.shift;
            tap_off[j] = ok ? a_off[j] + ((sy * p.Ws + sx) * pix + cblk) * 2 : 0x7f000000;     // out of range: the load returns zeros
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        if (MODE == 0)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, PEA_LDS(base + (lw * PA + j) * 1024), 16, a_off[j], k0 * 2, 0, 0);
        else
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, PEA_LDS(base + (lw * PA + j) * 1024), 16, tap_off[j], c0 * 2, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, PEA_LDS(base + A_BYTES + (lw * PB + j) * 1024), 16, w_off[j], k0 * 2, 0, 0);
    };
#else
    auto setup = [](int) {};
    auto issue = [](int, int) {};
#endif
    // producer position (tile ordinal, K-step) of the next stage to issue
    int ptile = 0, pt = 0;
    setup(0);
    auto produce = [&](int st) {
      issue(st, pt * BK);
      if (++pt == nt) {
        pt = 0;
        if (++ptile < my_n) setup(ptile);
      }
    };
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (i < G) produce(i);
    if (G >= S) wait_vmcnt<(S - 1) * PP>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                              // prologue barrier: K-step 0 landed
    int cur = 0;
    for (int g = 0; g + 1 < G; ++g) {
      if (g + S - 1 < G) wait_vmcnt<(S - 2) * PP>();           // K-step g+1 landed; g+2 .. g+S-1 may stay in flight
      else wait_vmcnt<0>();
      if (!PEA_PROBE(2)) __builtin_amdgcn_s_barrier();         // barrier_g: slot of K-step g is free
      if (g + S < G && !PEA_PROBE(1)) produce(cur);
      cur = cur + 1 == S ? 0 : cur + 1;
    }
    dma_prefetch_next(p, blockIdx.x * LW + lw, gridDim.x * LW, lane);
    if (SW > 0) {
      __builtin_amdgcn_s_barrier();                            // barrier of the last K-step (staged form only)
      __builtin_amdgcn_s_barrier();                            // final barrier (store waves drain the last tile after it)
    }
    return;
  }

  // ================================ consumer waves
  constexpr int MT = BM / WM / 16, NT = BN / WN / 16;
  const int wr = wave / WN, wc = wave % WN;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int a_row0 = wr * (BM / WM) + r16, w_row0 = wc * (BN / WN) + r16;
  bf16x8 af[2][MT], wf[2][NT];
  // fragment addresses as (per-lane base) + (compile-time offset): rows 16 apart share the swizzle term ((row >> 1) & 7)
  // and the two k32 halves differ by XOR 64 bytes, so FOUR per-lane offsets address all 2 x (MT + NT) fragments (the
  // per-fragment form kept up to 18 loop-invariant address registers live beside 152 accumulator + fragment registers)
  int a_off[2] = {swz_off(a_row0, q4), swz_off(a_row0, 4 + q4)};
  int w_off[2] = {A_BYTES + swz_off(w_row0, q4), A_BYTES + swz_off(w_row0, 4 + q4)};
  // re-derived at the top of every tile from laundered lane ids (same values): the four registers are then not live across the
  // epilogue -- where the fused GEGLU-backward instantiation spilled them and RELOADED them from scratch in every K-step
  auto frag_offsets = [&]() {
    int r16l = r16, q4l = q4;
    asm volatile("" : "+v"(r16l), "+v"(q4l));
    const int ar = wr * (BM / WM) + r16l, wrw = wc * (BN / WN) + r16l;
    a_off[0] = swz_off(ar, q4l); a_off[1] = swz_off(ar, 4 + q4l);
    w_off[0] = A_BYTES + swz_off(wrw, q4l); w_off[1] = A_BYTES + swz_off(wrw, 4 + q4l);
  };
  auto load_frags = [&](int which, const char* tile, int s2) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) af[which][mt] = *(const bf16x8*)(tile + a_off[s2] + mt * 2048);
#pragma unroll
    for (int nt_ = 0; nt_ < NT; ++nt_) wf[which][nt_] = *(const bf16x8*)(tile + w_off[s2] + nt_ * 2048);
  };
  __builtin_amdgcn_s_barrier();                                // prologue barrier
  load_frags(0, smem, 0);
  int cur = 0, g = 0;
  f32x4 accp[DF ? NT : 1][DF ? MT : 1];                        // DF: the previous tile, waiting to be written out
  int pm = 0, pn = 0, pdone = MT;                              // its origin; slices already written (MT = none pending)
  const int par = (wave >> 2) & 1;                             // waves w and w+4 share a SIMD
  auto slice = [&](int sidx) {
    if constexpr (DF) {
      static_assert(!DF || MT <= 4, "deferred epilogue: at most 4 slices");
      switch (sidx) {
        case 0: gemm_epilogue16_lean<MT, NT, 0, 1>(p, accp, pm, pn, r16, q4); break;
        case 1: if constexpr (MT > 1) gemm_epilogue16_lean<MT, NT, 1, (MT > 1 ? 2 : MT)>(p, accp, pm, pn, r16, q4); break;
        case 2: if constexpr (MT > 2) gemm_epilogue16_lean<MT, NT, 2, (MT > 2 ? 3 : MT)>(p, accp, pm, pn, r16, q4); break;
        default: if constexpr (MT > 3) gemm_epilogue16_lean<MT, NT, 3, (MT > 3 ? 4 : MT)>(p, accp, pm, pn, r16, q4); break;
      }
    }
  };
  for (int ti = 0; ti < my_n; ++ti) {
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ti > 0) frag_offsets();
    for (int t = 0; t < nt; ++t, ++g) {
      const char* tile = smem + cur * STAGE;
      const int nxt = cur + 1 == S ? 0 : cur + 1;
      if constexpr (DF) {
        if (pdone < MT && (t & 1) == par) { slice(pdone); ++pdone; }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bool late_frags = false;
        if (s2 == 1) {
          if (g + 1 < G) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (!PEA_PROBE(2)) __builtin_amdgcn_s_barrier();   // barrier_g
            late_frags = true;                                 // first fragments of K-step g+1 (maybe the next tile's): issued BEHIND this half's first MFMAs
          } else if (SW > 0) {
            __builtin_amdgcn_s_barrier();                      // staged form: the last K-step keeps its barrier
          }
        } else if (MT < 4) {
          if (!PEA_PROBE(4)) load_frags(1, tile, 1);           // (32-row wave tiles: hipcc's own placement measures better)
        }
        if (MT >= 4) {                                         // 64-row wave tiles: the other half's fragment reads interleaved with this half's MFMAs
          __builtin_amdgcn_sched_barrier(0);
          if (s2 == 0) { if (!PEA_PROBE(4)) load_frags(1, tile, 1); }
          else if (!PEA_PROBE(4)) load_frags(0, smem + nxt * STAGE, 0);     // unconditional (behind the block's last K-step: a harmless read of a stale slot)
          mfma_half_interleaved<MT, NT>(acc, wf[s2], af[s2]);
          __builtin_amdgcn_sched_barrier(0);
          continue;
        }
#pragma unroll
        for (int nt_ = 0; nt_ < NT; ++nt_) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[nt_][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s2][nt_], af[s2][mt], acc[nt_][mt], 0, 0, 0);
          if (s2 == 1 && nt_ == 0) {
            // (issued right behind the barrier, hipcc's wait in front of this half's first MFMA covered these reads as well: every
            // wave of the CU then sat out an LDS round trip per K-step with the MFMA pipes idle)
            __builtin_amdgcn_sched_barrier(0);
            if (late_frags && !PEA_PROBE(4)) load_frags(0, smem + nxt * STAGE, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      cur = nxt;
    }
    int bm, bn;
    tile_of(ti, bm, bn);
    if constexpr (SW > 0) {
      // staged epilogue: values -> bf16 -> LDS image (row = tile row, column = tile column), no global stores here
      const int m_base = bm * BM + wr * (BM / WM), n_base = bn * BN + wc * (BN / WN);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = wr * (BM / WM) + mt * 16 + r16;
        const int bidx = p.rowvec ? min(m_base + mt * 16 + r16, p.M - 1) / p.rows_per_batch : 0;
#pragma unroll
        for (int nt_ = 0; nt_ < NT; ++nt_) {
          const int col = wc * (BN / WN) + nt_ * 16 + 4 * q4;
          const int n = min(n_base + nt_ * 16 + 4 * q4, p.N - 4);      // clamp: out-of-range columns are never stored
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = acc[nt_][mt][j] * p.alpha;
          if (p.bias) {
            const f32x4 bb = *(const f32x4*)(p.bias + n);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += bb[j];
          }
          if (p.rowvec) {
            const bf16x4 rv = *(const bf16x4*)(p.rowvec + (long long)bidx * p.ldrv + n);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += (float)rv[j];
          }
          if (p.geglu_y) {
            bf16x2 y;
            y[0] = (bf16)(v[0] * gelu_erf(v[1]));
            y[1] = (bf16)(v[2] * gelu_erf(v[3]));
            *(bf16x2*)(stg + row * PITCH + col) = y;               // column col/2, 2 bytes each
            continue;
          }
          if (p.act == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
          } else if (p.act == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = siluf_(v[j]);
          } else if (p.act == 3) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] * sigmoidf_(1.702f * v[j]);
          }
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
          *(bf16x4*)(stg + row * PITCH + col * 2) = o;
        }
      }
    } else if constexpr (DF) {
      while (pdone < MT) { slice(pdone); ++pdone; }            // short K: the parked tile must leave before it is replaced
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) accp[i][j] = acc[i][j];
      pm = bm * BM + wr * (BM / WM); pn = bn * BN + wc * (BN / WN); pdone = 0;
    } else {
      if (FASTONLY || p.epi_fast) {
        // lane constants laundered through an empty asm: the epilogue's per-lane address arithmetic is then derived
        // inside the epilogue instead of being hoisted to kernel entry and kept (spilled) across the whole tile loop
        int r16e = r16, q4e = q4;
        asm volatile("" : "+v"(r16e), "+v"(q4e));
        if constexpr (EPI == 2) gemm_epilogue16_lnf<MT, NT>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16e, q4e);
        else if (!PEA_PROBE(16)) gemm_epilogue16_fast<MT, NT, (EPI == 3 ? 2 : 0)>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16e, q4e);
        else if (acc[0][0][0] == 12345.678f) *(float*)p.C = 1.f;   // timing probe: keep the accumulators alive
        // the next tile's first fragments were fetched at the last barrier already; fetching them AGAIN here makes that
        // copy dead across the epilogue, so its 36 registers are free for the residual quads (the K-loop body itself
        // stays as it was: a special-cased last K-step made the compiler peel the loop and spill fragments inside it)
        load_frags(0, smem + cur * STAGE, 0);                  // unconditional (after the last tile: a harmless read of a stale slot)
      } else if constexpr (!FASTONLY) {
        if (!PEA_PROBE(16)) gemm_epilogue16<MT, NT>(p, acc, bm * BM + wr * (BM / WM), bn * BN + wc * (BN / WN), r16, q4);
        else if (acc[0][0][0] == 12345.678f) *(float*)p.C = 1.f;   // timing probe: keep the accumulators alive
      }
    }
  }
  if constexpr (DF) {
    while (pdone < MT) { slice(pdone); ++pdone; }
  }
  if constexpr (SW > 0) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                              // final barrier
  }
}

// CUs a GEMM launch may occupy: the device's count, or PEA_CU_LIMIT (two half-batch chains on two streams, each on half the chip)
static int g_num_cus = 0;
static hipError_t gemm_query_cus() {
  int dev = 0, n = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  if (const char* lim = getenv("PEA_CU_LIMIT")) {
    const int l = atoi(lim);
    if (l > 0 && l < n) n = l;
  }
  g_num_cus = n;
  return hipSuccess;
}
template <int MODE, int BM, int BN, int WM, int WN, int LW, int S, int SW = 0, int DF = 0, int EPI = 0, int OCC = 1>
static int launch_lcp(const GemmP& p, hipStream_t stream) {
  constexpr int lds = S * (BM + BN) * 128 + (SW ? BM * (BN * 2 + 16) : 0);
  static_assert(lds * OCC <= 160 * 1024, "LDS budget");
  static_assert(OCC == 1 || (WM * WN + LW + SW) * OCC <= 12, "OCC = 2: three waves per SIMD");
  static bool attr_set = false;
  if (!attr_set) {
    HIPCHK(hipFuncSetAttribute((const void*)gemm_lcp_kernel<MODE, BM, BN, WM, WN, LW, S, SW, DF, EPI, OCC>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    attr_set = true;
  }
  if (!g_num_cus) HIPCHK(gemm_query_cus());
  SHAPECHK(p.ksplit <= 1, "gemm: the persistent kernel has no split-K path");
  const int tiles = cdiv(p.M, BM) * cdiv(p.N, BN);
  const int grid = tiles < g_num_cus * OCC ? tiles : g_num_cus * OCC;
  SHAPECHK(EPI == 0 || p.epi_fast, "gemm: variant needs the batched-load epilogue");
  hipLaunchKernelGGL((gemm_lcp_kernel<MODE, BM, BN, WM, WN, LW, S, SW, DF, EPI, OCC>), dim3(grid),
                     dim3((WM * WN + LW + SW) * 64), lds, stream, p);
  return PEA_OK;
}

// ---- variant table (tile shape x wave grid x ring depth); gemm_decide picks one row per problem
// X(id, launcher, carries column scale / GEGLU, has a row-vector + fused (GEGLU backward, folded LayerNorm) form,
//   id to take for the generic epilogue (0: the row carries it itself), template arguments behind MODE...)
//   24 / 27 = 256x160 tile, 4x2 consumer waves (64x80 each) + 4 DMA waves, 3 stages   (27: persistent)
//   25 / 28 = 128x160 tile, 4x2 consumer waves (32x80 each) + 4 DMA waves, 3 stages   (28: persistent)
//   29      = 128x160 tile, 2x2 consumer waves (64x80 each) + 4 DMA waves, 4 stages, persistent
//   31      =  64x160 tile, 2x2 consumer waves (32x80 each) + 4 DMA waves, 4 stages, persistent
// What a row's kernel cannot do is a fact of the row, not of the launcher:
//   34 / 35 (staged / deferred epilogue) carry no column scale and no GEGLU epilogue (34 drops the stash, 35 the output);
//   39 / 40 (192-row tiles) have no fused instantiation, and a 48-row wave tile of theirs would straddle two samples of a
//           per-sample row vector in the batched-load epilogue (the shape rule never picks them with one; a pinned id must not either);
//   27 / 40 / 33 (256- and 192-row persistent tiles) are compiled with the batched-load epilogue only (FASTONLY).
//   (36 / 37 are FASTONLY too and have no generic stand-in: launch_lcp refuses them.)
#define GEMM_TABLE(X)                                                                   \
  X(18, launch_lc,  1, 1,  0, 128, 128, 2, 2, 4, 4)                                     \
  X(19, launch_lc,  1, 1,  0, 128, 160, 4, 1, 4, 3)                                     \
  X(20, launch_lc,  1, 1,  0, 128, 160, 4, 1, 4, 3, true)       /* timing probe only */ \
  X(22, launch_lc,  1, 1,  0, 128, 160, 2, 2, 4, 4, false, true)                        \
  X(23, launch_lc,  1, 1,  0, 128, 128, 2, 2, 4, 4, false, true)                        \
  X(24, launch_lc,  1, 1,  0, 256, 160, 4, 2, 4, 3, false, true)                        \
  X(25, launch_lc,  1, 1,  0, 128, 160, 4, 2, 4, 3, false, true)                        \
  X(27, launch_lcp, 1, 1, 28, 256, 160, 4, 2, 4, 3, 0, 0, 1)                            \
  X(28, launch_lcp, 1, 1,  0, 128, 160, 4, 2, 4, 3)                                     \
  X(29, launch_lcp, 1, 1,  0, 128, 160, 2, 2, 4, 4)                                     \
  X(30, launch_lcp, 1, 1,  0, 128, 128, 2, 2, 4, 4)                                     \
  X(31, launch_lcp, 1, 1,  0, 64, 160, 2, 2, 4, 4)                                      \
  X(33, launch_lcp, 1, 1, 30, 256, 128, 4, 2, 4, 3, 0, 0, 1)                            \
  X(34, launch_lcp, 0, 1,  0, 128, 160, 4, 2, 4, 3, 4)          /* staged epilogue */   \
  X(35, launch_lcp, 0, 1,  0, 128, 160, 4, 2, 4, 3, 0, 1)       /* deferred epilogue */ \
  X(36, launch_lcp, 1, 1,  0, 128, 160, 2, 2, 2, 2, 0, 0, 1, 2) /* two workgroups per CU */ \
  X(37, launch_lcp, 1, 1,  0, 128, 128, 2, 2, 2, 2, 0, 0, 1, 2)                         \
  X(39, launch_lc,  1, 0,  0, 192, 160, 4, 2, 4, 3, false, true) /* 48 x 80 wave tiles: row counts that leave 128- / 256-row tiles a partial round */ \
  X(40, launch_lcp, 1, 0, 28, 192, 160, 4, 2, 4, 3, 0, 0, 1)                            \
  X(41, launch_lc,  1, 1,  0, 128, 160, 2, 2, 4, 3, false, true, 1, false, true) /* intra-workgroup K split */

// One enumerator per kernel instantiation launch_gemm can launch (each table row exists for MODE 0 and 1, the fused forms for
// MODE 0 only).  A table row's enumerator is its variant id; the fused forms are 100 / 200 + the id of the tile form they share.
enum GemmInst : int {
#define X(id, fn, cg, rf, gen, ...) GEMM_V##id = id,
  GEMM_TABLE(X)
#undef X
  // fused GEGLU backward (GemmP::gbwd_pre): persistent kernels with EPI = 3
  GEMM_GBWD_256 = 127, GEMM_GBWD_128 = 128, GEMM_GBWD_64 = 131,
  // folded LayerNorm (GemmP::ln_stats): the five tile forms the shape rule can pick for a plain GEMM
  GEMM_LNF_LC256 = 224, GEMM_LNF_LC128 = 225, GEMM_LNF_256 = 227, GEMM_LNF_128 = 228, GEMM_LNF_64 = 231,
};
static constexpr GemmInst kGemmInsts[] = {
#define X(id, fn, cg, rf, gen, ...) GEMM_V##id,
    GEMM_TABLE(X)
#undef X
    GEMM_GBWD_256, GEMM_GBWD_128, GEMM_GBWD_64, GEMM_LNF_LC256, GEMM_LNF_LC128, GEMM_LNF_256, GEMM_LNF_128, GEMM_LNF_64};
struct GemmVariantRow { int id; bool colscale_geglu, rowvec_fused; int generic_id; };
static constexpr GemmVariantRow kGemmRows[] = {
#define X(id, fn, cg, rf, gen, ...) {id, cg != 0, rf != 0, gen},
    GEMM_TABLE(X)
#undef X
};
static const GemmVariantRow* gemm_row(int id) {
  for (const GemmVariantRow& r : kGemmRows)
    if (r.id == id) return &r;
  return nullptr;
}

// Environment switches of the launcher, read once per process.
struct GemmEnv {
  bool defer;            // PEA_GEMM_DEFER: variant 35 (deferred lean epilogue) where the shape rule would take 25 / 28 with a lean epilogue
  int ksw_mink;          // PEA_GEMM_KSW_MINK: smallest K for the K-split form 41 on one-round launches (default 0 = never)
  bool slow_epilogue;    // PEA_GEMM_SLOW_EPILOGUE: never the batched-load epilogue (A/B switch)
  bool pf_on;            // PEA_GEMM_PF=0 switches the next-op weight prefetch off (A/B)
  long long pf_max;      // PEA_GEMM_PF_MAX_MB caps what one launch touches (default 64)
};
static const GemmEnv& gemm_env() {
  static const GemmEnv e = {getenv("PEA_GEMM_DEFER") != nullptr, getenv("PEA_GEMM_KSW_MINK") ? atoi(getenv("PEA_GEMM_KSW_MINK")) : 0,
                            getenv("PEA_GEMM_SLOW_EPILOGUE") != nullptr, !(getenv("PEA_GEMM_PF") && atoi(getenv("PEA_GEMM_PF")) == 0),
                            (getenv("PEA_GEMM_PF_MAX_MB") ? atoll(getenv("PEA_GEMM_PF_MAX_MB")) : 64) << 20};
  return e;
}

// Whether the batched-load epilogue (gemm_epilogue16_fast) applies to p: its preconditions.
static bool gemm_epi_fast(const GemmP& p, const GemmEnv& env) {
  // wave-tile rows of the 16x16x32 kernels are 32 or 64: a per-sample row vector must not change inside them
  const bool rv_ok = !p.rowvec || (p.rows_per_batch % 64 == 0);
  const bool gg_ok = !p.geglu_y || (p.ldy % 4 == 0 && (((unsigned long long)p.geglu_y & 7) == 0) && !p.res && !p.rowvec && !p.geglu_tanh);
  return !env.slow_epilogue && !p.out_f32 && p.act == 0 && !p.preact && p.ksplit <= 1 && p.N % 16 == 0 && rv_ok && gg_ok &&
         (p.geglu_y ? (!p.C || (p.ldc % 8 == 0 && (((unsigned long long)p.C & 15) == 0)))
                    : (p.ldc % 8 == 0 && (((unsigned long long)p.C & 15) == 0))) &&
         (!p.res || (p.ldres % 8 == 0 && (((unsigned long long)p.res & 15) == 0)));      // residual read as 16-byte pieces
}

// The shape rule: the variant id for a problem nobody pinned.
static int pick_variant(const GemmP& p, bool epi_fast, int cus, const GemmEnv& env) {
  // measured on the step's shapes with scripts/gemm_bench.py / gemm_ksweep.py (profiles/r01_gemm_variants.log); all
  // loader/consumer kernels with 16x16x32 MFMAs.
  // A launch of at most one tile per CU gains nothing from the persistent form; beyond that it hides every
  // tile's prologue behind the previous tile's epilogue.
  if (p.N % 160 != 0 && p.N % 128 == 0 && p.M >= 1024)                // VAE widths 128/256/512: exact 128-wide tiles
    return cdiv(p.M, 256) * (p.N / 128) >= cus ? 33 : 30;
  const int t128 = cdiv(p.M, 128) * cdiv(p.N, 160), t256 = cdiv(p.M, 256) * cdiv(p.N, 160);
  if (p.mode == 1) {
    if (t256 >= cus) return 27;                      // 128^2- and 64^2-level convs (N = 320 / 640)
    return 29;                                       // 32^2-level convs (M = 4096, N = 1280)
  }
  if (p.M < 1024 && t128 > 2 * cus)                      // stacked cross-attention K|V projection (M = 2B*77, N = 166400): many
    return p.M * 100 >= cdiv(p.M, 256) * 256 * 78 ? 27 : 29;   // tiles per CU, so the large wave tile pays (profiles/r03_kv_stack.log)
  if (p.M < 1024 || t128 <= cus * 5 / 8) return 31;          // embeddings, adapter (tall-skinny, few tiles)
  // 35 = 28 with the deferred (lean: alpha / bias / bf16) epilogue: the finished tile leaves in 16-row slices during
  // the next tile's K-steps, the two MFMA waves of a SIMD taking turns
  // measured (in-run A/B, profiles/r01_gemm_variants.log): +4..11 % in the hot microbenchmark, nothing in situ -> off
  // unless PEA_GEMM_DEFER is set
  const bool lean = env.defer && !p.out_f32 && !p.res && !p.rowvec && !p.act && !p.geglu_y && !p.gbwd_pre && !p.preact && !p.qscale_cols && p.ksplit <= 1 &&
                    p.ldc % 8 == 0 && (((unsigned long long)p.C & 15) == 0);
  // Row counts between the multiples the rules below were tuned on (6144 = the merged pass of a batch with dead teacher rows,
  // batch 3 / 6 per GPU): both tile heights leave a partial last round.  A 192-row tile (48 x 80 wave tiles) is taken when it
  // cuts rounds x rows by at least 10 % against what the rules would pick (never for the SDXL batch-4 / batch-8 shapes: their
  // tile counts are whole rounds).  No per-sample row vector (a 48-row wave tile may straddle two samples), batched-load epilogue only.
  if (!p.rowvec && p.mode == 0 && epi_fast && p.M >= 1024) {
    const int t192 = cdiv(p.M, 192) * cdiv(p.N, 160);
    const int r128 = cdiv(t128, cus) * 128, r192 = cdiv(t192, cus) * 192, r256 = cdiv(t256, cus) * 256;
    const int cur = t128 <= cus ? r128 : (t256 <= cus ? (t256 > cus * 3 / 4 ? r256 : r128)
                                                       : (t256 * 100 >= cdiv(t256, cus) * cus * 85 ? r256 : r128));
    if (r192 * 10 <= cur * 9) return t192 <= cus ? 39 : 40;
  }
  // one round of 128 x 160 tiles with a long K: the K-split form (41); PEA_GEMM_KSW_MINK sets the threshold (0 = never)
  if (t128 <= cus && env.ksw_mink > 0 && p.K >= env.ksw_mink && (p.K / BK) % 2 == 0 && epi_fast && p.ksplit <= 1 && p.mode == 0 && t128 > cus * 5 / 8) return 41;
  if (t128 <= cus) return lean ? 35 : 25;            // at most one 128x160 tile per CU
  if (t256 <= cus) return t256 > cus * 3 / 4 ? 24 : (lean ? 35 : 28);
  // more than one 256x160 tile per CU: the large tile wins (less L2 -> LDS traffic per flop) unless its tile count
  // leaves the last round of CUs mostly idle (e.g. 384 tiles = 1.5 rounds), then the 128x160 form balances better
  const int rounds = cdiv(t256, cus);
  if (t256 * 100 >= rounds * cus * 85) return 27;
  return lean ? 35 : 28;
}

// THE decision: which instantiation a problem launches.  Pure: no HIP call, no global state -- `cus` is the CU count the launch may
// occupy (0: 256), `forced` a pinned variant id or -1.  launch_gemm launches what this returns and nothing else decides.
struct GemmDecision { GemmInst inst; bool epi_fast; };
static GemmDecision gemm_decide(const GemmP& p, int cus, int forced, const GemmEnv& env) {
  const bool epi_fast = gemm_epi_fast(p, env);
  int v = forced >= 0 ? forced : pick_variant(p, epi_fast, cus > 0 ? cus : 256, env);
  const GemmVariantRow* row = gemm_row(v);
  // a row that cannot carry what the problem asks of its epilogue gives way to the persistent 128 x 160 form
  if (row && !row->colscale_geglu && (p.qscale_cols || p.geglu_y)) v = 28;
  if (row && !row->rowvec_fused && (p.gbwd_pre || p.ln_stats || (p.rowvec && epi_fast))) v = 28;
  if (p.ksplit > 1) v = 18;                         // loader/consumer 128x128 (the only kernel with the split-K path)
  if (p.gbwd_pre) {
    // every tile form the shape rule picks for the FF output projection's dgrad maps to one of the three
    return {v == 27 || v == 24 ? GEMM_GBWD_256 : (v == 31 ? GEMM_GBWD_64 : GEMM_GBWD_128), epi_fast};   // (128-row tiles for 27 / 24: +1.0-1.5 ms per step)
  }
  row = gemm_row(v);
  if (!epi_fast && row && row->generic_id) v = row->generic_id;
  if (p.ln_stats) {
    switch (v) {
      case 27: return {GEMM_LNF_256, epi_fast};
      case 24: return {GEMM_LNF_LC256, epi_fast};
      case 28: case 35: return {GEMM_LNF_128, epi_fast};
      case 31: return {GEMM_LNF_64, epi_fast};
      default: return {GEMM_LNF_LC128, epi_fast};   // 25 and the rest
    }
  }
  return {gemm_row(v) ? (GemmInst)v : GEMM_V23, epi_fast};   // an id outside the table: the loader/consumer 128 x 128 form
}

int g_gemm_variant = -1;   // >= 0: forced (benchmark / debug)
extern "C" void pea_debug_set_gemm_variant(int v) { g_gemm_variant = v; }
int g_gemm_debug = 0;
extern "C" void pea_debug_set_gemm_debug(int v) { g_gemm_debug = v; }
// pea_debug_set_gemm_prefetch arms the NEXT launch_gemm with a target (operator-level experiments: scripts/chain_probe.py)
static const void* g_dbg_pf_ptr = nullptr;
static long long g_dbg_pf_bytes = 0;
extern "C" void pea_debug_set_gemm_prefetch(const void* p, long long bytes) { g_dbg_pf_ptr = p; g_dbg_pf_bytes = bytes; }

// gemm_decide for tests, on a problem described by integers (include/pea_hip.h has the feature bits); no device needed
extern "C" int pea_debug_gemm_dispatch(int M, int N, int K, int mode, int rows_per_batch, int features, int cus, int forced) {
  if (M <= 0) return N >= 0 && N < (int)(sizeof(kGemmInsts) / sizeof(kGemmInsts[0])) ? (int)kGemmInsts[N] : -1;
  GemmP p = {};
  const bool al = (features & 1024) != 0;
  char* const base = (char*)(uintptr_t)(al ? 0x1000 : 0x1004);   // never dereferenced
  const int pad = al ? 0 : 4;
  p.mode = mode; p.M = M; p.N = N; p.K = K; p.alpha = 1.f;
  p.lda = K; p.ldw = K;
  p.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : M;
  p.C = base; p.ldc = ((features & 64) ? 2 * N : N) + pad;
  if (features & 1) { p.res = (const bf16*)base; p.ldres = N + pad; }
  if (features & 2) { p.rowvec = (const bf16*)base; p.ldrv = N; }
  if (features & 4) p.out_f32 = 1;
  if (features & 8) p.act = 1;
  if (features & 32) { p.geglu_y = (bf16*)base; p.ldy = N / 2 + pad; if (!(features & 16)) p.C = nullptr; }
  else if (features & 16) { p.preact = (bf16*)base; p.ldpre = N + pad; }
  if (features & 64) { p.gbwd_pre = (const bf16*)base; p.ldgp = 2 * N + pad; }
  if (features & 128) { p.ln_stats = (const float*)base; p.ln_s = (const float*)base; }
  if (features & 256) { p.qscale_cols = 16; p.qscale = 1.f; }
  if (features & 512) p.ksplit = 2;
  return gemm_decide(p, cus, forced, gemm_env()).inst;
}

int launch_gemm(const GemmP& p_in, hipStream_t stream) {
  const GemmP& p0 = p_in;
  SHAPECHK(p0.M > 0 && p0.N > 0 && p0.K > 0, "gemm: empty problem M=%d N=%d K=%d", p0.M, p0.N, p0.K);
  SHAPECHK(p0.K % BK == 0, "gemm: K=%d must be a multiple of %d", p0.K, BK);
  SHAPECHK(p0.N % 4 == 0, "gemm: N=%d must be a multiple of 4", p0.N);
  SHAPECHK(p0.ldw % 8 == 0 && p0.ldc % 4 == 0, "gemm: ldw=%d ldc=%d alignment", p0.ldw, p0.ldc);
  if (p0.mode == 0) {
    SHAPECHK(p0.lda % 8 == 0, "gemm: lda=%d must be a multiple of 8", p0.lda);
  } else {
    const int ntaps = p0.kside == 2 ? 4 : (p0.kside == 4 ? 16 : 9);
    SHAPECHK(p0.kside == 0 || p0.kside == 2 || p0.kside == 3 || p0.kside == 4, "conv: kside=%d", p0.kside);
    SHAPECHK(p0.Cin % BK == 0 && p0.K == ntaps * p0.Cin, "conv: Cin=%d must be a multiple of %d and K=%d*Cin", p0.Cin, BK, ntaps);
    SHAPECHK(p0.pix == 0 || (p0.pix % 8 == 0 && p0.pix >= (p0.kside == 4 ? 4 : 1) * p0.Cin), "conv: pixel stride %d vs Cin=%d", p0.pix, p0.Cin);
    SHAPECHK(p0.kside < 4 || (!p0.shift && !p0.parity && p0.stride == 1), "conv: the 16-tap form is stride 1 on a plain source");
    SHAPECHK(p0.zeros != nullptr, "conv: zero page missing");
    SHAPECHK(p0.M % (p0.Ho * p0.Wo) == 0, "conv: M=%d not a multiple of Ho*Wo", p0.M);
  }
  {
    // 32-bit buffer offsets of the DMA loaders (tile_rsrc): relative to the row tile for A, to the tensor for W
    const long long hw = p0.mode ? (long long)p0.Ho * p0.Wo : 1;
    const long long pix = p0.pix ? p0.pix : p0.Cin;
    const long long span = p0.mode ? (256 / hw + 2) * (long long)p0.Hs * p0.Ws * pix * 2 : 256LL * p0.lda * 2;
    const long long whole = p0.mode ? (p0.M / hw) * (long long)p0.Hs * p0.Ws * pix * 2 : (long long)p0.M * p0.lda * 2;
    SHAPECHK((span < whole ? span : whole) <= 0x7f000000LL, "gemm: one row tile of A spans %lld bytes (limit 0x7f000000)", span);
    SHAPECHK((long long)p0.N * p0.ldw * 2 <= 0x7fffffffLL, "gemm: W of %d x %d exceeds the 2 GB buffer range", p0.N, p0.ldw);
  }
  {
    // algorithmic work: 2*M*N*K; a transposed (zero-stuffed) conv only has 1/4 of its taps real
    double fl = 2.0 * p0.M * (double)p0.N * p0.K * (p0.parity ? 0.25 : 1.0);
    double by = 2.0 * ((double)p0.M * p0.N + (double)p0.N * p0.K + (p0.mode ? (double)p0.M * p0.K / (p0.kside == 2 ? 4.0 : (p0.kside == 4 ? 4.0 : 9.0)) : (double)p0.M * p0.K));
    if (g_prof_on) { g_prof_tag[0] = p0.M; g_prof_tag[1] = p0.N; g_prof_tag[2] = p0.K; g_prof_tag[3] = (p0.res ? 1 : 0) | (p0.bias ? 2 : 0) | (p0.rowvec ? 4 : 0); }
    PROF_BEGIN(p0.mode ? 1 : 0, fl, by, stream);
  }
  const GemmEnv& env = gemm_env();
  GemmP p = p_in;
  p.debug = g_gemm_debug;
  if (g_dbg_pf_ptr) { p.pf_ptr = g_dbg_pf_ptr; p.pf_bytes = g_dbg_pf_bytes; g_dbg_pf_ptr = nullptr; }
  if (!env.pf_on || p.pf_bytes <= 0) { p.pf_ptr = nullptr; p.pf_bytes = 0; }
  if (p.pf_bytes > env.pf_max) p.pf_bytes = env.pf_max;
  SHAPECHK(p.qscale_cols % 16 == 0 && p.qscale_cols >= 0 && p.qscale_cols <= p.N && (!p.qscale_cols || (!p.act && !p.geglu_y && !p.gbwd_pre && p.ksplit <= 1)),
           "gemm: qscale_cols=%d must be a multiple of 16 within N, on a plain (no activation / GEGLU / split-K) epilogue", p.qscale_cols);
  // refusals that depend on the shape alone: ahead of the CU query, so they answer without a device
  if (p.ksplit > 1) {
    SHAPECHK(p.out_f32 && !p.accum_f32 && !p.bias && !p.res && !p.rowvec && !p.preact && p.act == 0 && p.mode == 0,
             "gemm: split-K writes plain fp32 partials");
    // partial s is the [M][ldc] matrix at C + s * split_stride, stored as 16-byte quads
    SHAPECHK(p.split_stride >= (long long)(p.M - 1) * p.ldc + p.N && p.split_stride % 4 == 0,
             "gemm: split-K split_stride=%lld (M=%d N=%d ldc=%d): partials overlap or leave 16-byte alignment", p.split_stride, p.M, p.N, p.ldc);
  }
  // the stash_grad branch of the GEGLU epilogues knows the erf form only (the tape's geglu_stash_form never asks for both)
  SHAPECHK(!(p.stash_grad && p.geglu_tanh), "gemm: the gradient-form GEGLU stash exists for the erf gate only (geglu_tanh set)");
  if (!g_num_cus) HIPCHK(gemm_query_cus());
  const GemmDecision d = gemm_decide(p, g_num_cus, g_gemm_variant, env);
  p.epi_fast = d.epi_fast;
  if (p.gbwd_pre) {
    // fused GEGLU backward: own instantiations of the persistent kernels
    SHAPECHK(p.epi_fast && p.mode == 0 && !p.res && !p.rowvec && !p.bias && !p.geglu_y && !p.ln_stats && p.ldgp % 8 == 0 &&
                 p.ldc >= 2 * p.N && (((unsigned long long)p.gbwd_pre & 15) == 0),
             "gemm: the fused GEGLU backward needs the batched-load epilogue (bf16 [M][2N] output, no bias / residual / row vector)");
  } else if (p.ln_stats) {
    SHAPECHK(p.epi_fast && p.ln_s && p.alpha == 1.f && p.mode == 0 && !p.res && !p.rowvec,
             "gemm: the folded-LayerNorm epilogue needs the batched-load epilogue (bf16 output, no activation / residual)");
  }
  int rc = PEA_OK;
  switch (d.inst) {
#define X(id, fn, cg, rf, gen, ...) \
    case GEMM_V##id: rc = p.mode == 0 ? fn<0, __VA_ARGS__>(p, stream) : fn<1, __VA_ARGS__>(p, stream); break;
    GEMM_TABLE(X)
#undef X
    case GEMM_GBWD_256: rc = launch_lcp<0, 256, 160, 4, 2, 4, 3, 0, 0, 3>(p, stream); break;
    case GEMM_GBWD_128: rc = launch_lcp<0, 128, 160, 4, 2, 4, 3, 0, 0, 3>(p, stream); break;
    case GEMM_GBWD_64: rc = launch_lcp<0, 64, 160, 2, 2, 4, 4, 0, 0, 3>(p, stream); break;
    case GEMM_LNF_256: rc = launch_lcp<0, 256, 160, 4, 2, 4, 3, 0, 0, 2>(p, stream); break;
    case GEMM_LNF_LC256: rc = launch_lc<0, 256, 160, 4, 2, 4, 3, false, true, 1, true>(p, stream); break;
    case GEMM_LNF_128: rc = launch_lcp<0, 128, 160, 4, 2, 4, 3, 0, 0, 2>(p, stream); break;
    case GEMM_LNF_64: rc = launch_lcp<0, 64, 160, 2, 2, 4, 4, 0, 0, 2>(p, stream); break;
    case GEMM_LNF_LC128: rc = launch_lc<0, 128, 160, 4, 2, 4, 3, false, true, 1, true>(p, stream); break;
  }
  PROF_END(stream);
  if (rc != PEA_OK) return rc;
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ------------------------------------------------------------------------------------------
// 4-channel ends of the UNet (conv_in: K = 36, conv_out: N = 4): negligible FLOPs, direct form.
// conv_in (Cin = 4, K = 36): weights transposed into LDS [36][Cout] fp32; a thread owns 8 output channels and
// walks pixels; the 36 input taps are read once per pixel (L1-shared by the threads of that pixel).
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, bf16* __restrict__ y, int B,
                                                      int Cin, int H, int W, int Cout, int pix_per_block, int ldy,
                                                      int silu) {
  extern __shared__ __attribute__((aligned(16))) char cism[];
  float* wl = (float*)cism;                       // [Cin*9][Cout]
  const int K = Cin * 9;
  for (int i = threadIdx.x; i < K * Cout; i += blockDim.x) {
    const int co = i / K, k = i - co * K;        // w[co][ci][ky][kx] -> k = ci*9 + ky*3 + kx
    wl[k * Cout + co] = w[i];
  }
  __syncthreads();
  const int nchunk = Cout / 8;
  const int ppb = blockDim.x / nchunk;
  const int ck = threadIdx.x % nchunk, pl = threadIdx.x / nchunk;
  if (pl >= ppb) return;
  const int c0 = ck * 8;
  float bs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bs[j] = bias[c0 + j];
  const long long npix = (long long)B * H * W;
  const long long p0 = (long long)blockIdx.x * pix_per_block;
  const long long p1 = p0 + pix_per_block < npix ? p0 + pix_per_block : npix;
  for (long long pix = p0 + pl; pix < p1; pix += ppb) {
    const int xw = (int)(pix % W), yh = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = bs[j];
    for (int ci = 0; ci < Cin; ++ci)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = yh + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = xw + kx - 1;
          const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
          const float v = ok ? x[(((long long)b * Cin + ci) * H + iy) * W + ix] : 0.f;
          const float* wr = wl + (ci * 9 + ky * 3 + kx) * Cout + c0;
          const f32x4 w0 = *(const f32x4*)wr, w1 = *(const f32x4*)(wr + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc[j] += v * w0[j];
            acc[4 + j] += v * w1[j];
          }
        }
      }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)(silu ? siluf_(acc[j]) : acc[j]);
    *(bf16x8*)(y + pix * ldy + c0) = o;
  }
}

// The same with 4 consecutive pixels of a row per thread (W % 4 == 0): a weight vector read from LDS feeds 4 pixels and a
// row segment of 6 inputs feeds 3 taps x 4 pixels, so the loop is bound by its FMAs, not by the LDS reads (1 byte of LDS per
// FMA instead of 4).  It serves both 4-channel ends that produce a wide NHWC tensor from a narrow fp32 NCHW one:
//   FLIP = false: conv_in                x [B][Cs][H][W], w [N][Cs][3][3]  ->  y [pix][N] (+ bias, optional SiLU)
//   FLIP = true : dgrad of conv_out     dy [B][Cs][H][W], w [Cs][3][3][N] ->  dx [pix][N]   (taps mirrored)
// GATHER (with FLIP = false): the inpainting UNet's conv_in reads its Cs = 2 C + 1 input channels from three tensors instead of
// their torch.cat (tests/test_sdxl_zh_inpaint.py: cat([cat([latents] * 2), mask, masked_image_latents], dim=1)); channel ci of
// image b is latents[b % lat_b][ci] (ci < C), mask[b % cond_b][0] (ci == C), masked[b % cond_b][ci - C - 1] (ci > C).  Same
// loop, same summation order: the result equals the plain kernel on the concatenated tensor bit for bit.
struct ConvGatherSrc {
  const float* lat; const float* mask; const float* masked;
  int C, lat_b, cond_b;
};
template <bool FLIP, bool GATHER = false>
__global__ __launch_bounds__(256) void conv_few4_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, bf16* __restrict__ y, int B,
                                                        int Cs, int H, int W, int N, int groups_per_block, int ldy,
                                                        int silu, ConvGatherSrc gs) {
  extern __shared__ __attribute__((aligned(16))) char cfsm[];
  float* wl = (float*)cfsm;                       // [Cs*9][N]
  const int K = Cs * 9;
  for (int i = threadIdx.x; i < K * N; i += blockDim.x) {
    if (FLIP) {
      wl[i] = w[i];                               // already [k = co*9 + tap][n]
    } else {
      const int n = i / K, k = i - n * K;         // w[n][ci][ky][kx] -> k = ci*9 + ky*3 + kx
      wl[k * N + n] = w[i];
    }
  }
  __syncthreads();
  const int nchunk = N / 8;
  const int ppb = blockDim.x / nchunk;
  const int ck = threadIdx.x % nchunk, pl = threadIdx.x / nchunk;
  if (pl >= ppb) return;
  const int c0 = ck * 8;
  float bs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bs[j] = bias ? bias[c0 + j] : 0.f;
  const int W4 = W / 4;
  const long long ngroups = (long long)B * H * W4;
  const long long g0 = (long long)blockIdx.x * groups_per_block;
  const long long g1 = g0 + groups_per_block < ngroups ? g0 + groups_per_block : ngroups;
  for (long long grp = g0 + pl; grp < g1; grp += ppb) {
    const int x0 = (int)(grp % W4) * 4, yh = (int)((grp / W4) % H), b = (int)(grp / ((long long)W4 * H));
    float acc[4][8];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[p][j] = bs[j];
    const long long HW = (long long)H * W;
    const int bl = GATHER ? b % gs.lat_b : 0, bc = GATHER ? b % gs.cond_b : 0;
    for (int ci = 0; ci < Cs; ++ci)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = FLIP ? yh + 1 - ky : yh + ky - 1;
        if ((unsigned)iy >= (unsigned)H) continue;
        const float* row;
        if constexpr (GATHER) {
          const float* plane = ci < gs.C    ? gs.lat + ((long long)bl * gs.C + ci) * HW
                               : ci == gs.C ? gs.mask + (long long)bc * HW
                                            : gs.masked + ((long long)bc * (Cs - gs.C - 1) + (ci - gs.C - 1)) * HW;
          row = plane + (long long)iy * W;
        } else {
          row = x + (((long long)b * Cs + ci) * H + iy) * W;
        }
        float v[6];                               // inputs x0-1 .. x0+4 (x0 % 4 == 0: the middle four are one aligned 16-byte load)
        const f32x4 mid = *(const f32x4*)(row + x0);
        v[0] = x0 > 0 ? row[x0 - 1] : 0.f;
        v[1] = mid[0]; v[2] = mid[1]; v[3] = mid[2]; v[4] = mid[3];
        v[5] = x0 + 4 < W ? row[x0 + 4] : 0.f;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float* wr = wl + (ci * 9 + ky * 3 + kx) * N + c0;
          const f32x4 w0 = *(const f32x4*)wr, w1 = *(const f32x4*)(wr + 4);
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const float vv = FLIP ? v[p + 2 - kx] : v[p + kx];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[p][j] += vv * w0[j];
              acc[p][4 + j] += vv * w1[j];
            }
          }
        }
      }
    const long long pix = ((long long)b * H + yh) * W + x0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (bf16)(silu ? siluf_(acc[p][j]) : acc[p][j]);
      *(bf16x8*)(y + (pix + p) * ldy + c0) = o;
    }
  }
}

// shared launcher of the uses; returns false when the shape needs the one-pixel-per-thread kernels (the gather form has none:
// its caller refuses those shapes first)
template <bool FLIP, bool GATHER = false>
static bool launch_conv_few4(const float* x, const float* w, const float* bias, bf16* y, int B, int Cs, int H, int W, int N,
                             int ldy, int silu, hipStream_t s, int* rc, const ConvGatherSrc& gs = ConvGatherSrc{}) {
  const size_t lds = (size_t)Cs * 9 * N * 4;
  if (!GATHER && (W % 4 != 0 || N % 8 != 0 || N / 8 > 256 || lds > 160 * 1024 || (((unsigned long long)x) & 15) != 0))
    return false;
  *rc = PEA_OK;
  if (lds > 64 * 1024) {
    static bool attr_set = false;
    if (!attr_set) {
      if (hipFuncSetAttribute((const void*)conv_few4_kernel<FLIP, GATHER>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        *rc = PEA_E_HIP;
        return true;
      }
      attr_set = true;
    }
  }
  const int ppb = 256 / (N / 8);
  const long long ngroups = (long long)B * H * (W / 4);
  // two to three workgroups per CU each walk their share of the pixel groups (the weights are staged once per workgroup)
  long long per = cdivl(ngroups, 768);
  per = cdivl(per, ppb) * ppb;
  hipLaunchKernelGGL((conv_few4_kernel<FLIP, GATHER>), dim3((unsigned)cdivl(ngroups, per)), dim3(256), lds, s, x, w, bias, y, B, Cs,
                     H, W, N, (int)per, ldy, silu, gs);
  if (hipGetLastError() != hipSuccess) *rc = PEA_E_HIP;
  return true;
}

int launch_conv_in(const float* x, const float* w, const float* bias, bf16* y, int B, int Cin, int H, int W,
                   int Cout, hipStream_t s, int ldy, int silu) {
  if (ldy <= 0) ldy = Cout;
  {
    int rc;
    if (launch_conv_few4<false>(x, w, bias, y, B, Cin, H, W, Cout, ldy, silu, s, &rc)) return rc;
  }
  SHAPECHK(Cout % 8 == 0 && Cout / 8 <= 256 && Cin * 9 * Cout * 4 <= 160 * 1024, "conv_in: Cout=%d Cin=%d", Cout, Cin);
  if (Cin * 9 * Cout * 4 > 64 * 1024) {           // VAE decoder conv_in (4 -> 512): 72 KB of fp32 weights in LDS
    static bool attr_set = false;
    if (!attr_set) {
      HIPCHK(hipFuncSetAttribute((const void*)conv_in_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_set = true;
    }
  }
  const int nchunk = Cout / 8;
  const int ppb = 256 / nchunk;
  const int per = ppb * 8;
  const long long npix = (long long)B * H * W;
  hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)cdivl(npix, per)), dim3(256), (size_t)Cin * 9 * Cout * 4, s, x, w,
                     bias, y, B, Cin, H, W, Cout, per, ldy, silu);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

int launch_conv_in_gather(const float* lat, const float* mask, const float* masked, const float* w, const float* bias, bf16* y,
                          int B, int C, int lat_b, int cond_b, int H, int W, int Cout, hipStream_t s, int ldy) {
  if (ldy <= 0) ldy = Cout;
  const int Cs = 2 * C + 1;
  auto al16 = [](const float* p) { return p != nullptr && (((unsigned long long)p) & 15) == 0; };
  SHAPECHK(C > 0 && lat_b > 0 && cond_b > 0 && B % lat_b == 0 && B % cond_b == 0,
           "conv_in_gather: B=%d must be a multiple of latent_batch=%d and cond_batch=%d", B, lat_b, cond_b);
  SHAPECHK(W % 4 == 0 && Cout % 8 == 0 && Cout / 8 <= 256 && (size_t)Cs * 9 * Cout * 4 <= 160 * 1024,
           "conv_in_gather: W=%d must be a multiple of 4, Cout=%d of 8 (%d input channels)", W, Cout, Cs);
  SHAPECHK(al16(lat) && al16(mask) && al16(masked), "conv_in_gather: latents / mask / masked latents must be 16-byte aligned");
  int rc = PEA_OK;
  launch_conv_few4<false, true>(nullptr, w, bias, y, B, Cs, H, W, Cout, ldy, 0, s, &rc,
                                ConvGatherSrc{lat, mask, masked, C, lat_b, cond_b});
  if (rc != PEA_OK) pea_set_error("conv_in_gather: launch failed");
  return rc;
}

// conv_out: one wave per output pixel; lanes split the (tap, ci) reduction, 16-byte loads.
__global__ __launch_bounds__(256) void conv_out_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y,
                                                       int B, int Cin, int H, int W, int Cout) {
  const int lane = threadIdx.x & 63;
  const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pix >= (long long)B * H * W) return;
  const int xw = (int)(pix % W), yh = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // Cout <= 8 (UNet eps: 4, VAE moments: 8)
  const int cchunks = Cin / 8;
  for (int i = lane; i < 9 * cchunks; i += 64) {
    const int tap = i / cchunks, c8 = (i - tap * cchunks) * 8;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int iy = yh + ky - 1, ix = xw + kx - 1;
    if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
    const bf16x8 v = *(const bf16x8*)(x + (((long long)b * H + iy) * W + ix) * Cin + c8);
#pragma unroll
    for (int co = 0; co < 8; ++co) {
      if (co < Cout) {
        const float* wp = w + ((long long)co * 9 + tap) * Cin + c8;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += (float)v[j] * wp[j];
        acc[co] += a;
      }
    }
  }
#pragma unroll
  for (int co = 0; co < 8; ++co) {
    if (co >= Cout) break;
    const float r = wave_sum(acc[co]);
    if (lane == 0) y[(((long long)b * Cout + co) * H + yh) * W + xw] = r + bias[co];
  }
}

// conv_out on the matrix cores.  The GEMM is [pixels][9 Cin] x [9 Cin][Cout <= 8]: Cout fills at most half of a 16-wide
// MFMA, so the spare rows carry the LOW halves of the fp32 weights (w = hi + lo, both bf16: the fp32 weights of the layer
// are kept to 16 mantissa bits instead of being rounded to bf16) and one v_mfma_f32_16x16x32_bf16 multiplies 16 pixels x 32
// channels of one tap by both.  Weights (rows n = 4 q + r: hi parts in the first Cq = ceil(Cout / 4) quads, lo parts in
// the next Cq) are split once per workgroup into LDS, laid out so that a lane's fragment is one 16-byte read; the pixel
// operand comes straight from global memory (16 bytes per lane, the 9 taps of a pixel re-read through L1 / L2).
// A wave owns 4 strips of 16 consecutive pixels (one weight fragment feeds 4 MFMAs); 4 waves per workgroup, 46 KB of LDS
// for the UNet's 320 -> 4 (three workgroups per CU).
// The direct form below (one wave per pixel, weights re-read per pixel) took 232 us on the UNet's [8][128][128][320].
__global__ __launch_bounds__(256) void conv_out_mfma_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y,
                                                            int B, int Cin, int H, int W, int Cout) {
  extern __shared__ __attribute__((aligned(16))) char cosm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c32n = Cin / 32, ksteps = 9 * c32n;
  const int Cq = (Cout + 3) / 4;
  const int NR = 8 * Cq;                                    // weight rows kept in LDS: hi parts, then lo parts (the rest are zero)
  // ---- weights -> LDS: [kstep][g][n < NR][8] bf16
  for (int i = tid; i < ksteps * 4 * NR; i += 256) {
    const int n = i % NR, g = (i / NR) & 3, ks = i / (4 * NR);
    const int tap = ks / c32n, c0 = (ks - tap * c32n) * 32 + g * 8;
    const int part = n / (4 * Cq), co = n - part * 4 * Cq;
    bf16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (co < Cout) {
      const float* wp = w + ((long long)co * 9 + tap) * Cin + c0;
      const f32x4 w0 = *(const f32x4*)wp, w1 = *(const f32x4*)(wp + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float wv = j < 4 ? w0[j] : w1[j - 4];
        const float hi = (float)(bf16)wv;
        o[j] = (bf16)(part ? wv - hi : hi);
      }
    }
    *(bf16x8*)(cosm + (long long)i * 16) = o;
  }
  __syncthreads();
  const long long npix = (long long)B * H * W;
  const long long p0 = (long long)blockIdx.x * 256 + wave * 64;
  const int pr = lane & 15, g = lane >> 4;
  int py[4], px[4];
  long long pb[4];                                          // element offset of sample b
  bool pv[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
    const long long P = p0 + s4 * 16 + pr;
    pv[s4] = P < npix;
    const long long Pc = pv[s4] ? P : 0;
    px[s4] = (int)(Pc % W);
    py[s4] = (int)((Pc / W) % H);
    pb[s4] = (Pc / ((long long)W * H)) * H * W * Cin;
  }
  f32x4 acc[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) acc[s4] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool wrow = pr < NR;                                // lanes of the zero rows read a valid address and drop it
  const int wlane = g * NR + (wrow ? pr : 0);
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const bf16* src[4];
    bool ok[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int iy = py[s4] + ky - 1, ix = px[s4] + kx - 1;
      ok[s4] = pv[s4] && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      src[s4] = x + pb[s4] + ((long long)(ok[s4] ? iy : 0) * W + (ok[s4] ? ix : 0)) * Cin + g * 8;   // always a valid address
    }
    const char* wl = cosm + ((long long)tap * c32n * 4 * NR + wlane) * 16;
#pragma unroll 5
    for (int c = 0; c < c32n; ++c) {
      bf16x8 wf = *(const bf16x8*)(wl + c * (4 * NR * 16));
      wf = wrow ? wf : zero8;
      bf16x8 xf[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) xf[s4] = *(const bf16x8*)(src[s4] + c * 32);     // unconditional: the loads of an unrolled
#pragma unroll                                                                        // group leave back to back
      for (int s4 = 0; s4 < 4; ++s4) {
        const bf16x8 xv = ok[s4] ? xf[s4] : zero8;
        acc[s4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xv, acc[s4], 0, 0, 0);
      }
    }
  }
  // lane (pixel pr, quad g) holds rows n = 4 g + r: quads [0, Cq) = hi parts of couts 4 g + r, quads [Cq, 2 Cq) = lo parts
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float lo = __shfl(acc[s4][r], (lane + 16 * Cq) & 63, 64);
      const int co = 4 * g + r;
      if (g < Cq && co < Cout && pv[s4]) {
        const long long P = p0 + s4 * 16 + pr;
        const long long bq = P / ((long long)W * H), rem = P - bq * W * H;
        y[(bq * Cout + co) * H * W + rem] = acc[s4][r] + lo + bias[co];
      }
    }
  }
}

int launch_conv_out(const bf16* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W,
                    int Cout, hipStream_t s) {
  SHAPECHK(Cout <= 8 && Cin % 8 == 0, "conv_out: Cout<=8, Cin%%8");
  const long long pix = (long long)B * H * W;
  const size_t lds = (size_t)9 * (Cin / 32) * 4 * 8 * ((Cout + 3) / 4) * 16;       // [9 Cin / 32][4][8 or 16 rows][16 bytes]
  if (Cin % 32 == 0 && lds <= 160 * 1024) {
    if (lds > 64 * 1024) {
      static bool attr_set = false;
      if (!attr_set) {
        HIPCHK(hipFuncSetAttribute((const void*)conv_out_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
      }
    }
    hipLaunchKernelGGL(conv_out_mfma_kernel, dim3((unsigned)cdivl(pix, 256)), dim3(256), lds, s, x, w, bias, y, B, Cin, H, W, Cout);
    HIPCHK(hipGetLastError());
    return PEA_OK;
  }
  hipLaunchKernelGGL(conv_out_kernel, dim3((unsigned)cdivl(pix, 4)), dim3(256), 0, s, x, w, bias, y, B, Cin, H, W,
                     Cout);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// dgrad of conv_out: dx[b][y][x][ci] = sum_{co,ky,kx} dy[b][co][y+1-ky][x+1-kx] * w[co][ky][kx][ci]
__global__ void conv_out_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                      bf16* __restrict__ dx, int B, int Cin, int H, int W, int Cout) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cq = Cin / 8;
  const long long total = (long long)B * H * W * cq;
  if (idx >= total) return;
  const int c8 = (int)(idx % cq) * 8;
  const long long pix = idx / cq;
  const int xw = (int)(pix % W), yh = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int co = 0; co < Cout; ++co)
    for (int ky = 0; ky < 3; ++ky) {
      const int oy = yh + 1 - ky;
      if ((unsigned)oy >= (unsigned)H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ox = xw + 1 - kx;
        if ((unsigned)ox >= (unsigned)W) continue;
        const float g = dy[(((long long)b * Cout + co) * H + oy) * W + ox];
        const float* wp = w + ((long long)co * 9 + ky * 3 + kx) * Cin + c8;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += g * wp[j];
      }
    }
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)acc[j];
  *(bf16x8*)(dx + pix * Cin + c8) = o;
}

int launch_conv_out_dgrad(const float* dy, const float* w, bf16* dx, int B, int Cin, int H, int W, int Cout,
                          hipStream_t s) {
  {
    int rc;
    if (launch_conv_few4<true>(dy, w, nullptr, dx, B, Cout, H, W, Cin, Cin, 0, s, &rc)) return rc;
  }
  const long long total = (long long)B * H * W * (Cin / 8);
  hipLaunchKernelGGL(conv_out_dgrad_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, s, dy, w, dx, B, Cin,
                     H, W, Cout);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// out[m][n] (+)= sum_s partial[s][m][n]  (splits added in order: deterministic)
__global__ void splitk_reduce_kernel(const float* __restrict__ part, int nsplit, long long stride, bf16* __restrict__ out,
                                     int ldo, int M, int N, int accum) {
  const long long total = (long long)M * (N / 4);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / (N / 4)), n = (int)(i % (N / 4)) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < nsplit; ++s) {
      const f32x4 v = *(const f32x4*)(part + s * stride + (long long)m * N + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += v[j];
    }
    bf16* dst = out + (long long)m * ldo + n;
    bf16x4 o;
    if (accum) o = *(const bf16x4*)dst;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (bf16)(a[j] + (accum ? (float)o[j] : 0.f));
    *(bf16x4*)dst = o;
  }
}
int launch_splitk_reduce(const float* part, int nsplit, long long stride, bf16* out, int ldo, int M, int N, int accum,
                         hipStream_t s) {
  // the kernel moves 4 columns per thread (one 16-byte load, one 8-byte store): N % 4 columns would be dropped without a word
  SHAPECHK(M > 0 && N > 0 && nsplit >= 1 && N % 4 == 0 && ldo % 4 == 0 && ldo >= N && stride % 4 == 0,
           "splitk_reduce: M=%d N=%d ldo=%d nsplit=%d stride=%lld (N, ldo and stride multiples of 4, ldo >= N)", M, N, ldo, nsplit, stride);
  const long long total = (long long)M * (N / 4);
  const int grid = (int)(cdivl(total, 256) < 2048 ? cdivl(total, 256) : 2048);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid), dim3(256), 0, s, part, nsplit, stride, out, ldo, M, N, accum);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
