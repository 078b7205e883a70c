// Flash-style fused attention for head_dim 64 (SDXL: 10 heads x 4096 tokens, 20 heads x 1024
// tokens, cross-attention with <= 77 keys), forward + data-gradient backward.
//
// Replaces diffusers' AttnProcessor2_0 -> F.scaled_dot_product_attention inside the
// UNet calls of train_sdxl_zh.py:397,415 and its autograd backward.
//
// Forward / dQ kernels: a workgroup = 4 waves = 128 queries, each wave owns 32 queries.  The
// scores are computed TRANSPOSED, S^T = K . Q^T (v_mfma_f32_32x32x16_bf16 with K rows as the A
// operand), so a lane holds one query column and 32 keys in registers: the softmax row
// reduction is in-lane plus one cross-half shuffle, and the bf16-packed P^T accumulator is
// directly the B operand of O^T = V^T . P^T (no LDS round trip for P).  V^T fragments come from
// the row-major V tile in LDS through ds_read_b64_tr_b16 (hardware transpose read).
// dK/dV kernel: a wave owns 32 keys (key on the lane), loops over query tiles; P and dS
// accumulators feed dV^T = dO^T . P and dK^T = Q^T . dS directly; Q / dO tiles are read
// row-wise for S / dP and through the transpose read for the two gradient products.
// K/V (or Q/dO) tiles are 64 x 64 bf16 (128-byte rows) staged by LDS-DMA into a 2-deep ring
// with the same source-side XOR swizzle as gemm.hip.
// Cross-attention (<= 128 keys: the 77-token text context) has its own kernels with K / V resident in LDS for a
// workgroup's whole life: xattn_fwd_kernel; backward xattn_bwd3_kernel (<= 80 keys: S / dP / P / dS evaluated once by
// key-on-the-lane waves, dS handed to a dQ wave through an LDS image -- five products), xattn_bwd2_kernel (<= 96 keys:
// both orientations on specialised waves), xattn_bwd_kernel (round 3: any key count up to 128), each with an ordered
// fp32 split reduce over query ranges (attn_dkv_reduce_kernel).  Every output tile (O, dQ, dK, dV) leaves through a
// per-wave LDS image as whole 128-byte rows.
// Few queries (<= 32: the Resampler latents of the IP-Adapter "plus" files) over the union of two key sets under one softmax:
// attn_fewq_kernel shares out the KEYS among a workgroup's waves and merges their partials in a fixed order.
// Heat maps (the head-mean cross-attention probabilities of a layer, fp32 [B][Skv][Sq], no V / O / lse): xattn_maps_kernel deals
// the HEADS of a 32-query block over a workgroup's eight waves and adds their partial sums in a fixed order; its launcher, like the
// regional one, stands beside the decision table.
// StyleAligned shared self-attention (bottom of the file): attn_shared_kernel runs the forward loop of attn_q_body over the keys of
// a target sample and then over its reference's, with a second resident Q fragment set and a per-segment constant in the C operand
// of the S^T products; plain samples of the same launch run attn_q_body itself.  attn_adain_part_kernel / attn_adain_coef_kernel
// make the per-channel coefficients it reads.  Their launchers, too, stand beside the decision table.
// The four forward kernels with resident keys (xattn_fwd / _regions_fwd / _maps / _edit_fwd) are sequences of one set of building
// blocks that stands above xattn_fwd_kernel (Q stager, scores, key mask, one-shot softmax, value product, O image): one copy of
// the arithmetic whose bits the tests compare between them.  The kernels that stream keys through the ring with the query on the
// lane (attn_q_body as forward and as dQ role, attn_shared_body) are sequences of a second set that stands above attn_q_body (ring
// offsets, row-fragment product, tail mask, online-softmax step, P pack, transposed-fragment product, forward exit); the two with
// the key on the lane (attn_dkv_body, attn_colsum_kernel) share their preamble and row-constant DMA.
// The three backward cross-attention kernels take their per-workgroup context (unit range, operand rows of the head, key
// count, score factor) from xattn_ctx.  They still repeat, as text: K / V staging, the unit stage (stage_unit / fetch_o /
// unit_head), the key-on-the-lane task, the query-on-the-lane key-block step, and the dQ and dK / dV exits -- so a fix to
// one copy has to be carried to the others by hand.  Each of these was tried as a shared __forceinline__ helper; the table
// in profiles/EXPERIMENTS.md ("Cross-attention backward: one launcher, one context helper") says per piece whether it
// moved register counts (not wanted) or only the instruction order (open: needs a bit-identity and timing A/B on a GPU).
// Host side (bottom of the file): attn_decide_fwd / attn_decide_bwd turn a problem into an AttnPlan (which instantiations, grids,
// LDS bytes, in which order); attn_launch maps a plan's enumerator to its instantiation; launch_lds raises a kernel's dynamic-LDS
// limit once and launches it.
#include <stdlib.h>

#include "pea_kernels.h"

#define TILE_BYTES 8192   // 64 rows x 128 bytes
// raw v_exp_f32: exp2f() expands to a denormal-safe 5-instruction sequence; every argument here is <= 0 (scores
// minus a running max / the log-sum-exp), so a flushed denormal result is an exact zero after bf16 rounding anyway
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
#define LOG2E 1.4426950408889634f
// max over the two 32-lane halves of the wave (lane l and l ^ 32), in every lane: one v_permlane32_swap + one v_max.
// __shfl_xor(x, 32) goes through ds_bpermute_b32 -- six address instructions and an LDS round trip in the middle of the
// softmax's dependency chain (scores -> row max -> exp arguments), every key tile.  (The clang builtin folds
// max(swap(x, x)) away, hence the assembly; the s_nops are the data hazards of the swap.)
__device__ __forceinline__ float xhalf_max(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

// The softmax scale rides in the RESIDENT operand: the fragments a workgroup keeps in registers for its whole life (the
// queries of the forward / dQ role, the keys of the dK/dV role) are multiplied once by scale * log2(e), so every score
// leaves the MFMA already in the log2 domain and the row constant (running max, log-sum-exp) is the MFMA's C operand:
// p = exp2(acc) with no per-score FMA.  These loops are bound by vector issue (profiles/EXPERIMENTS.md, attention): the
// forward goes from fma + exp + add + 3/4 max + 1/2 cvt per score to exp + add + 1/2 max + 1/2 cvt.
// AttnP::q_prescaled (the product path: the Q|K|V / to_q projection's epilogue applies the factor to its fp32 accumulator,
// GemmP::qscale): Q arrives scaled, nothing is rounded twice, and the dK/dV role -- which streams Q -- needs no scaled K
// (dK = ln2 * dS^T Q').  Otherwise (operator-level calls with a plain Q) the resident fragments are scaled here, which
// rounds them to bf16 once more: relative 2^-9 per element, i.e. a log2-score error of about 1e-3 for unit-variance scores
// and proportionally more for large logits.
__device__ __forceinline__ bf16x8 scale_frag(bf16x8 f, float c) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)f[j] * c);
  return o;
}
// Running-max threshold of the forward (log2 units): the accumulated offset m_run of a query only moves when a tile's
// scores exceed it by more than this, so p <= 2^8 per score (fp32 sums and bf16's 8-bit mantissa keep their RELATIVE
// precision at any magnitude; nothing overflows) and the rescale branch -- subtract, rescale O and l, rebuild the C operand
// -- runs in the first tile and then almost never.  The result is exact for any threshold: O / l and lse do not depend on
// the offset used.  tests/test_ops_gpu.py forces the branch in a late tile (spiked key).
#define ATTN_MOVE_THR 8.0f

// XOR term of a tile row: the bits of (row >> 1) & 7 rotated so that rows r and r + 2 differ in bit 2.  Any bijection of
// (row >> 1) & 7 keeps the 16-byte row reads (ds_read_b128) conflict free; with this one the transposed reads
// (ds_read_b64_tr_b16: 32 lanes = 4 rows x 4 chunks x 8-byte halves) are conflict free too -- with the plain term rows r and
// r + 2 of such a read hit the same four chunks (2-way conflict: 25-32 % of the LDS cycles of these kernels were conflicts).
__device__ __forceinline__ int swz_x(int row) {
  const int x = (row >> 1) & 7;
  return ((x & 1) << 2) | (x >> 1);
}
__device__ __forceinline__ int swz_rc(int row, int col) {   // byte offset of element (row, col) in a tile
  return row * 128 + ((((col >> 3)) ^ swz_x(row)) << 4) + (col & 7) * 2;
}

// LDS-DMA issued through inline assembly.  With the builtin, hipcc's waitcnt pass knows that an LDS write is pending and puts
// `s_waitcnt vmcnt(0)` in front of the next LDS read it cannot prove disjoint -- every ds_read_b64_tr_b16 (an intrinsic
// without a memory operand) -- i.e. in the middle of the very iteration whose compute is meant to hide the prefetch of the
// next tile (forward: before the P.V reads; dQ role: before the first read).  The asm form is invisible to that pass; the
// loops order DMA and reads themselves (`s_waitcnt vmcnt(0)` + barrier at the end of every iteration).
// vmcnt(0) as the BUILTIN (expcnt / lgkmcnt left at their maxima): the waitcnt pass must see it, or it keeps believing
// that the prologue's global loads are outstanding and re-waits for them with counted vmcnt(N) inside the loop -- which, with
// DMA pieces it does not know about in flight, waits for those pieces instead.
#define WAIT_VM0()                           \
  do {                                       \
    __builtin_amdgcn_s_waitcnt(0x0F70);      \
    asm volatile("" ::: "memory");           \
  } while (0)
__device__ __forceinline__ unsigned lds_addr_u32(const void* p) {
  return (unsigned)(unsigned long long)p;      // a flat pointer into LDS is (shared aperture base << 32) | LDS byte offset
}
__device__ __forceinline__ void lds_dma16(const void* gsrc, const char* lds_dst) {     // 64 lanes x 16 bytes -> lds_dst[0..1023]
  const unsigned a = __builtin_amdgcn_readfirstlane(lds_addr_u32(lds_dst));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(a), "v"(gsrc) : "m0");
}
__device__ __forceinline__ void lds_dma4(const void* gsrc, const char* lds_dst) {      // 64 lanes x 4 bytes -> lds_dst[0..255]
  const unsigned a = __builtin_amdgcn_readfirstlane(lds_addr_u32(lds_dst));
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" ::"s"(a), "v"(gsrc) : "m0");
}

// A 64x64-tile source for the LDS-DMA in BUFFER form (buffer_load_dwordx4 ... offen lds): a buffer resource over the
// matrix (rows beyond `rows` read as zeros -- they are masked keys / ragged query rows), and this lane's two byte offsets
// inside a tile; the tile's first row goes into the scalar offset.  The 64-bit address form cost ~10 integer vector
// instructions per 1 KiB piece (row clamp, swizzle, 64-bit multiply-add), every key tile, in loops whose bound is the
// vector issue port that the MFMAs share.
typedef int i32x4 __attribute__((ext_vector_type(4)));
struct TileSrc {
  i32x4 rsrc;
  int voff[2];
  int row_bytes;
};
__device__ __forceinline__ TileSrc tile_src(const bf16* base, int ld, int rows, int wave, int lane) {
  TileSrc t;
  const unsigned long long a = (unsigned long long)base;
  t.rsrc[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  t.rsrc[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
  t.rsrc[2] = __builtin_amdgcn_readfirstlane((rows - 1) * ld * 2 + 128);      // num_records (bytes): last valid row's 128 bytes
  t.rsrc[3] = 0x00020000;
  t.row_bytes = ld * 2;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wave * 2 + j) * 8 + (lane >> 3);
    t.voff[j] = r * ld * 2 + (((lane & 7) ^ swz_x(r)) << 4);
  }
  return t;
}
// stage rows r0 .. r0+63 -> dst (LDS image of 64 rows x 128 bytes, source-side XOR swizzle); 4 waves x 2 pieces
__device__ __forceinline__ void stage_tile(const TileSrc& t, int r0, char* dst, int wave) {
  const int soff = __builtin_amdgcn_readfirstlane(r0 * t.row_bytes);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const unsigned a = __builtin_amdgcn_readfirstlane(lds_addr_u32(dst + (wave * 2 + j) * 1024));
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(a), "v"(t.voff[j]), "s"(t.rsrc), "s"(soff) : "m0");
  }
}

// MFMA A-operand fragment of T^T for the k-permuted accumulator-as-operand product:
// elements j=0..3 <- rows kbase+4h+j, j=4..7 <- rows kbase+8+4h+(j-4) of the LDS tile, column c0 + (lane&31)
template <bool USE_TR>
__device__ __forceinline__ bf16x8 read_transposed_frag(const char* tile, int kbase, int c0, int lane) {
  bf16x8 out;
  const int h = lane >> 5;
  if (USE_TR) {
    const int i = lane & 15;
    const int col = c0 + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
    const int row = kbase + 4 * h + (i >> 2);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)PEA_LDS(tile + swz_rc(row, col)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)PEA_LDS(tile + swz_rc(row + 8, col)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      short a = lo[j], b = hi[j];
      out[j] = *(bf16*)&a;
      out[4 + j] = *(bf16*)&b;
    }
  } else {
    const int col = c0 + (lane & 31);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = kbase + 8 * (j >> 2) + 4 * h + (j & 3);
      out[j] = *(const bf16*)(tile + swz_rc(row, col));
    }
  }
  return out;
}

// the same fragment from precomputed per-lane byte offsets of its two 8-row halves (see attn_q_body)
__device__ __forceinline__ bf16x8 read_transposed_frag_at(const char* lo_addr, const char* hi_addr) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)PEA_LDS(lo_addr));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)PEA_LDS(hi_addr));
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    short a = lo[j], b = hi[j];
    out[j] = *(bf16*)&a;
    out[4 + j] = *(bf16*)&b;
  }
  return out;
}

__device__ __forceinline__ bf16x8 read_row_frag(const char* tile, int row, int s, int h) {
  return *(const bf16x8*)(tile + row * 128 + ((((2 * s + h)) ^ swz_x(row)) << 4));
}

// Per-lane LDS byte offsets of the two fragment kinds inside a swizzled image, computed once per kernel.  rf[s]: the row
// fragment (ds_read_b128) of row lane & 31, k-slice s.  tr[db][hl]: the transposed fragment (read_transposed_frag_at) of
// column block db, 8-row half hl, of a 16-row k-slice.  The swizzle term of a row is unchanged by +16 / +32 rows, so every
// fragment address is (image base) + (one of these) + (a compile-time offset: 4096 per 32-row block for rf, 2048 per 16-row
// slice for tr): integer adds per key tile instead of one address computation per ds_read (45 of the ~200 VALU instructions
// of a tile of the VALU-bound forward loop were address arithmetic).
struct AttnFragOff { int rf[4], tr[2][2]; };
__device__ __forceinline__ AttnFragOff attn_frag_off(int lane) {
  AttnFragOff o;
  const int frow = lane & 31, fh = lane >> 5;
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) o.rf[s4] = frow * 128 + (((2 * s4 + fh) ^ swz_x(frow)) << 4);
  const int i16 = lane & 15, rr = 4 * fh + (i16 >> 2), cc = 16 * ((lane >> 4) & 1) + 4 * (i16 & 3);
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int hl = 0; hl < 2; ++hl) o.tr[db][hl] = swz_rc(rr + 8 * hl, db * 32 + cc);
  return o;
}

// A wave's 32 x 64 output block (O, dQ, dK, dV) leaves through an LDS image of its own.  The accumulator layout X^T has a row
// per lane -- acc[db][4g + j] = X^T[d = db * 32 + 8g + 4 fh + j][row = lane & 31] -- which written straight out is eight 8-byte
// stores per lane that each touch 32 different 128-byte lines; from the image every store instruction writes eight whole rows,
// 16 bytes per lane.  val(db, i): the fp32 value of element i of accumulator db (the caller's normalisation), rounded to bf16
// once here.  Rows row0 + r < nrows go to base[(row0 + r) * ld + 0..63]; accum: added to what is there (fp32 sum, one more
// rounding).  Two layouts of the image: 144-byte pitch (4 608 bytes), or XOR-swizzled at a 128-byte pitch (4 096 bytes: where
// the LDS total decides how many workgroups a CU holds); the 8-byte writes conflict two ways in either.
template <bool SWZ, class Val>
__device__ __forceinline__ void store_o_image(char* ost, int lane, Val val, bf16* base, int ld, int row0, int nrows, bool accum) {
  const int frow = lane & 31, fh = lane >> 5, r8 = lane >> 3, ch = lane & 7;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)val(db, 4 * g + j);
      if constexpr (SWZ) *(bf16x4*)(ost + frow * 128 + (((db * 4 + g) ^ swz_x(frow)) << 4) + fh * 8) = o;
      else *(bf16x4*)(ost + frow * 144 + (db * 32 + 8 * g + 4 * fh) * 2) = o;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i * 8 + r8;
    bf16x8 v = *(const bf16x8*)(SWZ ? ost + row * 128 + ((ch ^ swz_x(row)) << 4) : ost + row * 144 + ch * 16);
    if (row0 + row < nrows) {
      bf16* dst = base + (long long)(row0 + row) * ld + ch * 8;
      if (accum) {
        const bf16x8 old = *(const bf16x8*)dst;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16)((float)v[j] + (float)old[j]);
      }
      *(bf16x8*)dst = v;
    }
  }
}
template <class Val>
__device__ __forceinline__ void store_o_image_144(char* ost, int lane, Val val, bf16* base, int ld, int row0, int nrows, bool accum = false) {
  store_o_image<false>(ost, lane, val, base, ld, row0, nrows, accum);
}
template <class Val>
__device__ __forceinline__ void store_o_image_swz(char* ost, int lane, Val val, bf16* base, int ld, int row0, int nrows) {
  store_o_image<true>(ost, lane, val, base, ld, row0, nrows, false);
}

// XCD-aware workgroup order.  Workgroups are handed to the 8 XCDs round-robin in dispatch order (x fastest), so the
// query blocks of one head -- which all stream that head's K and V (or Q and dO) -- would land on 8 different L2s and
// every XCD would see every head: a working set of all heads per 4-MB L2.  Remapped, XCD x runs a contiguous range of
// (batch, head, block) triples, i.e. whole heads, and a head's operands are read into one L2 once.
// xcd_contiguous: the rule on a range of `total` workgroups -- dispatch position -> position in an order where each XCD runs one
// contiguous stretch (positions are dealt to the 8 XCDs round-robin).
__device__ __forceinline__ unsigned xcd_contiguous(unsigned lin, unsigned total) {
  const unsigned q = total >> 3, r = total & 7, xcd = lin & 7, j = lin >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
__device__ __forceinline__ void attn_block_coords(int& bx, int& by, int& bz) {
  const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z;
  const unsigned lin = xcd_contiguous(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx * gy * gz);
  bx = (int)(lin % gx);
  const unsigned t = lin / gx;
  by = (int)(t % gy);
  bz = (int)(t / gy);
}

// ----------------------------------------------------------------------------- streamed-key building blocks, query on the lane
// What attn_q_body (forward and dQ role) and attn_shared_body are made of: a wave's 32 queries (query lane & 31 on the lane, both
// half-waves) against the 64-row tile in the current stage of the LDS-DMA ring.  One copy of the arithmetic, so that the bit-equality
// the tests assert between these kernels holds by construction.  In an accumulator of the first product slot r of half-wave fh of
// block kb is tile row kb * 32 + (r & 3) + 8 (r >> 2) + 4 fh.
// The fragment offsets of one stage: row fragments from ring byte sb on (the stage), transposed fragments from ring byte tb on (the
// first sub-tile that the second product reads).
__device__ __forceinline__ AttnFragOff attn_ring_off(const AttnFragOff& fo, int sb, int tb) {
  AttnFragOff o;
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) o.rf[s4] = fo.rf[s4] + sb;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int hl = 0; hl < 2; ++hl) o.tr[db][hl] = fo.tr[db][hl] + tb;
  return o;
}
// First product: acc^T[row][q] = c0 + T . B^T, summed over the ND 64 x 64 sub-tiles that begin `sub` bytes into the stage, bf[nd]
// the resident B fragments of sub-tile nd (S^T = K . Q^T; dP^T = V . dO^T).  All row fragments of a sub-tile are requested before
// its first MFMA: read-wait-MFMA per fragment (what the compiler emits for the fused loop under a 128-register budget) exposes one
// LDS latency per MFMA, i.e. the matrix pipe runs at a quarter of its rate in this phase.
template <int ND>
__device__ __forceinline__ void attn_rows_product(const char* smem, const AttnFragOff& ro, int sub, const bf16x8 (*bf)[4], const f32x16& c0,
                                                  f32x16 (&acc)[2]) {
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) {
    bf16x8 fr[2][4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 4; ++s) fr[kb][s] = *(const bf16x8*)(smem + ro.rf[s] + (sub + nd * TILE_BYTES + kb * 4096));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[kb][s], bf[nd][s], (nd == 0 && s == 0) ? c0 : acc[kb], 0, 0, 0);
  }
}
// keys at or past kmax of the tile that begins at key kv0 score -inf (P = exp2(-inf) = 0); the caller asks only for a tile that holds one
__device__ __forceinline__ void attn_mask_tail(f32x16 (&sacc)[2], int kv0, int kmax, int fh) {
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kv0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
      sacc[kb][r] = key < kmax ? sacc[kb][r] : -INFINITY;
    }
}
// One tile's step of the online softmax in the log2 domain.  sacc holds (scaled score - m_run): the offset came in through the MFMA's
// C operand, so p = exp2(sacc) as it stands.  Only when some query's tile maximum exceeds its offset by more than ATTN_MOVE_THR
// (always in the first tile) does the wave take the rescale branch (exact for any threshold).  The ORDER is the contract between the
// kernels:
//   the maximum starts at max(sacc[0][0], sacc[1][0]) and takes max(max(mx, sacc[0][r]), sacc[1][r]) for r = 1 .. 15 (one v_max3 per
//   pair of scores); the half-wave combine (xhalf_max) comes last;
//   moved = (first || mx > ATTN_MOVE_THR), FINITE: and mx > -inf.  If any lane moved: mrel = moved ? mx : 0; sacc -= mrel;
//   alpha = first ? 0 : exp2(-mrel) (O and l are still zero before the first valid key); l_run *= alpha; every oacc *= alpha;
//   m_run += mrel; rowc = rowc_of(m_run) in all 16 slots -- the kernel's C operand of the next score product;
//   e = exp2(sacc) in place; their sum starts at 0 and adds in (kb, r) order; l_run += that sum.
// first: this lane's query has not seen a valid key yet.  FINITE (the text instance, where whole tiles can be masked): a tile whose
// maximum is -inf moves nothing -- with m_run = -inf the next tile's scores would be absorbed by the C operand.  Returns mx.
template <bool FINITE, int NACC, class RowC>
__device__ __forceinline__ float attn_online_softmax(f32x16 (&sacc)[2], bool first, float& m_run, float& l_run, f32x16 (&oacc)[NACC],
                                                     f32x16& rowc, RowC rowc_of) {
  float mx = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, sacc[0][r]), sacc[1][r]);
  mx = xhalf_max(mx);
  const bool moved = (first || mx > ATTN_MOVE_THR) && (!FINITE || mx > -INFINITY);
  if (__any(moved)) {
    const float mrel = moved ? mx : 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[kb][r] -= mrel;
    const float alpha = first ? 0.f : fast_exp2(-mrel);
    l_run *= alpha;
#pragma unroll
    for (int i = 0; i < NACC; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
    m_run += mrel;
#pragma unroll
    for (int r = 0; r < 16; ++r) rowc[r] = rowc_of(m_run);
  }
  float ls = 0.f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = fast_exp2(sacc[kb][r]);
      sacc[kb][r] = e;
      ls += e;
    }
  l_run += ls;
  return mx;
}
// P^T (forward) or dS^T (dQ role) rounded to bf16, as the B-operand fragments of the second product (k-permuted)
__device__ __forceinline__ void attn_pack_p(const f32x16 (&sacc)[2], bf16x8 (&pf)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[ks][j] = (bf16)sacc[ks >> 1][8 * (ks & 1) + j];
}
// Second product: acc^T[d][q] += T^T[d][row] P^T[row][q] for one 64 x 64 sub-tile, `sub` bytes past the stage's transposed-fragment
// base (O^T += V^T P^T; dQ^T += K^T dS^T).  All eight transposed fragments first (the score registers are free by now), then the
// MFMAs.  The gathering instances (USE_TR = false) read the same fragments element by element from the tile at Ts.
template <bool USE_TR>
__device__ __forceinline__ void attn_cols_product(const char* smem, const AttnFragOff& ro, int sub, const char* Ts, int lane,
                                                  const bf16x8 (&pf)[4], f32x16* acc) {
  bf16x8 tfr[4][2];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      if constexpr (USE_TR)
        tfr[ks][db] = read_transposed_frag_at(smem + ro.tr[db][0] + (sub + ks * 2048), smem + ro.tr[db][1] + (sub + ks * 2048));
      else tfr[ks][db] = read_transposed_frag<false>(Ts, ks * 16, db * 32, lane);
    }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int db = 0; db < 2; ++db) acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfr[ks][db], pf[ks], acc[db], 0, 0, 0);
}
// Forward exit: l over both half-waves (without an LDS round trip), the row's lse where the caller wants it (lse non-null, and
// lse_lane on the one lane that writes), and the NO chunks of O = oacc / l through the wave's LDS image `ost` as whole 128-byte rows.
// oacc[2 * no + db][4g + j] = O^T[d = no * 64 + db * 32 + 8g + 4 fh + j][q = lane & 31]
template <int NO>
__device__ __forceinline__ void attn_fwd_exit(const f32x16 (&oacc)[2 * NO], float m_run, float l_run, float* lse, long long lse_i,
                                              bool lse_lane, char* ost, int lane, bf16* Ob, int ldo, int q0, int Sq) {
  float la = l_run, lb = l_run;
  swap_halves32(la, lb);
  const float l_tot = la + lb;
  const float inv = 1.f / l_tot;
  if (lse && lse_lane) lse[lse_i] = (m_run + log2f(l_tot)) * 0.6931471805599453f;
#pragma unroll
  for (int no = 0; no < NO; ++no)
    store_o_image_144(ost, lane, [&](int db, int i) { return oacc[2 * no + db][i] * inv; }, Ob + no * 64, ldo, q0, Sq);
}

// ============================================================================= forward / dQ
// MODE 0: forward (writes O, lse).  MODE 1: dQ (reads dO, lse, delta; writes dQ).
// ND = head_dim / 64 (heads are stored padded to ND*64 columns; the padding columns of Q/K/V are zero).  Every
// K/V (Q/dO) tile is kept as ND sub-tiles of 64 x 64 so all LDS images stay 128-byte-row images.
// MODE 0 produces all ND output chunks in one pass; MODE 1 produces ONE 64-wide chunk of dQ per workgroup
// (blockIdx.x enumerates query blocks x ND chunks) so its register budget does not grow with ND.
// WRITE_DELTA: the dQ pass also stores delta[q] for the dK/dV kernel launched behind it (two-launch form); the fused
// backward launch gets delta from attn_delta_kernel instead (both roles run concurrently there)
template <int MODE, bool USE_TR, int ND, bool TXT, bool WRITE_DELTA>
__device__ __forceinline__ void attn_q_body(const AttnP& p, char* smem, int blk_x, int head, int b) {
  constexpr int STG = 2 * ND * TILE_BYTES;                       // smem: [2 stages][K sub-tiles ND | V sub-tiles ND]
  constexpr int NO = MODE == 0 ? ND : 1;                         // output chunks held by this workgroup
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qblk = MODE == 0 ? blk_x : blk_x / ND;
  const int chunk = MODE == 0 ? 0 : blk_x % ND;                  // dQ output chunk
  const int q0 = qblk * 128 + wave * 32;
  const int frow = lane & 31, fh = lane >> 5;
  const float c = p.scale * LOG2E;

  const bf16* Qb = p.Q + (long long)b * p.Sq * p.ldq + head * 64 * ND;
  const bf16* Kb = p.K + (long long)b * p.Skv * p.ldk + head * 64 * ND;
  const bf16* Vb = p.V + (long long)b * p.Skv * p.ldv + head * 64 * ND;

  int qrow = q0 + frow;
  const bool qvalid = qrow < p.Sq;
  qrow = qvalid ? qrow : p.Sq - 1;
  bf16x8 qf[ND][4], dof[MODE == 1 ? ND : 1][4];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[nd][s] = *(const bf16x8*)(Qb + (long long)qrow * p.ldq + nd * 64 + 16 * s + 8 * fh);
      if (!p.q_prescaled && !TXT) qf[nd][s] = scale_frag(qf[nd][s], c);
    }
  // TXT with a plain Q: the factor is applied to the fp32 scores (qs), not rounded into the Q fragment.  A causal row 0, or a
  // sample with one valid key, has lse = that one logit, and the 2^-9 of a bf16 Q * scale * log2(e) on it is all of the error
  // (measured 2.4e-3 .. 4.6e-3 on unit inputs, against 1e-6 this way); with many keys it averages out.  The C operand then
  // carries -m_run / qs.  A prescaled Q has qs = 1: the same bits as before.
  [[maybe_unused]] const float qs = (TXT && !p.q_prescaled) ? c : 1.f;
  [[maybe_unused]] const float inv_qs = (TXT && !p.q_prescaled) ? 1.f / c : 1.f;
  float lse2 = 0.f, dlt = 0.f;
  if (MODE == 1) {
    const bf16* dOb = p.dO + (long long)b * p.Sq * p.lddo + head * 64 * ND;
#pragma unroll
    for (int nd = 0; nd < ND; ++nd)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        dof[nd][s] = *(const bf16x8*)(dOb + (long long)qrow * p.lddo + nd * 64 + 16 * s + 8 * fh);
    const long long li = ((long long)b * p.H + head) * p.Sq + qrow;
    if (!WRITE_DELTA) {
      // fused launch: attn_delta_kernel ran in front of this grid and left -delta[q] and -lse[q] * log2(e) for the dK/dV role;
      // the dQ role takes the same two floats instead of re-reading its O row (4 x 16 bytes per lane over 32 lines per
      // instruction) and redoing the 64 multiply-adds -- bit-identical inputs for both roles
      dlt = -p.delta[li];
      lse2 = -p.delta[(long long)p.B * p.H * p.Sq + li];
    } else {
      lse2 = p.lse[li] * LOG2E;
      // delta[q] = sum_d dO[q][d] * O[q][d], computed here from the dO fragments already in registers (one extra read of
      // the O row) instead of a separate kernel; the dK/dV kernel, launched after this one, reads it from p.delta
      const bf16* Ob = p.O + (long long)b * p.Sq * p.ldo + head * 64 * ND;
      float dsum = 0.f;
#pragma unroll
      for (int nd = 0; nd < ND; ++nd)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bf16x8 o = *(const bf16x8*)(Ob + (long long)qrow * p.ldo + nd * 64 + 16 * s + 8 * fh);
#pragma unroll
          for (int j = 0; j < 8; ++j) dsum += (float)dof[nd][s][j] * (float)o[j];
        }
      { float da = dsum, db = dsum; swap_halves32(da, db); dsum = da + db; }
      dlt = dsum;
      if (WRITE_DELTA && qvalid && fh == 0 && chunk == 0) {       // row constants of the dK/dV kernel (see attn_delta_kernel)
        p.delta[li] = -dsum;
        p.delta[(long long)p.B * p.H * p.Sq + li] = -lse2;
      }
    }
  }
  // dP^T accumulates ON TOP OF -delta[q] (the MFMA's C operand: this lane's query, the same value in all 16 registers, for
  // every key tile), so dS^T = P^T (dP^T - delta) costs one multiply per score; the softmax scale is applied once, to the
  // finished dQ^T.  The backward loops are VALU-issue-bound (a probe with a 4-cycle stand-in for the 8-cycle v_exp_f32 ran
  // 11 % faster): per score fma + exp + mul + half a conversion instead of fma + exp + sub + mul + mul + conversion.
  // rowc: the C operand of the S^T products -- forward: -m_run (the accumulated offset of this lane's query, 0 before the
  // first tile); dQ role: -lse2 (so that P^T = exp2(S^T) directly)
  f32x16 negd, rowc;
#pragma unroll
  for (int r = 0; r < 16; ++r) { negd[r] = -dlt; rowc[r] = MODE == 1 ? -lse2 : 0.f; }

  f32x16 oacc[2 * NO];
#pragma unroll
  for (int i = 0; i < 2 * NO; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
  float m_run = 0.f, l_run = 0.f;            // m_run: log2-domain offset the P values of this query are relative to
  [[maybe_unused]] bool seen = false;        // TXT instance: this lane's query has met a key that is not masked

  TileSrc ksrc[ND], vsrc[ND];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) {
    ksrc[nd] = tile_src(Kb + nd * 64, p.ldk, p.Skv, wave, lane);
    vsrc[nd] = tile_src(Vb + nd * 64, p.ldv, p.Skv, wave, lane);
  }
  auto stage_kv = [&](char* dst, int r0) {
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) {
      stage_tile(ksrc[nd], r0, dst + nd * TILE_BYTES, wave);
      stage_tile(vsrc[nd], r0, dst + (ND + nd) * TILE_BYTES, wave);
    }
  };
  const int nt = (p.Skv + 63) / 64;
  // read ONCE, before the loop: a global load inside it makes the compiler wait for vmcnt(0) there, i.e. for the DMA
  // prefetch of the next tile as well
  const int skv_all = __builtin_amdgcn_readfirstlane(p.kv_len ? p.kv_len[b] : p.Skv);
  stage_kv(smem, 0);
  WAIT_VM0();
  __syncthreads();

  const AttnFragOff fo = attn_frag_off(lane);

  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) stage_kv(smem + (cur ^ 1) * STG, (t + 1) * 64);
    const char* Ks = smem + cur * STG;
    const char* Vs = Ks + ND * TILE_BYTES;
    const int sb = cur * STG;                  // transposed fragments -- fwd: the V sub-tiles; dQ: this chunk's K sub-tile
    const AttnFragOff ro = attn_ring_off(fo, sb, sb + (MODE == 0 ? ND * TILE_BYTES : chunk * TILE_BYTES));

    // S^T[key][q] = K . Q^T  (sum over the ND sub-tiles of the head dimension)
    f32x16 sacc[2];
    attn_rows_product<ND>(smem, ro, 0, qf, rowc, sacc);
    const int kv0 = t * 64;
    if constexpr (MODE == 0) {
      // keys beyond Skv are masked only in the tile that contains them.
      // TXT (text encoders, inference): causal mask and / or a per-sample key count (padding) -- a separate instance
      // so the UNet's kernel keeps its register budget
      int skv_b = p.Skv;
      if constexpr (TXT) skv_b = skv_all;
      if constexpr (TXT) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[kb][r] *= qs;              // (K . Q^T - m_run / qs) qs: the log2 domain
        if (p.bias) {
          // additive score bias (T5 relative positions), given in the log2 domain with a row pitch of 64 * ceil(Skv / 64)
          const int pitch = ((p.Skv + 63) >> 6) << 6;
          const float* brow = p.bias + ((long long)head * p.Sq + qrow) * pitch + kv0 + 4 * fh;
#pragma unroll
          for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const f32x4 bv = *(const f32x4*)(brow + kb * 32 + 8 * g);
#pragma unroll
              for (int j = 0; j < 4; ++j) sacc[kb][4 * g + j] += bv[j];
            }
        }
      }
      const bool boundary = (TXT && p.causal) || kv0 + 64 > skv_b;   // wave-uniform
      if (boundary) {
        int kmax = skv_b;
        if constexpr (TXT) kmax = p.causal ? min(skv_b, qrow + 1) : skv_b;
        attn_mask_tail(sacc, kv0, kmax, fh);
      }
      // "first" = this query has not seen a valid key yet.  The UNet instance always has one in tile 0 (Skv >= 1, checked on the
      // host).  TXT: a per-sample key count of 0 (or a padded context shorter than a tile boundary) leaves whole tiles at -inf;
      // the offset then stays 0 -- with m_run = -inf the next tile's scores would be absorbed by the C operand and every key
      // would come out with weight 1 -- and is set by the first tile with a finite maximum (a row without any key ends as 0 / 0).
      const float mx = attn_online_softmax<TXT>(sacc, TXT ? !seen : t == 0, m_run, l_run, oacc, rowc,
                                                [&](float m) { return TXT ? -m * inv_qs : -m; });
      if constexpr (TXT) seen = seen || mx > -INFINITY;
    } else {
      // P^T = exp2(S^T) (scale in Q, -lse2[q] in the C operand);  dP^T = V . dO^T;  dS^T = P^T (dP^T - delta[q]) scale
      const int skv_b = skv_all;                                 // per-sample valid keys (padded contexts)
      f32x16 dpacc[2];
      attn_rows_product<ND>(smem, ro, ND * TILE_BYTES, dof, negd, dpacc);
      if (kv0 + 64 > skv_b) {                                    // uniform: only the tile that holds masked keys
        attn_mask_tail(sacc, kv0, skv_b, fh);
        __builtin_amdgcn_sched_barrier(0);                         // (keeps the compiler from if-converting the block into 64 selects per tile)
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = fast_exp2(sacc[kb][r]);                 // S^T came out of the MFMA as c s - lse2 (C operand)
          sacc[kb][r] = pr * dpacc[kb][r];                         // = P (dP - delta); x scale in the epilogue
        }
    }
    bf16x8 pf[4];   // P^T (fwd) or dS^T (dQ) as B-operand fragments, k-permuted
    attn_pack_p(sacc, pf);
    // fwd: O^T[d][q] += V^T[d][key] P^T[key][q]  (all chunks);   dQ: dQ^T[d][q] += K^T[d][key] dS^T[key][q]  (one chunk)
#pragma unroll
    for (int no = 0; no < NO; ++no)
      attn_cols_product<USE_TR>(smem, ro, no * TILE_BYTES, MODE == 0 ? Vs + no * TILE_BYTES : Ks + chunk * TILE_BYTES, lane, pf, oacc + 2 * no);
    WAIT_VM0();
    __syncthreads();
  }

  // the wave's image: its own 4.5 KiB of the K / V ring, which every wave has left behind the loop's last barrier
  char* const ost = smem + wave * (32 * 144);
  if constexpr (MODE == 0)
    attn_fwd_exit<NO>(oacc, m_run, l_run, p.lse, ((long long)b * p.H + head) * p.Sq + qrow, qvalid && fh == 0, ost, lane,
                      p.O + (long long)b * p.Sq * p.ldo + head * 64 * ND, p.ldo, q0, p.Sq);
  else   // the softmax scale is applied once, to the finished dQ^T
    store_o_image_144(ost, lane, [&](int db, int i) { return oacc[db][i] * p.scale; }, p.dQ + (long long)b * p.Sq * p.lddq + head * 64 * ND + chunk * 64,
                      p.lddq, q0, p.Sq, p.accum_dq != 0);
}

template <int MODE, bool USE_TR, int ND, bool TXT = false>
__global__ __launch_bounds__(256, (ND == 1 ? (MODE == 0 ? 3 : 2) : 1)) void attn_q_kernel(const AttnP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int blk_x, head, b;
  attn_block_coords(blk_x, head, b);
  attn_q_body<MODE, USE_TR, ND, TXT, true>(p, smem, blk_x, head, b);
}

// ----------------------------------------------------------------------------- streamed-query building blocks, key on the lane
// What attn_dkv_body and attn_colsum_kernel share: a workgroup = 4 waves = 128 keys, a wave owns 32 (key lane & 31 on the lane, both
// half-waves); 64-query tiles stream through the ring with their per-row constants beside them.  (The resident key fragments and
// the row fragments + C operand of a 32-query block stay each kernel's own text: as blocks they moved attn_dkv_body's register
// counts -- profiles/EXPERIMENTS.md, "Streamed-key attention: one tile loop".)
// A lane's key: k0 the wave's first; kstored: the lane's row exists in K / V -- a lane past the end computes on the last stored
// row (krow) and stores nothing; wave_active: the wave holds any key at all (wave-uniform).
struct AttnKeyLane { int k0, krow; bool kstored, wave_active; };
__device__ __forceinline__ AttnKeyLane attn_key_lane(int kblk, int wave, int frow, int Skv) {
  AttnKeyLane k;
  k.k0 = kblk * 128 + wave * 32;
  k.kstored = k.k0 + frow < Skv;
  k.krow = k.kstored ? k.k0 + frow : Skv - 1;
  k.wave_active = k.k0 < Skv;
  return k;
}
// the 64 per-row constants of the query tile at row r0 (src[r0 .. r0 + 63]; rows at or past rmax repeat row rmax - 1) -> dst[0..255]
// by LDS-DMA, 4 bytes per lane of the calling wave
__device__ __forceinline__ void stage_rowconst(const float* src, int r0, int rmax, char* dst, int lane) {
  int r = r0 + lane;
  r = r < rmax ? r : rmax - 1;
  lds_dma4(src + r, dst);
}

// ============================================================================= dK / dV
// workgroup = 4 waves = 128 keys (wave owns 32, key on the lane); loops over 64-query tiles.  ONE 64-wide chunk of
// dK/dV per workgroup: blockIdx.x enumerates (key block, query split, chunk).
// With p.nsplit > 1 (cross-attention: few keys, many queries) blockIdx.x also enumerates query ranges and the
// block writes fp32 partial dK/dV to p.dkv_part[split][b][h][key][2][64*ND]; attn_dkv_reduce_kernel adds the
// splits in order (deterministic, no atomics).
template <bool USE_TR, int ND>
__device__ __forceinline__ void attn_dkv_body(const AttnP& p, char* smem, int blk_x, int head, int b) {
  constexpr int STG = 2 * ND * TILE_BYTES + 512;                 // smem: [2 stages][Q sub-tiles | dO sub-tiles | lse,delta]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsplit = p.nsplit > 1 ? p.nsplit : 1;
  const int chunk = blk_x % ND;
  const int bx = blk_x / ND;
  const int kblk = bx / nsplit, split = bx - kblk * nsplit;
  const int frow = lane & 31, fh = lane >> 5;
  const auto [k0, krow, kstored, wave_active] = attn_key_lane(kblk, wave, frow, p.Skv);
  const float c = p.scale * LOG2E;

  const bf16* Qb = p.Q + (long long)b * p.Sq * p.ldq + head * 64 * ND;
  const bf16* dOb = p.dO + (long long)b * p.Sq * p.lddo + head * 64 * ND;
  const bf16* Kb = p.K + (long long)b * p.Skv * p.ldk + head * 64 * ND;
  const bf16* Vb = p.V + (long long)b * p.Skv * p.ldv + head * 64 * ND;
  // row constants written by attn_delta_kernel (or the dQ pass): -delta[q] and -lse[q] * log2(e)
  const float* dltb = p.delta + ((long long)b * p.H + head) * p.Sq;
  const float* lseb = dltb + (long long)p.B * p.H * p.Sq;

  const int skv_b = p.kv_len ? p.kv_len[b] : p.Skv;   // keys >= skv_b are padding: P = 0, so their dK = dV = 0
  const bool kvalid = k0 + frow < skv_b;
  bf16x8 kf[ND][4], vf[ND][4];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      // K is only the operand of S here (dK^T = Q^T dS uses the staged Q tiles): it carries scale * log2(e)
      kf[nd][s] = *(const bf16x8*)(Kb + (long long)krow * p.ldk + nd * 64 + 16 * s + 8 * fh);
      if (!p.q_prescaled) kf[nd][s] = scale_frag(kf[nd][s], c);        // (a prescaled Q tile already carries the factor)
      vf[nd][s] = *(const bf16x8*)(Vb + (long long)krow * p.ldv + nd * 64 + 16 * s + 8 * fh);
    }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] = dv[i][r] = 0.f;
  const bool all_valid = __all(kvalid);        // wave-uniform: no padding key among this wave's 32

  TileSrc qsrc[ND], dosrc[ND];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) {
    qsrc[nd] = tile_src(Qb + nd * 64, p.ldq, p.Sq, wave, lane);
    dosrc[nd] = tile_src(dOb + nd * 64, p.lddo, p.Sq, wave, lane);
  }
  auto stage_q = [&](char* dst, int r0) {
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) {
      stage_tile(qsrc[nd], r0, dst + nd * TILE_BYTES, wave);
      stage_tile(dosrc[nd], r0, dst + (ND + nd) * TILE_BYTES, wave);
    }
    if (wave == 0) {                                     // the tile's row constants: lse, then delta
      stage_rowconst(lseb, r0, p.Sq, dst + 2 * ND * TILE_BYTES, lane);
      stage_rowconst(dltb, r0, p.Sq, dst + 2 * ND * TILE_BYTES + 256, lane);
    }
  };
  const int nt_all = (p.Sq + 63) / 64;
  const int tps = (nt_all + nsplit - 1) / nsplit;            // query tiles per split
  const int t_begin = split * tps;
  const int nt = min(nt_all, t_begin + tps);
  if (t_begin < nt) stage_q(smem, t_begin * 64);
  WAIT_VM0();
  __syncthreads();

  for (int t = t_begin; t < nt; ++t) {
    const int cur = (t - t_begin) & 1;
    if (t + 1 < nt) stage_q(smem + (cur ^ 1) * STG, (t + 1) * 64);
    const char* Qs = smem + cur * STG;
    const char* dOs = Qs + ND * TILE_BYTES;
    const float* rc = (const float*)(Qs + 2 * ND * TILE_BYTES);
    if (t * 64 + 64 > p.Sq) {
      // ragged last tile (uniform, once per workgroup): the staged rows >= Sq repeat row Sq-1; give them -lse*log2e = -inf
      // (P = exp2(-inf) = 0) so the loop below needs no per-row predicate
      if (wave == 0 && t * 64 + lane >= p.Sq) {
        float* rw = (float*)(Qs + 2 * ND * TILE_BYTES);
        rw[lane] = -INFINITY;
        rw[64 + lane] = 0.f;
      }
      __syncthreads();
    }
    if (wave_active) {
      // S[q][key] = Q . K^T ; dP[q][key] = dO . V^T   (rows q in registers, key on the lane).  Both accumulations start
      // from a C operand instead of zero -- the staged row constants (row q = register index: the four 16-byte LDS loads ARE
      // the MFMA's C operand): S from -lse[q] * log2(e) (-inf on the lane of a padding key: P = 0 without a select per
      // score), dP from -delta[q].  With scale * log2(e) in the K fragments, P = exp2(S) as the MFMA leaves it.
      // LDS reads run one step ahead of the MFMAs that consume them (registers: two buffers of row fragments, two of
      // transposed fragments): as read -> wait -> MFMA pairs (what the fused loop compiled to) every pair of MFMAs stood
      // behind an LDS round trip, and with two waves per SIMD nothing covers it -- a key tile took 2.6 k cycles of its SIMD
      // for 1 k cycles of matrix work.
      f32x16 sacc[2], dpacc[2];
      bf16x8 rq[2][ND * 4], rd[2][ND * 4];
      auto load_rows = [&](int buf, int qb) {
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            rq[buf][nd * 4 + s] = read_row_frag(Qs + nd * TILE_BYTES, qb * 32 + frow, s, fh);
            rd[buf][nd * 4 + s] = read_row_frag(dOs + nd * TILE_BYTES, qb * 32 + frow, s, fh);
          }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 d4 = *(const f32x4*)(rc + 64 + qb * 32 + 8 * g + 4 * fh);
          const f32x4 l4 = *(const f32x4*)(rc + qb * 32 + 8 * g + 4 * fh);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dpacc[qb][4 * g + j] = d4[j];
            sacc[qb][4 * g + j] = l4[j];
          }
        }
      };
      bf16x8 dot[2][2][2], qt[2][2][2];          // [k-slice pair][kk][db]
      auto load_tr = [&](int bt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dot[bt][kk][db] = read_transposed_frag<USE_TR>(dOs + chunk * TILE_BYTES, (2 * bt + kk) * 16, db * 32, lane);
            qt[bt][kk][db] = read_transposed_frag<USE_TR>(Qs + chunk * TILE_BYTES, (2 * bt + kk) * 16, db * 32, lane);
          }
      };
      load_rows(0, 0);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        if (qb == 1) load_rows(1, 1);
        __builtin_amdgcn_sched_barrier(0);
        if (!all_valid) {
#pragma unroll
          for (int r = 0; r < 16; ++r) sacc[qb][r] = kvalid ? sacc[qb][r] : -INFINITY;
        }
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            sacc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rq[qb][nd * 4 + s], kf[nd][s], sacc[qb], 0, 0, 0);
            dpacc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rd[qb][nd * 4 + s], vf[nd][s], dpacc[qb], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      bf16x8 pfr[4], dsfr[4];
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * g + j;
            const float pr = fast_exp2(sacc[qb][r]);
            const float ds = pr * dpacc[qb][r];                // P (dP - delta); x scale on the finished dK
            const int ks = qb * 2 + (g >> 1), e = (g & 1) * 4 + j;
            pfr[ks][e] = (bf16)pr;
            dsfr[ks][e] = (bf16)ds;
          }
        }
      // dV^T[d][key] += dO^T[d][q] P[q][key] ;  dK^T[d][key] += Q^T[d][q] dS[q][key]   (d in this block's chunk)
      // two k-slices (8 transposed fragments = 32 registers) per batch of 8 MFMAs; the second batch's fragments are read
      // while the first batch's MFMAs run
      __builtin_amdgcn_sched_barrier(0);
      load_tr(0);
      load_tr(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot[bt][kk][db], pfr[2 * bt + kk], dv[db], 0, 0, 0);
            dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt[bt][kk][db], dsfr[2 * bt + kk], dk[db], 0, 0, 0);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WAIT_VM0();
    __syncthreads();
  }
  // (whole waves store rows there: ragged lanes stay; an accumulating store keeps the direct form -- fp32 sum, ONE rounding)
  const bool lds_epi = p.nsplit <= 1 && !p.accum_dkv;
  if (lds_epi ? !wave_active : !kstored) return;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] *= p.q_prescaled ? 0.6931471805599453f : p.scale;   // dS^T Q' = scale log2(e) dS^T Q
  const int D = 64 * ND;
  if (p.nsplit > 1) {
    float* pr = p.dkv_part + ((((long long)split * p.B + b) * p.H + head) * p.Skv + krow) * 2 * D + chunk * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * fh;
        f32x4 a, cc;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = dk[db][4 * g + j]; cc[j] = dv[db][4 * g + j]; }
        *(f32x4*)(pr + d) = a;
        *(f32x4*)(pr + D + d) = cc;
      }
    return;
  }
  if (lds_epi) {
    // A key row per lane here: sixteen 8-byte stores per lane written straight out (store-issue-bound: ~9 k cycles per
    // workgroup, paid once per 16 query tiles at 1024 tokens).  Each wave's blocks of dK, then dV, go through its own image
    // (the ring is free behind the loop's last barrier).
    char* const ost = smem + wave * (32 * 144);
    store_o_image_144(ost, lane, [&](int db, int i) { return dk[db][i]; }, p.dK + (long long)b * p.Skv * p.lddk + head * D + chunk * 64,
                      p.lddk, k0, p.Skv, p.accum_dkv != 0);
    store_o_image_144(ost, lane, [&](int db, int i) { return dv[db][i]; }, p.dV + (long long)b * p.Skv * p.lddv + head * D + chunk * 64,
                      p.lddv, k0, p.Skv, p.accum_dkv != 0);
    return;
  }
  bf16* dKr = p.dK + ((long long)b * p.Skv + krow) * p.lddk + head * D + chunk * 64;
  bf16* dVr = p.dV + ((long long)b * p.Skv + krow) * p.lddv + head * D + chunk * 64;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = db * 32 + 8 * g + 4 * fh;
      bf16x4 ok, ov;
      if (p.accum_dkv) {
        ok = *(const bf16x4*)(dKr + d);
        ov = *(const bf16x4*)(dVr + d);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ok[j] = (bf16)(dk[db][4 * g + j] + (p.accum_dkv ? (float)ok[j] : 0.f));
        ov[j] = (bf16)(dv[db][4 * g + j] + (p.accum_dkv ? (float)ov[j] : 0.f));
      }
      *(bf16x4*)(dKr + d) = ok;
      *(bf16x4*)(dVr + d) = ov;
    }
}

template <bool USE_TR, int ND>
__global__ __launch_bounds__(256, (ND == 1 ? 2 : 1)) void attn_dkv_kernel(const AttnP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int blk_x, head, b;
  attn_block_coords(blk_x, head, b);
  attn_dkv_body<USE_TR, ND>(p, smem, blk_x, head, b);
}

// ============================================================================= fused backward launch
// dQ workgroups and dK/dV workgroups of ONE attention in ONE grid.  As two launches each pass ends on a partly filled
// last round of workgroups (self-attention over 1024 tokens, B*H = 80: 640 workgroups on 512 slots = 1.25 rounds, i.e.
// 62 % of the slots busy; 4096 tokens: 2.5 rounds, 83 %); together they are 2.5 / 5 rounds.  Both roles keep their own
// code (the role is uniform per workgroup).  Task order: all workgroups of one (batch, head) are adjacent -- dQ blocks,
// then dK/dV blocks -- and XCD x owns a contiguous range of heads, so a head's Q / K / V / dO are read into one L2 once
// for both roles.  delta comes from attn_delta_kernel (the roles run concurrently, so the dQ role cannot hand it over).
template <bool USE_TR, int ND>
__global__ __launch_bounds__(256, (ND == 1 ? 2 : 1)) void attn_bwd_fused_kernel(const AttnP p, int n_dq, int n_dkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lin = xcd_contiguous(blockIdx.x, gridDim.x);
  const int per_head = n_dq + n_dkv;
  const int bh = (int)(lin / per_head), rem = (int)(lin - (unsigned)bh * per_head);
  const int b = bh / p.H, head = bh - b * p.H;
  if (rem < n_dkv) attn_dkv_body<USE_TR, ND>(p, smem, rem, head, b);          // heavier role (4 products) first
  else attn_q_body<1, USE_TR, ND, false, false>(p, smem, rem - n_dkv, head, b);
}

// ============================================================================= cross-attention forward, K / V resident
// <= 128 keys (the 77-token text context: KB = 3 blocks of 32), head_dim 64.  The general forward spends a workgroup per 128
// queries on two 64-key tiles (25 % of them padding), a K / V staging round trip and two barriers for 2 x 8 MFMAs per wave.
// Here a workgroup stages K and V ONCE and its four waves then walk 128-query units independently -- no barrier in the loop:
// Q fragments straight from HBM (this lane's query row: four 16-byte loads), S^T over KB key blocks, the softmax in one
// shot (all scores of a query are in registers: no running max, no rescale), O^T = V^T P^T, store.  Per-sample key counts
// (merged passes with a shorter student context) mask through the same compare as the padding keys.
// What a cross-attention workgroup knows about its (split, batch, head): its run of UQ-query units, the rows of that head in
// every operand, the sample's key count, and the factor c that takes a score into the log2 domain (1 when Q arrives
// prescaled).  PRE: 1 / 0 where the instantiation knows whether Q is prescaled, -1: AttnP::q_prescaled decides at run time.
struct XattnCtx {
  int split, head, b, u_begin, u_end, skv_b;
  float c;
  const bf16 *Qb, *dOb, *Ob, *Kb, *Vb;
  const float* lseb;
};
template <int UQ, int PRE = -1>
__device__ __forceinline__ XattnCtx xattn_ctx(const AttnP& p, int upw) {
  XattnCtx x;
  attn_block_coords(x.split, x.head, x.b);
  const int nu = (p.Sq + UQ - 1) >> (UQ == 128 ? 7 : 6);         // a shift, not a division: Sq is signed
  x.u_begin = x.split * upw;
  x.u_end = min(nu, x.u_begin + upw);
  x.c = (PRE < 0 ? p.q_prescaled != 0 : PRE != 0) ? 1.f : p.scale * LOG2E;
  x.Qb = p.Q + (long long)x.b * p.Sq * p.ldq + x.head * 64;
  x.dOb = p.dO + (long long)x.b * p.Sq * p.lddo + x.head * 64;
  x.Ob = p.O + (long long)x.b * p.Sq * p.ldo + x.head * 64;
  x.Kb = p.K + (long long)x.b * p.Skv * p.ldk + x.head * 64;
  x.Vb = p.V + (long long)x.b * p.Skv * p.ldv + x.head * 64;
  x.lseb = p.lse + ((long long)x.b * p.H + x.head) * p.Sq;
  x.skv_b = __builtin_amdgcn_readfirstlane(p.kv_len ? p.kv_len[x.b] : p.Skv);
  return x;
}
__device__ __forceinline__ float xhalf_sum(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return a + b;
}

// ----------------------------------------------------------------------------- cross-attention building blocks
// What xattn_fwd_kernel, xattn_regions_fwd_kernel, xattn_maps_kernel and xattn_edit_fwd_kernel are made of: a wave's 32 queries
// (query lane & 31 on the lane, both half-waves) against KB resident blocks of 32 keys.  One copy of the arithmetic, so that
// the bit-equality the tests assert between these kernels holds by construction.  A block of K or V is 32 rows x 128 bytes
// (4 096 bytes, source-side XOR swizzle), block kb at kb * 4096 -- a 64-row tile is two of them.  In the S^T accumulator slot
// r of half-wave fh of block kb is key kb * 32 + (r & 3) + 8 (r >> 2) + 4 fh.
__device__ __forceinline__ f32x16 zero_f32x16() {
  return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}
// A wave's 32 query rows as a 4 KiB swizzled image in its own LDS region, filled by LDS-DMA (whole 128-byte rows per 8 lanes)
// one unit ahead; direct 16-byte loads of a row per lane touched 32 lines per instruction.  src: tile_src(.., wave 0, lane) --
// pieces 0 / 1 of a tile are rows 0..15, the other 16 rows come through the scalar offset.  The caller waits (WAIT_VM0) before
// load() and for lgkmcnt(0) behind it before it stages the next unit over the image.
struct XattnQStage {
  TileSrc src;
  char* img;
  __device__ __forceinline__ void stage(int row0) const {
    stage_tile(src, row0, img, 0);
    stage_tile(src, row0 + 16, img + 2048, 0);
  }
  __device__ __forceinline__ void load(bf16x8 (&qf)[4], const AttnFragOff& fo) const {
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(img + fo.rf[s]);
  }
};
// S^T[key][q] = K . Q^T over the KB key blocks at Ksm
template <int KB>
__device__ __forceinline__ void xattn_scores(const char* Ksm, const AttnFragOff& fo, const bf16x8 (&qf)[4], f32x16 (&sacc)[KB]) {
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    bf16x8 kfr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) kfr[s] = *(const bf16x8*)(Ksm + fo.rf[s] + kb * 4096);
    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0], qf[0], zero_f32x16(), 0, 0, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[s], qf[s], sacc[kb], 0, 0, 0);
  }
}
// keys at or past nkeys (padding slots, keys past a sample's count) score -inf; only blocks FIRST.. are looked at, and of
// those only the ones that hold such a key (wave-uniform).  FIRST = KB - 1 where nkeys > (KB - 1) * 32 is known.
template <int KB, int FIRST = 0>
__device__ __forceinline__ void xattn_mask_keys(f32x16 (&sacc)[KB], int nkeys, int fh) {
#pragma unroll
  for (int kb = FIRST; kb < KB; ++kb)
    if (kb * 32 + 32 > nkeys) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        sacc[kb][r] = key < nkeys ? sacc[kb][r] : -INFINITY;
      }
    }
}
// The softmax in one shot (all scores of a query are in registers: no running max, no rescale): e = exp2(c s - c max), handed
// to put(kb, r, e); returns the sum of e over all keys, mx the maximum of the raw scores.  A masked key gives exp2(-inf) = 0.
// The ORDER is the contract between the kernels: the maximum starts at sacc[0][0] and takes the blocks in order, registers in
// order; the sum starts at 0 and adds in (kb, r) order; the half-wave combine (xhalf_max / xhalf_sum) comes last.
template <int KB, class Put>
__device__ __forceinline__ float xattn_softmax(const f32x16 (&sacc)[KB], float c, float& mx, Put put) {
  mx = sacc[0][0];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = (kb == 0 ? 1 : 0); r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
  mx = xhalf_max(mx);
  const float mc = mx * c;
  float ls = 0.f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = fast_exp2(fmaf(sacc[kb][r], c, -mc));
      ls += e;
      put(kb, r, e);
    }
  return xhalf_sum(ls);
}
// ... leaving the un-normalised P^T rounded to bf16, as the B-operand fragments of the value product (k-permuted)
template <int KB>
__device__ __forceinline__ float xattn_softmax_bf16(const f32x16 (&sacc)[KB], float c, float& mx, bf16x8 (&pf)[2 * KB]) {
  return xattn_softmax<KB>(sacc, c, mx, [&](int kb, int r, float e) { pf[2 * kb + (r >> 3)][r & 7] = (bf16)e; });
}
// ... leaving the fp32 exponentials in place of the scores
template <int KB>
__device__ __forceinline__ float xattn_softmax_f32(f32x16 (&sacc)[KB], float c, float& mx) {
  return xattn_softmax<KB>(sacc, c, mx, [&](int kb, int r, float e) { sacc[kb][r] = e; });
}
// O^T[d][q] = V^T[d][key] P^T[key][q] over the 2 KB 16-key slices at Vsm (transposed reads of the row-major V blocks)
template <int KB>
__device__ __forceinline__ void xattn_pv(const char* Vsm, const AttnFragOff& fo, const bf16x8 (&pf)[2 * KB], f32x16 (&oacc)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2 * KB; ++ks)
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const bf16x8 tf = read_transposed_frag_at(Vsm + fo.tr[db][0] + ks * 2048, Vsm + fo.tr[db][1] + ks * 2048);
      if (ks == 0) oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf, pf[0], zero_f32x16(), 0, 0, 0);
      else oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf, pf[ks], oacc[db], 0, 0, 0);
    }
}

// IP: the decoupled cross-attention of an image prompt (IP-Adapter), O = softmax(s Q K^T) V + scale2 * softmax(s Q K2^T) V2
// with 1..32 image keys (AttnP::K2 / V2 / Skv2).  Unfused that is two of these launches and an add: Q read twice, three
// O-sized writes and two O-sized reads, where the output alone is already most of this kernel's traffic.  Here the image
// keys are ONE more 32-key block on the resident Q fragments: S2 from the same qf, a softmax of its own (own max, own sum --
// a spike in either key set cannot underflow the other), O2^T = V2^T P2^T, and oacc * inv + scale2 * (oacc2 * inv2) in fp32,
// rounded to bf16 once, through the same LDS image.  K2 / V2 are staged as two 32-row HALF tiles behind the Q images
// (2 x 4 096 bytes: 75 776 bytes with 77 text keys, still two workgroups per CU; two full tiles would not fit, and the free
// fourth block of the text tiles would only serve <= 96 text keys).  kv_len masks text keys only; lse is the text softmax's.
// scale2 rides in inv2 (scale2 / sum): one multiply per element fewer, and scale2 = 0 returns the text term bit for bit.
// The LDS allows two workgroups per CU at most, so the launch bound asks for no more.  What hipcc makes of the four instances
// (profiles/ip_adapter_bench_regs.txt): 104 / 108 / 130 / 153 VGPRs for 1..4 text key blocks, no AGPRs, no scratch -- against
// 68 / 78 / 91 / 130 without the image keys; all under the 256 a two-workgroup CU leaves a wave.
//
// MS (with IP): several image prompts at once, O = o_text + sum_j w_j m_j[b][q] softmax(s Q K2_j^T) V2_j for 1..4 sets that lie
// back to back in the SAME 32-key block (4 + 16, 16 + 16, 4 + 4 + 16 slots of it), each with a weight and an optional per-query
// mask (AttnP::nset / set_end / set_w / set_mask).  No more LDS and no more MFMAs than one set: what is added is a softmax per
// set -- every set its own maximum and its own sum over its rows of the one score tile, so a spike in one set cannot underflow
// another set or the text term.  A query row lives on one lane (both half-waves), so w_j m_j is one scalar per lane, set and
// unit.  Normalisation: w_j m_j / sum_j is folded into P BEFORE its bf16 rounding (|factor x e| <= |w_j m_j|: the product is
// rounded once, like P of the one-set instance), and all sets go through the ONE PV product of the block; one accumulator per
// set would cost 32 more VGPRs and 4 more MFMAs per set.  A set with w_j m_j = 0 therefore contributes exact zeros, and a mask
// of ones gives the bits of no mask (w x 1.0f).  Padding slots (score -inf, e = 0) count as keys of the last set.  The instance
// serves whatever the one-set instance does not: its launch is decided in launch_attention_fwd (attn_resolve_sets).
template <int KB, bool IP = false, bool MS = false>
__global__ __launch_bounds__(256, IP ? 2 : 3) void xattn_fwd_kernel(const AttnP p, int upw) {
  static_assert(IP || !MS, "several image key sets are sets of the image key block");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KT = (KB + 1) / 2;                               // 64-key tiles
  char* const Ksm = smem;
  char* const Vsm = smem + KT * TILE_BYTES;
  char* const Osm = smem + 2 * KT * TILE_BYTES;                  // 4 waves x 32 rows x 144 bytes
  char* const K2sm = Osm + 4 * 32 * 144 + 4 * 4096;              // IP: image keys, then image values (32 rows x 128 bytes each)
  char* const V2sm = K2sm + 4096;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const XattnCtx x = xattn_ctx<128>(p, upw);
  const int head = x.head, b = x.b, u_begin = x.u_begin, u_end = x.u_end, skv_b = x.skv_b;
  const float c = x.c;                                           // prescaled Q: 1, the scores are in the log2 domain already
  {
    const TileSrc ksrc = tile_src(x.Kb, p.ldk, p.Skv, wave, lane), vsrc = tile_src(x.Vb, p.ldv, p.Skv, wave, lane);
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      stage_tile(ksrc, t * 64, Ksm + t * TILE_BYTES, wave);
      stage_tile(vsrc, t * 64, Vsm + t * TILE_BYTES, wave);
    }
    if constexpr (IP) {                                          // waves 0 / 1: the 32 rows of K2, waves 2 / 3: those of V2
      const bool isv = wave >= 2;
      const bf16* b2 = isv ? p.V2 + (long long)b * p.k2_brows * p.ldv2 : p.K2 + (long long)b * p.k2_brows * p.ldk2;
      const TileSrc src2 = tile_src(b2 + head * 64, isv ? p.ldv2 : p.ldk2, p.Skv2, wave & 1, lane);
      stage_tile(src2, 0, isv ? V2sm : K2sm, wave & 1);
    }
  }
  const AttnFragOff fo = attn_frag_off(lane);
  int qrow = u_begin * 128 + wave * 32 + frow;
  bf16x8 qf[4];
  const XattnQStage qs = {tile_src(x.Qb, p.ldq, p.Sq, 0, lane), Osm + 4 * 32 * 144 + wave * 4096};
  if (u_begin < u_end) qs.stage(u_begin * 128 + wave * 32);
  WAIT_VM0();
  __syncthreads();
  for (int u = u_begin; u < u_end; ++u, qrow += 128) {
    const bool qvalid = qrow < p.Sq;
    WAIT_VM0();                                                  // this wave's Q image (and its stores of the last unit)
    qs.load(qf, fo);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (u + 1 < u_end) qs.stage((u + 1) * 128 + wave * 32);     // next unit's rows fly under this unit's work
    [[maybe_unused]] float wm[4];                                // MS: w_j m_j[b][this lane's query]; the loads fly under the score products
    if constexpr (MS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wm[j] = 0.f;
        if (j < p.nset) {
          const float* mj = p.set_mask[j];
          wm[j] = p.set_w[j] * (mj && qvalid ? mj[(long long)b * p.set_mstride[j] + qrow] : 1.f);
        }
      }
    }
    f32x16 sacc[KB];
    xattn_scores<KB>(Ksm, fo, qf, sacc);
    xattn_mask_keys<KB>(sacc, skv_b, fh);                        // padding keys / keys past this sample's count
    [[maybe_unused]] f32x16 sacc2[1];                            // IP: S2^T = K2 . Q^T, slots past Skv2 -inf
    if constexpr (IP) {
      xattn_scores<1>(K2sm, fo, qf, sacc2);
      xattn_mask_keys<1>(sacc2, p.Skv2, fh);
    }
    float mx;
    bf16x8 pf[2 * KB];
    const float l_tot = xattn_softmax_bf16<KB>(sacc, c, mx, pf);
    f32x16 oacc[2];
    xattn_pv<KB>(Vsm, fo, pf, oacc);
    const float inv = 1.f / l_tot;
    [[maybe_unused]] f32x16 oacc2[2];
    [[maybe_unused]] float inv2 = 0.f;                           // scale2 / (sum of the image softmax)
    if constexpr (IP) {
      bf16x8 pf2[2];
      if constexpr (MS) {
        // slot r of this lane holds key kc(r) + 4 fh, kc(r) = (r & 3) + 8 (r >> 2); set j owns keys set_end[j - 1] .. set_end[j].
        // The sets lie in key order and padding slots score -inf, so "at or behind the first key of set j" is all that is ever
        // asked: kb >= set_end[j - 1] - kc(r), a lane value against a scalar.  Sets are peeled off from the last one down -- what
        // is left when set 0's turn comes is set 0 -- and the passes of a set that is not there are skipped as a whole.
        const int kb = 4 * fh;
        const auto from = [&](int j, int r) { return kb >= p.set_end[j - 1] - ((r & 3) + 8 * (r >> 2)); };
        float mcs[4], fs[4], cur[16], mcr[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[r] = sacc2[0][r];
#pragma unroll
        for (int j = 3; j >= 1; --j) {
          mcs[j] = 0.f;
          if (j < p.nset) {
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              m = fmaxf(m, from(j, r) ? cur[r] : -INFINITY);
              cur[r] = from(j, r) ? -INFINITY : cur[r];
            }
            mcs[j] = xhalf_max(m) * c;
          }
        }
        {
          float m = cur[0];
#pragma unroll
          for (int r = 1; r < 16; ++r) m = fmaxf(m, cur[r]);
          mcs[0] = xhalf_max(m) * c;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mcr[r] = mcs[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
          if (j < p.nset) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mcr[r] = from(j, r) ? mcs[j] : mcr[r];
          }
        float e2[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cur[r] = e2[r] = fast_exp2(fmaf(sacc2[0][r], c, -mcr[r]));
#pragma unroll
        for (int j = 3; j >= 1; --j) {
          fs[j] = 0.f;
          if (j < p.nset) {
            float ls2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              ls2 += from(j, r) ? cur[r] : 0.f;
              cur[r] = from(j, r) ? 0.f : cur[r];
            }
            fs[j] = wm[j] / xhalf_sum(ls2);
          }
        }
        {
          float ls2 = cur[0];
#pragma unroll
          for (int r = 1; r < 16; ++r) ls2 += cur[r];
          fs[0] = wm[0] / xhalf_sum(ls2);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mcr[r] = fs[0];                // (the register array serves both chains)
#pragma unroll
        for (int j = 1; j < 4; ++j)
          if (j < p.nset) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mcr[r] = from(j, r) ? fs[j] : mcr[r];
          }
#pragma unroll
        for (int r = 0; r < 16; ++r) pf2[r >> 3][r & 7] = (bf16)(e2[r] * mcr[r]);
      } else {
        float mx2;
        inv2 = p.scale2 / xattn_softmax_bf16<1>(sacc2, c, mx2, pf2);
      }
      xattn_pv<1>(V2sm, fo, pf2, oacc2);
    }
    if (qvalid && p.lse && fh == 0)
      p.lse[((long long)b * p.H + head) * p.Sq + qrow] = mx * (p.q_prescaled ? 0.6931471805599453f : p.scale) + log2f(l_tot) * 0.6931471805599453f;
    // with 77 keys the output is most of this kernel's traffic
    store_o_image_144(Osm + wave * (32 * 144), lane,
                      [&](int db, int i) {
                        if constexpr (MS) return oacc[db][i] * inv + oacc2[db][i];                // the factors are in P
                        else if constexpr (IP) return oacc[db][i] * inv + oacc2[db][i] * inv2;
                        else return oacc[db][i] * inv;
                      },
                      p.O + (long long)b * p.Sq * p.ldo + head * 64, p.ldo, u * 128 + wave * 32, p.Sq);
  }
}

// ============================================================================= regional text prompts
// O[b][q] = sum_r w[b][r][q] softmax(s Q K_r^T) V_r over R <= 4 key sets ("regions") of Lr <= 96 keys each that lie back to back
// in ONE K / V buffer [B][R * Lr][ld]: what a UNet context of R * 77 rows leaves in its stacked K|V projection.  Unfused that is
// R launches of xattn_fwd_kernel and R weighted adds: Q read R times, O written and re-read R times, in a kernel whose output
// is most of its traffic.  Here a workgroup stages all R regions once, each padded to KB = ceil(Lr / 32) whole 32-key blocks
// (half tiles of 4 096 bytes, region r at r * KB * 8 192: its K blocks, then its V blocks), and a wave walks the regions on
// its resident Q fragments: the building blocks per region (scores, mask, softmax with the region's OWN maximum and sum -- a
// spike in one region cannot underflow another --, value product), and one fmaf per element by w / sum into a running fp32
// total: 32 more VGPRs whatever R is.  O is rounded once.
// LDS: R x KB x 8 192 bytes of keys and values, four O images and four Q images of 4 096 bytes each: 81 920 bytes for two regions
// of 77 keys, which is exactly two workgroups per CU, 131 072 at the maximum of twelve blocks.  The O image is the swizzled one
// (store_o_image_swz) for that reason: at a 144-byte pitch the two-region launch took 83 968 bytes and
// ran one workgroup per CU (same bits; 9.11 -> 8.64 us at 10 heads x 4096 queries, 8.36 -> 7.21 us at 20 x 1024, the other
// region counts unchanged: profiles/EXPERIMENTS.md section 9, f9).
// Every block goes through a descriptor that starts at the block's first row and ends with the region's last (as the blocks
// of attn_fewq_kernel do), so no row of the next region, the next sample or anything behind the buffer is read: such slots
// arrive as zeros and score -inf.
// Skipping: a region whose weight is 0 on every valid query of a wave's 32 (a wave-uniform vote) costs that wave nothing -- both
// products skipped, contribution exactly zero; with disjoint regions a wave's queries are a short run of one latent row and lie
// in one or two regions.  A wave with nothing left writes zeros.  One-hot weights on region r therefore give the bits of
// xattn_fwd_kernel on that region's rows (fmaf(o, 1 / sum, 0) is o * (1 / sum)).  The weights are not normalised here, any
// finite value goes; rows at or past Sq are never read.  No atomics: the same bits every run.
template <int KB>
__global__ __launch_bounds__(256, 2) void xattn_regions_fwd_kernel(const AttnRegionsP p, int upw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RB = KB * 2 * 4096;                              // bytes of a region: KB key blocks, then KB value blocks
  char* const Osm = smem + p.R * RB;                             // 4 waves x 32 rows x 128 bytes, then the 4 Q images
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  int split, head, b;
  attn_block_coords(split, head, b);
  const int nu = (p.Sq + 127) >> 7;
  const int u_begin = split * upw, u_end = min(nu, u_begin + upw);
  const float c = p.q_prescaled ? 1.f : p.scale * LOG2E;
  const bf16* Qb = p.Q + (long long)b * p.Sq * p.ldq + head * 64;
  {                                                              // waves 0 / 1: the 32 rows of every K block, waves 2 / 3: of every V block
    const bool isv = wave >= 2;
    const int ld = isv ? p.ldv : p.ldk;
    const bf16* base = (isv ? p.V : p.K) + (long long)b * p.R * p.Lr * ld + head * 64;
    for (int r = 0; r < p.R; ++r)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const TileSrc src = tile_src(base + ((long long)r * p.Lr + kb * 32) * ld, ld, p.Lr - kb * 32, wave & 1, lane);
        stage_tile(src, 0, smem + r * RB + (isv ? KB * 4096 : 0) + kb * 4096, wave & 1);
      }
  }
  const AttnFragOff fo = attn_frag_off(lane);
  int qrow = u_begin * 128 + wave * 32 + frow;
  bf16x8 qf[4];
  const XattnQStage qs = {tile_src(Qb, p.ldq, p.Sq, 0, lane), Osm + 4 * 4096 + wave * 4096};
  if (u_begin < u_end) qs.stage(u_begin * 128 + wave * 32);
  WAIT_VM0();
  __syncthreads();
  const float* const wb = p.w + (p.Bw == 1 ? 0 : (long long)b * p.R * p.Sq);
  for (int u = u_begin; u < u_end; ++u, qrow += 128) {
    const bool qvalid = qrow < p.Sq;
    WAIT_VM0();                                                  // this wave's Q image (and its stores of the last unit)
    qs.load(qf, fo);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (u + 1 < u_end) qs.stage((u + 1) * 128 + wave * 32);
    float wv[4];                                                 // w[b][r][this lane's query]; 0 for a region that is not there
#pragma unroll
    for (int r = 0; r < 4; ++r) wv[r] = r < p.R && qvalid ? wb[(long long)r * p.Sq + qrow] : 0.f;
    f32x16 tot[2] = {zero_f32x16(), zero_f32x16()};
    for (int r = 0; r < p.R; ++r) {
      const float wr = r == 0 ? wv[0] : r == 1 ? wv[1] : r == 2 ? wv[2] : wv[3];
      if (__builtin_amdgcn_ballot_w64(wr != 0.f) == 0) continue; // nobody in this wave weighs region r: skip both products
      const char* const Ksm = smem + r * RB;
      f32x16 sacc[KB];
      xattn_scores<KB>(Ksm, fo, qf, sacc);
      xattn_mask_keys<KB, KB - 1>(sacc, p.Lr, fh);               // padding slots of the region's last block
      float mx;
      bf16x8 pf[2 * KB];
      const float f = wr / xattn_softmax_bf16<KB>(sacc, c, mx, pf);
      f32x16 oacc[2];
      xattn_pv<KB>(Ksm + KB * 4096, fo, pf, oacc);
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) tot[db][i] = fmaf(oacc[db][i], f, tot[db][i]);
    }
    store_o_image_swz(Osm + wave * 4096, lane, [&](int db, int i) { return tot[db][i]; },
                      p.O + (long long)b * p.Sq * p.ldo + head * 64, p.ldo, u * 128 + wave * 32, p.Sq);
  }
}

// ============================================================================= cross-attention heat maps
// M[b][key][q] (op)= (1 / H) sum_h softmax_key(s Q[b, q, h, :] . K[b, key, h, :]): the head-mean cross-attention probability of
// every (key, query) pair, fp32, laid out [B][Skv][Sq] so that one token's map is one contiguous h_l x w_l image ("DAAM", diffusion
// attentive attribution maps).  xattn_fwd_kernel keeps S and P in registers and writes O alone, and the heads of one (sample,
// query) live in different workgroups there; summing them without atomics needs a kernel that has all heads of a query in ONE
// workgroup.  No V, no O, no lse; 1 <= Skv <= 128 (KB = ceil(Skv / 32) key blocks), head_dim 64, any Sq.
// A workgroup owns 32 queries of one sample (one MFMA column block) and deals the HEADS over its EIGHT waves: wave w runs heads
// w, w + 8, w + 16, ... in that order.  Every wave has an LDS slot of its own -- the head's KB key blocks (32 rows x 128 bytes
// each, descriptors that start at the block's first row and end with the sample's last key, as in attn_fewq_kernel: nothing
// behind a sample's keys is read) and the 32 query rows of that head -- filled by LDS-DMA at the top of the head's iteration; no
// barrier in the loop.  There is no second slot: what hides a wave's fetch is the other wave of its SIMD.  The first form had four
// waves with a ring two slots deep (the same LDS); one wave per SIMD then ran fetch wait, 12 MFMAs and ~300 vector instructions
// per head back to back with nothing to overlap them: 8.03 / 10.46 us at the two SDXL shapes against 6.49 / 7.62 us in this form
// (profiles/EXPERIMENTS.md section 9, f10).  Per head, of the building blocks: scores (in the S^T accumulator layout one register
// index is one key over 32 consecutive queries), the mask (padding keys and keys at or past kv_len[b]) and the softmax that keeps
// its exponentials in fp32; then p = e x (1 / sum), the reciprocal taken once per query -- P is never rounded to bf16 -- and one
// fmaf per element into the wave's fp32 partial sum.
// Reduction order (fixed, the same bits every run): within a wave its heads in ascending order; then the eight partial sums
// meet in LDS (each wave's own, by now idle, slot: [KB x 32 keys][32 queries] fp32) and every element is summed in wave order,
// ((((w0 + w1) + w2) + ...) + w7), and multiplied by 1 / H once.  A wave without a head contributes zeros.  The thread that owns an
// element stores it, or with `accumulate` loads, adds and stores it (one fp32 add; plain vector memory instructions, no atomics;
// no other workgroup of the launch touches that element).  32 lanes write 32 consecutive queries of one key: whole 128-byte runs
// where Sq is a multiple of 32.  A cut key's probability is an exact 0.0f in every head, so its map is.
// LDS: 8 waves x (KB + 1) x 4 096 bytes = 65 536 .. 163 840.
#define MAPS_WAVES 8
template <int KB>
__global__ __launch_bounds__(64 * MAPS_WAVES) void xattn_maps_kernel(const AttnMapsP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int SLOT = (KB + 1) * 4096;                          // a wave's slot: KB key blocks, then the query rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const int q0 = blockIdx.x * 32, b = blockIdx.y;
  const float c = p.q_prescaled ? 1.f : p.scale * LOG2E;
  const bf16* Qb = p.Q + ((long long)b * p.Sq + q0) * p.ldq;     // this unit's first query row, head 0
  const bf16* Kb = p.K + (long long)b * p.Skv * p.ldk;
  const int qrows = min(p.Sq - q0, 32);                          // >= 1: the grid has no unit past Sq
  const int skv_b = __builtin_amdgcn_readfirstlane(p.kv_len ? p.kv_len[b] : p.Skv);
  char* const my = smem + wave * SLOT;
  // head `h`: its key blocks -> dst + kb * 4096, its query rows -> dst + KB * 4096 (pieces 0 / 1 of a tile: rows 0..15, 16..31)
  auto stage_head = [&](int h, char* dst) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const bf16* kblk = Kb + (long long)kb * 32 * p.ldk + h * 64;
      const int left = min(p.Skv - kb * 32, 32);                 // >= 1: KB = ceil(Skv / 32)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) stage_tile(tile_src(kblk, p.ldk, left, hf, lane), 0, dst + kb * 4096, hf);
    }
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) stage_tile(tile_src(Qb + h * 64, p.ldq, qrows, hf, lane), 0, dst + KB * 4096, hf);
  };
  const AttnFragOff fo = attn_frag_off(lane);
  f32x16 macc[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) macc[kb] = zero_f32x16();
  for (int h = wave; h < p.H; h += MAPS_WAVES) {
    char* const cur = my;
    stage_head(h, cur);                                          // (the slot's last reader: the iteration before, closed below)
    WAIT_VM0();                                                  // this head's rows have landed
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(cur + KB * 4096 + fo.rf[s]);
    f32x16 sacc[KB];
    xattn_scores<KB>(cur, fo, qf, sacc);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // every read of `cur` is done before a later DMA may land in it
    xattn_mask_keys<KB>(sacc, skv_b, fh);                        // padding keys / keys past this sample's count
    float mx;
    const float inv = 1.f / xattn_softmax_f32<KB>(sacc, c, mx);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) macc[kb][r] = fmaf(sacc[kb][r], inv, macc[kb][r]);
  }
  // this wave's partial sum into its own slot (no DMA is in flight: each staged head was waited for and consumed)
  float* const part = (float*)my;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh) * 32 + frow] = macc[kb][r];
  __syncthreads();
  // merge: thread -> query tid & 31, keys (tid >> 5), (tid >> 5) + 16, ...; partials in wave order
  const int q = tid & 31;
  if (q >= qrows) return;                                        // rows of a ragged last unit
  const float inv_h = 1.f / (float)p.H;
  float* const mrow = p.maps + (long long)b * p.Skv * p.Sq + q0 + q;
  for (int key = tid >> 5; key < p.Skv; key += 2 * MAPS_WAVES) {
#pragma clang fp contract(off)                                   // `+=` is ONE fp32 add of the rounded mean, not an fma with 1 / H
    const int e = (key * 32 + q) * 4;
    float sum = *(const float*)(smem + e);
#pragma unroll
    for (int w = 1; w < MAPS_WAVES; ++w) sum = sum + *(const float*)(smem + w * SLOT + e);
    const float v = sum * inv_h;
    float* const dst = mrow + (long long)key * p.Sq;
    if (p.accumulate) *dst = *dst + v;
    else *dst = v;
  }
}

// ============================================================================= self-attention column sums
// Self-attention guidance: part[b][g][key] = (1 / H) sum_{h in group g} sum_q softmax(scale Q_h K_h^T)[q][key], the probability
// mass a key receives from all queries, at any key count (the maps kernel above needs its keys resident: <= 128).  The score half
// of the dK / dV role with an in-lane sum: a workgroup = 4 waves = 128 keys of one (sample, head group), a wave owns 32 keys (key
// on the lane); the Q tiles of the group's heads stream through the 2-deep LDS-DMA ring, four to a stage, with the softmax's row
// constant lse[q] beside them; S^T leaves the MFMA with a query per register.  PRE (a prescaled Q): the constant -lse log2(e) is the accumulator
// operand and p = exp2(acc).  Otherwise scale log2(e) multiplies the fp32 score -- no bf16 operand is rounded a second time -- so
// both forms see the same scores to fp32 rounding.  p stays fp32: no V, no O, no second product.
// Order of the sum (the same bits every run): a lane adds the 32 queries of a tile that it holds (16 per 32-query block: four
// chains over j, ((j0 + j1) + (j2 + j3)), block 0 then block 1), adds tile sums in ascending tile order, heads in ascending order;
// after the last head the two halves of the wave (queries 8 g + 0..3 and 8 g + 4..7) are added, then x 1 / H.
// Queries at or past Sq of the last tile: their rows read as zeros (buffer bounds) and their p is replaced by 0, not multiplied.
// Keys at or past Skv of the last block: the lane computes on the last stored row and stores nothing.
#define COLSUM_NT 4                                            // 64-query tiles per stage of the ring: one for each wave's row constants
#define COLSUM_STG (COLSUM_NT * (TILE_BYTES + 256))            // a stage: four Q tiles and their 4 x 64 row constants
// A stage is 256 queries, not 64: a quarter of the barriers, and a step's work stays above the DMA's latency with one wave per
// SIMD.  At SDXL's mid block it measures the same as one tile per stage (profiles/EXPERIMENTS.md section 9, f13: the stage depth
// is not what bounds this launch).
template <bool PRE>
__global__ __launch_bounds__(256, 2) void attn_colsum_kernel(const AttnColsumP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int kblk, grp, b;
  attn_block_coords(kblk, grp, b);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const auto [k0, krow, kstored, wave_active] = attn_key_lane(kblk, wave, frow, p.Skv);
  const int h0 = grp * p.hpg, h1 = min(p.H, h0 + p.hpg);
  const int nt = (p.Sq + 63) / 64, ns = (nt + COLSUM_NT - 1) / COLSUM_NT, nit = (h1 - h0) * ns;
  const bf16* Qb = p.Q + (long long)b * p.Sq * p.ldq;
  const bf16* Kr = p.K + ((long long)b * p.Skv + krow) * p.ldk;
  const float* lseb = p.lse + (long long)b * p.H * p.Sq;
  const float c = p.scale * LOG2E;

  auto stage = [&](char* dst, int h, int t0) {           // tiles t0 .. t0 + 3 of head h, those that exist
    const TileSrc q = tile_src(Qb + h * 64, p.ldq, p.Sq, wave, lane);
#pragma unroll
    for (int j = 0; j < COLSUM_NT; ++j)
      if (t0 + j < nt) stage_tile(q, (t0 + j) * 64, dst + j * TILE_BYTES, wave);
    // wave w brings the row constants of tile t0 + w
    if (t0 + wave < nt) stage_rowconst(lseb + (long long)h * p.Sq, (t0 + wave) * 64, p.Sq, dst + COLSUM_NT * TILE_BYTES + wave * 256, lane);
  };
  if (nit > 0) stage(smem, h0, 0);
  WAIT_VM0();
  __syncthreads();

  float col = 0.f;
  bf16x8 kf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) kf[s] = bf16x8{};
  int h = h0, st = 0;
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1;
    int hn = h, sn = st + 1;
    if (sn == ns) { sn = 0; ++hn; }
    if (it + 1 < nit) stage(smem + (cur ^ 1) * COLSUM_STG, hn, sn * COLSUM_NT);
    if (wave_active) {
      if (st == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[s] = *(const bf16x8*)(Kr + h * 64 + 16 * s + 8 * fh);
      }
      for (int j = 0; j < COLSUM_NT; ++j) {
        const int t = st * COLSUM_NT + j;
        if (t >= nt) break;                              // uniform
        const char* Qs = smem + cur * COLSUM_STG + j * TILE_BYTES;
        const float* rc = (const float*)(smem + cur * COLSUM_STG + COLSUM_NT * TILE_BYTES + j * 256);
        f32x16 acc[2], nl[2];
        bf16x8 rq[2][4];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
          for (int s = 0; s < 4; ++s) rq[qb][s] = read_row_frag(Qs, qb * 32 + frow, s, fh);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 l4 = *(const f32x4*)(rc + qb * 32 + 8 * g + 4 * fh);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              nl[qb][4 * g + e] = -l4[e] * LOG2E;
              acc[qb][4 * g + e] = PRE ? nl[qb][4 * g + e] : 0.f;
            }
          }
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
          for (int s = 0; s < 4; ++s) acc[qb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rq[qb][s], kf[s], acc[qb], 0, 0, 0);
        const bool ragged = t * 64 + 64 > p.Sq;        // uniform: the last tile of a head only
        float ts = 0.f;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          float sj[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 4 * g + e;
              float pr = fast_exp2(PRE ? acc[qb][r] : fmaf(acc[qb][r], c, nl[qb][r]));
              if (ragged) pr = t * 64 + qb * 32 + 8 * g + 4 * fh + e < p.Sq ? pr : 0.f;
              sj[e] += pr;
            }
          ts += (sj[0] + sj[1]) + (sj[2] + sj[3]);
        }
        col += ts;
      }
    }
    WAIT_VM0();
    __syncthreads();
    h = hn;
    st = sn;
  }
  const float other = __shfl_xor(col, 32);
  if (wave_active && kstored && fh == 0)
    p.part[((long long)b * p.G + grp) * p.Skv + k0 + frow] = (col + other) * (1.f / (float)p.H);
}

// ============================================================================= prompt-to-prompt editing
// A batch of prompts denoised from the same latents; sample b with s = src[b] >= 0 is "edited": per head
//   P0 = softmax(scale Q[s] K[s]^T)   the source's probabilities at the same query positions,   P1 = softmax(scale Q[b] K[b]^T)
//   A[q][j] = c[b][j] sum_k P0[q][k] Mt[b][j][k] + d[b][j] P1[q][j],   O[b] = A V[b]            (no renormalisation)
// in ONE launch over the whole batch.  The branch is per workgroup: one of an unedited sample (src[b] < 0) stages its own K and V,
// runs the building blocks as xattn_fwd_kernel does (same bits) and reads no table; one of an edited sample stages K of the
// source, its own K and V (KB = ceil(Skv / 32) half tiles of 32 keys each, through descriptors that end with the sample's last
// row: padding slots arrive as zeros and score -inf), Mt[b] and c[b] / d[b], and every wave walks its 128-query units with the
// Q fragments of both samples resident (two LDS-DMA images per wave, one unit ahead).
// The mapper product needs no shuffle: S^T is keys x queries, and the un-normalised bf16 P0^T fragments pf0[] that the softmax
// leaves are the B operand of mfma_f32_32x32x16_bf16 exactly as the value product uses them, so (Mt P0^T)[j][q] is one more
// product of that shape, 2 KB^2 MFMAs per 32 queries, whose result lands in the layout P1^T has.  Slot (fh, i) of fragment ks
// holds key 16 ks + 4 fh + (i & 3) + 8 (i >> 2); the Mt image is written with the two middle quads of every 16 columns swapped,
// so that a lane's A fragment is one 16-byte read of row j (pitch KB * 64 + 16 bytes).  Mt is staged by ordinary loads, not by
// LDS-DMA: rows are ldm wide and columns at or past Skv must be ZERO (P0 is 0 there, but 0 x anything the caller left is not).
// Each softmax has its own maximum and sum (a spike in the source cannot underflow the target).  The mixture is formed in fp32,
// mix = fmaf(mapped, c (sum1 / sum0), d e1), rounded to bf16 ONCE, and O is scaled by 1 / sum1 at the end as in the plain kernel:
// with c = 0, d = 1 that is fmaf(x, 0, e1) = e1, the bits of xattn_fwd_kernel.  No atomics: the same bits every run.
// Units per workgroup differ: an edited unit is 54 MFMAs and two softmaxes where a plain one is 24 and one, and an edited workgroup
// stages twice as much, so an edited sample's workgroups take upw_edit units and an unedited sample's upw_plain (attn_plan_edit
// balances them: with one count for both, 28.6 - 34.9 us at 10 heads x 4096 queries against 19.2 with 8 and 3).
// LDS: 3 KB 4096 (K, V, source K) + KB 32 (KB 64 + 16) (Mt) + KB 256 (c, d) + 4 x 4096 (O images, the swizzled form) +
// 8 x 4096 (Q images): 106 752 bytes at three key blocks -- one workgroup per CU.
template <int KB>
__global__ __launch_bounds__(256, KB == 1 ? 2 : 1) void xattn_edit_fwd_kernel(const AttnEditP p, int upw_plain, int upw_edit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MP = KB * 64 + 16;                               // bytes of an Mt row in LDS
  char* const K1sm = smem;
  char* const Vsm = smem + KB * 4096;
  char* const K0sm = smem + 2 * KB * 4096;
  char* const Mtsm = smem + 3 * KB * 4096;
  float* const cdsm = (float*)(Mtsm + KB * 32 * MP);             // c[KB * 32], then d[KB * 32]; zeros past Skv
  char* const Osm = (char*)(cdsm + 2 * KB * 32);                 // 4 waves x 32 rows x 128 bytes, then the 8 Q images
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  // blockIdx.x counts the workgroups that have work, the edited samples' first (the longer ones), then the unedited samples':
  // H x splits each, with the split count of its kind.  A 1-D grid without idle workgroups: dispatch order deals it evenly over
  // the XCDs whatever the mix (a 3-D grid with early exits put 40 workgroups on one XCD's 32 CUs: two rounds there).
  const int nu = (p.Sq + 127) >> 7;
  const int s_edit = (nu + upw_edit - 1) / upw_edit, s_plain = (nu + upw_plain - 1) / upw_plain;
  int id = blockIdx.x, b = -1;
  for (int pass = 0; pass < 2 && b < 0; ++pass)
    for (int bb = 0; bb < p.B; ++bb) {
      if ((p.src[bb] >= 0) != (pass == 0)) continue;
      const int cnt = p.H * (pass == 0 ? s_edit : s_plain);
      if (id < cnt) { b = bb; break; }
      id -= cnt;
    }
  if (b < 0) return;                                             // (never: the grid is sized by the same count)
  const int sb = __builtin_amdgcn_readfirstlane(p.src[b]);
  const bool ed = sb >= 0;
  const int upw = ed ? upw_edit : upw_plain, splits = ed ? s_edit : s_plain;
  const int head = id / splits, split = id % splits;
  const int u_begin = split * upw, u_end = min(nu, u_begin + upw);
  const float sc = p.q_prescaled ? 1.f : p.scale * LOG2E;
  {                                                              // waves 0 / 1: the 32 rows of every K block, waves 2 / 3: of every V block
    const bool isv = wave >= 2;
    const int ld = isv ? p.ldv : p.ldk;
    const bf16* base = (isv ? p.V : p.K) + (long long)b * p.Skv * ld + head * 64;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const TileSrc src = tile_src(base + (long long)kb * 32 * ld, ld, p.Skv - kb * 32, wave & 1, lane);
      stage_tile(src, 0, (isv ? Vsm : K1sm) + kb * 4096, wave & 1);
    }
    if (ed && !isv) {
      const bf16* base0 = p.K + (long long)sb * p.Skv * p.ldk + head * 64;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const TileSrc src = tile_src(base0 + (long long)kb * 32 * p.ldk, p.ldk, p.Skv - kb * 32, wave & 1, lane);
        stage_tile(src, 0, K0sm + kb * 4096, wave & 1);
      }
    }
  }
  if (ed) {
    const bf16* Mtb = p.Mt + (long long)b * p.Skv * p.ldm;
    for (int idx = tid; idx < KB * 32 * KB * 4; idx += 256) {    // 8-column pieces of the KB * 32 x KB * 32 image
      const int row = idx / (KB * 4), c8 = idx % (KB * 4);
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (bf16)0.f;
      if (row < p.Skv && 8 * c8 < p.Skv) {                       // (ldm is a multiple of 8 and >= Skv: the piece lies inside the row)
        const bf16x8 g = *(const bf16x8*)(Mtb + (long long)row * p.ldm + 8 * c8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 8 * c8 + j < p.Skv ? g[j] : (bf16)0.f;
      }
      bf16x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo[j] = v[j]; hi[j] = v[4 + j]; }
      char* const dst = Mtsm + row * MP + (c8 >> 1) * 32 + (c8 & 1) * 8;
      *(bf16x4*)dst = lo;                                        // columns 0..3 | 8..11 | 4..7 | 12..15 of every 16
      *(bf16x4*)(dst + 16) = hi;
    }
    for (int idx = tid; idx < 2 * KB * 32; idx += 256) {
      const int key = idx % (KB * 32);
      const float* const t = idx < KB * 32 ? p.c : p.d;
      cdsm[idx] = key < p.Skv ? t[(long long)b * p.Skv + key] : 0.f;
    }
  }
  const AttnFragOff fo = attn_frag_off(lane);
  // this wave's Q image, one unit ahead, and the same rows of the source sample
  const XattnQStage qs1 = {tile_src(p.Q + (long long)b * p.Sq * p.ldq + head * 64, p.ldq, p.Sq, 0, lane), Osm + 4 * 4096 + wave * 8192};
  const XattnQStage qs0 = {tile_src(p.Q + (long long)(ed ? sb : b) * p.Sq * p.ldq + head * 64, p.ldq, p.Sq, 0, lane), qs1.img + 4096};
  auto stage_q = [&](int row0) {
    qs1.stage(row0);
    if (ed) qs0.stage(row0);
  };
  if (u_begin < u_end) stage_q(u_begin * 128 + wave * 32);
  WAIT_VM0();
  __syncthreads();
  for (int u = u_begin; u < u_end; ++u) {
    WAIT_VM0();                                                  // this wave's Q images (and its stores of the last unit)
    bf16x8 qf1[4], qf0[4];
    qs1.load(qf1, fo);
    if (ed) qs0.load(qf0, fo);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (u + 1 < u_end) stage_q((u + 1) * 128 + wave * 32);
    bf16x8 pf[2 * KB];
    float l1, mx;
    if (ed) {
      f32x16 mp[KB];                                             // (Mt P0^T)[j][q], P0 un-normalised
      float l0;
      {
        f32x16 s0[KB];
        bf16x8 pf0[2 * KB];
        xattn_scores<KB>(K0sm, fo, qf0, s0);
        xattn_mask_keys<KB, KB - 1>(s0, p.Skv, fh);              // padding slots of the last block
        l0 = xattn_softmax_bf16<KB>(s0, sc, mx, pf0);
#pragma unroll
        for (int jb = 0; jb < KB; ++jb)
#pragma unroll
          for (int ks = 0; ks < 2 * KB; ++ks) {
            const bf16x8 mf = *(const bf16x8*)(Mtsm + (jb * 32 + frow) * MP + ks * 32 + fh * 16);
            mp[jb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mf, pf0[ks], ks == 0 ? zero_f32x16() : mp[jb], 0, 0, 0);
          }
      }
      f32x16 s1[KB];
      xattn_scores<KB>(K1sm, fo, qf1, s1);
      xattn_mask_keys<KB, KB - 1>(s1, p.Skv, fh);
      l1 = xattn_softmax_f32<KB>(s1, sc, mx);
      const float ratio = l1 / l0;                               // P0 = e0 / sum0, and O is divided by sum1 at the end
#pragma unroll
      for (int jb = 0; jb < KB; ++jb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 cj = *(const f32x4*)(cdsm + jb * 32 + 8 * g + 4 * fh);
          const f32x4 dj = *(const f32x4*)(cdsm + KB * 32 + jb * 32 + 8 * g + 4 * fh);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = 4 * g + j;
            pf[2 * jb + (i >> 3)][i & 7] = (bf16)fmaf(mp[jb][i], cj[j] * ratio, dj[j] * s1[jb][i]);
          }
        }
    } else {
      f32x16 s1[KB];
      xattn_scores<KB>(K1sm, fo, qf1, s1);
      xattn_mask_keys<KB, KB - 1>(s1, p.Skv, fh);
      l1 = xattn_softmax_bf16<KB>(s1, sc, mx, pf);
    }
    f32x16 oacc[2];                                              // O^T[d][q] = V^T[d][key] A^T[key][q]
    xattn_pv<KB>(Vsm, fo, pf, oacc);
    const float inv = 1.f / l1;
    store_o_image_swz(Osm + wave * 4096, lane, [&](int db, int i) { return oacc[db][i] * inv; },
                      p.O + (long long)b * p.Sq * p.ldo + head * 64, p.ldo, u * 128 + wave * 32, p.Sq);
  }
}

// ============================================================================= few queries, keys split across the waves
// O = softmax(scale [Q K1^T | Q K2^T]) [V1 ; V2]: at most 32 queries over ONE softmax of two key sets read in place (the
// Perceiver Resampler of the IP-Adapter "plus" files: 16 latents over 257 image rows and the 16 latents themselves; K1 / V1 and
// K2 / V2 are column blocks of two different projections, Tape::build_resampler).  There is no parallelism over queries at this
// shape -- attn_q_kernel would run one wave of four per (batch, head) down a serial key loop -- so the KEYS are what a
// workgroup's waves share out: all four hold the same 32-query fragments (rows past Sq read as zeros and are never stored), the
// 32-key blocks of set 1 followed by the block of set 2 are dealt round-robin (wave w: blocks w, w + 4, ...), and every wave
// runs an online softmax over its blocks: own K / V half tiles (32 rows x 128 bytes each, the layout and the loader of every
// other tile of this file) in a 2-deep ring of its own, the next block in flight under the current one, no barrier in the loop.
// Every block is staged through a descriptor that STARTS at the block's first row and ends with the set's last row, so the
// rows behind a set's tail -- the next sample's, another tensor's, or anything else the allocation holds -- are never read:
// they arrive as zeros, their scores are set to -inf, and a NaN there cannot reach 0 x V.
// The (max, sum, O^T) partials then meet in LDS (a wave's own, by now idle, ring) and all 256 threads merge them in wave order
// 0..3 with fmaf: no atomics, the same bits every run.  A wave without a block leaves (-inf, 0, 0); its factor exp2(-inf - M)
// is an exact zero, and M is finite because wave 0 always has block 0.  lse is that of the union.
#define FEWQ_WAVE_BYTES 16384     // 2 x (K half tile + V half tile); afterwards [64 d][32 q] fp32 partial O^T + 32 maxima + 32 sums
__global__ __launch_bounds__(256) void attn_fewq_kernel(const AttnP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Qsm = smem + 4 * FEWQ_WAVE_BYTES;                  // 32 rows x 128 bytes
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const int head = blockIdx.x, b = blockIdx.y;
  const float c = p.q_prescaled ? 1.f : p.scale * LOG2E;
  const bf16* Qb = p.Q + (long long)b * p.Sq * p.ldq + head * 64;
  const bf16* K1b = p.K + (long long)b * p.Skv * p.ldk + head * 64;
  const bf16* V1b = p.V + (long long)b * p.Skv * p.ldv + head * 64;
  const bf16* K2b = p.K2 ? p.K2 + (long long)b * p.Skv2 * p.ldk2 + head * 64 : nullptr;
  const bf16* V2b = p.V2 ? p.V2 + (long long)b * p.Skv2 * p.ldv2 + head * 64 : nullptr;
  const int nb1 = (p.Skv + 31) >> 5, nb = nb1 + ((p.Skv2 + 31) >> 5);
  // block `blk` of the union: its K rows -> dst, its V rows -> dst + 4096 (pieces 0 / 1 of a tile: rows 0..15, then 16..31)
  auto stage_blk = [&](int blk, char* dst) {
    const bool s2 = blk >= nb1;
    const int r0 = (s2 ? blk - nb1 : blk) * 32, left = (s2 ? p.Skv2 : p.Skv) - r0;
    const int ldk = s2 ? p.ldk2 : p.ldk, ldv = s2 ? p.ldv2 : p.ldv;
    const bf16* kb = (s2 ? K2b : K1b) + (long long)r0 * ldk;
    const bf16* vb = (s2 ? V2b : V1b) + (long long)r0 * ldv;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      stage_tile(tile_src(kb, ldk, left, h, lane), 0, dst, h);
      stage_tile(tile_src(vb, ldv, left, h, lane), 0, dst + 4096, h);
    }
  };
  char* const my = smem + wave * FEWQ_WAVE_BYTES;
  if (wave < 2) stage_tile(tile_src(Qb, p.ldq, p.Sq, wave, lane), 0, Qsm, wave);
  int blk = wave;
  if (blk < nb) stage_blk(blk, my);
  const AttnFragOff fo = attn_frag_off(lane);
  WAIT_VM0();
  __syncthreads();                                               // the Q image (waves 0 / 1 staged it)
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(Qsm + fo.rf[s]);
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;                          // log2 domain; l_run: this half's 16 keys of every block
  f32x16 oacc[2] = {zero16, zero16};
  for (int i = 0; blk < nb; blk += 4, ++i) {
    char* const cur = my + (i & 1) * 8192;
    WAIT_VM0();                                                  // this block's rows have landed
    if (blk + 4 < nb) stage_blk(blk + 4, my + ((i + 1) & 1) * 8192);   // (its last reader: iteration i - 1, closed below)
    const bool s2 = blk >= nb1;
    const int valid = (s2 ? p.Skv2 : p.Skv) - (s2 ? blk - nb1 : blk) * 32;     // >= 1; >= 32: a full block
    // S^T[key][q] = K . Q^T
    f32x16 sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(cur + fo.rf[0]), qf[0], zero16, 0, 0, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(cur + fo.rf[s]), qf[s], sacc, 0, 0, 0);
    if (valid < 32) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[r] = (r & 3) + 8 * (r >> 2) + 4 * fh < valid ? sacc[r] : -INFINITY;
    }
    float mx = sacc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
    const float m_new = fmaxf(m_run, xhalf_max(mx) * c);         // finite: the block holds a valid key
    const float alpha = fast_exp2(m_run - m_new);                // first block: exp2(-inf) = 0 on a zero accumulator
    float ls = 0.f;
    bf16x8 pf[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = fast_exp2(fmaf(sacc[r], c, -m_new));       // masked key: exp2(-inf) = 0
      ls += e;
      pf[r >> 3][r & 7] = (bf16)e;
    }
    l_run = fmaf(l_run, alpha, ls);
    m_run = m_new;
    // O^T[d][q] = alpha O^T + V^T[d][key] P^T[key][q]
#pragma unroll
    for (int db = 0; db < 2; ++db) {
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            read_transposed_frag_at(cur + 4096 + fo.tr[db][0] + ks * 2048, cur + 4096 + fo.tr[db][1] + ks * 2048), pf[ks], oacc[db], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // every read of `cur` is done before a later DMA may land in it
  }
  // this wave's partial into its own ring (no DMA is in flight: each staged block was waited for and consumed)
  float* const part = (float*)my;
  float* const ml = (float*)(my + 8192);
  const float l_tot = xhalf_sum(l_run);                          // both halves rescaled by the same alpha every block
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(db * 32 + 8 * (r >> 2) + 4 * fh + (r & 3)) * 32 + frow] = oacc[db][r];
  if (fh == 0) { ml[frow] = m_run; ml[32 + frow] = l_tot; }
  __syncthreads();
  // merge: thread -> query tid & 31, eight output columns; partials in wave order
  const int q = tid & 31, ch = tid >> 5;
  float f[4], M = -INFINITY, L = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) M = fmaxf(M, *(const float*)(smem + w * FEWQ_WAVE_BYTES + 8192 + q * 4));
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    f[w] = fast_exp2(*(const float*)(smem + w * FEWQ_WAVE_BYTES + 8192 + q * 4) - M);
    L = fmaf(f[w], *(const float*)(smem + w * FEWQ_WAVE_BYTES + 8192 + (32 + q) * 4), L);
  }
  if (q >= p.Sq) return;                                         // padded query rows
  const float inv = 1.f / L;
  bf16* const orow = p.O + ((long long)b * p.Sq + q) * p.ldo + head * 64 + ch * 8;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    bf16x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) acc = fmaf(f[w], *(const float*)(smem + w * FEWQ_WAVE_BYTES + ((ch * 8 + g * 4 + j) * 32 + q) * 4), acc);
      o[j] = (bf16)(acc * inv);
    }
    *(bf16x4*)(orow + g * 4) = o;                                // 8-byte stores: ldo % 4
  }
  if (p.lse && ch == 0) p.lse[((long long)b * p.H + head) * p.Sq + q] = (M + log2f(L)) * 0.6931471805599453f;
}

// ============================================================================= cross-attention backward, ONE pass
// Few keys (the text context: 77 tokens -> KB = 3 blocks of 32), many queries, head_dim 64.  The general path costs three
// launches (delta, dQ + dK/dV roles, split reduce) that each stream Q / dO again and are latency-bound on their short
// key loops.  Here a workgroup owns a run of 128-query units of one (batch, head): K and V stay in LDS for its whole
// life, a unit's Q / dO tiles (+ lse) arrive by LDS-DMA one unit ahead, delta = rowsum(dO * O) is formed in-kernel
// (dO from the staged tile, O prefetched from HBM one unit ahead), and both orientations run off the same tiles:
//   query on the lane (wave w = queries 32w..32w+31):  S^T, dP^T -> dS^T -> dQ^T = K^T dS^T           (written per unit)
//   key on the lane   (wave w = keys 32w..32w+31, w < KB):  S, dP -> P, dS -> dV^T += dO^T P, dK^T += Q^T dS
// dK / dV partial sums of the workgroup go to p.dkv_part[split] (fixed-order reduce, attn_dkv_reduce_kernel) or, with
// one split, straight to dK / dV.
template <int KB>
__global__ __launch_bounds__(256, 2) void xattn_bwd_kernel(const AttnP p, int upw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS: K rows 0..127 | V rows 0..127 (two 64-row tiles each; 32 KB) | ONE stage: Q tiles 0,1 | dO tiles 0,1 | lse | delta
  // = 65 KB, two workgroups per CU: the other workgroup's compute covers this one's DMA wait (the stage is not double
  // buffered: with one wave per SIMD and 98 KB the single resident workgroup ran its dependency chains back to back,
  // 10 us per unit)
  char* const Ksm = smem;
  char* const Vsm = smem + 2 * TILE_BYTES;
  char* const S0 = smem + 4 * TILE_BYTES;
  float* const rc = (float*)(S0 + 4 * TILE_BYTES);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const XattnCtx x = xattn_ctx<128>(p, upw);
  const int head = x.head, b = x.b, u_begin = x.u_begin, u_end = x.u_end, skv_b = x.skv_b;
  const float c = x.c;

  const TileSrc qsrc = tile_src(x.Qb, p.ldq, p.Sq, wave, lane), dosrc = tile_src(x.dOb, p.lddo, p.Sq, wave, lane);
  auto stage_unit = [&](int u) {
    const int r0 = u * 128;
    stage_tile(qsrc, r0, S0, wave);
    stage_tile(qsrc, r0 + 64, S0 + TILE_BYTES, wave);
    stage_tile(dosrc, r0, S0 + 2 * TILE_BYTES, wave);
    stage_tile(dosrc, r0 + 64, S0 + 3 * TILE_BYTES, wave);
    if (wave < 2) {
      int r = r0 + wave * 64 + lane;
      r = r < p.Sq ? r : p.Sq - 1;
      lds_dma4(x.lseb + r, S0 + 4 * TILE_BYTES + wave * 256);
    }
  };
  // delta: thread = (query of the unit, half of the head dimension); its O values are fetched together with the stage
  const int dq_l = tid >> 1, dhalf = tid & 1;
  bf16x8 o_pf[4];
  auto fetch_o = [&](int u) {
    int r = u * 128 + dq_l;
    r = r < p.Sq ? r : p.Sq - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) o_pf[i] = *(const bf16x8*)(x.Ob + (long long)r * p.ldo + dhalf * 32 + 8 * i);
  };

  {
    const TileSrc ksrc = tile_src(x.Kb, p.ldk, p.Skv, wave, lane), vsrc = tile_src(x.Vb, p.ldv, p.Skv, wave, lane);
    stage_tile(ksrc, 0, Ksm, wave);
    stage_tile(vsrc, 0, Vsm, wave);
    if (KB > 2) {
      stage_tile(ksrc, 64, Ksm + TILE_BYTES, wave);
      stage_tile(vsrc, 64, Vsm + TILE_BYTES, wave);
    }
  }
  if (u_begin < u_end) {
    stage_unit(u_begin);
    fetch_o(u_begin);
  }
  // key-on-the-lane role: this wave's 32 keys as B-operand fragments, for the whole kernel
  int krow = wave * 32 + frow;
  const bool kstored = krow < p.Skv, kvalid = krow < skv_b;
  krow = kstored ? krow : p.Skv - 1;
  const bool wave_keys = wave < KB && wave * 32 < p.Skv;       // wave-uniform
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] = dv[i][r] = 0.f;
  // this wave's keys as B-operand fragments come from the K / V images in LDS, per query block (kept in registers for the
  // whole kernel they cost 32 VGPRs and the 256-register budget of two workgroups per CU spills)
  const bool wave_pad = wave * 32 + 32 > skv_b;                 // wave-uniform: this wave's key block holds padding keys
  const char* const Kmine = Ksm + (wave >> 1) * TILE_BYTES;
  const char* const Vmine = Vsm + (wave >> 1) * TILE_BYTES;
  const int kmine_row = (wave & 1) * 32 + frow;

  for (int u = u_begin; u < u_end; ++u) {
    WAIT_VM0();
    __syncthreads();                                             // the unit's tiles, lse and this thread's O values are here
    {
      const char* dt = S0 + (2 + (dq_l >> 6)) * TILE_BYTES;
      const int row = dq_l & 63;
      float dsum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 d = *(const bf16x8*)(dt + row * 128 + (((dhalf * 4 + i) ^ swz_x(row)) << 4));
#pragma unroll
        for (int j = 0; j < 8; ++j) dsum += (float)d[j] * (float)o_pf[i][j];
      }
      dsum += dpp_move<0xB1>(dsum);                          // lane ^ 1, a DPP move
      if (dhalf == 0) {                       // the unit's row constants, negated: C operand of dP, addend of the exp2 argument
        const bool rv = u * 128 + dq_l < p.Sq;             // rows past Sq (ragged last unit): P = exp2(-inf) = 0
        rc[128 + dq_l] = rv ? -dsum : 0.f;
        rc[dq_l] = rv ? -rc[dq_l] * LOG2E : -INFINITY;
      }
    }
    __syncthreads();

    // ---- query on the lane: dQ of this wave's 32 queries
    {
      const char* Qt = S0 + (wave >> 1) * TILE_BYTES;
      const char* dOt = S0 + (2 + (wave >> 1)) * TILE_BYTES;
      const int rb0 = (wave & 1) * 32;
      const int qg = u * 128 + wave * 32 + frow;
      bf16x8 qf[4], dof[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qf[s] = read_row_frag(Qt, rb0 + frow, s, fh);
        dof[s] = read_row_frag(dOt, rb0 + frow, s, fh);
      }
      const float nlse2 = rc[wave * 32 + frow], ndlt = rc[128 + wave * 32 + frow];
      f32x16 negd;
#pragma unroll
      for (int r = 0; r < 16; ++r) negd[r] = ndlt;
      f32x16 oacc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
#pragma unroll 1
      for (int kb = 0; kb < KB; ++kb) {
        const char* Kt = Ksm + (kb >> 1) * TILE_BYTES;
        const char* Vt = Vsm + (kb >> 1) * TILE_BYTES;
        const int kr0 = (kb & 1) * 32;
        f32x16 sacc, dpacc;
        {
          bf16x8 kfr[4], vfr[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            kfr[s] = read_row_frag(Kt, kr0 + frow, s, fh);
            vfr[s] = read_row_frag(Vt, kr0 + frow, s, fh);
          }
          const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0], qf[0], zero16, 0, 0, 0);
          dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0], dof[0], negd, 0, 0, 0);
#pragma unroll
          for (int s = 1; s < 4; ++s) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[s], qf[s], sacc, 0, 0, 0);
            dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[s], dof[s], dpacc, 0, 0, 0);
          }
        }
        bf16x8 tfr[2][2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db) tfr[k2][db] = read_transposed_frag<true>(Kt, kr0 + k2 * 16, db * 32, lane);
        bf16x8 pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pr = fast_exp2(fmaf(sacc[r], c, nlse2));
          if (kb * 32 + 32 > skv_b)                               // uniform: only the key block that holds padding keys
            pr = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh < skv_b ? pr : 0.f;
          pf[r >> 3][r & 7] = (bf16)(pr * dpacc[r]);
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db)
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfr[k2][db], pf[k2], oacc[db], 0, 0, 0);
      }
      if (qg < p.Sq) {
        bf16* dst0 = p.dQ + ((long long)b * p.Sq + qg) * p.lddq + head * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            bf16* dst = dst0 + db * 32 + 8 * g + 4 * fh;
            bf16x4 o;
            if (p.accum_dq) o = *(const bf16x4*)dst;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (bf16)(oacc[db][4 * g + j] * p.scale + (p.accum_dq ? (float)o[j] : 0.f));
            *(bf16x4*)dst = o;
          }
      }
    }
    // ---- key on the lane: dK / dV of this wave's 32 keys, the unit's four 32-query blocks
    if (wave_keys) {
#pragma unroll 1
      for (int qb = 0; qb < 4; ++qb) {
        const char* Qt = S0 + (qb >> 1) * TILE_BYTES;
        const char* dOt = S0 + (2 + (qb >> 1)) * TILE_BYTES;
        const int rb0 = (qb & 1) * 32;
        f32x16 sacc, dpacc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {                            // dP starts from -delta[q] (row = register index)
          const f32x4 d4 = *(const f32x4*)(rc + 128 + qb * 32 + 8 * g + 4 * fh);
#pragma unroll
          for (int j = 0; j < 4; ++j) dpacc[4 * g + j] = d4[j];
        }
        {
          bf16x8 qfr[4], kf[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            qfr[s] = read_row_frag(Qt, rb0 + frow, s, fh);
            kf[s] = read_row_frag(Kmine, kmine_row, s, fh);
          }
          const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[0], kf[0], zero16, 0, 0, 0);
#pragma unroll
          for (int s = 1; s < 4; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[s], kf[s], sacc, 0, 0, 0);
        }
        {
          bf16x8 dfr[4], vf[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            dfr[s] = read_row_frag(dOt, rb0 + frow, s, fh);
            vf[s] = read_row_frag(Vmine, kmine_row, s, fh);
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[s], vf[s], dpacc, 0, 0, 0);
        }
        bf16x8 dot[2][2], qt[2][2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dot[k2][db] = read_transposed_frag<true>(dOt, rb0 + k2 * 16, db * 32, lane);
            qt[k2][db] = read_transposed_frag<true>(Qt, rb0 + k2 * 16, db * 32, lane);
          }
        bf16x8 pfr[2], dsfr[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 l4 = *(const f32x4*)(rc + qb * 32 + 8 * g + 4 * fh);     // -lse * log2(e) of 4 consecutive query rows
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = 4 * g + j;
            float pr = fast_exp2(fmaf(sacc[r], c, l4[j]));
            if (wave_pad) pr = kvalid ? pr : 0.f;                // only the wave whose key block holds padding keys
            const float ds = pr * dpacc[r];
            pfr[g >> 1][(g & 1) * 4 + j] = (bf16)pr;
            dsfr[g >> 1][(g & 1) * 4 + j] = (bf16)ds;
          }
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot[k2][db], pfr[k2], dv[db], 0, 0, 0);
            dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt[k2][db], dsfr[k2], dk[db], 0, 0, 0);
          }
      }
    }
    __syncthreads();                                             // every wave is done with the stage
    if (u + 1 < u_end) {
      stage_unit(u + 1);
      fetch_o(u + 1);
    }
  }
  if (!wave_keys || !kstored) return;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] *= p.q_prescaled ? 0.6931471805599453f : p.scale;
  if (p.nsplit > 1) {
    float* pr = p.dkv_part + ((((long long)x.split * p.B + b) * p.H + head) * p.Skv + krow) * 128;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * fh;
        f32x4 a, cc;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = dk[db][4 * g + j]; cc[j] = dv[db][4 * g + j]; }
        *(f32x4*)(pr + d) = a;
        *(f32x4*)(pr + 64 + d) = cc;
      }
    return;
  }
  bf16* dKr = p.dK + ((long long)b * p.Skv + krow) * p.lddk + head * 64;
  bf16* dVr = p.dV + ((long long)b * p.Skv + krow) * p.lddv + head * 64;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = db * 32 + 8 * g + 4 * fh;
      bf16x4 ok, ov;
      if (p.accum_dkv) {
        ok = *(const bf16x4*)(dKr + d);
        ov = *(const bf16x4*)(dVr + d);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ok[j] = (bf16)(dk[db][4 * g + j] + (p.accum_dkv ? (float)ok[j] : 0.f));
        ov[j] = (bf16)(dv[db][4 * g + j] + (p.accum_dkv ? (float)ov[j] : 0.f));
      }
      *(bf16x4*)(dKr + d) = ok;
      *(bf16x4*)(dVr + d) = ov;
    }
}

// ============================================================================= cross-attention backward, v2 (round 6)
// The one-pass kernel above runs BOTH orientations on every wave, one after the other, off a single-buffered 128-query
// stage: per unit a wave walks LDS read -> MFMA -> exp -> MFMA chains of 100 MFMAs with nothing beside it on its SIMD but
// the other workgroup's wave, and the DMA of the next unit starts only when the unit is done (30 us for 42 MB of traffic).
// Here the unit is 64 queries, the stage is double buffered (the next unit's Q / dO / lse fly under this unit's work) and
// the waves SPECIALISE, so the two orientations run side by side on different SIMDs:
//   waves 0, 1  query on the lane: S^T, dP^T -> dS^T -> dQ^T = K^T dS^T of 32 queries each; dQ leaves through a per-wave
//               LDS image as whole 128-byte rows (the row-per-lane accumulator layout is sixteen 8-byte pieces over 32 lines)
//   waves 2, 3  key on the lane: S, dP -> P, dS -> dV^T += dO^T P, dK^T += Q^T dS.  KB = 3 key blocks x 2 query blocks
//               = 6 tasks of 16 MFMAs: wave 2 takes (kb 0, both query blocks) + (kb 2, queries 0..31), wave 3 takes
//               (kb 1, both) + (kb 2, queries 32..63) -- 48 MFMAs each against 36 on the dQ waves; the two partial sums
//               of key block 2 meet through LDS behind the loop, (wave 2) + (wave 3), a fixed order.
// LDS: K | V images (2 x 16 KB) + 2 stages x (Q tile | dO tile | lse | delta = 16.5 KB) + 2 x 4.5 KB dQ images = 74 KB:
// two workgroups per CU.  KB = 2 (<= 64 keys: the 52-token student context un-merged) and KB = 3 (77 keys); other key
// counts keep the kernel above.  PRE (Q prescaled by its projection, the product path): the scores leave the MFMA in the
// log2 domain with -lse log2(e) as the C operand, p = exp2(acc) with no per-score FMA.
template <int KB, bool PRE>
__global__ __launch_bounds__(256, 2) void xattn_bwd2_kernel(const AttnP p, int upw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STG = 2 * TILE_BYTES + 512;
  char* const Ksm = smem;
  char* const Vsm = smem + 2 * TILE_BYTES;
  char* const St = smem + 4 * TILE_BYTES;            // [2 stages][Q tile | dO tile | lse[64] | delta[64]]
  char* const Ost = St + 2 * STG;                    // [2 waves][32 rows x 144 bytes]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const XattnCtx x = xattn_ctx<64, PRE>(p, upw);
  const int head = x.head, b = x.b, u_begin = x.u_begin, u_end = x.u_end, skv_b = x.skv_b;
  const float c = x.c;

  const TileSrc qsrc = tile_src(x.Qb, p.ldq, p.Sq, wave, lane), dosrc = tile_src(x.dOb, p.lddo, p.Sq, wave, lane);
  auto stage_unit = [&](int u, int st) {
    char* const S0 = St + st * STG;
    const int r0 = u * 64;
    stage_tile(qsrc, r0, S0, wave);
    stage_tile(dosrc, r0, S0 + TILE_BYTES, wave);
    if (wave == 0) {
      int r = r0 + lane;
      r = r < p.Sq ? r : p.Sq - 1;
      lds_dma4(x.lseb + r, S0 + 2 * TILE_BYTES);
    }
  };
  // delta = rowsum(dO * O): thread = (query of the unit, quarter of the head dimension); O fetched one unit ahead
  const int dq_l = tid >> 2, dqt = tid & 3;
  bf16x8 o_pf[2];
  auto fetch_o = [&](int u) {
    int r = u * 64 + dq_l;
    r = r < p.Sq ? r : p.Sq - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) o_pf[i] = *(const bf16x8*)(x.Ob + (long long)r * p.ldo + dqt * 16 + 8 * i);
  };
  {
    const TileSrc ksrc = tile_src(x.Kb, p.ldk, p.Skv, wave, lane), vsrc = tile_src(x.Vb, p.ldv, p.Skv, wave, lane);
    stage_tile(ksrc, 0, Ksm, wave);
    stage_tile(vsrc, 0, Vsm, wave);
    if (KB > 2) {
      stage_tile(ksrc, 64, Ksm + TILE_BYTES, wave);
      stage_tile(vsrc, 64, Vsm + TILE_BYTES, wave);
    }
  }
  if (u_begin < u_end) {
    stage_unit(u_begin, 0);
    fetch_o(u_begin);
  }
  const bool key_wave = wave >= 2;
  // the shared head of a unit, executed by every wave: wait for the unit's tiles, start the next unit's, form delta.
  // Both role loops below call it once per unit, so every wave passes the same sequence of workgroup barriers.
  auto unit_head = [&](int u) -> char* {
    const int cur = (u - u_begin) & 1;
    char* const S0 = St + cur * STG;
    float* const rc = (float*)(S0 + 2 * TILE_BYTES);           // [0..63] lse -> -lse log2(e); [64..127] -delta
    WAIT_VM0();
    __syncthreads();                                           // unit u landed; every wave has left unit u - 1
    if (u + 1 < u_end) stage_unit(u + 1, cur ^ 1);             // flies under this unit's work
    {
      const char* dt = S0 + TILE_BYTES;
      float dsum = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bf16x8 d = *(const bf16x8*)(dt + dq_l * 128 + (((dqt * 2 + i) ^ swz_x(dq_l)) << 4));
#pragma unroll
        for (int j = 0; j < 8; ++j) dsum += (float)d[j] * (float)o_pf[i][j];
      }
      dsum += dpp_move<0xB1>(dsum);                            // lanes ^ 1, ^ 2: the four quarters of a query
      dsum += dpp_move<0x4E>(dsum);
      if (dqt == 0) {
        const bool rv = u * 64 + dq_l < p.Sq;                  // rows past Sq (ragged last unit): P = exp2(-inf) = 0
        rc[64 + dq_l] = rv ? -dsum : 0.f;
        rc[dq_l] = rv ? -rc[dq_l] * LOG2E : -INFINITY;
      }
    }
    if (u + 1 < u_end) fetch_o(u + 1);
    __syncthreads();
    return S0;
  };

  if (!key_wave) {
    // ================= waves 0, 1: query on the lane -- dQ of queries 32 wave .. 32 wave + 31 of every unit
    for (int u = u_begin; u < u_end; ++u) {
      const char* const S0 = unit_head(u);
      const char* const Qt = S0;
      const char* const dOt = S0 + TILE_BYTES;
      const float* const rc = (const float*)(S0 + 2 * TILE_BYTES);
      const int rb0 = wave * 32;
      const int qg = u * 64 + rb0;
      bf16x8 qf[4], dof[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qf[s] = read_row_frag(Qt, rb0 + frow, s, fh);
        dof[s] = read_row_frag(dOt, rb0 + frow, s, fh);
      }
      const float nlse2 = rc[rb0 + frow], ndlt = rc[64 + rb0 + frow];
      f32x16 negd, rowc;
#pragma unroll
      for (int r = 0; r < 16; ++r) { negd[r] = ndlt; rowc[r] = PRE ? nlse2 : 0.f; }
      f32x16 oacc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
#pragma unroll 1
      for (int kb = 0; kb < KB; ++kb) {
        const char* Kt = Ksm + (kb >> 1) * TILE_BYTES;
        const char* Vt = Vsm + (kb >> 1) * TILE_BYTES;
        const int kr0 = (kb & 1) * 32;
        f32x16 sacc, dpacc;
        {
          bf16x8 kfr[4], vfr[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            kfr[s] = read_row_frag(Kt, kr0 + frow, s, fh);
            vfr[s] = read_row_frag(Vt, kr0 + frow, s, fh);
          }
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[0], qf[0], rowc, 0, 0, 0);
          dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[0], dof[0], negd, 0, 0, 0);
#pragma unroll
          for (int s = 1; s < 4; ++s) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[s], qf[s], sacc, 0, 0, 0);
            dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[s], dof[s], dpacc, 0, 0, 0);
          }
        }
        bf16x8 tfr[2][2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db) tfr[k2][db] = read_transposed_frag<true>(Kt, kr0 + k2 * 16, db * 32, lane);
        bf16x8 pf[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pr = PRE ? fast_exp2(sacc[r]) : fast_exp2(fmaf(sacc[r], c, nlse2));
          if (kb * 32 + 32 > skv_b)                               // uniform: only the key block that holds padding keys
            pr = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh < skv_b ? pr : 0.f;
          pf[r >> 3][r & 7] = (bf16)(pr * dpacc[r]);
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int db = 0; db < 2; ++db)
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfr[k2][db], pf[k2], oacc[db], 0, 0, 0);
      }
      // dQ^T[d][q] -> LDS image [q][d] -> whole rows, 16 bytes per lane
      store_o_image_144(Ost + wave * (32 * 144), lane, [&](int db, int i) { return oacc[db][i] * p.scale; },
                        p.dQ + (long long)b * p.Sq * p.lddq + head * 64, p.lddq, qg, p.Sq, p.accum_dq != 0);
    }
    if (KB > 2) {                                                // the two barriers of the key waves' hand-over below
      __syncthreads();
      __syncthreads();
    }
    return;
  }

  // ================= waves 2, 3: key on the lane.  Accumulator slots: 0 = the wave's own key block (wave 2: kb 0, wave 3:
  // kb 1), 1 = its half of kb 2.  (The role loops are separate code paths so that these 128 registers are not live across
  // the dQ role's code: as one loop with a branch per unit the kernel needed 312 registers and spilled 110.)
  constexpr int NS = KB > 2 ? 2 : 1;
  f32x16 dk[NS][2], dv[NS][2];
#pragma unroll
  for (int sl = 0; sl < NS; ++sl)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) dk[sl][i][r] = dv[sl][i][r] = 0.f;
  const int kw = wave - 2;                                        // 0 / 1
  for (int u = u_begin; u < u_end; ++u) {
    const char* const S0 = unit_head(u);
    const char* const Qt = S0;
    const char* const dOt = S0 + TILE_BYTES;
    const float* const rc = (const float*)(S0 + 2 * TILE_BYTES);
    // three (key block, query block) tasks per wave (two when KB == 2); phases fenced (sched_barrier) so that hipcc does not
    // hoist the next phase's fragment reads over the MFMAs beside the 128 accumulator registers
    auto key_task = [&](const int kb, const int qb, f32x16 (&dkt)[2], f32x16 (&dvt)[2]) {
      if (kb * 32 >= p.Skv) return;                             // uniform
      const char* Kmine = Ksm + (kb >> 1) * TILE_BYTES;
      const char* Vmine = Vsm + (kb >> 1) * TILE_BYTES;
      const int kmine_row = (kb & 1) * 32 + frow;
      const bool kvalid = kb * 32 + frow < skv_b;
      const bool blk_pad = kb * 32 + 32 > skv_b;                // uniform: this key block holds padding keys
      const int rb0 = qb * 32;
      f32x16 sacc, dpacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {                            // rows = queries: the staged row constants ARE the C operands
        const f32x4 d4 = *(const f32x4*)(rc + 64 + rb0 + 8 * g + 4 * fh);
        const f32x4 l4 = *(const f32x4*)(rc + rb0 + 8 * g + 4 * fh);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dpacc[4 * g + j] = d4[j];
          sacc[4 * g + j] = PRE ? l4[j] : 0.f;
        }
      }
      {
        bf16x8 qfr[4], kf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          qfr[s] = read_row_frag(Qt, rb0 + frow, s, fh);
          kf[s] = read_row_frag(Kmine, kmine_row, s, fh);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[s], kf[s], sacc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        bf16x8 dfr[4], vf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          dfr[s] = read_row_frag(dOt, rb0 + frow, s, fh);
          vf[s] = read_row_frag(Vmine, kmine_row, s, fh);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[s], vf[s], dpacc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 pfr[2], dsfr[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 l4 = {0.f, 0.f, 0.f, 0.f};
        if (!PRE) l4 = *(const f32x4*)(rc + rb0 + 8 * g + 4 * fh);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j;
          float pr = PRE ? fast_exp2(sacc[r]) : fast_exp2(fmaf(sacc[r], c, l4[j]));
          if (blk_pad) pr = kvalid ? pr : 0.f;
          const float ds = pr * dpacc[r];
          pfr[g >> 1][(g & 1) * 4 + j] = (bf16)pr;
          dsfr[g >> 1][(g & 1) * 4 + j] = (bf16)ds;
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
        __builtin_amdgcn_sched_barrier(0);
        bf16x8 dot[2], qt[2];
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dot[db] = read_transposed_frag<true>(dOt, rb0 + k2 * 16, db * 32, lane);
          qt[db] = read_transposed_frag<true>(Qt, rb0 + k2 * 16, db * 32, lane);
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          dvt[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot[db], pfr[k2], dvt[db], 0, 0, 0);
          dkt[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt[db], dsfr[k2], dkt[db], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    key_task(kw, 0, dk[0], dv[0]);
    key_task(kw, 1, dk[0], dv[0]);
    if (KB > 2) key_task(2, kw, dk[NS - 1], dv[NS - 1]);
  }
  // ---- dK / dV out.  KB == 3: wave 3 hands its half of key block 2 to wave 2 through LDS (lane-private 16-byte slots:
  // both waves hold the same (key, d) elements on the same lanes); (wave 2) + (wave 3), always in that order.
  if (KB > 2) {
    __syncthreads();                                             // every wave is done with the stages
    float* const X = (float*)St;                                 // 16 slots x 64 lanes x 16 bytes = 16 KB
    if (wave == 3) {
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 a, cc;
#pragma unroll
          for (int j = 0; j < 4; ++j) { a[j] = dk[NS - 1][db][4 * g + j]; cc[j] = dv[NS - 1][db][4 * g + j]; }
          *(f32x4*)(X + ((db * 4 + g) * 2 + 0) * 256 + lane * 4) = a;
          *(f32x4*)(X + ((db * 4 + g) * 2 + 1) * 256 + lane * 4) = cc;
        }
    }
    __syncthreads();
    if (wave == 2) {
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 a = *(const f32x4*)(X + ((db * 4 + g) * 2 + 0) * 256 + lane * 4);
          const f32x4 cc = *(const f32x4*)(X + ((db * 4 + g) * 2 + 1) * 256 + lane * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { dk[NS - 1][db][4 * g + j] += a[j]; dv[NS - 1][db][4 * g + j] += cc[j]; }
        }
    }
  }
  const float dks = PRE ? 0.6931471805599453f : p.scale;         // dS^T Q' = scale log2(e) dS^T Q
#pragma unroll
  for (int sl = 0; sl < NS; ++sl) {
    if (sl == 1 && wave != 2) break;                              // the shared block leaves from wave 2
    const int kb = sl == 0 ? wave - 2 : 2;
    const int krow = kb * 32 + frow;
    if (krow >= p.Skv) continue;
    if (p.nsplit > 1) {
      float* pr = p.dkv_part + ((((long long)x.split * p.B + b) * p.H + head) * p.Skv + krow) * 128;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = db * 32 + 8 * g + 4 * fh;
          f32x4 a, cc;
#pragma unroll
          for (int j = 0; j < 4; ++j) { a[j] = dk[sl][db][4 * g + j] * dks; cc[j] = dv[sl][db][4 * g + j]; }
          *(f32x4*)(pr + d) = a;
          *(f32x4*)(pr + 64 + d) = cc;
        }
    } else {
      bf16* dKr = p.dK + ((long long)b * p.Skv + krow) * p.lddk + head * 64;
      bf16* dVr = p.dV + ((long long)b * p.Skv + krow) * p.lddv + head * 64;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = db * 32 + 8 * g + 4 * fh;
          bf16x4 ok, ov;
          if (p.accum_dkv) {
            ok = *(const bf16x4*)(dKr + d);
            ov = *(const bf16x4*)(dVr + d);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ok[j] = (bf16)(dk[sl][db][4 * g + j] * dks + (p.accum_dkv ? (float)ok[j] : 0.f));
            ov[j] = (bf16)(dv[sl][db][4 * g + j] + (p.accum_dkv ? (float)ov[j] : 0.f));
          }
          *(bf16x4*)(dKr + d) = ok;
          *(bf16x4*)(dVr + d) = ov;
        }
    }
  }
}

// ============================================================================= cross-attention backward, v3: FIVE products
// v2 above still computes S and dP twice (once per orientation): 7 matrix products and two exponentials per score for an
// algorithm that has 5 and one.  With <= 80 keys the whole key range of a (batch, head) sits in one workgroup, so dQ needs no
// sum across workgroups and the two orientations can share one evaluation: the KEY waves (key on the lane) compute S, dP ->
// P, dS once, feed dV^T += dO^T P and dK^T += Q^T dS from their accumulators as before, and drop dS (bf16) into an LDS
// image [key][query]; the dQ wave reads it back through the transpose read as the B operand of dQ^T = K^T dS^T (the same
// k-permutation as its A operand, the transposed K fragment), one unit behind the key waves.
//   wave 0 = dQ of all 64 queries of the previous unit (KB = 3: 20 MFMAs -- the sixth 16-key slice, keys 80..95, is padding
//   and skipped), waves 1 .. KB = key blocks 0 .. KB - 1 (32 MFMAs each); KB = 2 (33..64 keys) leaves wave 3 idle.
// 120 MFMAs and 96 exponentials per 64-query unit instead of 168 and 192, no accumulator hand-over behind the loop.
// LDS: K | V images of 96 rows (24 KB) + 2 stages x 16.5 KB + 2 dS images of 80 key rows (20 KB) = 77 KB: two workgroups
// per CU; the dQ wave's output image reuses the dS image it has just read into registers.
template <int KB, bool PRE>
__global__ __launch_bounds__(256, 2) void xattn_bwd3_kernel(const AttnP p, int upw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int STG = 2 * TILE_BYTES + 512;
  constexpr int KV_IMG = TILE_BYTES + TILE_BYTES / 2;            // 96 rows
  constexpr int DS_IMG = TILE_BYTES + 2048;                      // 80 key rows x 128 bytes (64 queries)
  char* const Ksm = smem;
  char* const Vsm = smem + KV_IMG;
  char* const St = smem + 2 * KV_IMG;                            // [2 stages][Q tile | dO tile | lse[64] | delta[64]]
  char* const Dsm = St + 2 * STG;                                // [2][80 keys][64 queries] bf16, tile format
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 31, fh = lane >> 5;
  const XattnCtx x = xattn_ctx<64, PRE>(p, upw);
  const int head = x.head, b = x.b, u_begin = x.u_begin, u_end = x.u_end, skv_b = x.skv_b;
  const float c = x.c;

  const TileSrc qsrc = tile_src(x.Qb, p.ldq, p.Sq, wave, lane), dosrc = tile_src(x.dOb, p.lddo, p.Sq, wave, lane);
  auto stage_unit = [&](int u, int st) {
    char* const S0 = St + st * STG;
    const int r0 = u * 64;
    stage_tile(qsrc, r0, S0, wave);
    stage_tile(dosrc, r0, S0 + TILE_BYTES, wave);
    if (wave == 0) {
      int r = r0 + lane;
      r = r < p.Sq ? r : p.Sq - 1;
      lds_dma4(x.lseb + r, S0 + 2 * TILE_BYTES);
    }
  };
  const int dq_l = tid >> 2, dqt = tid & 3;                       // delta: thread = (query of the unit, quarter of the head dim)
  bf16x8 o_pf[2];
  auto fetch_o = [&](int u) {
    int r = u * 64 + dq_l;
    r = r < p.Sq ? r : p.Sq - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) o_pf[i] = *(const bf16x8*)(x.Ob + (long long)r * p.ldo + dqt * 16 + 8 * i);
  };
  {
    const TileSrc ksrc = tile_src(x.Kb, p.ldk, p.Skv, wave, lane), vsrc = tile_src(x.Vb, p.ldv, p.Skv, wave, lane);
    stage_tile(ksrc, 0, Ksm, wave);
    stage_tile(vsrc, 0, Vsm, wave);
    if (KB > 2 && wave < 2) {                                     // rows 64..95: the first four 1 KiB pieces of the second tile
      stage_tile(ksrc, 64, Ksm + TILE_BYTES, wave);
      stage_tile(vsrc, 64, Vsm + TILE_BYTES, wave);
    }
  }
  if (u_begin < u_end) {
    stage_unit(u_begin, 0);
    fetch_o(u_begin);
  }
  // wave roles
  const bool key_wave = wave >= 1 && wave <= KB;
  const bool dq_wave = wave == 0;
  const int my_kb = wave - 1;                                     // key waves

  auto unit_head = [&](int u) -> char* {                          // (as in xattn_bwd2_kernel)
    const int cur = (u - u_begin) & 1;
    char* const S0 = St + cur * STG;
    float* const rc = (float*)(S0 + 2 * TILE_BYTES);
    WAIT_VM0();
    __syncthreads();                                              // unit u landed; unit u - 1 is complete (its dS image too)
    if (u + 1 < u_end) stage_unit(u + 1, cur ^ 1);
    {
      const char* dt = S0 + TILE_BYTES;
      float dsum = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bf16x8 d = *(const bf16x8*)(dt + dq_l * 128 + (((dqt * 2 + i) ^ swz_x(dq_l)) << 4));
#pragma unroll
        for (int j = 0; j < 8; ++j) dsum += (float)d[j] * (float)o_pf[i][j];
      }
      dsum += dpp_move<0xB1>(dsum);
      dsum += dpp_move<0x4E>(dsum);
      if (dqt == 0) {
        const bool rv = u * 64 + dq_l < p.Sq;
        rc[64 + dq_l] = rv ? -dsum : 0.f;
        rc[dq_l] = rv ? -rc[dq_l] * LOG2E : -INFINITY;
      }
    }
    if (u + 1 < u_end) fetch_o(u + 1);
    __syncthreads();
    return S0;
  };

  if (!key_wave) {
    // ================= dQ wave (and, with KB == 2, an idle wave that only keeps the barriers' count):
    // dQ^T[d][q] = K^T[d][key] dS^T[key][q] of the PREVIOUS unit, from its dS image
    auto dq_unit = [&](int u) {                                   // u: the unit whose dS image is complete
      char* const img = Dsm + ((u - u_begin) & 1) * DS_IMG;
      constexpr int NSL = KB > 2 ? 5 : 4;                         // 16-key slices that hold keys (< 80)
      f32x16 oacc[2][2];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[q2][i][r] = 0.f;
      // all dS fragments first: the image is then free and becomes this wave's output image
      bf16x8 dsf[2][NSL];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl)
          dsf[q2][sl] = read_transposed_frag<true>(img + (sl >> 2) * TILE_BYTES, (sl & 3) * 16, q2 * 32, lane);
#pragma unroll
      for (int sl = 0; sl < NSL; ++sl) {
        bf16x8 kt[2];
#pragma unroll
        for (int db = 0; db < 2; ++db) kt[db] = read_transposed_frag<true>(Ksm + (sl >> 2) * TILE_BYTES, (sl & 3) * 16, db * 32, lane);
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
          for (int db = 0; db < 2; ++db)
            oacc[q2][db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt[db], dsf[q2][sl], oacc[q2][db], 0, 0, 0);
      }
      const int r8 = lane >> 3, ch = lane & 7;
      bf16* dQb = p.dQ + (long long)b * p.Sq * p.lddq + head * 64 + ch * 8;
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
        char* const o2 = img + q2 * (32 * 144);                   // (2 x 4.5 KiB <= the 10 KiB image)
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            bf16x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (bf16)(oacc[q2][db][4 * g + j] * p.scale);
            *(bf16x4*)(o2 + frow * 144 + (db * 32 + 8 * g + 4 * fh) * 2) = o;
          }
        const int qg = u * 64 + q2 * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = i * 8 + r8;
          if (qg + row < p.Sq) {
            bf16x8 v = *(const bf16x8*)(o2 + row * 144 + ch * 16);
            bf16* dst = dQb + (long long)(qg + row) * p.lddq;
            if (p.accum_dq) {
              const bf16x8 old = *(const bf16x8*)dst;
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = (bf16)((float)v[j] + (float)old[j]);
            }
            *(bf16x8*)dst = v;
          }
        }
      }
    };
    for (int u = u_begin; u < u_end; ++u) {
      (void)unit_head(u);
      if (dq_wave && u > u_begin) dq_unit(u - 1);
    }
    if (u_begin < u_end) {
      __syncthreads();                                            // the key waves have finished the last unit's dS image
      if (dq_wave) dq_unit(u_end - 1);
    }
    return;
  }

  // ================= key waves: one key block each, S / dP / P / dS ONCE per (key block, query block)
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] = dv[i][r] = 0.f;
  const int kb = my_kb;
  const bool blk_live = kb * 32 < p.Skv;                          // uniform
  const char* const Kmine = Ksm + (kb >> 1) * TILE_BYTES;
  const char* const Vmine = Vsm + (kb >> 1) * TILE_BYTES;
  const int kmine_row = (kb & 1) * 32 + frow;
  const int key = kb * 32 + frow;
  const bool kvalid = key < skv_b;
  const bool blk_pad = kb * 32 + 32 > skv_b;                      // uniform: this key block holds padding keys
  for (int u = u_begin; u < u_end; ++u) {
    const char* const S0 = unit_head(u);
    const char* const Qt = S0;
    const char* const dOt = S0 + TILE_BYTES;
    const float* const rc = (const float*)(S0 + 2 * TILE_BYTES);
    char* const img = Dsm + ((u - u_begin) & 1) * DS_IMG;
#pragma unroll 1
    for (int qb = 0; qb < 2; ++qb) {
      const int rb0 = qb * 32;
      f32x16 sacc, dpacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 d4 = *(const f32x4*)(rc + 64 + rb0 + 8 * g + 4 * fh);
        const f32x4 l4 = *(const f32x4*)(rc + rb0 + 8 * g + 4 * fh);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dpacc[4 * g + j] = d4[j];
          sacc[4 * g + j] = PRE ? l4[j] : 0.f;
        }
      }
      {
        bf16x8 qfr[4], kf[4], dfr[4], vf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          qfr[s] = read_row_frag(Qt, rb0 + frow, s, fh);
          kf[s] = read_row_frag(Kmine, kmine_row, s, fh);
          dfr[s] = read_row_frag(dOt, rb0 + frow, s, fh);
          vf[s] = read_row_frag(Vmine, kmine_row, s, fh);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {                             // two independent accumulation chains, interleaved
          sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[s], kf[s], sacc, 0, 0, 0);
          dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[s], vf[s], dpacc, 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 pfr[2], dsfr[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 l4 = {0.f, 0.f, 0.f, 0.f};
        if (!PRE) l4 = *(const f32x4*)(rc + rb0 + 8 * g + 4 * fh);
        bf16x4 ds4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j;
          float pr = PRE ? fast_exp2(sacc[r]) : fast_exp2(fmaf(sacc[r], c, l4[j]));
          if (blk_pad) pr = kvalid ? pr : 0.f;
          const float ds = pr * dpacc[r];
          pfr[g >> 1][(g & 1) * 4 + j] = (bf16)pr;
          dsfr[g >> 1][(g & 1) * 4 + j] = (bf16)ds;
          ds4[j] = (bf16)ds;
        }
        // dS[key][q = rb0 + 8 g + 4 fh .. + 3] -> the image row of this lane's key (keys >= 80 have no row: they are padding)
        if (key < 80) *(bf16x4*)(img + (kb >> 1) * TILE_BYTES + swz_rc(kmine_row, rb0 + 8 * g + 4 * fh)) = ds4;
      }
      if (blk_live) {
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          __builtin_amdgcn_sched_barrier(0);
          bf16x8 dot[2], qt[2];
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dot[db] = read_transposed_frag<true>(dOt, rb0 + k2 * 16, db * 32, lane);
            qt[db] = read_transposed_frag<true>(Qt, rb0 + k2 * 16, db * 32, lane);
          }
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dot[db], pfr[k2], dv[db], 0, 0, 0);
            dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt[db], dsfr[k2], dk[db], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (u_begin < u_end) __syncthreads();                           // (the dQ waves' last hand-over)
  const int krow = kb * 32 + frow;
  if (krow >= p.Skv) return;
  const float dks = PRE ? 0.6931471805599453f : p.scale;
  if (p.nsplit > 1) {
    float* pr = p.dkv_part + ((((long long)x.split * p.B + b) * p.H + head) * p.Skv + krow) * 128;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * fh;
        f32x4 a, cc;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = dk[db][4 * g + j] * dks; cc[j] = dv[db][4 * g + j]; }
        *(f32x4*)(pr + d) = a;
        *(f32x4*)(pr + 64 + d) = cc;
      }
  } else {
    bf16* dKr = p.dK + ((long long)b * p.Skv + krow) * p.lddk + head * 64;
    bf16* dVr = p.dV + ((long long)b * p.Skv + krow) * p.lddv + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = db * 32 + 8 * g + 4 * fh;
        bf16x4 ok, ov;
        if (p.accum_dkv) {
          ok = *(const bf16x4*)(dKr + d);
          ov = *(const bf16x4*)(dVr + d);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ok[j] = (bf16)(dk[db][4 * g + j] * dks + (p.accum_dkv ? (float)ok[j] : 0.f));
          ov[j] = (bf16)(dv[db][4 * g + j] + (p.accum_dkv ? (float)ov[j] : 0.f));
        }
        *(bf16x4*)(dKr + d) = ok;
        *(bf16x4*)(dVr + d) = ov;
      }
  }
}

// row constants of the backward kernels: delta[0][b][h][q] = -sum_d dO[q][h*D+d] * O[q][h*D+d], delta[1][b][h][q] = -lse * log2(e);
// 8 lanes per (row, head), each sums D/8 elements
// (row, head) slots per thread, all requested before the first use: a thread with ONE pair of 16-byte loads in flight left the
// kernel latency-bound (9.6 us for 21 MB)
constexpr int ATTN_DELTA_ROWS = 4;
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnP p) {
  constexpr int NR = ATTN_DELTA_ROWS;
  const long long total = (long long)p.B * p.Sq * p.H * 8;            // one lane per (b, q, head, 8-lane slot)
  const long long stride = (long long)gridDim.x * 256;                // slot r of a thread: idx + r * stride (coalesced per r)
  const long long idx0 = (long long)blockIdx.x * 256 + threadIdx.x;
  const int D = 64 * p.nd;
  bf16x8 a[NR], o[NR];
  float lse[NR];
  long long li[NR];
  bool ok[NR];
  if (p.nd == 1) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const long long idx = idx0 + r * stride;
      ok[r] = idx < total;
      const int sub = (int)(idx & 7);
      const long long row = (ok[r] ? idx : 0) >> 3;
      const int head = (int)(row % p.H);
      const long long bq = row / p.H;
      const int b = (int)(bq / p.Sq), q = (int)(bq % p.Sq);
      li[r] = ((long long)b * p.H + head) * p.Sq + q;
      a[r] = *(const bf16x8*)(p.dO + bq * p.lddo + head * D + sub * 8);
      o[r] = *(const bf16x8*)(p.O + bq * p.ldo + head * D + sub * 8);
      lse[r] = p.lse[li[r]];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)a[r][j] * (float)o[r][j];
      s += dpp_move<0xB1>(s);                                  // xor 1, xor 2, xor 4 over the 8 lanes of a row: DPP moves, no LDS
      s += dpp_move<0x4E>(s);
      s += dpp_move<0x141>(s);
      if (ok[r] && ((idx0 + r * stride) & 7) == 0) {
        p.delta[li[r]] = -s;                                                     // C operand of the dP products
        p.delta[(long long)p.B * p.H * p.Sq + li[r]] = -lse[r] * LOG2E;          // addend of the exp2 argument
      }
    }
    return;
  }
  for (int r = 0; r < NR; ++r) {                                // padded head widths (text towers, SD1.5): the plain loop
    const long long idx = idx0 + r * stride;
    const int sub = (int)(idx & 7);
    float s = 0.f, l = 0.f;
    long long row = idx >> 3, lin = 0;
    if (idx < total) {
      const int head = (int)(row % p.H);
      const long long bq = row / p.H;
      const int b = (int)(bq / p.Sq), q = (int)(bq % p.Sq);
      lin = ((long long)b * p.H + head) * p.Sq + q;
      if (sub == 0) l = p.lse[lin];
      for (int nd = 0; nd < p.nd; ++nd) {
        const bf16x8 av = *(const bf16x8*)(p.dO + bq * p.lddo + head * D + nd * 64 + sub * 8);
        const bf16x8 ov = *(const bf16x8*)(p.O + bq * p.ldo + head * D + nd * 64 + sub * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (float)av[j] * (float)ov[j];
      }
    }
    s += dpp_move<0xB1>(s);
    s += dpp_move<0x4E>(s);
    s += dpp_move<0x141>(s);
    if (idx < total && sub == 0) {
      p.delta[lin] = -s;
      p.delta[(long long)p.B * p.H * p.Sq + lin] = -l * LOG2E;
    }
  }
}

// out[b][key][h*D+d] (+)= sum_split part[split][b][h][key][{dK,dV}][d]   (splits added in order)
__global__ void attn_dkv_reduce_kernel(const AttnP p) {
  const int D = 64 * p.nd, D4 = D / 4;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // (b, h, key, which, d/4)
  const long long total = (long long)p.B * p.H * p.Skv * 2 * D4;
  if (idx >= total) return;
  const int d4 = (int)(idx % D4) * 4;
  long long r = idx / D4;
  const int which = (int)(r & 1); r >>= 1;
  const int key = (int)(r % p.Skv); r /= p.Skv;
  const int head = (int)(r % p.H);
  const int b = (int)(r / p.H);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.nsplit; ++s) {
    const f32x4 v = *(const f32x4*)(p.dkv_part + ((((long long)s * p.B + b) * p.H + head) * p.Skv + key) * 2 * D +
                                    which * D + d4);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += v[j];
  }
  bf16* dst = which ? p.dV + ((long long)b * p.Skv + key) * p.lddv + head * D + d4
                    : p.dK + ((long long)b * p.Skv + key) * p.lddk + head * D + d4;
  bf16x4 o;
  if (p.accum_dkv) o = *(const bf16x4*)dst;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (bf16)(acc[j] + (p.accum_dkv ? (float)o[j] : 0.f));
  *(bf16x4*)dst = o;
}

// ============================================================================= host: what a call launches
// attn_decide_fwd / attn_decide_bwd: pure functions of the problem (AttnP) and the four switches (AttnEnv) that fill an AttnPlan
// -- up to three launches in order, each a kernel enumerator, its grid, its dynamic LDS bytes and its scalar arguments.  A launcher
// is the shape checks, that call and a walk over the plan through attn_launch, the one switch that names the instantiations.
// pea_debug_attn_dispatch exports the plan without a device (tests/test_attn_dispatch_cpu.py, tests/golden/attn_dispatch.json).
enum AttnKernel : int {   // a family's enumerators are arithmetic in its template arguments (include/pea_hip.h has the formulas)
  AK_XFWD = 0, AK_Q = 12, AK_Q_TXT = 24, AK_DKV = 25, AK_FUSED = 31, AK_XBWD1 = 37, AK_XBWD2 = 41, AK_XBWD3 = 45, AK_FEWQ = 49,
  AK_DELTA = 50, AK_REDUCE = 51, AK_COUNT = 52
};
struct AttnLaunch { int kernel; dim3 grid; int lds, a0, a1; };   // a0: upw (cross-attention) or n_dq (fused backward); a1: n_dkv
struct AttnPlan {
  AttnLaunch l[3]; int n = 0, nsplit = 1;                         // nsplit: query-range splits of the backward (attn_nsplit)
  void add(int kernel, dim3 grid, int lds, int a0 = 0, int a1 = 0) { l[n++] = AttnLaunch{kernel, grid, lds, a0, a1}; }
};
// The switches, read once from the environment (A/B runs) and written by the pea_debug_set_* calls (parity tests).  xattn_ver
// (PEA_XATTN_BWD_VER=n), which one-pass cross-attention backward kernel: 0 = v1, xattn_bwd_kernel (round 3), for every key count;
// 2 = v2, xattn_bwd2_kernel, where it applies (33..96 keys), v1 elsewhere; 1, 3 (default) = the newest that applies: v3,
// xattn_bwd3_kernel, for 33..80 keys, v2 for 81..96, v1 elsewhere.  use_tr 0: the general kernels gather their fragments;  xattn 0
// (PEA_XATTN_OFF=1): cross-attention on the general kernels;  fused_bwd 0 (PEA_ATTN_BWD_SPLIT=1): dQ and dK / dV as two launches
struct AttnEnv { int xattn_ver, use_tr, xattn, fused_bwd; };
static AttnEnv g_attn_env = {getenv("PEA_XATTN_BWD_VER") ? atoi(getenv("PEA_XATTN_BWD_VER")) : 3, 1, getenv("PEA_XATTN_OFF") ? 0 : 1,
                             getenv("PEA_ATTN_BWD_SPLIT") ? 0 : 1};
extern "C" void pea_debug_set_xattn_bwd_v2(int v) { g_attn_env.xattn_ver = v; }
extern "C" void pea_debug_set_attn_tr(int v) { g_attn_env.use_tr = v; }
extern "C" void pea_debug_set_attn_xattn(int v) { g_attn_env.xattn = v; }
extern "C" void pea_debug_set_attn_fused_bwd(int v) { g_attn_env.fused_bwd = v; }
static bool xattn_v2_keys(int Skv, const AttnEnv& e) { return e.xattn_ver && Skv > 32 && Skv <= 96; }     // v2 OR v3: 64-query units
// The resident-K/V kernels size their grids to ONE round of the workgroups the chip holds at once: 256 CUs x the workgroups
// per CU that the kernel's LDS allows (160 KiB per CU, never more than two here).
static int wgs_per_cu(int lds) { return 2 * lds <= 160 * 1024 ? 2 : 1; }
static int wg_slots(int per_cu) { return 256 * per_cu; }
// units per workgroup for that one round: `units` of work in all, `nu` of them per (batch, head)
static int units_per_wg(long long units, int nu, int per_cu) {
  const long long upw = (units + wg_slots(per_cu) - 1) / wg_slots(per_cu);
  return (int)(upw < 1 ? 1 : (upw > nu ? nu : upw));
}
// query-range splitting of the cross-attention backward (few keys, many queries): a workgroup owns `u` consecutive
// 128-query units of one (batch, head); pick the u that minimises (rounds of 512 workgroups: two per CU) x u, then the
// split count (fp32 partials per split).  1024 tokens, B*H = 80: u = 2 -> 320 workgroups, 4 splits; 4096 tokens, 40:
// u = 3 -> 440 workgroups, 11 splits.
static int attn_nsplit(int B, int H, int Sq, int Skv, const AttnEnv& e) {
  if (Skv > 128 || Sq < 512) return 1;
  const bool v2 = xattn_v2_keys(Skv, e);
  const int uq = v2 ? 64 : 128;                                          // queries per unit
  // v2: a workgroup's fixed part (K / V staging, the first unit's flight, the hand-over and the partial stores) is worth
  // about two of its 64-query units; without it the rule cut B * H = 160 (per-GPU batch 8) into 2560 one-unit workgroups:
  // 57.8 us against the 41.2 us of the round-3 kernel.  (v1 keeps the rule it was tuned with.)
  const int fixed = v2 ? 2 : 0;
  const int nu = (Sq + uq - 1) / uq;
  const long long bh = (long long)B * H;
  long long best = -1;
  int best_ns = 1;
  for (int u = 1; u <= nu; ++u) {
    const int ns = (nu + u - 1) / u;
    const long long rounds = (bh * ns + wg_slots(2) - 1) / wg_slots(2);
    const long long cost = rounds * (u + fixed) * (uq / 2) + ns;
    if (best < 0 || cost < best) { best = cost; best_ns = ns; }
  }
  return best_ns;
}
int attention_bwd_nsplit(int B, int H, int Sq, int Skv) { return attn_nsplit(B, H, Sq, Skv, g_attn_env); }
size_t attention_bwd_scratch_bytes(int B, int H, int Sq, int Skv, int nd) {
  const int ns = attention_bwd_nsplit(B, H, Sq, Skv);
  return ns > 1 ? (size_t)ns * B * H * Skv * 128 * nd * sizeof(float) : 0;
}
// the kernels with K / V resident in LDS exist for head_dim 64 and at most 128 keys, and read through the transpose path
static bool attn_resident_kv(const AttnP& p, const AttnEnv& e) { return e.xattn && e.use_tr && p.nd == 1 && p.Skv <= 128; }
static int attn_decide_fwd(const AttnP& p, const AttnEnv& e, AttnPlan& plan) {
  const int nu = cdiv(p.Sq, 128);
  // cross-attention: K / V resident.  With a second key set (attn_check_ip has passed: head_dim 64, <= 128 keys) always, at any
  // query count: there is no other kernel for it
  if (p.K2 || (attn_resident_kv(p, e) && !p.causal && !p.bias && p.Sq >= 128)) {
    const int kb = cdiv(p.Skv, 32), kt = (kb + 1) / 2;
    const int lds = 2 * kt * TILE_BYTES + 4 * 32 * 144 + 4 * 4096 + (p.K2 ? 2 * 4096 : 0);
    const int upw = units_per_wg((long long)p.B * p.H * nu, nu, 2);   // two workgroups per CU (66 KB of LDS each, 74 KB with image keys)
    plan.add(AK_XFWD + 4 * (!p.K2 ? 0 : p.nset ? 2 : 1) + (kb - 1), dim3(cdiv(nu, upw), p.H, p.B), lds, upw);
    return PEA_OK;
  }
  const bool txt = p.causal || p.kv_len || p.bias;              // text-encoder masks / score bias: separate instance (head_dim 64 only)
  SHAPECHK(!txt || p.nd == 1, "attention: causal / key-length masks need head_dim 64");
  plan.add(txt ? AK_Q_TXT : AK_Q + 3 * (e.use_tr != 0) + (p.nd - 1), dim3(nu, p.H, p.B), 2 * 2 * p.nd * TILE_BYTES);
  return PEA_OK;
}
static int attn_decide_bwd(const AttnP& p, const AttnEnv& e, AttnPlan& plan) {
  const int ns = plan.nsplit = p.dkv_part ? attn_nsplit(p.B, p.H, p.Sq, p.Skv, e) : 1;
  const int nd = p.nd, tr = e.use_tr != 0;
  bool all = p.dQ && p.dK && p.dV, partials = true;                // partials: some launch writes dK / dV (fp32 partials where ns > 1)
  if (attn_resident_kv(p, e) && all) {                             // the one-pass cross-attention backward
    const int kb = cdiv(p.Skv, 32);
    const dim3 grid(ns, p.H, p.B);
    if (xattn_v2_keys(p.Skv, e)) {                                 // v2 or v3 (2 or 3 key blocks): 64-query units
      const bool v3 = e.xattn_ver != 2 && p.Skv <= 80;
      const int lds = v3 ? 2 * (TILE_BYTES + TILE_BYTES / 2) + 2 * (2 * TILE_BYTES + 512) + 2 * (TILE_BYTES + 2048)
                         : 4 * TILE_BYTES + 2 * (2 * TILE_BYTES + 512) + 2 * 32 * 144;
      plan.add((v3 ? AK_XBWD3 : AK_XBWD2) + 2 * (kb - 2) + (p.q_prescaled != 0), grid, lds, cdiv(cdiv(p.Sq, 64), ns));
    } else {                                                       // v1: 128-query units
      plan.add(AK_XBWD1 + (kb - 1), grid, 4 * TILE_BYTES + (4 * TILE_BYTES + 1024), cdiv(cdiv(p.Sq, 128), ns));
    }
  } else {
    const int lq = 2 * 2 * nd * TILE_BYTES, lk = 2 * (2 * nd * TILE_BYTES + 512);
    const int n_dq = cdiv(p.Sq, 128) * nd, n_dkv = cdiv(p.Skv, 128) * ns * nd;
    const bool fused = all && e.fused_bwd;
    // delta: its own (memory-bound) kernel for the fused launch and for dK/dV-only calls; the two-launch form computes it in the dQ pass
    if (fused || !p.dQ) plan.add(AK_DELTA, dim3((unsigned)cdivl((long long)p.B * p.Sq * p.H * 8, 256 * ATTN_DELTA_ROWS)), 0);
    partials = fused || (p.dK && p.dV);
    if (fused) plan.add(AK_FUSED + 3 * tr + (nd - 1), dim3((unsigned)((n_dq + n_dkv) * p.H * p.B)), lk, n_dq, n_dkv);
    if (!fused && p.dQ) plan.add(AK_Q + 6 + 3 * tr + (nd - 1), dim3(n_dq, p.H, p.B), lq);
    if (!fused && partials) plan.add(AK_DKV + 3 * tr + (nd - 1), dim3(n_dkv, p.H, p.B), lk);
  }
  // the ordered sum of the query-range splits' fp32 dK / dV partials, behind whichever kernel wrote them
  if (ns > 1 && partials) plan.add(AK_REDUCE, dim3((unsigned)cdivl((long long)p.B * p.H * p.Skv * 2 * 16 * nd, 256)), 0);
  return PEA_OK;
}
// a second key set (AttnP::K2, the image prompt's): forward only, served by xattn_fwd_kernel<KB, true> alone
static int attn_check_ip(const AttnP& p) {
  SHAPECHK(p.K2 != nullptr && p.V2 != nullptr, "attention: a second key set needs both K2 and V2");
  SHAPECHK(p.nd == 1, "attention: a second key set needs head_dim 64 (nd=%d)", p.nd);
  SHAPECHK(!p.causal && !p.bias, "attention: a second key set cannot be combined with a causal mask or a score bias");
  SHAPECHK(p.Skv <= 128, "attention: a second key set needs at most 128 text keys (Skv=%d)", p.Skv);
  SHAPECHK(p.Skv2 >= 1 && p.Skv2 <= 32, "attention: the second key set holds 1..32 keys (Skv2=%d)", p.Skv2);
  SHAPECHK(p.ldk2 % 8 == 0 && p.ldv2 % 8 == 0 && p.ldk2 >= 64 * p.H && p.ldv2 >= 64 * p.H,
           "attention: ldk2 / ldv2 must be multiples of 8 and hold every head (ldk2=%d ldv2=%d)", p.ldk2, p.ldv2);
  SHAPECHK(p.nset >= 0 && p.nset <= 4, "attention: 1..4 image key sets (%d)", p.nset);
  for (int j = 0, lo = 0; j < p.nset; lo = p.set_end[j++]) {
    SHAPECHK(p.set_end[j] > lo, "attention: image key set %d is empty", j);
    SHAPECHK(!p.set_mask[j] || p.set_mstride[j] == 0 || p.set_mstride[j] >= p.Sq,
             "attention: the mask of image key set %d has batch stride %lld: 0 (shared) or >= Sq=%d", j, p.set_mstride[j], p.Sq);
  }
  SHAPECHK(p.nset == 0 || p.set_end[p.nset - 1] == p.Skv2, "attention: the image key sets end at row %d of %d", p.set_end[p.nset - 1], p.Skv2);
  return PEA_OK;
}
// several image key sets -> the launch that serves them: all weights 0 is the plain attention (as the one-set caller does at scale
// 0), one set without a mask is the one-set instance (same bits as pea_op_attention_fwd_ip), everything else the MS instances
static void attn_resolve_sets(AttnP& p) {
  if (!p.nset) return;
  bool any = false;
  for (int j = 0; j < p.nset; ++j) any = any || p.set_w[j] != 0.f;
  if (!any) {
    p.K2 = p.V2 = nullptr;
    p.nset = 0;
  } else if (p.nset == 1 && !p.set_mask[0]) {
    p.scale2 = p.set_w[0];
    p.nset = 0;
  } else {
    for (int j = p.nset; j < 4; ++j) { p.set_end[j] = p.Skv2; p.set_w[j] = 0.f; p.set_mask[j] = nullptr; }
  }
}
// at most 32 queries over one softmax of two key sets (attn_fewq_kernel); AttnP::K2 / V2 / Skv2 are the second SET here, not
// a second softmax.  Everything outside the kernel's shape is refused before any launch.
static int attn_plan_fewq(const AttnP& p, AttnPlan& plan) {
  SHAPECHK(p.B > 0 && p.B <= 65535 && p.H > 0 && p.Sq >= 1 && p.Skv >= 1, "attention_fewq: empty problem (B=%d H=%d Sq=%d Skv=%d)", p.B, p.H, p.Sq, p.Skv);
  SHAPECHK(p.Sq <= 32, "attention_fewq: at most 32 queries (Sq=%d); larger counts belong to pea_op_attention_fwd", p.Sq);
  SHAPECHK(p.nd == 1, "attention_fewq: head_dim 64 only (nd=%d)", p.nd);
  SHAPECHK((p.K2 != nullptr) == (p.V2 != nullptr), "attention_fewq: a second key set needs both K2 and V2");
  SHAPECHK(p.Skv2 >= 0 && p.Skv2 <= 32, "attention_fewq: the second key set holds 0..32 keys (Skv2=%d)", p.Skv2);
  SHAPECHK((p.Skv2 > 0) == (p.K2 != nullptr), "attention_fewq: Skv2=%d %s K2 / V2", p.Skv2, p.K2 ? "with" : "without");
  SHAPECHK(p.Q && p.K && p.V && p.O, "attention_fewq: null operand");
  SHAPECHK(p.scale > 0.f && !p.causal && !p.kv_len && !p.bias, "attention_fewq: a positive scale, no mask, no score bias");
  const int C = 64 * p.H;
  SHAPECHK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.ldq >= C && p.ldk >= C && p.ldv >= C,
           "attention_fewq: ldq / ldk / ldv must be multiples of 8 and hold every head (%d %d %d)", p.ldq, p.ldk, p.ldv);
  SHAPECHK(!p.K2 || (p.ldk2 % 8 == 0 && p.ldv2 % 8 == 0 && p.ldk2 >= C && p.ldv2 >= C),
           "attention_fewq: ldk2 / ldv2 must be multiples of 8 and hold every head (ldk2=%d ldv2=%d)", p.ldk2, p.ldv2);
  SHAPECHK(p.ldo % 4 == 0 && p.ldo >= C, "attention_fewq: ldo %% 4, ldo >= 64 H (ldo=%d)", p.ldo);
  const unsigned long long in_bits = (unsigned long long)p.Q | (unsigned long long)p.K | (unsigned long long)p.V |
                                     (unsigned long long)p.K2 | (unsigned long long)p.V2;
  SHAPECHK(in_bits % 16 == 0 && (unsigned long long)p.O % 8 == 0, "attention_fewq: Q / K / V 16-byte, O 8-byte aligned");
  plan.add(AK_FEWQ, dim3(p.H, p.B), 4 * FEWQ_WAVE_BYTES + 4096);   // the one kernel there is: nothing to decide
  return PEA_OK;
}
// all of a call that needs no device: the shape checks, attn_resolve_sets, the decision.  dir: 0 forward, 1 backward, 2 few-query
static int attn_plan(int dir, AttnP& p, const AttnEnv& e, AttnPlan& plan) {
  if (dir == 2) return attn_plan_fewq(p, plan);
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.H > 0 && p.Sq > 0 && p.Skv > 0, "attention: empty problem");
  SHAPECHK(p.nd >= 1 && p.nd <= 3, "attention: padded head_dim must be 64, 128 or 192 (nd=%d)", p.nd);
  SHAPECHK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0, "attention: leading dims must be multiples of 8");
  if (dir == 1) {
    // no backward kernel knows a causal mask or a score bias (the text encoders are frozen): unmasked gradients would be wrong
    SHAPECHK(!p.causal && !p.bias, "attention bwd: no backward with a causal mask or a score bias");
    SHAPECHK(!p.kv_len || p.nd == 1, "attention bwd: key-length masks need head_dim 64 (nd=%d)", p.nd);
    SHAPECHK(p.lse && p.delta && p.dO && p.O, "attention bwd: lse/delta/dO/O required");
    SHAPECHK(p.Sq % 4 == 0, "attention bwd: Sq=%d must be a multiple of 4", p.Sq);
    const int rc = attn_decide_bwd(p, e, plan);
    p.nsplit = plan.nsplit;
    return rc;
  }
  SHAPECHK(p.ldo % 4 == 0, "attention: ldo %% 4");
  if (p.K2 || p.V2) {
    const int rc = attn_check_ip(p);
    if (rc) return rc;
    SHAPECHK(p.k2_brows == 0 || p.k2_brows >= p.Skv2, "attention: %d image key rows per sample hold no %d keys", p.k2_brows, p.Skv2);
    if (!p.k2_brows) p.k2_brows = p.Skv2;
    attn_resolve_sets(p);
  }
  return attn_decide_fwd(p, e, plan);
}
// hipFuncAttributeMaxDynamicSharedMemorySize of kernel K raised once per process, then the launch with THREADS per workgroup:
// every kernel of this file that takes dynamic LDS goes through here, so no list of instantiations has to be kept by hand.
// The limit is raised to LIMIT bytes, the most any launch of K takes, or (LIMIT = 0: every launch of K takes the same) to the
// first launch's.  The attribute call belongs to an instantiation's FIRST launch: if that launch is inside a stream capture,
// the call happens during the capture (it is not a stream operation and is not recorded).
template <auto K, int THREADS = 256, int LIMIT = 0, typename... Args>
static int launch_lds(dim3 grid, int bytes, hipStream_t s, const Args&... args) {
  static bool raised = false;
  if (!raised) {
    HIPCHK(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, LIMIT ? LIMIT : bytes));
    raised = true;
  }
  hipLaunchKernelGGL(K, grid, dim3(THREADS), bytes, s, args...);
  return PEA_OK;
}
// enumerator -> instantiation: the one place that names them
static int attn_launch(const AttnLaunch& l, const AttnP& p, hipStream_t s) {
#define ATTN_CASE(e, K, ...) case e: return launch_lds<K>(l.grid, l.lds, s, p, ##__VA_ARGS__);
  switch (l.kernel) {
    ATTN_CASE(AK_XFWD + 0, (xattn_fwd_kernel<1, false, false>), l.a0) ATTN_CASE(AK_XFWD + 1, (xattn_fwd_kernel<2, false, false>), l.a0)
    ATTN_CASE(AK_XFWD + 2, (xattn_fwd_kernel<3, false, false>), l.a0) ATTN_CASE(AK_XFWD + 3, (xattn_fwd_kernel<4, false, false>), l.a0)
    ATTN_CASE(AK_XFWD + 4, (xattn_fwd_kernel<1, true, false>), l.a0) ATTN_CASE(AK_XFWD + 5, (xattn_fwd_kernel<2, true, false>), l.a0)
    ATTN_CASE(AK_XFWD + 6, (xattn_fwd_kernel<3, true, false>), l.a0) ATTN_CASE(AK_XFWD + 7, (xattn_fwd_kernel<4, true, false>), l.a0)
    ATTN_CASE(AK_XFWD + 8, (xattn_fwd_kernel<1, true, true>), l.a0) ATTN_CASE(AK_XFWD + 9, (xattn_fwd_kernel<2, true, true>), l.a0)
    ATTN_CASE(AK_XFWD + 10, (xattn_fwd_kernel<3, true, true>), l.a0) ATTN_CASE(AK_XFWD + 11, (xattn_fwd_kernel<4, true, true>), l.a0)
    ATTN_CASE(AK_Q + 0, (attn_q_kernel<0, false, 1>)) ATTN_CASE(AK_Q + 1, (attn_q_kernel<0, false, 2>)) ATTN_CASE(AK_Q + 2, (attn_q_kernel<0, false, 3>))
    ATTN_CASE(AK_Q + 3, (attn_q_kernel<0, true, 1>)) ATTN_CASE(AK_Q + 4, (attn_q_kernel<0, true, 2>)) ATTN_CASE(AK_Q + 5, (attn_q_kernel<0, true, 3>))
    ATTN_CASE(AK_Q + 6, (attn_q_kernel<1, false, 1>)) ATTN_CASE(AK_Q + 7, (attn_q_kernel<1, false, 2>)) ATTN_CASE(AK_Q + 8, (attn_q_kernel<1, false, 3>))
    ATTN_CASE(AK_Q + 9, (attn_q_kernel<1, true, 1>)) ATTN_CASE(AK_Q + 10, (attn_q_kernel<1, true, 2>)) ATTN_CASE(AK_Q + 11, (attn_q_kernel<1, true, 3>))
    ATTN_CASE(AK_Q_TXT, (attn_q_kernel<0, true, 1, true>)) ATTN_CASE(AK_FEWQ, attn_fewq_kernel)
    ATTN_CASE(AK_DKV + 0, (attn_dkv_kernel<false, 1>)) ATTN_CASE(AK_DKV + 1, (attn_dkv_kernel<false, 2>)) ATTN_CASE(AK_DKV + 2, (attn_dkv_kernel<false, 3>))
    ATTN_CASE(AK_DKV + 3, (attn_dkv_kernel<true, 1>)) ATTN_CASE(AK_DKV + 4, (attn_dkv_kernel<true, 2>)) ATTN_CASE(AK_DKV + 5, (attn_dkv_kernel<true, 3>))
    ATTN_CASE(AK_FUSED + 0, (attn_bwd_fused_kernel<false, 1>), l.a0, l.a1) ATTN_CASE(AK_FUSED + 1, (attn_bwd_fused_kernel<false, 2>), l.a0, l.a1)
    ATTN_CASE(AK_FUSED + 2, (attn_bwd_fused_kernel<false, 3>), l.a0, l.a1) ATTN_CASE(AK_FUSED + 3, (attn_bwd_fused_kernel<true, 1>), l.a0, l.a1)
    ATTN_CASE(AK_FUSED + 4, (attn_bwd_fused_kernel<true, 2>), l.a0, l.a1) ATTN_CASE(AK_FUSED + 5, (attn_bwd_fused_kernel<true, 3>), l.a0, l.a1)
    ATTN_CASE(AK_XBWD1 + 0, xattn_bwd_kernel<1>, l.a0) ATTN_CASE(AK_XBWD1 + 1, xattn_bwd_kernel<2>, l.a0)
    ATTN_CASE(AK_XBWD1 + 2, xattn_bwd_kernel<3>, l.a0) ATTN_CASE(AK_XBWD1 + 3, xattn_bwd_kernel<4>, l.a0)
    ATTN_CASE(AK_XBWD2 + 0, (xattn_bwd2_kernel<2, false>), l.a0) ATTN_CASE(AK_XBWD2 + 1, (xattn_bwd2_kernel<2, true>), l.a0)
    ATTN_CASE(AK_XBWD2 + 2, (xattn_bwd2_kernel<3, false>), l.a0) ATTN_CASE(AK_XBWD2 + 3, (xattn_bwd2_kernel<3, true>), l.a0)
    ATTN_CASE(AK_XBWD3 + 0, (xattn_bwd3_kernel<2, false>), l.a0) ATTN_CASE(AK_XBWD3 + 1, (xattn_bwd3_kernel<2, true>), l.a0)
    ATTN_CASE(AK_XBWD3 + 2, (xattn_bwd3_kernel<3, false>), l.a0) ATTN_CASE(AK_XBWD3 + 3, (xattn_bwd3_kernel<3, true>), l.a0)
    case AK_DELTA: hipLaunchKernelGGL(attn_delta_kernel, l.grid, dim3(256), 0, s, p); return PEA_OK;       // (no dynamic LDS)
    case AK_REDUCE: hipLaunchKernelGGL(attn_dkv_reduce_kernel, l.grid, dim3(256), 0, s, p); return PEA_OK;
  }
#undef ATTN_CASE
  pea_set_error("attention: no kernel for enumerator %d", l.kernel);
  return PEA_E_SHAPE;
}
static int attn_go(int dir, const AttnP& p0, hipStream_t s) {
  AttnP p = p0;
  AttnPlan plan;
  int rc = attn_plan(dir, p, g_attn_env, plan);
  if (rc) return rc;
  const int keys = p.Skv + (dir != 1 && p.K2 ? p.Skv2 : 0);        // both key sets: one more score / value product each
  if (g_prof_on) { g_prof_tag[0] = p.B * p.H; g_prof_tag[1] = p.Sq; g_prof_tag[2] = dir == 2 ? keys : p.Skv; g_prof_tag[3] = p.nd; }
  // algorithmic: 2 products forward, 5 backward (S, dP, dV, dK, dQ) = 10*B*H*Sq*Skv*D flops (the two-kernel form recomputes S and dP)
  const double w = dir == 1 ? 4.0 : 2.0;
  PROF_BEGIN(dir == 1 ? 3 : 2, (dir == 1 ? 10.0 : 4.0) * p.B * p.H * (double)p.Sq * keys * 64 * p.nd,
             2.0 * p.B * p.H * 64 * p.nd * (w * p.Sq + w * keys), s);
  for (int i = 0; i < plan.n && !rc; ++i) rc = attn_launch(plan.l[i], p, s);
  PROF_END(s);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
int launch_attention_fwd(const AttnP& p, hipStream_t s) { return attn_go(0, p, s); }
int launch_attention_bwd(const AttnP& p, hipStream_t s) { return attn_go(1, p, s); }
int launch_attention_fwd_fewq(const AttnP& p, hipStream_t s) { return attn_go(2, p, s); }
// What the pea_debug_attn_*_dispatch exports plan over: struct F (AttnP or a feature's) with non-null, aligned stand-ins for the
// common operands (nothing is launched, nothing is read), scale 1 / 8 and every leading dimension 64 H nd; ldk > 0: that of K.
static float g_standin_page[64] __attribute__((aligned(16)));
template <class F>
static F attn_standin(int B, int H, int Sq, int Skv, int nd, int ldk = 0) {
  AttnP a = AttnP();
  a.Q = a.K = a.V = a.O = (bf16*)g_standin_page; a.scale = 0.125f;
  a.B = B; a.H = H; a.Sq = Sq; a.Skv = Skv; a.nd = nd;
  a.ldq = a.ldk = a.ldv = a.ldo = 64 * H * (nd > 0 ? nd : 1);
  if (ldk > 0) a.ldk = ldk;
  return attn_feature_p<F>(a);
}
// include/pea_hip.h
extern "C" int pea_debug_attn_dispatch(const int* q, int* out) {
  const int dir = q[0], feat = q[6];
  if (dir < 0 || dir > 2) return q[1] >= 0 && q[1] < AK_COUNT ? q[1] : -1;
  const AttnEnv e = {q[10] < 0 ? g_attn_env.xattn_ver : q[10], q[11] < 0 ? g_attn_env.use_tr : q[11],
                     q[12] < 0 ? g_attn_env.xattn : q[12], q[13] < 0 ? g_attn_env.fused_bwd : q[13]};
  float* const page = g_standin_page;
  bf16* const any = (bf16*)page;
  AttnP p = attn_standin<AttnP>(q[1], q[2], q[3], q[4], q[5]);
  p.dO = any; p.lse = p.delta = page;
  p.lddo = p.lddq = p.lddk = p.lddv = p.ldk2 = p.ldv2 = p.ldq;
  p.causal = feat & 1; p.kv_len = feat & 2 ? (const int*)page : nullptr; p.bias = feat & 4 ? page : nullptr; p.q_prescaled = feat >> 3 & 1;
  if (feat & 16) { p.K2 = p.V2 = any; p.Skv2 = q[7]; p.scale2 = 1.f; p.nset = dir == 2 ? 0 : q[8]; }
  for (int j = 0; j < p.nset && j < 4; ++j) {                       // the sets share the Skv2 keys evenly; bit j of q[9]: set j has a mask
    p.set_end[j] = (int)((long long)(j + 1) * p.Skv2 / p.nset);
    p.set_w[j] = feat & 32 ? 0.f : 1.f;
    p.set_mask[j] = q[9] >> j & 1 ? page : nullptr;
  }
  p.dQ = feat & 64 ? any : nullptr; p.dK = feat & 128 ? any : nullptr; p.dV = feat & 256 ? any : nullptr;
  p.dkv_part = feat & 512 ? page : nullptr; p.accum_dq = p.accum_dkv = feat >> 10 & 1;
  AttnPlan plan;
  const int rc = attn_plan(dir, p, e, plan);
  if (rc) return rc;
  out[0] = plan.n; out[1] = plan.nsplit;
  for (int i = 0; i < plan.n; ++i) {
    const AttnLaunch& l = plan.l[i];
    int* const o = out + 2 + 7 * i;
    o[0] = l.kernel; o[1] = (int)l.grid.x; o[2] = (int)l.grid.y; o[3] = (int)l.grid.z; o[4] = l.lds; o[5] = l.a0; o[6] = l.a1;
  }
  return PEA_OK;
}

// ============================================================================= host: what the feature launchers below share
// The operand checks of a feature launch (regions, maps, edit, shared), in this order: every operand there, a finite positive
// scale, Q / K / V rows that are multiples of 8 elements (16-byte loads, LDS-DMA) and hold all H heads of 64, the same for O
// at the width it is stored with (o_bytes 16: ldo % 8; 8: ldo % 4; 0: no O), base addresses aligned to match.  f32: the fp32
// operands (4-byte aligned), the first of which must be there where need_f32 says so.  A launch without V passes K in its place.
struct AttnOperands { const bf16 *Q, *K, *V; int ldq, ldk, ldv; const bf16* O; int ldo, o_bytes; const void *f32, *f32_opt; bool need_f32; };
static int attn_check_operands(const char* who, const AttnOperands& a, int H, float scale) {
  SHAPECHK(a.Q && a.K && a.V && (a.O || !a.o_bytes) && (a.f32 || !a.need_f32), "%s: null operand", who);
  SHAPECHK(scale > 0.f && scale <= 3.0e38f, "%s: a finite positive scale (%g)", who, (double)scale);
  const int C = 64 * H;
  SHAPECHK(a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 && a.ldq >= C && a.ldk >= C && a.ldv >= C,
           "%s: leading dimensions ldq / ldk / ldv must be multiples of 8 and hold every head (%d %d %d)", who, a.ldq, a.ldk, a.ldv);
  SHAPECHK(!a.o_bytes || (a.ldo % (a.o_bytes / 2) == 0 && a.ldo >= C),
           "%s: leading dimension ldo must be a multiple of %d and hold every head (ldo=%d)", who, a.o_bytes / 2, a.ldo);
  const unsigned long long in_bits = (unsigned long long)a.Q | (unsigned long long)a.K | (unsigned long long)a.V;
  SHAPECHK(in_bits % 16 == 0 && (!a.o_bytes || (unsigned long long)a.O % a.o_bytes == 0) &&
               ((unsigned long long)a.f32 | (unsigned long long)a.f32_opt) % 4 == 0,
           "%s: Q / K / V 16-byte, O %d-byte, fp32 operands 4-byte aligned", who, a.o_bytes);
  return PEA_OK;
}
// The tail of a feature launcher behind its plan: the profiling tag (B * H, queries, keys, nd = 1), PROF_BEGIN with the launch's
// flops and bytes, the launch itself (`launch`: the switch over the feature's instantiations), PROF_END, the launch error.
template <class Launch>
static int attn_feature_launch(int BH, int Sq, int keys, double flops, double bytes, hipStream_t s, Launch launch) {
  if (g_prof_on) { g_prof_tag[0] = BH; g_prof_tag[1] = Sq; g_prof_tag[2] = keys; g_prof_tag[3] = 1; }
  PROF_BEGIN(2, flops, bytes, s);
  const int rc = launch();
  PROF_END(s);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return PEA_OK;
}
// what the feature dispatch exports write: out[0..5] = first, the grid, the LDS bytes, last
static void attn_dispatch_out(int* out, int first, dim3 grid, int lds, int last) {
  out[0] = first; out[1] = (int)grid.x; out[2] = (int)grid.y; out[3] = (int)grid.z; out[4] = lds; out[5] = last;
}

// ============================================================================= host: regional text prompts
// A launcher of its own beside the decision table above (which, with AK_COUNT, attn_plan and pea_debug_attn_dispatch, does not
// know it): the shape checks, the LDS and grid rule, the launch.  Units per workgroup as attn_decide_fwd sizes them
// (units_per_wg): two workgroups per CU up to 80 KiB (two regions of 77 keys: 81 920 bytes exactly), one above.
constexpr int regions_lds(int R, int kb) { return R * kb * 2 * 4096 + 4 * 4096 + 4 * 4096; }   // K and V blocks, O images, Q images
struct AttnRegionsPlan { int kb, lds, upw; dim3 grid; };
static int attn_plan_regions(AttnRegionsP& p, AttnRegionsPlan& plan) {
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.B <= 65535 && p.H > 0 && p.H <= 65535 && p.Sq >= 1, "attention_regions: empty problem (B=%d H=%d Sq=%d)", p.B, p.H, p.Sq);
  SHAPECHK(p.nd == 1, "attention_regions: head_dim 64 only (nd=%d)", p.nd);
  SHAPECHK(p.R >= 1 && p.R <= 4, "attention_regions: 1..4 regions (R=%d)", p.R);
  SHAPECHK(p.Lr >= 1 && p.Lr <= 96, "attention_regions: 1..96 keys per region (Lr=%d)", p.Lr);
  SHAPECHK(p.Bw == 1 || p.Bw == p.B, "attention_regions: Bw=%d (1, or the batch %d)", p.Bw, p.B);
  if (int rc = attn_check_operands("attention_regions", {p.Q, p.K, p.V, p.ldq, p.ldk, p.ldv, p.O, p.ldo, 8, p.w, nullptr, true}, p.H, p.scale)) return rc;
  SHAPECHK((long long)p.R * p.Sq * (p.Bw == 1 ? 1 : p.B) < (1ll << 40), "attention_regions: weight table too large");
  plan.kb = cdiv(p.Lr, 32);
  plan.lds = regions_lds(p.R, plan.kb);
  const int nu = cdiv(p.Sq, 128);
  plan.upw = units_per_wg((long long)p.B * p.H * nu, nu, wgs_per_cu(plan.lds));
  plan.grid = dim3(cdiv(nu, plan.upw), p.H, p.B);
  return PEA_OK;
}
int launch_attention_fwd_regions(const AttnRegionsP& p0, hipStream_t s) {
  AttnRegionsP p = p0;
  AttnRegionsPlan plan;
  const int rc = attn_plan_regions(p, plan);
  if (rc) return rc;
  const double keys = (double)p.R * p.Lr;
  return attn_feature_launch(p.B * p.H, p.Sq, p.R * p.Lr, 4.0 * p.B * p.H * (double)p.Sq * keys * 64,
                             2.0 * p.B * p.H * 64 * (2.0 * p.Sq + 2.0 * keys), s, [&] {
    // an instantiation's LDS grows with R: its limit is raised to what four regions take
    switch (plan.kb) {
      case 1: return launch_lds<xattn_regions_fwd_kernel<1>, 256, regions_lds(4, 1)>(plan.grid, plan.lds, s, p, plan.upw);
      case 2: return launch_lds<xattn_regions_fwd_kernel<2>, 256, regions_lds(4, 2)>(plan.grid, plan.lds, s, p, plan.upw);
      default: return launch_lds<xattn_regions_fwd_kernel<3>, 256, regions_lds(4, 3)>(plan.grid, plan.lds, s, p, plan.upw);
    }
  });
}
// include/pea_hip.h
extern "C" int pea_debug_attn_regions_dispatch(const int* q, int* out) {
  AttnRegionsP p = attn_standin<AttnRegionsP>(q[0], q[1], q[2], 0, 1, q[6]);
  p.w = g_standin_page; p.R = q[3]; p.Lr = q[4]; p.nd = q[5]; p.Bw = q[7] > 0 ? q[7] : 1;
  AttnRegionsPlan plan;
  const int rc = attn_plan_regions(p, plan);
  if (rc) return rc;
  attn_dispatch_out(out, plan.kb, plan.grid, plan.lds, plan.upw);
  return PEA_OK;
}

// ============================================================================= host: cross-attention heat maps
// A launcher of its own, like the regions' above; the decision table does not know it.  The grid and LDS rule, in this one
// function: a workgroup is ONE 32-query unit of one sample (grid = ceil(Sq / 32) x B, every workgroup has work), its eight waves
// share out the heads, and its LDS is 8 slots of (KB + 1) half tiles of 4 096 bytes, KB = ceil(Skv / 32).  The sum over heads has
// to stay inside a workgroup (no atomics), and 32 queries are one MFMA column block, so a launch has B x Sq / 32 workgroups
// whatever H is: 256 at SDXL's 4096-query level with B = 2, 64 at its 1024-query level (20 heads: two or three per wave).
struct AttnMapsPlan { int kb, lds, upw; dim3 grid; };
static int attn_plan_maps(AttnMapsP& p, AttnMapsPlan& plan) {
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.B <= 65535 && p.H > 0 && p.H <= 65535 && p.Sq >= 1, "attention_maps: empty problem (B=%d H=%d Sq=%d)", p.B, p.H, p.Sq);
  SHAPECHK(p.nd == 1, "attention_maps: head_dim 64 only (nd=%d)", p.nd);
  SHAPECHK(p.Skv >= 1 && p.Skv <= 128, "attention_maps: 1..128 keys (Skv=%d)", p.Skv);
  if (int rc = attn_check_operands("attention_maps", {p.Q, p.K, p.K, p.ldq, p.ldk, p.ldk, nullptr, 0, 0, p.maps, p.kv_len, true}, p.H, p.scale)) return rc;
  SHAPECHK((long long)p.ldq * 64 < (1ll << 30) && (long long)p.ldk * 64 < (1ll << 30), "attention_maps: leading dimension too large");
  plan.kb = cdiv(p.Skv, 32);
  plan.lds = MAPS_WAVES * (plan.kb + 1) * 4096;
  plan.upw = 1;
  plan.grid = dim3(cdiv(p.Sq, 32), p.B, 1);
  return PEA_OK;
}
int launch_attention_maps(const AttnMapsP& p0, hipStream_t s) {
  AttnMapsP p = p0;
  AttnMapsPlan plan;
  const int rc = attn_plan_maps(p, plan);
  if (rc) return rc;
  return attn_feature_launch(p.B * p.H, p.Sq, p.Skv, 2.0 * p.B * p.H * (double)p.Sq * p.Skv * 64,
                             2.0 * p.B * p.H * 64 * ((double)p.Sq + p.Skv) + (p.accumulate ? 8.0 : 4.0) * p.B * (double)p.Sq * p.Skv, s, [&] {
    switch (plan.kb) {                                             // (this kernel's workgroup is eight waves)
      case 1: return launch_lds<xattn_maps_kernel<1>, 64 * MAPS_WAVES>(plan.grid, plan.lds, s, p);
      case 2: return launch_lds<xattn_maps_kernel<2>, 64 * MAPS_WAVES>(plan.grid, plan.lds, s, p);
      case 3: return launch_lds<xattn_maps_kernel<3>, 64 * MAPS_WAVES>(plan.grid, plan.lds, s, p);
      default: return launch_lds<xattn_maps_kernel<4>, 64 * MAPS_WAVES>(plan.grid, plan.lds, s, p);
    }
  });
}
// include/pea_hip.h
extern "C" int pea_debug_attn_maps_dispatch(const int* q, int* out) {
  AttnMapsP p = attn_standin<AttnMapsP>(q[0], q[1], q[2], q[3], 1, q[6]);
  p.maps = g_standin_page; p.nd = q[4];
  if (q[5] > 0) p.ldq = q[5];
  p.kv_len = q[7] & 1 ? (const int*)g_standin_page : nullptr; p.accumulate = q[7] >> 1 & 1; p.q_prescaled = q[7] >> 2 & 1;
  AttnMapsPlan plan;
  const int rc = attn_plan_maps(p, plan);
  if (rc) return rc;
  attn_dispatch_out(out, plan.kb, plan.grid, plan.lds, plan.upw);
  return PEA_OK;
}

// ============================================================================= host: self-attention column sums
// A launcher of its own, like the maps' above; the decision table does not know it.  The grid rule, in this one function: a
// workgroup is 128 keys of one (sample, head group), grid = ceil(Skv / 128) x G x B.  The heads are cut into the fewest groups that
// put at least one round of workgroups (wg_slots(2): the kernel takes 66 KiB of LDS, two workgroups a CU) on the
// chip, never more than H: heads per group = ceil(H / that), G = ceil(H / heads per group), so no group is empty.  SDXL's mid
// block (B = 2, H = 20, 1024 tokens: 16 key blocks x samples) gets G = 20, one head per group, 320 workgroups; at B = 64 of the
// same layer the key blocks alone fill the chip and G = 1.  A sum over heads inside a workgroup costs nothing but parallelism;
// one across workgroups is the consumer's G fp32 adds per key (no atomics, no reduce launch).
struct AttnColsumPlan { int G, hpg, lds; dim3 grid; };
static void colsum_groups(int B, int H, int Skv, int& G, int& hpg) {
  const long long base = (long long)B * cdiv(Skv, 128);
  long long g = (wg_slots(2) + base - 1) / base;
  g = g < 1 ? 1 : (g > H ? H : g);
  hpg = cdiv(H, (int)g);
  G = cdiv(H, hpg);
}
static int attn_plan_colsum(AttnColsumP& p, AttnColsumPlan& plan) {
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.B <= 65535 && p.H > 0 && p.H <= 65535 && p.Sq >= 1 && p.Skv >= 1,
           "attention_colsum: empty problem (B=%d H=%d Sq=%d Skv=%d; B, H <= 65535)", p.B, p.H, p.Sq, p.Skv);
  SHAPECHK(p.nd == 1, "attention_colsum: head_dim 64 only (nd=%d)", p.nd);
  if (int rc = attn_check_operands("attention_colsum", {p.Q, p.K, p.K, p.ldq, p.ldk, p.ldk, nullptr, 0, 0, p.part, p.lse, true}, p.H, p.scale)) return rc;
  SHAPECHK(p.lse != nullptr, "attention_colsum: null lse (fp32 [B][H][Sq], as pea_op_attention_fwd writes it)");
  SHAPECHK((long long)p.Sq * p.ldq < (1ll << 30) && (long long)p.Skv * p.ldk < (1ll << 30),
           "attention_colsum: a sample's Q or K takes 2 GiB or more (Sq=%d ldq=%d Skv=%d ldk=%d)", p.Sq, p.ldq, p.Skv, p.ldk);
  colsum_groups(p.B, p.H, p.Skv, plan.G, plan.hpg);
  p.G = plan.G; p.hpg = plan.hpg;
  plan.lds = 2 * COLSUM_STG;
  plan.grid = dim3(cdiv(p.Skv, 128), plan.G, p.B);
  return PEA_OK;
}
int attention_colsum_groups(int B, int H, int Sq, int Skv) {
  SHAPECHK(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Sq >= 1 && Skv >= 1, "attention_colsum_groups: empty problem (B=%d H=%d Sq=%d Skv=%d)", B, H, Sq, Skv);
  int G, hpg;
  colsum_groups(B, H, Skv, G, hpg);
  return G;
}
int launch_attention_colsum(const AttnColsumP& p0, hipStream_t s) {
  AttnColsumP p = p0;
  AttnColsumPlan plan;
  const int rc = attn_plan_colsum(p, plan);
  if (rc) return rc;
  return attn_feature_launch(p.B * p.H, p.Sq, p.Skv, 2.0 * p.B * p.H * (double)p.Sq * p.Skv * 64,
                             2.0 * p.B * p.H * 64 * ((double)p.Sq * cdiv(p.Skv, 128) + p.Skv) +
                                 4.0 * p.B * ((double)p.H * p.Sq + (double)plan.G * p.Skv), s, [&] {
    return p.q_prescaled ? launch_lds<attn_colsum_kernel<true>>(plan.grid, plan.lds, s, p)
                         : launch_lds<attn_colsum_kernel<false>>(plan.grid, plan.lds, s, p);
  });
}
// include/pea_hip.h
extern "C" int pea_debug_attn_colsum_dispatch(const int* q, int* out) {
  AttnColsumP p = attn_standin<AttnColsumP>(q[0], q[1], q[2], q[3], 1, q[6]);
  p.part = g_standin_page; p.lse = q[7] & 2 ? nullptr : g_standin_page; p.nd = q[4];
  if (q[5] > 0) p.ldq = q[5];
  p.q_prescaled = q[7] & 1;
  AttnColsumPlan plan;
  const int rc = attn_plan_colsum(p, plan);
  if (rc) return rc;
  attn_dispatch_out(out, plan.G, plan.grid, plan.lds, plan.hpg);
  return PEA_OK;
}

// ============================================================================= host: prompt-to-prompt editing
// A launcher of its own beside the decision table (which, with AK_COUNT, attn_plan and pea_debug_attn_dispatch, does not know
// it): the shape checks, src validated on the host before any launch, the LDS and the grid rule (units per workgroup for one
// round of the workgroups per CU the LDS allows -- two at one key block, one above --, as the regions launcher sizes them, but with
// a count of its own for the edited samples).
// plain_first: xattn_edit_fwd_kernel gives its unedited samples the bits of xattn_fwd_kernel.  Where the plain launch of the
// same problem is another kernel (fewer than 128 queries: attn_q_kernel; PEA_XATTN_OFF), that launch runs first over the whole
// batch and the edit kernel overwrites the edited samples only, so an unedited sample keeps the bits of pea_op_attention_fwd
// at every shape.  With no edited sample at all the plain launch is all there is.
// What a workgroup of xattn_edit_fwd_kernel<3> takes, in tenths of a microsecond: a fixed part (staging) and a part per 128-query
// unit, for a workgroup of an edited and of an unedited sample.  MEASURED at 77 keys (KB = 3) on one MI355X at 2089 MHz
// (profiles/EXPERIMENTS.md section 9, f11) and used at every KB for want of figures there: only their RATIOS enter the rule below,
// which balances the two kinds of workgroup.  A change to the kernel's unit loop or staging invalidates them: re-run the sweep of
// f11 (scripts/p2p_bench.py times the result) and tests/test_p2p_cpu.py, which pins the pairs they give at the SDXL shapes.
constexpr long long EDIT_WG_FIXED = 64, EDIT_WG_UNIT = 37, PLAIN_WG_FIXED = 30, PLAIN_WG_UNIT = 20;
struct AttnEditPlan { int kb, lds, upw, upw_edit, plain_first, n_edited; dim3 grid; AttnP plain; AttnPlan pplan; };
static int attn_plan_edit(AttnEditP& p, AttnEditPlan& plan) {
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.H > 0 && p.H <= 65535 && p.Sq >= 1 && p.Skv >= 1, "attention_edit: empty problem (B=%d H=%d Sq=%d Skv=%d)", p.B, p.H, p.Sq, p.Skv);
  SHAPECHK(p.B <= 32, "attention_edit: at most 32 samples, src travels in the kernel arguments (B=%d)", p.B);
  SHAPECHK(p.nd == 1, "attention_edit: head_dim 64 only (nd=%d)", p.nd);
  SHAPECHK(p.Skv <= 96, "attention_edit: 1..96 keys (Skv=%d)", p.Skv);
  if (int rc = attn_check_operands("attention_edit", {p.Q, p.K, p.V, p.ldq, p.ldk, p.ldv, p.O, p.ldo, 8, nullptr, nullptr, false}, p.H, p.scale)) return rc;
  plan.n_edited = 0;
  for (int b = 0; b < p.B; ++b)
    if (p.src[b] == b) p.src[b] = -1;                              // its own source: not edited
  for (int b = 0; b < p.B; ++b) {
    const int s = p.src[b];
    if (s < 0) continue;
    SHAPECHK(s < p.B, "attention_edit: src[%d]=%d is out of range (a sample of the batch of %d, or negative for an unedited sample)", b, s, p.B);
    SHAPECHK(p.src[s] < 0, "attention_edit: src[%d]=%d names a source that is itself edited (src[%d]=%d)", b, s, s, p.src[s]);
    ++plan.n_edited;
  }
  if (plan.n_edited) {
    SHAPECHK(p.Mt && p.c && p.d, "attention_edit: null table (Mt, c and d are needed while any sample is edited)");
    SHAPECHK(p.ldm % 8 == 0 && p.ldm >= p.Skv, "attention_edit: leading dimension ldm must be a multiple of 8 and hold %d keys (ldm=%d)", p.Skv, p.ldm);
    SHAPECHK((unsigned long long)p.Mt % 16 == 0 && ((unsigned long long)p.c | (unsigned long long)p.d) % 4 == 0,
             "attention_edit: Mt 16-byte, c / d 4-byte aligned");
  }
  plan.kb = cdiv(p.Skv, 32);
  plan.lds = 3 * plan.kb * 4096 + plan.kb * 32 * (plan.kb * 64 + 16) + plan.kb * 256 + 4 * 4096 + 8 * 4096;
  plan.plain = attn_plain_p(p);
  plan.pplan = AttnPlan();
  if (int rc = attn_plan(0, plan.plain, g_attn_env, plan.pplan)) return rc;
  const int k0 = plan.pplan.l[0].kernel;
  plan.plain_first = !(plan.pplan.n == 1 && k0 >= AK_XFWD && k0 < AK_XFWD + 4);
  // Units per workgroup, one count for the unedited samples' workgroups and one for the edited ones': ONE round of the
  // workgroups per CU the LDS allows (the aim of attn_plan_maps and the regions launcher; NOT their formula, which has one count
  // for all workgroups and left the edited ones as the critical path), and among the pairs that fit,
  // the one whose longest workgroup is shortest by the times measured at 77 keys (profiles/EXPERIMENTS.md section 9, f11): an edited
  // workgroup of u units 6.4 + 3.7 u us, a plain one 3.0 + 2.0 u.  Where not even one workgroup per (sample, head) fits in a
  // round, each takes all units of its head.  The grid is 1-D and holds exactly the workgroups that have work.
  const int nu = cdiv(p.Sq, 128), slots = wg_slots(wgs_per_cu(plan.lds));
  const long long n_ed = plan.n_edited, n_un = plan.plain_first ? 0 : p.B - n_ed;    // (plain first: the grid holds the edited samples only)
  plan.upw = plan.upw_edit = nu;
  long long best = -1;
  for (int ue = 1; ue <= nu; ++ue) {
    const long long left = slots - n_ed * p.H * cdiv(nu, ue);
    if (left < n_un * p.H) continue;
    int uu = nu;
    if (n_un) {
      const long long splits = left / (n_un * p.H);
      uu = cdiv(nu, (int)(splits > nu ? nu : splits));
    }
    const long long te = EDIT_WG_FIXED + EDIT_WG_UNIT * ue, tu = n_un ? PLAIN_WG_FIXED + PLAIN_WG_UNIT * uu : 0, cost = te > tu ? te : tu;
    if (best < 0 || cost < best) { best = cost; plan.upw = uu; plan.upw_edit = ue; }
  }
  plan.grid = dim3((unsigned)(p.H * (n_ed * cdiv(nu, plan.upw_edit) + n_un * cdiv(nu, plan.upw))));
  return PEA_OK;
}
int launch_attention_fwd_edit(const AttnEditP& p0, hipStream_t s) {
  AttnEditP p = p0;
  AttnEditPlan plan;
  int rc = attn_plan_edit(p, plan);
  if (rc) return rc;
  if (!plan.n_edited) return launch_attention_fwd(plan.plain, s);
  if (plan.plain_first) {
    rc = launch_attention_fwd(plan.plain, s);
    if (rc) return rc;
  }
  const double pairs = (double)(p.B + plan.n_edited) * p.H * (double)p.Sq * p.Skv;     // a second score product per edited sample
  return attn_feature_launch(p.B * p.H, p.Sq, p.Skv, 4.0 * pairs * 64 + 2.0 * plan.n_edited * p.H * (double)p.Sq * p.Skv * p.Skv,
                             2.0 * p.H * 64 * ((2.0 * p.B + plan.n_edited) * p.Sq + (2.0 * p.B + plan.n_edited) * p.Skv), s, [&] {
    switch (plan.kb) {
      case 1: return launch_lds<xattn_edit_fwd_kernel<1>>(plan.grid, plan.lds, s, p, plan.upw, plan.upw_edit);
      case 2: return launch_lds<xattn_edit_fwd_kernel<2>>(plan.grid, plan.lds, s, p, plan.upw, plan.upw_edit);
      default: return launch_lds<xattn_edit_fwd_kernel<3>>(plan.grid, plan.lds, s, p, plan.upw, plan.upw_edit);
    }
  });
}
// include/pea_hip.h
extern "C" int pea_debug_attn_edit_dispatch(const int* q, int* out) {
  AttnEditP p = attn_standin<AttnEditP>(q[0], q[1], q[2], q[3], 1, q[5]);
  p.nd = q[4];
  p.ldm = q[6] > 0 ? q[6] : (p.Skv + 7) / 8 * 8;
  if (!(q[7] & 1)) { p.Mt = (const bf16*)g_standin_page; p.c = p.d = g_standin_page; }
  for (int b = 0; b < 32; ++b) p.src[b] = b < p.B ? q[8 + b] : -1;
  AttnEditPlan plan;
  const int rc = attn_plan_edit(p, plan);
  if (rc) return rc;
  attn_dispatch_out(out, plan.kb, plan.grid, plan.lds, plan.upw);
  out[6] = plan.plain_first; out[7] = plan.upw_edit;
  return PEA_OK;
}

// ============================================================================= StyleAligned: shared self-attention
// (Hertz et al. 2023.)  Target sample b with reference r: its queries and keys are moved onto r's per-channel statistics (AdaIN,
// X' = a o X + s) and it attends to r's keys and values as well as its own, under one softmax.  Nothing of that is materialised:
//   q' . (a_k o k + s_k) = (q' o a_k) . k + q' . s_k
// so the own segment is a second resident Q fragment set (q' o a_k) against the untouched K tiles plus ONE constant per query,
// which enters where -m_run enters, in the C operand of the S^T MFMAs; the reference segment is the fragment set
// share_scale q' against K[r] with the constant share_shift log2(e).  K and V of both samples are staged by the same DMA from
// where the projection wrote them: the reference's tiles differ in the base address of the buffer resource only.
//
// ---- the coefficients: column statistics over the tokens, split over token slabs, merged in slab order (no atomics)
#define ADAIN_CG 16                // 8-channel column groups of a workgroup: 256 contiguous bytes of every row
#define ADAIN_RL 16                // row lanes: thread (rl, cg) takes rows rl, rl + 16, ... of its slab
struct AdainP {
  const bf16 *Q, *K; int ldq, ldk;
  int B, C, S, rps, nslab;
  float epsq, epsk; int adain_q, adain_k;
  unsigned used;                   // bit b: sample b is a target or a reference (the others are not read)
  float* part;                     // [B][2][nslab][2][C]: sums of (x - x[row 0]) and of its square, X = Q then K
  float* coef;
  int ref[32];
};
__global__ __launch_bounds__(256) void attn_adain_part_kernel(const AdainP p) {
  __shared__ float red[2][ADAIN_RL][ADAIN_CG * 8];
  const int b = blockIdx.z >> 1, x = blockIdx.z & 1, slab = blockIdx.y;
  if (!(p.used >> b & 1)) return;                                   // (workgroup-uniform)
  const int tid = threadIdx.x, cg = tid & (ADAIN_CG - 1), rl = tid / ADAIN_CG;
  const int col = (blockIdx.x * ADAIN_CG + cg) * 8, ld = x ? p.ldk : p.ldq;
  const bf16* X = (x ? p.K : p.Q) + (long long)b * p.S * ld;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (col < p.C) {
    // the shift: the channel's value in row 0 of the sample, the same for every slab, so the slabs' sums add up
    const bf16x8 sh = *(const bf16x8*)(X + col);
    const int r1 = min(p.S, (slab + 1) * p.rps);
    for (int r = slab * p.rps + rl; r < r1; r += ADAIN_RL) {
      const bf16x8 v = *(const bf16x8*)(X + (long long)r * ld + col);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = (float)v[j] - (float)sh[j];
        s1[j] += d;
        s2[j] = fmaf(d, d, s2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[0][rl][cg * 8 + j] = s1[j]; red[1][rl][cg * 8 + j] = s2[j]; }
  __syncthreads();
  const int k = tid >> 7, cc = tid & 127, oc = blockIdx.x * (ADAIN_CG * 8) + cc;
  if (oc < p.C) {
    float t = 0.f;
    for (int i = 0; i < ADAIN_RL; ++i) t += red[k][i][cc];
    p.part[((((long long)b * 2 + x) * p.nslab + slab) * 2 + k) * p.C + oc] = t;
  }
}
__global__ __launch_bounds__(256) void attn_adain_coef_kernel(const AdainP p) {
  const int i = blockIdx.x * 256 + threadIdx.x;                     // one thread per (sample, X, channel)
  if (i >= p.B * 2 * p.C) return;
  const int c = i % p.C, x = (i / p.C) & 1, b = i / (2 * p.C), r = p.ref[b];
  if (r < 0) return;
  float* out = p.coef + ((long long)b * 4 + 2 * x) * p.C + c;
  if (!(x ? p.adain_k : p.adain_q)) { out[0] = 1.f; out[p.C] = 0.f; return; }
  const bf16* X = x ? p.K : p.Q;
  const int ld = x ? p.ldk : p.ldq;
  const float n = (float)p.S, eps = x ? p.epsk : p.epsq;
  float mu[2], sg[2];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int bb = w ? r : b;
    const float* pp = p.part + (((long long)bb * 2 + x) * p.nslab) * 2 * p.C + c;
    float S1 = 0.f, S2 = 0.f;
    for (int sl = 0; sl < p.nslab; ++sl) { S1 += pp[(long long)(2 * sl) * p.C]; S2 += pp[(long long)(2 * sl + 1) * p.C]; }
    const float d = S1 / n;
    mu[w] = (float)X[(long long)bb * p.S * ld + c] + d;
    sg[w] = sqrtf(fmaxf(S2 - S1 * d, 0.f) / (n - 1.f) + eps);
  }
  const float a = sg[1] / sg[0];
  out[0] = a;
  out[p.C] = mu[1] - a * mu[0];
}
// token rows per slab: about two workgroups per CU over the samples that are read, a slab of at least 64 rows (four per row lane)
static int adain_rows_per_slab(int B, int H, int S) {
  const int wg = 2 * B * cdiv(8 * H, ADAIN_CG);
  const int want = std::max(1, cdiv(512, wg));
  return std::min(std::max(S, 1), cdiv(std::max(cdiv(S, want), 64), ADAIN_RL) * ADAIN_RL);
}
static int adain_shapechk(int B, int H, int S) {
  SHAPECHK(B >= 1 && H >= 1 && H <= 4096 && S >= 1, "attn_adain_coef: empty problem (B=%d H=%d S=%d)", B, H, S);
  SHAPECHK(B <= 32, "attn_adain_coef: at most 32 samples, ref travels in the kernel arguments (B=%d)", B);
  return PEA_OK;
}
size_t attn_adain_scratch_bytes(int B, int H, int S) {
  if (adain_shapechk(B, H, S) != PEA_OK) return 0;
  return sizeof(float) * (size_t)B * 2 * cdiv(S, adain_rows_per_slab(B, H, S)) * 2 * 64 * H;
}
// ref as the shared launcher reads it: ref[b] == b is a plain sample; -> bit masks of the targets and of everything that is read
static int shared_ref_check(const char* who, const int* ref, int B, unsigned& targets, unsigned& used) {
  targets = used = 0;
  for (int b = 0; b < B; ++b) {
    const int r = ref[b];
    if (r < 0 || r == b) continue;
    SHAPECHK(r < B, "%s: ref[%d]=%d is out of range (a sample of the batch of %d, or negative for a plain sample)", who, b, r, B);
    const int rr = ref[r];
    SHAPECHK(rr < 0 || rr == r, "%s: ref[%d]=%d names a reference that is itself a target (ref[%d]=%d)", who, b, r, r, rr);
    targets |= 1u << b;
    used |= 1u << b | 1u << r;
  }
  return PEA_OK;
}
int launch_attn_adain_coef(const bf16* Q, int ldq, const bf16* K, int ldk, int B, int H, int S, const int* ref, float scale,
                           int q_prescaled, int adain_queries, int adain_keys, float* coef, float* scratch, hipStream_t s) {
  if (int rc = adain_shapechk(B, H, S)) return rc;
  AdainP p = AdainP();
  unsigned targets = 0;
  if (int rc = shared_ref_check("attn_adain_coef", ref, B, targets, p.used)) return rc;
  if (!targets) return PEA_OK;                                      // no target: no row to write
  SHAPECHK(S >= 2, "attn_adain_coef: the unbiased variance needs at least two tokens (S=%d)", S);
  const int C = 64 * H;
  SHAPECHK(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= C && ldk >= C,
           "attn_adain_coef: leading dimensions ldq / ldk must be multiples of 8 and hold every head (%d %d)", ldq, ldk);
  SHAPECHK(Q && K && coef && scratch, "attn_adain_coef: null operand (Q, K, coef and the scratch of attn_adain_scratch_bytes)");
  SHAPECHK(((unsigned long long)Q | (unsigned long long)K) % 16 == 0 && ((unsigned long long)coef | (unsigned long long)scratch) % 4 == 0,
           "attn_adain_coef: Q / K 16-byte, coef / scratch 4-byte aligned");
  SHAPECHK(scale > 0.f && scale <= 3.0e38f, "attn_adain_coef: a finite positive scale (%g)", (double)scale);
  p.Q = Q; p.K = K; p.ldq = ldq; p.ldk = ldk; p.B = B; p.C = C; p.S = S;
  p.rps = adain_rows_per_slab(B, H, S); p.nslab = cdiv(S, p.rps);
  const float c = scale * LOG2E;
  p.epsk = 1e-5f; p.epsq = q_prescaled ? c * c * 1e-5f : 1e-5f;
  p.adain_q = adain_queries; p.adain_k = adain_keys; p.part = scratch; p.coef = coef;
  for (int b = 0; b < 32; ++b) p.ref[b] = (targets >> b & 1) ? ref[b] : -1;
  PROF_BEGIN(6, 6.0 * B * S * C, 4.0 * B * S * C, s);
  hipLaunchKernelGGL(attn_adain_part_kernel, dim3(cdiv(C / 8, ADAIN_CG), p.nslab, 2 * B), dim3(256), 0, s, p);
  hipLaunchKernelGGL(attn_adain_coef_kernel, dim3(cdiv(B * 2 * C, 256)), dim3(256), 0, s, p);
  PROF_END(s);
  HIPCHK(hipGetLastError());
  return PEA_OK;
}

// ---- the forward.  A target's workgroup is attn_q_body's forward loop -- the same calls into the streamed-key building blocks --
// run over 2 ceil(S / 64) key tiles: first the sample's own, then the reference's.  Its own: the two resident Q fragment sets, the
// two-segment tile source, and `segc`, the segment's score constant in the log2 domain (q' . s_k, then share_shift log2 e):
// rowc = segc - m_run, rebuilt where the loop changes segment and in the rescale branch.  Each segment's last tile is masked at S.
__device__ __forceinline__ void attn_shared_body(const AttnSharedP& p, char* smem, int blk_x, int head, int b, int r) {
  constexpr int STG = 2 * TILE_BYTES;                            // smem: [2 stages][K tile | V tile]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blk_x * 128 + wave * 32;
  const int frow = lane & 31, fh = lane >> 5;
  const int S = p.Sq, C = 64 * p.H;
  const float cq = p.q_prescaled ? 1.f : p.scale * LOG2E;        // what takes q into the log2 domain

  const bf16* Qb = p.Q + (long long)b * S * p.ldq + head * 64;
  int qrow = q0 + frow;
  const bool qvalid = qrow < S;
  qrow = qvalid ? qrow : S - 1;
  // both resident fragment sets from ONE read of the query row, each rounded to bf16 once from fp32; the own segment's constant
  // from the fp32 q' (this lane holds 32 of the 64 channels, its partner half the others)
  bf16x8 qo[4], qr[4];
  float kc = 0.f;
  {
    const float* cf = p.coef + (long long)b * 4 * C + head * 64 + 8 * fh;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 qv = *(const bf16x8*)(Qb + (long long)qrow * p.ldq + 16 * s + 8 * fh);
#pragma unroll
      for (int h4 = 0; h4 < 2; ++h4) {
        const f32x4 aq = *(const f32x4*)(cf + 16 * s + 4 * h4), sq = *(const f32x4*)(cf + C + 16 * s + 4 * h4);
        const f32x4 ak = *(const f32x4*)(cf + 2 * C + 16 * s + 4 * h4), sk = *(const f32x4*)(cf + 3 * C + 16 * s + 4 * h4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float qp = fmaf(aq[j], (float)qv[4 * h4 + j], sq[j]) * cq;
          qo[s][4 * h4 + j] = (bf16)(qp * ak[j]);
          qr[s][4 * h4 + j] = (bf16)(qp * p.share_scale);
          kc = fmaf(qp, sk[j], kc);
        }
      }
    }
    float ka = kc, kb = kc;
    swap_halves32(ka, kb);
    kc = ka + kb;
  }
  float segc = kc;
  f32x16 rowc;
#pragma unroll
  for (int i = 0; i < 16; ++i) rowc[i] = segc;

  f32x16 oacc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int i2 = 0; i2 < 16; ++i2) oacc[i][i2] = 0.f;
  float m_run = 0.f, l_run = 0.f;

  const TileSrc ko = tile_src(p.K + (long long)b * S * p.ldk + head * 64, p.ldk, S, wave, lane);
  const TileSrc vo = tile_src(p.V + (long long)b * S * p.ldv + head * 64, p.ldv, S, wave, lane);
  const TileSrc kr = tile_src(p.K + (long long)r * S * p.ldk + head * 64, p.ldk, S, wave, lane);
  const TileSrc vr = tile_src(p.V + (long long)r * S * p.ldv + head * 64, p.ldv, S, wave, lane);
  const int nt = (S + 63) / 64;
  stage_tile(ko, 0, smem, wave);
  stage_tile(vo, 0, smem + TILE_BYTES, wave);
  WAIT_VM0();
  __syncthreads();

  const AttnFragOff fo = attn_frag_off(lane);

  for (int t = 0; t < 2 * nt; ++t) {
    const int cur = t & 1;
    const bool own = t < nt;                                     // workgroup-uniform
    if (t + 1 < 2 * nt) {
      char* dst = smem + (cur ^ 1) * STG;
      if (t + 1 < nt) {
        stage_tile(ko, (t + 1) * 64, dst, wave);
        stage_tile(vo, (t + 1) * 64, dst + TILE_BYTES, wave);
      } else {
        stage_tile(kr, (t + 1 - nt) * 64, dst, wave);
        stage_tile(vr, (t + 1 - nt) * 64, dst + TILE_BYTES, wave);
      }
    }
    if (t == nt) {                                               // the reference segment begins: its constant in the C operand
      segc = p.share_shift * LOG2E;
#pragma unroll
      for (int i = 0; i < 16; ++i) rowc[i] = segc - m_run;
    }
    const AttnFragOff ro = attn_ring_off(fo, cur * STG, cur * STG + TILE_BYTES);
    f32x16 sacc[2];
    if (own) attn_rows_product<1>(smem, ro, 0, &qo, rowc, sacc);
    else attn_rows_product<1>(smem, ro, 0, &qr, rowc, sacc);
    const int kv0 = (own ? t : t - nt) * 64;                     // key index inside the segment
    if (kv0 + 64 > S) attn_mask_tail(sacc, kv0, S, fh);          // the segment's last tile, where it is ragged
    attn_online_softmax<false>(sacc, t == 0, m_run, l_run, oacc, rowc, [&](float m) { return segc - m; });
    bf16x8 pf[4];
    attn_pack_p(sacc, pf);
    attn_cols_product<true>(smem, ro, 0, nullptr, lane, pf, oacc);   // transpose read: V by ro / sub; Ts and lane serve the gather only
    WAIT_VM0();
    __syncthreads();
  }
  attn_fwd_exit<1>(oacc, m_run, l_run, nullptr, 0, false, smem + wave * (32 * 144), lane, p.O + (long long)b * S * p.ldo + head * 64, p.ldo, q0, S);
}

// One launch over the batch, 1-D grid: the n_tgt_wg workgroups of the target samples come FIRST in dispatch order (they run twice
// the key tiles of a plain one, so the tail of the launch is made of short workgroups), then those of the plain samples.  Inside
// each of the two ranges the XCD rule (xcd_contiguous) holds, so the query blocks of a (sample, head) -- which stream the same K and V, for a
// target its reference's too -- share an L2.  order[]: the samples in that order.  A plain workgroup is attn_q_body itself on an
// AttnP made of the same operands: the bits of attn_q_kernel<0, true, 1>.
__global__ __launch_bounds__(256, 3) void attn_shared_kernel(const AttnSharedP p, int n_tgt_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned nu = (unsigned)(p.Sq + 127) >> 7, per = nu * p.H, i = blockIdx.x, nt = (unsigned)n_tgt_wg;
  const bool tgt = i < nt;
  const unsigned lin = tgt ? xcd_contiguous(i, nt) : nt + xcd_contiguous(i - nt, gridDim.x - nt);
  const unsigned slot = lin / per, rem = lin - slot * per;
  const int head = (int)(rem / nu), blk = (int)(rem - head * nu), b = p.order[slot];
  if (tgt) {
    attn_shared_body(p, smem, blk, head, b, p.ref[b]);
  } else {
    attn_q_body<0, true, 1, false, true>(attn_plain_p(p), smem, blk, head, b);
  }
}

// ---- host.  A launcher of its own beside the decision table, like the regions, maps and edit launchers.
// plain_first: the plain workgroups above give attn_q_kernel<0, true, 1>'s bits.  Where pea_op_attention_fwd of the same problem
// is another kernel (S = 128: the resident-key kernel; the gather instance under pea_debug_set_attn_tr(0)), that launch runs first
// over the whole batch and the shared kernel's grid holds the targets only, so a plain sample keeps pea_op_attention_fwd's bits
// at every shape.  With no target at all the plain launch is all there is.
struct AttnSharedPlan { int lds, n_tgt, n_tgt_wg, n_plain_wg, plain_first; dim3 grid; AttnP plain; AttnPlan pplan; };
static int attn_plan_shared(AttnSharedP& p, AttnSharedPlan& plan) {
  if (p.nd == 0) p.nd = 1;
  SHAPECHK(p.B > 0 && p.H > 0 && p.H <= 65535 && p.Sq >= 1 && p.Skv >= 1, "attention_shared: empty problem (B=%d H=%d Sq=%d Skv=%d)", p.B, p.H, p.Sq, p.Skv);
  SHAPECHK(p.B <= 32, "attention_shared: at most 32 samples, ref travels in the kernel arguments (B=%d)", p.B);
  SHAPECHK(p.nd == 1, "attention_shared: head_dim 64 only (nd=%d)", p.nd);
  SHAPECHK(p.Sq == p.Skv, "attention_shared: self-attention only, Sq == Skv (Sq=%d Skv=%d)", p.Sq, p.Skv);
  if (int rc = attn_check_operands("attention_shared", {p.Q, p.K, p.V, p.ldq, p.ldk, p.ldv, p.O, p.ldo, 16, nullptr, nullptr, false}, p.H, p.scale)) return rc;
  unsigned targets = 0, used = 0;
  if (int rc = shared_ref_check("attention_shared", p.ref, p.B, targets, used)) return rc;
  plan.n_tgt = __builtin_popcount(targets);
  for (int b = 0; b < 32; ++b)
    if (!(targets >> b & 1)) p.ref[b] = -1;                        // (its own reference, or past the batch: plain)
  if (plan.n_tgt) {
    SHAPECHK(p.Sq >= 2, "attention_shared: a target needs S >= 2, the unbiased variance of its AdaIN has no value at one token (S=%d)", p.Sq);
    SHAPECHK(p.coef != nullptr, "attention_shared: null coef (the AdaIN coefficients are needed while any sample is a target)");
    SHAPECHK((unsigned long long)p.coef % 16 == 0, "attention_shared: coef 16-byte aligned");
    SHAPECHK(p.share_scale == p.share_scale && p.share_shift == p.share_shift && fabsf(p.share_scale) <= 3.0e38f && fabsf(p.share_shift) <= 1.0e30f,
             "attention_shared: finite shared_score_scale / shared_score_shift (%g %g)", (double)p.share_scale, (double)p.share_shift);
  }
  plan.lds = 2 * 2 * TILE_BYTES;
  plan.plain = attn_plain_p(p);
  plan.pplan = AttnPlan();
  if (int rc = attn_plan(0, plan.plain, g_attn_env, plan.pplan)) return rc;
  plan.plain_first = !(plan.pplan.n == 1 && plan.pplan.l[0].kernel == AK_Q + 3);
  const int nu = cdiv(p.Sq, 128);
  int n = 0;
  for (int b = 0; b < p.B; ++b)
    if (targets >> b & 1) p.order[n++] = b;
  for (int b = 0; b < p.B && !plan.plain_first; ++b)
    if (!(targets >> b & 1)) p.order[n++] = b;
  for (int b = n; b < 32; ++b) p.order[b] = 0;
  const long long tw = (long long)plan.n_tgt * p.H * nu, pw = (long long)(n - plan.n_tgt) * p.H * nu;
  SHAPECHK(tw + pw <= 0x7fffffffLL, "attention_shared: %lld workgroups", tw + pw);
  plan.n_tgt_wg = (int)tw; plan.n_plain_wg = (int)pw;
  plan.grid = dim3((unsigned)(tw + pw));
  return PEA_OK;
}
int launch_attention_fwd_shared(const AttnSharedP& p0, hipStream_t s) {
  AttnSharedP p = p0;
  AttnSharedPlan plan;
  int rc = attn_plan_shared(p, plan);
  if (rc) return rc;
  if (!plan.n_tgt) return launch_attention_fwd(plan.plain, s);
  if (plan.plain_first) {
    rc = launch_attention_fwd(plan.plain, s);
    if (rc) return rc;
  }
  const double pairs = (double)(plan.n_tgt * 2 + (plan.plain_first ? 0 : p.B - plan.n_tgt)) * p.H * (double)p.Sq * p.Skv;
  return attn_feature_launch(p.B * p.H, p.Sq, p.Skv, 4.0 * pairs * 64, 2.0 * p.H * 64 * 4.0 * (p.B + plan.n_tgt) * p.Sq, s,
                             [&] { return launch_lds<attn_shared_kernel>(plan.grid, plan.lds, s, p, plan.n_tgt_wg); });
}
// include/pea_hip.h (this one's out[] starts at the grid: it has no key-block count)
extern "C" int pea_debug_attn_shared_dispatch(const int* q, int* out) {
  AttnSharedP p = attn_standin<AttnSharedP>(q[0], q[1], q[2], q[3], 1, q[5]);
  p.nd = q[4]; p.share_scale = 1.f;
  if (!(q[6] & 1)) p.coef = g_standin_page;
  for (int b = 0; b < 32; ++b) p.ref[b] = b < p.B ? q[7 + b] : -1;
  AttnSharedPlan plan;
  const int rc = attn_plan_shared(p, plan);
  if (rc) return rc;
  out[0] = (int)plan.grid.x; out[1] = (int)plan.grid.y; out[2] = (int)plan.grid.z; out[3] = plan.lds;
  out[4] = plan.n_tgt_wg; out[5] = plan.n_plain_wg; out[6] = plan.plain_first; out[7] = plan.n_tgt;
  return PEA_OK;
}
