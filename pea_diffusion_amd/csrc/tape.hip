// The op tape at run time: arena layout and allocation, the weight store (diffusers state-dict keys -> packed bf16 layouts),
// the forward executor and the reverse data-gradient pass.  graph.hip builds the tapes this file runs.
#include <stdlib.h>

#include <algorithm>

#include "model.h"

int Tape::alloc() {
  tag_q_prescale();
  // a depth-to-space tensor (sub-pixel upsampler output) is only understood by concat's first operand and the feature taps
  for (const Op& o : ops) {
    const int in[5] = {o.a, o.kind == OP_LINEAR || o.kind == OP_EMBED ? -1 : o.b, o.kind == OP_LINEAR || o.kind == OP_EMBED ? -1 : o.c, o.res, o.rv};
    for (int k = 0; k < 5; ++k) {
      if (in[k] < 0 || in[k] >= (int)tn.size() || !tn[in[k]].d2s) continue;
      SHAPECHK(o.kind == OP_CONCAT && k == 0 && o.a != o.b, "tape: op kind %d reads a depth-to-space tensor", o.kind);
    }
  }
  // ---- weights
  size_t off = 0;
  size_t max_numel = 0;
  if (owns_weights) {
    for (FusedMat& f : fused) {
      f.off_w = off; off += al256((size_t)f.N * f.K * 2);
      if (f.need_wt) { f.off_wt = off; off += al256((size_t)f.N * f.K * 2); }
      if (f.has_bias) { f.off_bias = off; off += al256((size_t)f.N * 4); }
    }
    for (WSlot& s : slots) {
      max_numel = std::max(max_numel, (size_t)s.numel);
      if (s.fused_parent >= 0) continue;
      if (s.kind == W_VEC || s.kind == W_CONV_IN || s.kind == W_CONV_OUT) { s.off_f32 = off; off += al256(s.numel * 4); }
      else {
        const size_t st = s.kind == W_LINEAR ? (size_t)s.st_n * s.st_k
                          : (s.kind == W_CONV3 && s.subpix ? (size_t)16 * s.d0 * s.d1
                          : (s.kind == W_CONV3 && s.pad_dp ? (size_t)s.d0 * 9 * s.pad_dp : (size_t)s.numel));
        s.off_w = off; off += al256(st * 2);
        if (s.need_wt) { s.off_wt = off; off += al256(st * 2); }
      }
    }
    for (LnFold& f : folds) {
      f.off_wf = off; off += al256((size_t)f.N * f.K * 2);
      f.off_s = off; off += al256((size_t)f.N * 4);
      f.off_t = off; off += al256((size_t)f.N * 4);
    }
    wbytes = off;
    if (!plan_only) {
    HIPCHK(hipMalloc((void**)&warena, wbytes));
    for (FusedMat& f : fused) {
      f.w = (bf16*)(warena + f.off_w);
      if (f.need_wt) f.wt = (bf16*)(warena + f.off_wt);
      if (f.has_bias) f.bias = (float*)(warena + f.off_bias);
    }
    for (WSlot& s : slots) {
      if (s.fused_parent >= 0) {
        FusedMat& f = fused[s.fused_parent];
        if (s.kind == W_VEC) s.f32 = f.bias + s.row_off;
        else {
          s.w = f.w + (size_t)s.row_off * f.K; s.ldw = f.K * s.row_step;
          if (f.need_wt) { s.wt = f.wt + s.row_off; s.ldwt = f.N; s.need_wt = true; }
        }
        continue;
      }
      if (s.off_f32 != (size_t)-1) s.f32 = (float*)(warena + s.off_f32);
      if (s.off_w != (size_t)-1) {
        s.w = (bf16*)(warena + s.off_w);
        s.ldw = s.kind == W_CONV3 ? (s.subpix ? 4 * s.d1 : 9 * (s.pad_dp ? s.pad_dp : s.d1)) : s.st_k;
      }
      if (s.off_wt != (size_t)-1) {
        s.wt = (bf16*)(warena + s.off_wt);
        s.ldwt = s.kind == W_CONV3 ? (s.subpix ? 16 : 9) * s.d0 : s.st_n;
      }
    }
    for (LnFold& f : folds) {
      f.wf = (bf16*)(warena + f.off_wf); f.s = (float*)(warena + f.off_s); f.t = (float*)(warena + f.off_t);
    }
    tmp_f32_elems = max_numel;
    HIPCHK(hipMalloc((void**)&tmp_f32, tmp_f32_elems * 4));
    }
  }
  // ---- activations (+ per-op aux), gradients
  size_t ao = 0, go = 0;
  for (Tn& t : tn) {
    t.off_d = ao; ao += al256((size_t)t.rows * t.cols * 2);
    // gradients exist only for the differentiated samples (merged passes: the leading bwd_batch of B; every tensor is
    // batch-major and the backward pass works on rb(t) = rows / B * bwd_batch leading rows)
    if (needs_grad && t.rg) { t.off_g = go; go += al256((size_t)(bwd_batch > 0 ? t.rows / B * bwd_batch : t.rows) * t.cols * 2); }
  }
  for (Op& o : ops)
    if (o.aux_bytes) { o.aux_off = ao; ao += al256(o.aux_bytes); }
  abytes = ao; gbytes = go;
  return PEA_OK;
}

// Bytes of every scratch buffer of this graph (host only; order: GroupNorm partials, per-sample column sums, attention row
// constants, upsample-conv gradient, FF d(pre-activation), attention dK/dV split partials, stacked K|V split-K partials,
// fp32 time_emb_proj gradient).  Also sets kv_nsplit.
void Tape::scratch_needs(size_t need[8]) {
  size_t delta_elems = 0, ups_elems = 0, part_bytes = 0, geglu_elems = 0;
  for (Op& o : ops) {
    if (o.kind == OP_ATTN) {
      delta_elems = std::max(delta_elems, (size_t)B * o.p0 * o.p1);
      part_bytes = std::max(part_bytes, attention_bwd_scratch_bytes(B, o.p0, o.p1, o.p2, o.p3));
      // the backward runs on the leading bwd_batch samples, and a SMALLER batch can choose MORE dK / dV splits (fewer heads per
      // round): size for that launch too (a 12-sample merged pass differentiating 8 needs 8 splits x 160 heads = 50 MB where the
      // 12-sample count gives 4 x 240 = 38 MB -- a memory fault in round 4's dead-row contexts at batch 8)
      if (bwd_batch > 0) part_bytes = std::max(part_bytes, attention_bwd_scratch_bytes(bwd_batch, o.p0, o.p1, o.p2, o.p3));
    }
    if (o.kind == OP_LINEAR && o.p3 == 3 && o.c >= 0) geglu_elems = std::max(geglu_elems, (size_t)tn[o.c].rows * tn[o.c].cols);
    if (o.kind == OP_CONV3 && o.p1 == 1 && tn[o.a].rg)
      ups_elems = std::max(ups_elems, (size_t)tn[o.out].rows * tn[o.a].cols);
  }
  size_t gn_bytes = 256, cs_bytes = 256;
  for (Op& o : ops) {
    if (o.kind == OP_GN) gn_bytes = std::max(gn_bytes, groupnorm_scratch_bytes(tn[o.a].B, tn[o.a].H * tn[o.a].W, tn[o.a].cols, cfg.groups));
    if (o.kind == OP_CONV3 && o.rv >= 0) cs_bytes = std::max(cs_bytes, colsum_batched_scratch_bytes(tn[o.out].B, tn[o.out].H * tn[o.out].W, tn[o.out].cols));
  }
  for (int i = 0; i < 8; ++i) need[i] = 0;
  need[0] = gn_bytes;
  if (!needs_grad) return;
  need[1] = cs_bytes;
  need[2] = delta_elems * 4 * 2;               // two row constants per (b, h, q): -delta, -lse*log2e
  need[3] = ups_elems * 2;
  need[4] = geglu_elems * 2;
  need[5] = part_bytes;
  if (t_ehs >= 0 && kvall_total > 0) {
    const int ksteps = kvall_total / 64;
    kv_nsplit = std::max(1, std::min(32, ksteps / 128));
    need[6] = sizeof(float) * kv_nsplit * (size_t)tn[t_ehs].rows * tn[t_ehs].cols;
  }
  need[7] = sizeof(float) * (size_t)B * tproj_total;
}
size_t Tape::scratch_own_bytes() const {
  const size_t sz[8] = {sc_gn, sc_cs, sc_delta, sc_ups, sc_geglu, sc_part, sc_kv, sc_tproj};
  size_t t = 0;
  for (int i = 0; i < 8; ++i)
    if (!(scratch_borrowed & (1u << i))) t += sz[i];
  return t;
}

// Activation / gradient arenas and scratch are allocated on first use, not at creation: a trainer that runs merged
// passes never touches the activations of the student and teacher contexts it was given (they only carry the weights),
// which is half of the resident HBM at the benchmark size.
int Tape::ensure_acts() {
  if (aarena) return PEA_OK;
  if (arena_donor) {
    RC(arena_donor->ensure_acts());
    SHAPECHK(abytes <= arena_donor->abytes && gbytes <= arena_donor->gbytes, "tape: borrowed arenas are too small");
    aarena = arena_donor->aarena;
    garena = gbytes ? arena_donor->garena : nullptr;
    arena_borrowed = true;
  } else {
    HIPCHK(hipMalloc((void**)&aarena, abytes));
    if (gbytes) HIPCHK(hipMalloc((void**)&garena, gbytes));
  }
  for (Tn& t : tn) {
    t.d = (bf16*)(aarena + t.off_d);
    if (needs_grad && t.rg) t.g = (bf16*)(garena + t.off_g);
  }
  for (Op& o : ops)
    if (o.aux_bytes) o.aux = (float*)(aarena + o.aux_off);
  for (int e : ext_res) HIPCHK(hipMemset(tn[e].d, 0, (size_t)tn[e].rows * tn[e].cols * 2));   // "no residual" = zeros
  for (Tn& t : tn)
    if (t.zero_init) HIPCHK(hipMemset(t.d, 0, (size_t)t.rows * t.cols * 2));
  // ---- scratch
  for (Op& o : ops)
    if (o.kind == OP_ATTN_MAT && !am_scores) {
      const size_t HW = (size_t)tn[o.a].H * tn[o.a].W;
      HIPCHK(hipMalloc((void**)&am_scores, HW * HW * 2));
      HIPCHK(hipMalloc((void**)&am_vt, HW * tn[o.a].cols * 2));
    }
  size_t need[8];
  scratch_needs(need);
  // A context that borrows its arenas (dead-row contexts of a trainer: one per live-row count, never live together with the
  // donor) borrows the donor's scratch buffers too wherever they are large enough, instead of holding ~0.5 GB of its own each
  // (the FF scratch alone is 0.5 GB at 12 samples, 1024 x 1024): only what the donor cannot cover is allocated here.
  auto want = [&](void** ptr, void* const* donor_ptr, size_t* have, const size_t* donor_have, size_t need, int bit) -> int {
    *have = need;
    if (!need) return PEA_OK;
    if (arena_donor && donor_ptr && *donor_ptr && *donor_have >= need) { *ptr = *donor_ptr; scratch_borrowed |= 1u << bit; return PEA_OK; }
    HIPCHK(hipMalloc(ptr, need));
    return PEA_OK;
  };
  Tape* dn = arena_donor;
#define WANT(field, szf, need, bit) RC(want((void**)&field, dn ? (void* const*)&dn->field : nullptr, &szf, dn ? &dn->szf : nullptr, (need), bit))
  WANT(gn_scratch, sc_gn, need[0], 0);
  WANT(cs_scratch, sc_cs, need[1], 1);
  WANT(delta, sc_delta, need[2], 2);
  WANT(ups_tmp, sc_ups, need[3], 3);
  WANT(geglu_tmp, sc_geglu, need[4], 4);
  WANT(attn_part, sc_part, need[5], 5);
  WANT(kv_part, sc_kv, need[6], 6);
  WANT(tproj_grad, sc_tproj, need[7], 7);
#undef WANT
  if (graph == 1) {
    const Tn& t = tn[t_out_in];
    HIPCHK(hipMalloc((void**)&vae_h, sizeof(float) * (size_t)B * cfg.out_channels * t.H * t.W));
  }
  if (graph == 4) HIPCHK(hipMalloc((void**)&kvlen, sizeof(int) * B));
  if (graph == 4 && tcfg.flavor == 2) {
    const size_t n = (size_t)tcfg.heads * L * (((L + 63) >> 6) << 6);
    HIPCHK(hipMalloc((void**)&rel_bias, n * sizeof(float)));
    HIPCHK(hipMemset(rel_bias, 0, n * sizeof(float)));
    // |key - query| -> sub-bucket (T5Attention._relative_position_bucket): exact below nb/2, then log-spaced up to
    // max_distance; fp32 arithmetic in the order the reference evaluates it
    const int nb = tcfg.rel_buckets / 2, max_exact = nb / 2;
    std::vector<int> tab(L);
    for (int d = 0; d < L; ++d) {
      if (d < max_exact) { tab[d] = d; continue; }
      const float lg = logf((float)d / (float)max_exact) / (float)log((double)tcfg.rel_max_dist / (double)max_exact) * (float)(nb - max_exact);
      tab[d] = std::min(max_exact + (int)lg, nb - 1);
    }
    HIPCHK(hipMalloc((void**)&rel_bucket, sizeof(int) * L));
    HIPCHK(hipMemcpy(rel_bucket, tab.data(), sizeof(int) * L, hipMemcpyHostToDevice));
  }
  if (graph == 3) HIPCHK(hipMalloc((void**)&vae_h, sizeof(float) * (size_t)B * cfg.in_channels * H * W));   // post_quant_conv(z / s)
  RC(pea_zero_page(&zeros));
  return PEA_OK;
}

// Give the activation / gradient arenas and the scratch buffers back (weights stay).  The next forward allocates them
// again (ensure_acts).  For trainers that hold one context per aspect-ratio bucket (utils/custom_dataset_sdxl.py:30) and
// keep only the recently used ones resident.
int Tape::release_acts() {
  HIPCHK(hipDeviceSynchronize());
  if (arena_borrowed) { aarena = nullptr; garena = nullptr; arena_borrowed = false; }    // the donor frees them
  drop_borrowed_scratch();
  void** bufs[] = {(void**)&aarena, (void**)&garena, (void**)&gn_scratch, (void**)&delta, (void**)&ups_tmp, (void**)&tproj_grad,
                   (void**)&cs_scratch, (void**)&attn_part, (void**)&kv_part, (void**)&geglu_tmp, (void**)&am_scores,
                   (void**)&am_vt, (void**)&vae_h, (void**)&kvlen, (void**)&rel_bias, (void**)&rel_bucket};
  for (void** b : bufs)
    if (*b) { HIPCHK(hipFree(*b)); *b = nullptr; }
  for (Tn& t : tn) { t.d = nullptr; t.g = nullptr; }
  for (Op& o : ops) o.aux = nullptr;
  ce_valid = false;
  return PEA_OK;
}

// scratch pointers taken from the arena donor (ensure_acts) are the donor's to free
void Tape::drop_borrowed_scratch() {
  void** sc[] = {(void**)&gn_scratch, (void**)&cs_scratch, (void**)&delta, (void**)&ups_tmp, (void**)&geglu_tmp, (void**)&attn_part,
                 (void**)&kv_part, (void**)&tproj_grad};
  for (int i = 0; i < 8; ++i)
    if (scratch_borrowed & (1u << i)) *sc[i] = nullptr;
  scratch_borrowed = 0;
}

Tape::~Tape() {
  drop_borrowed_scratch();
  if (owns_weights && warena) (void)hipFree(warena);
  if (tmp_f32) (void)hipFree(tmp_f32);
  if (aarena && !arena_borrowed) (void)hipFree(aarena);
  if (garena && !arena_borrowed) (void)hipFree(garena);
  if (gn_scratch) (void)hipFree(gn_scratch);
  if (delta) (void)hipFree(delta);
  if (ups_tmp) (void)hipFree(ups_tmp);
  if (tproj_grad) (void)hipFree(tproj_grad);
  if (cs_scratch) (void)hipFree(cs_scratch);
  if (attn_part) (void)hipFree(attn_part);
  if (kv_part) (void)hipFree(kv_part);
  if (geglu_tmp) (void)hipFree(geglu_tmp);
  if (am_scores) (void)hipFree(am_scores);
  if (am_vt) (void)hipFree(am_vt);
  if (vae_h) (void)hipFree(vae_h);
  if (kvlen) (void)hipFree(kvlen);
  if (rel_bias) (void)hipFree(rel_bias);
  if (rel_bucket) (void)hipFree(rel_bucket);
  if (cross_kvlen) (void)hipFree(cross_kvlen);
  if (inp_buf) (void)hipFree(inp_buf);
  if (fu_buf) (void)hipFree(fu_buf);
  delete ip;
  delete regions;
  delete maps;
  delete edit;
  delete style;
  delete sag;
  delete perturb;
}

int Tape::set_inpaint_cond(const float* mask, const float* masked, int cond_b, int lat_b, hipStream_t s) {
  if (!inpaint_inputs) {
    pea_set_error("pea_unet_set_inpaint_cond: context created without PEA_UNET_INPAINT_INPUTS");
    return PEA_E_STATE;
  }
  SHAPECHK(cond_b > 0 && lat_b > 0 && B % cond_b == 0 && B % lat_b == 0,
           "pea_unet_set_inpaint_cond: cond_batch=%d and latent_batch=%d must each divide the UNet batch %d", cond_b, lat_b, B);
  if (!mask || !masked) {
    pea_set_error("pea_unet_set_inpaint_cond: null mask / masked latents");
    return PEA_E_INVALID;
  }
  const int C = cfg.out_channels;
  const size_t plane = (size_t)H * W;
  if (!inp_buf) HIPCHK(hipMalloc((void**)&inp_buf, sizeof(float) * (size_t)B * (1 + C) * plane));
  HIPCHK(hipMemcpyAsync(inp_buf, mask, sizeof(float) * cond_b * plane, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(inp_buf + (size_t)B * plane, masked, sizeof(float) * cond_b * C * plane, hipMemcpyDeviceToDevice, s));
  inp_set = true;
  inp_cond_b = cond_b;
  inp_lat_b = lat_b;
  return PEA_OK;
}

int Tape::set_freeu(float s1, float s2, float b1, float b2, hipStream_t s) {
  if (graph != 0) { pea_set_error("pea_unet_set_freeu: not a UNet handle (graph %d)", graph); return PEA_E_INVALID; }
  if (needs_grad) {
    pea_set_error("pea_unet_set_freeu: FreeU is an inference feature (no backward through it); this context was created with PEA_UNET_GRAD");
    return PEA_E_STATE;
  }
  for (float f : {s1, s2, b1, b2})
    if (!(f > 0.f && f <= 3.0e38f)) {
      pea_set_error("pea_unet_set_freeu: s1=%g s2=%g b1=%g b2=%g (every factor finite and positive)", (double)s1, (double)s2, (double)b1, (double)b2);
      return PEA_E_INVALID;
    }
  size_t coef = 0, part = 0;
  for (const Op& o : ops) {
    if (o.kind != OP_CONCAT || (o.p0 != 1 && o.p0 != 2)) continue;
    const Tn &a = tn[o.a], &b = tn[o.b];
    SHAPECHK(a.H >= 2 && a.W >= 2, "pea_unet_set_freeu: up block %d works on a %d x %d map (the filter needs H >= 2 and W >= 2)", o.p0 - 1, a.H, a.W);
    SHAPECHK(a.cols % 16 == 0 && b.cols % 8 == 0, "pea_unet_set_freeu: up block %d concatenates %d | %d channels (C1 / 2 and C2 %% 8)", o.p0 - 1, a.cols, b.cols);
    coef = std::max(coef, al256(sizeof(float) * (size_t)a.B * 7 * b.cols));
    part = std::max(part, freeu_scratch_bytes(a.B, a.H, a.W, b.cols));
  }
  if (!fu_buf) {
    HIPCHK(hipMalloc((void**)&fu_buf, coef + part + 256));
    HIPCHK(hipMemsetAsync(fu_buf, 0, coef + part + 256, s));
    fu_coef_bytes = coef;
  }
  fu_s[0] = s1; fu_s[1] = s2; fu_b[0] = b1; fu_b[1] = b2;
  fu_on = true;
  return PEA_OK;
}

int Tape::set_timestep_cond(const float* cond, hipStream_t s) {
  if (t_tcond < 0) {
    pea_set_error("pea_unet_set_timestep_cond: context created without a time_cond_proj_dim (pea_unet_create_cond)");
    return PEA_E_STATE;
  }
  RC(ensure_acts());
  Tn& t = tn[t_tcond];
  if (!cond) HIPCHK(hipMemsetAsync(t.d, 0, (size_t)t.rows * t.cols * 2, s));
  else RC(launch_cast_f32_bf16(cond, t.d, t.rows * t.cols, s));
  return PEA_OK;
}

int Tape::load_weight(const char* name, const float* src, long long numel, hipStream_t s) {
  auto it = slot_by_name.find(name);
  if (it == slot_by_name.end()) {
    pea_set_error("unet: unknown weight '%s'", name);
    return PEA_E_NOTFOUND;
  }
  WSlot& w = slots[it->second];
  SHAPECHK(numel == w.numel, "unet: weight '%s' has %lld elements, expected %lld", name, numel, w.numel);
  switch (w.kind) {
    case W_VEC:
      if (w.pad_mode == 3) { RC(launch_permute_geglu_vec(src, w.f32, (int)(numel / 2), s)); break; }
      if (w.pad_mode == 1) { RC(launch_pad_head_vec(src, w.f32, (int)(numel / w.pad_d), w.pad_d, w.pad_dp, s)); break; }
      HIPCHK(hipMemcpyAsync(w.f32, src, numel * 4, hipMemcpyDeviceToDevice, s));
      break;
    case W_CONV_IN:
      HIPCHK(hipMemcpyAsync(w.f32, src, numel * 4, hipMemcpyDeviceToDevice, s));
      break;
    case W_CONV_OUT:
      RC(launch_pack_conv_out(src, w.f32, w.d0, w.d1, s));
      break;
    case W_LINEAR:
      if (w.pad_mode) {
        RC(launch_pad_gather(src, w.d0, w.d1, w.pad_mode, w.pad_d, w.pad_dp, w.w, w.ldw, w.wt, w.ldwt, w.st_n, w.st_k, s));
      } else if (w.row_step > 1) {      // row-interleaved member of a fused matrix (T5 gated FF)
        RC(launch_pad_gather(src, w.d0, w.d1, 0, 0, 0, w.w, w.ldw, nullptr, 0, w.d0, w.d1, s));
      } else {
        RC(launch_cast_f32_bf16(src, w.w, numel, s));
        if (w.wt) RC(launch_transpose_f32_bf16(src, w.wt, w.d0, w.d1, w.ldwt, s));
      }
      break;
    case W_CONV3:
      if (w.subpix) {
        RC(launch_pack_conv_subpix(src, w.w, w.d0, w.d1, 0, s));
        if (w.wt) RC(launch_pack_conv_subpix(src, w.wt, w.d0, w.d1, 1, s));
        break;
      }
      RC(launch_pack_conv_fwd(src, w.w, w.d0, w.d1, s, w.pad_dp));
      if (w.wt) RC(launch_pack_conv_dgrad(src, w.wt, w.d0, w.d1, s));
      break;
  }
  w.loaded = true;
  fold_dirty = true;
  return PEA_OK;
}

// LoRA fusion: base + sum_i scales[i] * ups[i] . downs[i] composed in fp32 in the load-time staging buffer, then loaded like any
// weight (every packed layout, fold_dirty and the recorded weight sequences behave as for load_weight)
int Tape::load_weight_lora(const char* name, const float* base, long long numel, int n, const float* const* downs,
                           const float* const* ups, const int* ranks, const float* scales, hipStream_t s) {
  if (!owns_weights || plan_only) {
    pea_set_error("pea_unet_load_weight_lora: context borrows its weights");
    return PEA_E_STATE;
  }
  auto it = slot_by_name.find(name);
  if (it == slot_by_name.end()) {
    pea_set_error("unet: unknown weight '%s'", name);
    return PEA_E_NOTFOUND;
  }
  const WSlot& w = slots[it->second];
  SHAPECHK(w.kind != W_VEC, "unet: '%s' is a vector (bias / norm weight): LoRA factors apply to matrices and convolutions", name);
  SHAPECHK(numel == w.numel, "unet: weight '%s' has %lld elements, expected %lld", name, numel, w.numel);
  SHAPECHK(w.d0 > 0 && numel % w.d0 == 0, "unet: weight '%s': %lld elements do not split into %d rows", name, numel, w.d0);
  if (!tmp_f32 || tmp_f32_elems < (size_t)numel) {
    if (tmp_f32) (void)hipFree(tmp_f32);
    tmp_f32 = nullptr;
    tmp_f32_elems = (size_t)numel;
    HIPCHK(hipMalloc((void**)&tmp_f32, tmp_f32_elems * 4));
  }
  const float* acc = base;
  for (int i = 0; i < n; ++i) {
    RC(launch_lora_compose(acc, downs[i], ups[i], tmp_f32, w.d0, (int)(numel / w.d0), ranks[i], scales[i], s));
    acc = tmp_f32;
  }
  return load_weight(name, tmp_f32, numel, s);
}

// (re)compute W' / s / t of every folded LayerNorm from the current weights; blocks until they are in place, because
// contexts that share these weights may read them from other streams
int Tape::ensure_folded(hipStream_t s) {
  if (weights_owner) return weights_owner->ensure_folded(s);
  if (!fold_dirty || folds.empty()) { fold_dirty = false; return PEA_OK; }
  for (LnFold& f : folds) {
    const bf16* W; int ldw; const float* bias = nullptr;
    if (f.fused >= 0) { W = fused[f.fused].w; ldw = fused[f.fused].K; if (fused[f.fused].has_bias) bias = fused[f.fused].bias; }
    else { W = slots[f.w_slot].w; ldw = slots[f.w_slot].ldw; if (f.bias_slot >= 0) bias = slots[f.bias_slot].f32; }
    RC(launch_ln_fold(W, ldw, slots[f.gamma].f32, slots[f.beta].f32, bias, f.wf, f.s, f.t, f.N, f.K, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  fold_dirty = false;
  return PEA_OK;
}

static bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

int Tape::init_random(unsigned long long seed, hipStream_t s) {
  SHAPECHK(owns_weights, "unet: init_random on a context that shares weights");
  unsigned long long i = 0;
  for (WSlot& w : slots) {
    ++i;
    float scale = 0.02f, offset = 0.f;
    if (w.kind == W_LINEAR) scale = 1.0f / sqrtf((float)w.d1);
    else if (w.kind == W_CONV3 || w.kind == W_CONV_IN || w.kind == W_CONV_OUT) scale = 1.0f / sqrtf(9.0f * w.d1);
    else if (ends_with(w.name, ".weight")) { scale = 0.f; offset = 1.f; }    // norm gammas
    RC(launch_fill_random_f32(tmp_f32, w.numel, seed * 1000003ull + i, scale, offset, s));
    RC(load_weight(w.name.c_str(), tmp_f32, w.numel, s));
  }
  return PEA_OK;
}

int Tape::share_weights_from(const Tape& src) {
  SHAPECHK(!owns_weights, "unet: share_weights_from needs a context created without its own weights");
  SHAPECHK(src.slots.size() == slots.size() && src.fused.size() == fused.size(), "unet: configs differ");
  for (size_t i = 0; i < slots.size(); ++i) {
    const WSlot& a = src.slots[i];
    WSlot& b = slots[i];
    SHAPECHK(a.name == b.name && a.numel == b.numel, "unet: weight tables differ at %s", a.name.c_str());
    SHAPECHK(!b.need_wt || a.wt, "unet: source lacks the dgrad layout of %s", a.name.c_str());
    // the packed layout of a conv slot is decided when its tape is built (sub-pixel form of the upsampler convs: [4][Co][4 Ci]
    // against [Co][9 Ci]; padded head / channel widths): a borrower built with the other form would read the other layout
    SHAPECHK(a.subpix == b.subpix && a.pad_dp == b.pad_dp && a.pad_d == b.pad_d && a.pad_mode == b.pad_mode,
             "unet: packed weight layout of %s differs between the two contexts (sub-pixel %d/%d, padding %d/%d)", a.name.c_str(),
             (int)a.subpix, (int)b.subpix, a.pad_dp, b.pad_dp);
    b.f32 = a.f32; b.w = a.w; b.ldw = a.ldw; b.wt = a.wt; b.ldwt = a.ldwt; b.loaded = a.loaded;
  }
  for (size_t i = 0; i < fused.size(); ++i) {
    fused[i].w = src.fused[i].w; fused[i].wt = src.fused[i].wt; fused[i].bias = src.fused[i].bias;
  }
  SHAPECHK(src.folds.size() == folds.size(), "unet: LayerNorm folds differ");
  for (size_t i = 0; i < folds.size(); ++i) { folds[i].wf = src.folds[i].wf; folds[i].s = src.folds[i].s; folds[i].t = src.folds[i].t; }
  weights_owner = src.weights_owner ? src.weights_owner : const_cast<Tape*>(&src);
  wseq_drop();          // the recorded weight sequences name the OLD tables' matrices: the next pass records again
  return PEA_OK;
}

int Tape::all_loaded(std::string* missing) const {
  for (const WSlot& w : slots)
    if (!w.loaded) {
      if (missing) *missing = w.name;
      return 0;
    }
  return 1;
}

// ============================================================================ forward
// What a fused-GEGLU projection (op.p3 == 3 with a stash tensor op.c) leaves in its stash: 1 = (gelu(gate), h * gelu'(gate)),
// the two factors of the backward (GemmP::stash_grad); 0 = the raw (h, gate) pre-activation.  Form 0 is left to the tanh
// form (the T5 encoder's gated-gelu), which keeps no stash and has no backward: every stash a backward pass reads is form 1.
static int geglu_stash_form(const Op& o) {
  return (o.p3 == 3 && o.c >= 0 && o.p1 == 0) ? 1 : 0;
}

int Tape::forward(const float* x, const float* t, const void* ehs, int ehs_dtype, const void* text, int text_dtype,
                  const float* time_ids, float* eps, hipStream_t s) {
  std::string miss;
  if (!all_loaded(&miss)) {
    pea_set_error("unet: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  RC(attn_rules((ip ? AF_IP : 0) | (regions ? AF_REGIONS : 0) | (maps ? AF_MAPS : 0) | (edit ? AF_EDIT : 0) | (style ? AF_STYLE : 0) |
                    (sag ? AF_SAG : 0) | (perturb ? AF_PERTURB : 0), true));
  RC(ensure_acts());
  RC(ensure_folded(s));
  x_in = x; t_in = t; tid_in = time_ids; eps_out = eps;
  if (graph == 0 || graph == 2) {
    Tn& e = tn[t_ehs];
    const long long n = e.rows * e.cols;
    if ((const void*)e.d != ehs) {
      if (ehs_dtype == 0) RC(launch_cast_f32_bf16((const float*)ehs, e.d, n, s));
      else HIPCHK(hipMemcpyAsync(e.d, ehs, n * 2, hipMemcpyDeviceToDevice, s));
    }
    if (t_text >= 0) {
      Tn& q = tn[t_text];
      SHAPECHK(text != nullptr && time_ids != nullptr, "unet: text_embeds/time_ids required (text_time)");
      const long long m = q.rows * q.cols;
      if ((const void*)q.d != text) {
        if (text_dtype == 0) RC(launch_cast_f32_bf16((const float*)text, q.d, m, s));
        else HIPCHK(hipMemcpyAsync(q.d, text, m * 2, hipMemcpyDeviceToDevice, s));
      }
    }
  }
  if (graph == 0) wseq_begin(wseq_fwd);                              // (the UNet of the step / of the denoise loop)
  const int rc_ops = exec_ops(0, ops.size(), true, s);
  if (rc_ops == PEA_OK) wseq_end();
  else wseq_cur = nullptr;
  RC(rc_ops);
  if (graph == 2) ce_valid = true;
  return PEA_OK;
}

int Tape::gemm(GemmP& p, hipStream_t s) {
  if (WSeq* q = wseq_cur) {
    // contiguous weight matrices only (every Linear / conv / fused matrix of the tapes: ldw == K)
    const long long bytes = (p.ldw == p.K && p.ksplit <= 1) ? (long long)p.N * p.K * 2 : 0;
    if (!q->ready) q->w.push_back({(const void*)p.W, bytes});
    else {
      const size_t i = q->pos++;
      if (i >= q->w.size() || q->w[i].first != (const void*)p.W) { q->ready = false; q->w.clear(); wseq_cur = nullptr; }
      else {
        if (i + 1 < q->w.size()) {
          // armed only for a target inside the weights owner's arena: a recorded pointer that no longer is (a weights owner
          // re-created behind a borrower's back) would send the DMA waves' touch loads to unmapped memory -- a GPU page fault
          const Tape* ow = weights_owner ? weights_owner : this;
          const char* t = (const char*)q->w[i + 1].first;
          const long long nb = q->w[i + 1].second;
          if (ow->warena && t >= ow->warena && t + nb <= ow->warena + ow->wbytes) { p.pf_ptr = t; p.pf_bytes = nb; }
          else { q->ready = false; q->w.clear(); wseq_cur = nullptr; }
        }
      }
    }
  }
  return launch_gemm(p, s);
}

// ops [begin, end) of the tape in order; skip_cached: leave out the ControlNet conditioning embedding when it is valid
int Tape::exec_ops(size_t begin, size_t end, bool skip_cached, hipStream_t s) {
  RC(ensure_acts());
  for (size_t oi = begin; oi < end; ++oi) {
    Op& o = ops[oi];
    if (skip_cached && ce_valid && (int)oi >= ce_begin && (int)oi < ce_end) continue;   // cached conditioning embedding
    switch (o.kind) {
      case OP_TEMB: {
        Tn& out = tn[o.out];
        if (o.src == 0) RC(launch_timestep_embed(t_in, out.d, B, o.p0, s));
        else RC(launch_timestep_embed(tid_in, out.d, B * 6, o.p0, s));
        break;
      }
      case OP_LINEAR: {
        Tn &a = tn[o.a], &out = tn[o.out];
        GemmP p; fill_gemm(p);
        p.A = a.d; p.lda = a.cols; p.M = (int)a.rows; p.K = a.cols; p.N = out.cols;
        if (o.fused >= 0) { FusedMat& f = fused[o.fused]; p.W = f.w; p.ldw = f.K; p.bias = f.bias; }
        else { WSlot& w = slots[o.w]; p.W = w.w; p.ldw = w.ldw; p.bias = o.bias >= 0 ? slots[o.bias].f32 : nullptr; }
        p.C = out.d; p.ldc = out.cols; p.act = o.p2;
        p.qscale_cols = o.qs_cols; p.qscale = o.qs;
        if (o.p3 == 3) {                  // fused GEGLU: N = 8C interleaved, y -> out, pre-activation -> op.c (student only)
          p.N = 2 * out.cols; p.geglu_y = out.d; p.ldy = out.cols; p.geglu_tanh = o.p1;
          p.C = o.c >= 0 ? tn[o.c].d : nullptr; p.ldc = 2 * out.cols;
          if (bwd_batch > 0) p.stash_rows = (int)(out.rows / B * bwd_batch);   // only the differentiated samples are stashed
          p.stash_grad = o.stash_form = geglu_stash_form(o);        // the form travels with the stash (Op::stash_form)
        }
        if (o.res >= 0) { p.res = tn[o.res].d; p.ldres = tn[o.res].cols; }
        if (o.fold >= 0) {                // folded LayerNorm: the GEMM reads the un-normalised rows
          const LnFold& f = folds[o.fold];
          p.A = tn[ops[f.ln_op].a].d; p.W = f.wf; p.ldw = f.K; p.bias = f.t;
          p.ln_stats = ops[f.ln_op].aux; p.ln_s = f.s;
        }
        RC(gemm(p, s));
        break;
      }
      case OP_ATTN_MAT: {              // one head over all H*W tokens: S = Q K^T, row softmax, O = P V per image
        Tn &q = tn[o.a], &k = tn[o.b], &v = tn[o.c], &out = tn[o.out];
        const int HW = q.H * q.W, C = q.cols;
        for (int b = 0; b < B; ++b) {
          const long long off = (long long)b * HW * C;
          GemmP p; fill_gemm(p);
          p.A = q.d + off; p.lda = C; p.M = HW; p.K = C; p.W = k.d + off; p.ldw = C; p.N = HW; p.C = am_scores; p.ldc = HW;
          RC(launch_gemm(p, s));
          RC(launch_softmax_rows(am_scores, HW, HW, HW, o.f0, s));
          RC(launch_transpose_bf16(v.d + off, am_vt, HW, C, HW, s));
          GemmP r; fill_gemm(r);
          r.A = am_scores; r.lda = HW; r.M = HW; r.K = HW; r.W = am_vt; r.ldw = HW; r.N = C; r.C = out.d + off; r.ldc = C;
          RC(launch_gemm(r, s));
        }
        break;
      }
      case OP_EMBED: {
        SHAPECHK(ids_in != nullptr, "text encoder: no input ids");
        Tn& out = tn[o.out];
        RC(launch_embed_tokens(ids_in, slots[o.w].w,
                               o.bias >= 0 ? slots[o.bias].w + (long long)tcfg.pos_offset * out.cols : nullptr,
                               o.c >= 0 ? slots[o.c].w : nullptr, out.d, B, L, out.cols, tcfg.vocab, s));
        break;
      }
      case OP_VIS_EMBED: {
        Tn& out = tn[o.out];
        RC(launch_vision_embed(tn[o.a].d, slots[o.w].f32, slots[o.bias].w, slots[o.p0].f32, slots[o.p1].f32, out.d, B, L, out.cols,
                               o.f0, s));
        break;
      }
      case OP_CLS_ROW:
        RC(launch_copy2d(tn[o.a].d, L * tn[o.a].cols, tn[o.out].d, tn[o.out].cols, B, tn[o.out].cols, 0, s));
        break;
      case OP_GATHER_EOS:
        RC(launch_gather_eos(ids_in, tn[o.a].d, tn[o.out].d, B, L, tn[o.a].cols, tcfg.eos_id, s));
        break;
      case OP_ADD:
        RC(launch_add(tn[o.a].d, tn[o.b].d, tn[o.out].d, tn[o.out].rows * tn[o.out].cols, s));
        break;
      case OP_SILU:
        RC(launch_silu_fwd(tn[o.a].d, tn[o.out].d, tn[o.a].rows * tn[o.a].cols, s));
        break;
      case OP_CONCAT:
        if (fu_on && (o.p0 == 1 || o.p0 == 2)) {   // FreeU: the skip's low-frequency sums, then the concat that scales and filters
          const Tn &a = tn[o.a], &b = tn[o.b];
          const float fs = fu_s[o.p0 - 1], fb = fu_b[o.p0 - 1];
          if (fs != 1.f) RC(launch_freeu_coef(b.d, a.B, a.H, a.W, b.cols, fu_buf, (float*)((char*)fu_buf + fu_coef_bytes), s));
          RC(launch_concat2_freeu(a.d, a.cols, b.d, b.cols, fu_buf, tn[o.out].d, a.B, a.H, a.W, fs, fb, s, a.d2s ? a.H : 0,
                                  a.d2s ? a.W : 0));
          break;
        }
        RC(launch_concat2(tn[o.a].d, tn[o.a].cols, tn[o.b].d, tn[o.b].cols, tn[o.out].d, tn[o.a].rows, s,
                          tn[o.a].d2s ? tn[o.a].H : 0, tn[o.a].d2s ? tn[o.a].W : 0));
        break;
      case OP_CONV_IN:
        if (o.src == 1) {              // ControlNet conditioning image -> first (channel-padded) embedding tensor
          SHAPECHK(cond_in != nullptr, "controlnet: no conditioning image set");
          RC(launch_conv_in(cond_in, slots[o.w].f32, slots[o.bias].f32, tn[o.out].d, B, 3, tn[o.out].H, tn[o.out].W,
                            o.p0, s, tn[o.out].cols, o.p3 == 2));
          break;
        }
        if (inp_set) {                 // inpainting: latents from x_in, mask / masked latents from the context
          RC(launch_conv_in_gather(x_in, inp_buf, inp_buf + (size_t)B * H * W, slots[o.w].f32, slots[o.bias].f32, tn[o.out].d,
                                   B, cfg.out_channels, inp_lat_b, inp_cond_b, H, W, tn[o.out].cols, s));
          break;
        }
        RC(launch_conv_in(x_in, slots[o.w].f32, slots[o.bias].f32, tn[o.out].d, B, cfg.in_channels, H, W,
                          tn[o.out].cols, s));
        break;
      case OP_CONV3: {
        Tn &a = tn[o.a], &out = tn[o.out];
        GemmP p; fill_gemm(p);
        p.mode = 1; p.A = a.d; p.W = slots[o.w].w; p.ldw = slots[o.w].ldw; p.C = out.d; p.ldc = out.cols;
        p.Hs = a.H; p.Ws = a.W; p.Cin = a.cols; p.Ho = out.H; p.Wo = out.W; p.stride = o.p0; p.shift = o.p1 ? 1 : 0;
        p.M = (int)out.rows; p.N = slots[o.w].d0; p.K = 9 * a.cols; p.bias = slots[o.bias].f32; p.zeros = zeros;
        p.act = o.p3;
        p.rows_per_batch = out.H * out.W; p.pad_off = o.p2;
        if (o.rv >= 0) { p.rowvec = tn[o.rv].d + o.rv_off; p.ldrv = tn[o.rv].cols; }
        if (o.res >= 0) { p.res = tn[o.res].d; p.ldres = tn[o.res].cols; }
        if (o.p1 == 2) {
          // sub-pixel form: one 2 x 2 conv over the SOURCE per output parity, written into that parity's channel block of the
          // depth-to-space output (row stride 4 Cout).  pack_conv_subpix_kernel has the tap sums.
          SHAPECHK(o.rv < 0 && o.res < 0 && !o.p3 && !o.p2 && o.p0 == 1, "unet: sub-pixel upsampler conv with an epilogue operand");
          const int Cout = slots[o.w].d0;
          p.shift = 0; p.kside = 2; p.Ho = a.H; p.Wo = a.W; p.M = (int)a.rows; p.K = 4 * a.cols; p.ldc = 4 * Cout;
          p.rows_per_batch = a.H * a.W;
          for (int pl = 0; pl < 4; ++pl) {
            p.W = slots[o.w].w + (size_t)pl * Cout * 4 * a.cols;
            p.C = out.d + (size_t)pl * Cout;
            p.pad_off = pl >> 1; p.pad_dx = (pl & 1) - (pl >> 1);
            RC(gemm(p, s));
          }
          break;
        }
        RC(gemm(p, s));
        break;
      }
      case OP_GN: {
        Tn& a = tn[o.a];
        RC(launch_groupnorm_fwd(a.d, slots[o.w].f32, slots[o.bias].f32, tn[o.out].d, o.aux, gn_scratch, a.B,
                                a.H * a.W, a.cols, cfg.groups, o.f0, o.p0, s));
        break;
      }
      case OP_LN: {
        Tn& a = tn[o.a];
        if (o.fold >= 0) {                // folded into its consumer: statistics only
          RC(launch_layernorm_stats(a.d, o.aux, (int)a.rows, a.cols, o.f0, s));
          break;
        }
        if (o.p0 == 1) {                  // T5LayerNorm
          RC(launch_rmsnorm_fwd(a.d, slots[o.w].f32, tn[o.out].d, (int)a.rows, a.cols, o.f0, s));
          break;
        }
        RC(launch_layernorm_fwd(a.d, slots[o.w].f32, slots[o.bias].f32, tn[o.out].d, o.aux, (int)a.rows, a.cols, o.f0,
                                s));
        break;
      }
      case OP_ATTN:                     // the plain launch, or what the inference features make of it (attn_features.hip)
        RC(attn_forward(oi, s));
        break;
      case OP_ATTN_FEWQ: {             // the latents over the image rows' keys and their own, one softmax, both read in place
        AttnP p; memset(&p, 0, sizeof(p));
        const Tn &a = tn[o.a], &k = tn[o.b], &v = tn[o.c];
        p.Q = a.d + o.acol; p.ldq = a.cols; p.K = k.d + o.bcol; p.ldk = k.cols; p.V = v.d + o.ccol; p.ldv = v.cols;
        p.K2 = a.d + o.k2col; p.V2 = a.d + o.v2col; p.ldk2 = p.ldv2 = a.cols; p.Skv2 = o.p1;
        p.O = tn[o.out].d; p.ldo = tn[o.out].cols;
        p.B = B; p.H = o.p0; p.Sq = o.p1; p.Skv = o.p2; p.scale = o.f0; p.nd = o.p3; p.q_prescaled = o.pre;
        RC(launch_attention_fwd_fewq(p, s));
        break;
      }
      case OP_GEGLU:
        RC(launch_geglu_fwd(tn[o.a].d, tn[o.out].d, tn[o.a].rows, tn[o.out].cols, s));
        break;
      case OP_CONV_OUT:
        RC(launch_conv_out(tn[o.a].d, slots[o.w].f32, slots[o.bias].f32, eps_out, B, tn[o.a].cols, tn[o.a].H, tn[o.a].W,
                           cfg.out_channels, s));
        break;
    }
  }
  return PEA_OK;
}

// ============================================================================ backward
// 1 (default): the GEGLU backward runs in the epilogue of the FF output projection's dgrad GEMM; 0: as its own kernel (A/B,
// and the cross-check of tests/test_model_gpu.py).  PEA_GEGLU_BWD_UNFUSED in the environment starts with 0.
static int g_geglu_bwd_fused = getenv("PEA_GEGLU_BWD_UNFUSED") ? 0 : 1;
extern "C" void pea_debug_set_geglu_bwd_fused(int v) { g_geglu_bwd_fused = v; }
void Tape::begin_backward() {
  for (Tn& t : tn) { t.gw = false; t.gpend = nullptr; }
}

int Tape::backward(const float* deps, hipStream_t s) {
  SHAPECHK(needs_grad, "unet: created without gradient support");
  RC(ensure_acts());
  // bwd_batch < B: the forward ran on B samples (student rows first, teacher rows behind them: merged passes of a
  // trainer whose teacher IS the student checkpoint) and only the first bwd_batch samples are differentiated.
  // Every tensor is batch-major, so the restricted pass is the same tape on the leading rows of every tensor.
  const int Bb = bwd_batch > 0 ? bwd_batch : B;
  auto rb = [&](const Tn& t) -> long long { return t.rows / B * Bb; };
  HIPCHK(hipMemsetAsync(tproj_grad, 0, sizeof(float) * Bb * tproj_total, s));
  struct WSeqScope {                       // record / replay the pass's weight sequence (next-op prefetch); an error path drops it
    Tape* t; bool ok = false;
    ~WSeqScope() { if (ok) t->wseq_end(); else t->wseq_cur = nullptr; }
  } wscope{this};
  if (graph == 0) wseq_begin(wseq_bwd);
  // A residual connection hands its gradient on unchanged.  Instead of copying / adding it into the skip tensor's
  // buffer at once, the skip tensor remembers it as a PENDING alias (Tn::gpend) and the next kernel that writes that
  // tensor's gradient (LayerNorm / GroupNorm backward, dgrad GEMM) takes it as its addend: one launch and one
  // read+write of the tensor less per residual.  Writers without an addend input materialise the alias first.
  auto addend = [](Tn& t) -> const bf16* {       // addend for a kernel about to write t.g (consumes a pending alias)
    if (t.gw) return t.g;
    const bf16* p = t.gpend;
    t.gpend = nullptr;
    return p;
  };
  auto materialize = [&](Tn& t) -> int {         // for writers that can only accumulate in place
    if (!t.gw && t.gpend) {
      RC(launch_accum(t.gpend, t.g, rb(t) * t.cols, 0, s));
      t.gpend = nullptr;
      t.gw = true;
    }
    return PEA_OK;
  };
  auto pass_on = [&](Tn& from, Tn& r) -> int {   // residual: r.g += from.g, deferred when r has no gradient yet
    if (!r.gw && !r.gpend) { r.gpend = from.g; return PEA_OK; }
    RC(materialize(r));
    RC(launch_accum(from.g, r.g, rb(r) * r.cols, 1, s));
    return PEA_OK;
  };
  int dpre_of = -1;          // tensor whose gradient currently lives in geglu_tmp as d(pre-activation) (fused GEGLU backward)
  for (int oi = (int)ops.size() - 1; oi >= 0; --oi) {
    Op& o = ops[oi];
    if (o.kind == OP_CONV_OUT) {
      if (!deps) continue;
      Tn& a = tn[o.a];
      SHAPECHK(!a.gw, "unet: conv_out input gradient already written");
      RC(launch_conv_out_dgrad(deps, slots[o.w].f32, a.g, Bb, a.cols, H, W, cfg.out_channels, s));
      a.gw = true;
      continue;
    }
    if (o.out < 0) continue;
    Tn& out = tn[o.out];
    if (!out.rg) continue;
    if (o.kind == OP_LINEAR && o.p3 == 1) {   // fused time_emb_proj: gradient collected in fp32
      RC(launch_cast_f32_bf16(tproj_grad, out.g, (long long)Bb * tproj_total, s));
      out.gw = true;
    }
    RC(materialize(out));
    if (!out.gw) continue;                     // no consumer produced a gradient for this tensor
    switch (o.kind) {
      case OP_LINEAR: {
        Tn& a = tn[o.a];
        if (a.rg && o.p3 == 2) {          // stacked K|V projection: M = B*L rows, K = sum(2C) -> split-K + ordered reduce
          FusedMat& f = fused[o.fused];
          GemmP p; fill_gemm(p);
          p.A = out.g; p.lda = out.cols; p.M = (int)rb(out); p.K = out.cols; p.N = a.cols;
          p.W = f.wt; p.ldw = f.N; p.C = kv_part; p.ldc = a.cols; p.out_f32 = 1;
          p.ksplit = kv_nsplit; p.split_stride = rb(out) * a.cols;
          RC(gemm(p, s));
          RC(materialize(a));
          RC(launch_splitk_reduce(kv_part, kv_nsplit, p.split_stride, a.g, a.cols, (int)rb(a), a.cols, a.gw, s));
          a.gw = true;
          break;
        }
        if (a.rg && o.p3 == 3) {          // fused GEGLU: d(pre-activation) into scratch, then the dgrad GEMM over K = 8C
          Tn& hg = tn[o.c];
          SHAPECHK(o.stash_form == 1, "unet: GEGLU op %d has no stash from a forward pass", oi);
          if (dpre_of != o.out) RC(launch_geglu_bwd_il(hg.d, out.g, geglu_tmp, rb(out), out.cols, s));
          dpre_of = -1;
          WSlot& w = slots[o.w];
          GemmP p; fill_gemm(p);
          p.A = geglu_tmp; p.lda = hg.cols; p.M = (int)rb(out); p.K = hg.cols; p.N = a.cols;
          p.W = w.wt; p.ldw = w.ldwt; p.C = a.g; p.ldc = a.cols;
          SHAPECHK(p.W != nullptr, "unet: dgrad weights missing for op %d", oi);
          if (const bf16* ad = addend(a)) { p.res = ad; p.ldres = a.cols; }
          RC(gemm(p, s));
          a.gw = true;
          break;
        }
        if (a.rg) {
          GemmP p; fill_gemm(p);
          p.A = out.g; p.lda = out.cols; p.M = (int)rb(out); p.K = out.cols; p.N = a.cols;
          if (o.fused >= 0) { FusedMat& f = fused[o.fused]; p.W = f.wt; p.ldw = f.N; }
          else { WSlot& w = slots[o.w]; p.W = w.wt; p.ldw = w.ldwt; }
          SHAPECHK(p.W != nullptr, "unet: dgrad weights missing for op %d", oi);
          // The FF output projection right behind a fused-GEGLU projection: its input gradient d y is only ever consumed
          // by the GEGLU backward, so that runs in this GEMM's epilogue and d(pre-activation) lands in the scratch the
          // next (GEGLU) op's dgrad reads -- d y is never written, one launch and a read + write of it less per block.
          const Op* prev = oi > 0 ? &ops[oi - 1] : nullptr;
          if (g_geglu_bwd_fused && prev && prev->kind == OP_LINEAR && prev->p3 == 3 && prev->out == o.a && prev->c >= 0 &&
              tn[prev->a].rg && !a.gw && !a.gpend && geglu_tmp && a.cols % 16 == 0) {
            Tn& hg = tn[prev->c];
            SHAPECHK(prev->stash_form >= 0, "unet: GEGLU op %d has no stash from a forward pass", oi - 1);
            p.gbwd_pre = hg.d; p.ldgp = hg.cols; p.gbwd_form = prev->stash_form;
            p.C = geglu_tmp; p.ldc = hg.cols;
            RC(gemm(p, s));
            a.gw = true;
            dpre_of = o.a;
          } else {
            p.C = a.g; p.ldc = a.cols;
            if (const bf16* ad = addend(a)) { p.res = ad; p.ldres = a.cols; }
            RC(gemm(p, s));
            a.gw = true;
          }
        }
        if (o.res >= 0 && tn[o.res].rg) RC(pass_on(out, tn[o.res]));
        break;
      }
      case OP_SILU: {
        Tn& a = tn[o.a];
        if (a.rg) { RC(materialize(a)); RC(launch_silu_bwd(a.d, out.g, a.g, rb(a) * a.cols, a.gw, s)); a.gw = true; }
        break;
      }
      case OP_CONCAT: {
        Tn &a = tn[o.a], &b = tn[o.b];
        if (o.a == o.b) {                 // cat(x, x): a UNet without a mid block feeds the last down output to the first
          if (a.rg) {                     // up resnet both as hidden state and as skip -> two ordered passes into one buffer
            RC(materialize(a));
            RC(launch_split2(out.g, a.cols, b.cols, a.g, a.gw, nullptr, false, rb(a), s));
            RC(launch_split2(out.g, a.cols, b.cols, nullptr, false, a.g, true, rb(a), s));
            a.gw = true;
          }
          break;
        }
        if (a.rg) RC(materialize(a));
        if (b.rg) RC(materialize(b));
        RC(launch_split2(out.g, a.cols, b.cols, a.rg ? a.g : nullptr, a.gw, b.rg ? b.g : nullptr, b.gw, rb(a), s,
                         a.d2s ? a.H : 0, a.d2s ? a.W : 0));
        if (a.rg) a.gw = true;
        if (b.rg) b.gw = true;
        break;
      }
      case OP_CONV3: {
        Tn& a = tn[o.a];
        if (a.rg) {
          WSlot& w = slots[o.w];
          SHAPECHK(w.wt != nullptr, "unet: conv dgrad weights missing for %s", w.name.c_str());
          GemmP p; fill_gemm(p);
          p.mode = 1; p.A = out.g; p.W = w.wt; p.ldw = w.ldwt; p.Hs = out.H; p.Ws = out.W; p.Cin = out.cols;
          p.N = a.cols; p.K = 9 * out.cols; p.zeros = zeros; p.stride = 1;
          if (o.p1 == 2) {       // sub-pixel form: 16 taps (4 parity blocks x 2 x 2) over the depth-to-space d out, one launch
            p.W = w.wt; p.ldw = w.ldwt; p.Hs = a.H; p.Ws = a.W; p.pix = 4 * out.cols; p.kside = 4; p.K = 16 * out.cols;
            p.pad_off = 1; p.Ho = a.H; p.Wo = a.W; p.M = (int)rb(a); p.C = a.g; p.ldc = a.cols;
            if (const bf16* ad = addend(a)) { p.res = ad; p.ldres = a.cols; }
            RC(gemm(p, s));
          } else if (o.p1) {     // upsample-folded conv: gradient at the upsampled resolution, then 2x2 sum
            p.Ho = out.H; p.Wo = out.W; p.M = (int)rb(out); p.C = ups_tmp; p.ldc = a.cols;
            RC(gemm(p, s));
            RC(materialize(a));
            RC(launch_sumpool2(ups_tmp, a.g, Bb, a.H, a.W, a.cols, a.gw, s));
          } else {
            if (o.p0 == 2) { p.shift = 1; p.parity = 1; }
            p.Ho = a.H; p.Wo = a.W; p.M = (int)rb(a); p.C = a.g; p.ldc = a.cols;
            if (const bf16* ad = addend(a)) { p.res = ad; p.ldres = a.cols; }
            RC(gemm(p, s));
          }
          a.gw = true;
        }
        if (o.rv >= 0 && tn[o.rv].rg)
          RC(launch_colsum_batched(out.g, tproj_grad + o.rv_off, Bb, out.H * out.W, out.cols, tproj_total, cs_scratch, s));
        if (o.res >= 0 && tn[o.res].rg) RC(pass_on(out, tn[o.res]));
        break;
      }
      case OP_GN: {
        Tn& a = tn[o.a];
        if (a.rg) {
          RC(launch_groupnorm_bwd(a.d, out.g, slots[o.w].f32, slots[o.bias].f32, o.aux, a.g, gn_scratch, Bb,
                                  a.H * a.W, a.cols, cfg.groups, o.p0, addend(a), s));
          a.gw = true;
        }
        break;
      }
      case OP_LN: {
        Tn& a = tn[o.a];
        if (a.rg) {
          RC(launch_layernorm_bwd(a.d, out.g, slots[o.w].f32, o.aux, a.g, nullptr, nullptr, (int)rb(a), a.cols,
                                  addend(a), s));
          a.gw = true;
        }
        break;
      }
      case OP_ATTN: {
        Tn &q = tn[o.a], &k = tn[o.b], &v = tn[o.c];
        AttnP p; memset(&p, 0, sizeof(p));
        p.Q = q.d + o.acol; p.ldq = q.cols; p.K = k.d + o.bcol; p.ldk = k.cols; p.V = v.d + o.ccol; p.ldv = v.cols;
        p.O = out.d; p.ldo = out.cols; p.lse = o.aux; p.B = Bb; p.H = o.p0; p.Sq = o.p1; p.Skv = o.p2; p.scale = o.f0;
        p.nd = o.p3; p.q_prescaled = o.pre;
        p.dO = out.g; p.lddo = out.cols; p.delta = delta; p.dkv_part = attn_part;
        if (cross_kvlen && o.b == t_kvall) p.kv_len = cross_kvlen;
        SHAPECHK(!q.gw && !q.gpend && !k.gpend && (!k.gw || o.b == t_kvall), "unet: attention operand gradient written twice");
        if (q.rg) { p.dQ = q.g + o.acol; p.lddq = q.cols; }
        if (k.rg) { p.dK = k.g + o.bcol; p.lddk = k.cols; p.dV = v.g + o.ccol; p.lddv = v.cols; }
        RC(launch_attention_bwd(p, s));
        if (q.rg) q.gw = true;
        if (k.rg) { k.gw = true; v.gw = true; }
        break;
      }
      case OP_GEGLU: {
        Tn& a = tn[o.a];
        if (a.rg) {
          SHAPECHK(!a.gw, "unet: geglu input gradient written twice");
          RC(launch_geglu_bwd(a.d, out.g, a.g, rb(a), out.cols, s));
          a.gw = true;
        }
        break;
      }
      default:
        break;
    }
  }
  for (Tn& t : tn)
    if (t.rg) RC(materialize(t));              // graph inputs that only ever received a passed-on gradient
  wscope.ok = true;
  return PEA_OK;
}
