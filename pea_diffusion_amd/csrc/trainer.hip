// The fused KD training step (train_sdxl_zh.py:311-441 after the frozen encoders): two-stream, merged-pass and dead-row forms.
#include <stdlib.h>

#include <memory>

#include "model.h"

Trainer::~Trainer() {
  if (side) { (void)hipStreamDestroy(side); (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join); }
  for (void* p : {(void*)xt, (void*)eps_s, (void*)eps_t, (void*)deps, (void*)ac, (void*)t_ehs_sel, (void*)dehs_full, (void*)t_f32,
                  (void*)losses, (void*)kd_ws, (void*)tehs_c, (void*)tehs_n, (void*)xt2, (void*)eps2, (void*)t2, (void*)tid2})
    if (p) (void)hipFree(p);
  for (auto& kv : merged_n) delete kv.second;           // (their arenas are borrowed from `merged`: freed below)
  if (tmap_d) (void)hipFree(tmap_d);
  if (tpool_c) (void)hipFree(tpool_c);
  delete merged;
}

int Trainer::prepare() {
  if (const char* e = getenv("PEA_TWO_STREAM")) two_stream = atoi(e);
  if (const char* e = getenv("PEA_MERGE_PASSES")) merge_passes = atoi(e);
  Tape& S = *student;
  Tape& Tt = *teacher;
  SHAPECHK(S.needs_grad, "trainer: student context needs gradient support");
  SHAPECHK(S.B == Tt.B && S.H == Tt.H && S.W == Tt.W, "trainer: student/teacher shapes differ");
  // the noise, eps and KD-loss buffers below are sized by in_channels: a UNet whose input is wider than its output (the 9-channel
  // inpainting UNet) has no KD step here
  SHAPECHK(S.cfg.in_channels == S.cfg.out_channels && Tt.cfg.in_channels == Tt.cfg.out_channels,
           "trainer: in_channels must equal out_channels (student %d -> %d, teacher %d -> %d); an inpainting UNet is not trained",
           S.cfg.in_channels, S.cfg.out_channels, Tt.cfg.in_channels, Tt.cfg.out_channels);
  // feature taps are paired by hook name (d0.., m, u0..: cast_hook, train_sdxl_zh.py:79-84).  A student without a mid
  // block (SSD-1B-style, mid_block_type null) has no 'm' tap: that term leaves the feature loss (the reference's
  // cast_hook would fail on `unet.mid_block is None`; every other tap must exist on both sides).
  tap_pairs.clear();
  for (size_t k = 0; k < S.taps.size(); ++k) {
    int found = -1;
    for (size_t j = 0; j < Tt.taps.size(); ++j)
      if (Tt.tap_names[j] == S.tap_names[k]) found = (int)j;
    SHAPECHK(found >= 0, "trainer: the teacher has no '%s' tap", S.tap_names[k].c_str());
    SHAPECHK(S.tn[S.taps[k]].rows == Tt.tn[Tt.taps[found]].rows && S.tn[S.taps[k]].cols == Tt.tn[Tt.taps[found]].cols,
             "trainer: tap '%s' shapes differ", S.tap_names[k].c_str());
    tap_pairs.push_back({(int)k, found});
  }
  for (size_t j = 0; j < Tt.taps.size(); ++j) {
    bool used = false;
    for (auto& pr : tap_pairs) used = used || pr.second == (int)j;
    SHAPECHK(used || Tt.tap_names[j] == "m", "trainer: the student has no '%s' tap", Tt.tap_names[j].c_str());
  }
  SHAPECHK(tap_pairs.size() <= 9, "trainer: %d taps", (int)tap_pairs.size());
  SHAPECHK(ad->B2 == 2 * S.B && ad->L == S.L, "trainer: adapter prepared for %d x %d, need %d x %d", ad->B2, ad->L,
           2 * S.B, S.L);
  const int tok_dim = ad->out1 ? ad->out1 : ad->out_dim;
  SHAPECHK(tok_dim == S.cfg.cross_dim, "trainer: adapter token dim %d != student cross_attention_dim %d", tok_dim,
           S.cfg.cross_dim);
  const size_t n = (size_t)S.B * S.cfg.in_channels * S.H * S.W;
  HIPCHK(hipMalloc((void**)&xt, n * 4));
  HIPCHK(hipMalloc((void**)&eps_s, n * 4));
  HIPCHK(hipMalloc((void**)&eps_t, n * 4));
  HIPCHK(hipMalloc((void**)&deps, n * 4));
  HIPCHK(hipMalloc((void**)&losses, 16));
  {
    std::vector<long long> per;
    for (auto& pr : tap_pairs) per.push_back(S.tn[S.taps[pr.first]].rows / S.B * S.tn[S.taps[pr.first]].cols);
    HIPCHK(hipMalloc((void**)&kd_ws, kd_loss_workspace_bytes((int)per.size(), per.data(), (long long)S.cfg.in_channels * S.H * S.W, S.B)));
  }
  HIPCHK(hipMalloc((void**)&tehs_c, (size_t)Tt.B * Tt.L * Tt.cfg.cross_dim * 2));
  HIPCHK(hipMalloc((void**)&tehs_n, (size_t)Tt.B * Tt.L * Tt.cfg.cross_dim * 2));
  // DDPM alphas_cumprod, scaled_linear betas (train_sdxl_zh.py:140)
  std::vector<float> acv(1000);
  {
    const float b0 = sqrtf(0.00085f), b1 = sqrtf(0.012f);
    float prod = 1.f;
    for (int i = 0; i < 1000; ++i) {
      const float sb = b0 + (b1 - b0) * (float)i / 999.0f;
      prod *= 1.0f - sb * sb;
      acv[i] = prod;
    }
  }
  HIPCHK(hipMalloc((void**)&ac, 4000));
  HIPCHK(hipMemcpy(ac, acv.data(), 4000, hipMemcpyHostToDevice));
  return PEA_OK;
}

// One KD training step on one batch (train_sdxl_zh.py:311-441 after the frozen encoders):
// add_noise -> adapter (cond | uncond) -> CFG-dropout select -> student UNet (taps) -> teacher UNet
// -> fused KD loss + gradient seeds -> student data-gradient pass -> adapter dgrad + wgrad.
int Trainer::step(const float* latents, const float* noise, const long long* timesteps, const float* enc,
                  const float* enc_uncond, const unsigned char* prompt_mask, const long long* zh,
                  const float* teacher_ehs, const float* teacher_neg, const float* teacher_pooled,
                  const float* time_ids, float grad_scale, float* grads, int accumulate, float* losses_out,
                  hipStream_t s) {
  Tape& S = *student;
  Tape& Tt = *teacher;
  Adapter& A = *ad;
  const int B = S.B;
  SHAPECHK(A.B2 == 2 * B && A.L == S.L, "trainer: adapter is prepared for %d x %d rows, the step needs %d x %d", A.B2, A.L,
           2 * B, S.L);
  if (merge_passes && merge_state == 0) {
    // eligible: the teacher context shares the student's weight arena (same checkpoint, train_sdxl_zh.py:138,151 load
    // the same model_path) and both see the same context length
    // (merge_passes 1: for per-GPU batches <= 8 -- end of round 2, one box: 109.2 vs 114.0 ms at B = 4, 203.5 vs 205.2 ms
    // at B = 8 against the two-stream path; 2: always when eligible)
    // A student context shorter than the teacher's (the reference's default: Chinese-CLIP emits 52 tokens,
    // utils/custom_dataset_sdxl.py:352-353, the teacher's CLIP towers 77) merges too: the merged context is Tt.L tokens
    // long, the student rows carry S.L tokens + zero padding and a per-sample key count masks the padding in the
    // cross-attention forward / backward kernels (head_dim 64 instances only).
    bool all_nd1 = true;
    for (const Op& o : S.ops)
      if (o.kind == OP_ATTN && o.p3 != 1) all_nd1 = false;
    bool ok = (merge_passes >= 2 || B <= 8) && !Tt.owns_weights && Tt.slots.size() == S.slots.size() &&
              (S.L == Tt.L || (S.L < Tt.L && all_nd1)) &&
              S.graph == 0 && Tt.graph == 0 &&
              memcmp(&S.cfg, &Tt.cfg, sizeof(PeaUnetCfg)) == 0;
    for (size_t i = 0; ok && i < S.slots.size(); ++i)
      ok = S.slots[i].w == Tt.slots[i].w && S.slots[i].f32 == Tt.slots[i].f32;
    if (ok) {
      if (!merged) RC(new_context(2 * B, &merged));      // (a failure leaves the decision open: the next step tries again)
      const size_t n = (size_t)B * S.cfg.in_channels * S.H * S.W;
      HIPCHK(hipMalloc((void**)&xt2, 2 * n * 4));
      HIPCHK(hipMalloc((void**)&eps2, 2 * n * 4));
      HIPCHK(hipMalloc((void**)&t2, 2 * B * 4));
      HIPCHK(hipMalloc((void**)&tid2, 2 * B * 6 * 4));
    }
    merge_state = ok ? 1 : -1;
  }
  if (merge_passes && merge_state == 1)
    return step_merged(latents, noise, timesteps, enc, enc_uncond, prompt_mask, zh, teacher_ehs, teacher_neg,
                       teacher_pooled, time_ids, grad_scale, grads, accumulate, losses_out, s);
  RC(S.ensure_acts());
  RC(Tt.ensure_acts());
  const long long per_img = (long long)S.cfg.in_channels * S.H * S.W;
  if (!t_f32) HIPCHK(hipMalloc((void**)&t_f32, sizeof(float) * B));
  RC(launch_add_noise(latents, noise, timesteps, ac, xt, B, per_img, s));
  RC(launch_cast_i64_f32(timesteps, t_f32, B, s));
  // The teacher forward (no_grad, :410-415) is independent of the adapter and of the student forward: it runs
  // on a side HIP stream so the two UNet passes fill each other's under-occupied launches.
  hipStream_t ts = s;
  if (two_stream) {
    if (!side) {
      HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(ev_fork, s));
    HIPCHK(hipStreamWaitEvent(side, ev_fork, 0));
    ts = side;
  }
  const long long per_tt = (long long)Tt.L * Tt.cfg.cross_dim;
  RC(launch_cast_f32_bf16(teacher_ehs, tehs_c, B * per_tt, ts));
  RC(launch_cast_f32_bf16(teacher_neg, tehs_n, B * per_tt, ts));
  Tn& tehs = Tt.tn[Tt.t_ehs];
  RC(launch_select_rows(tehs_c, tehs_n, prompt_mask, tehs.d, B, per_tt, ts));                    // :413
  RC(Tt.forward(xt, t_f32, tehs.d, 1, teacher_pooled, 0, time_ids, eps_t, ts));
  if (two_stream) HIPCHK(hipEventRecord(ev_join, side));
  // adapter on (cond | uncond) rows; train_sdxl_zh.py:383-384
  RC(A.forward(enc, enc_uncond, 0, s));
  const long long per_tok = (long long)S.L * S.cfg.cross_dim;
  const bf16* tokens = A.out1 ? A.tok : A.z2;
  Tn& ehs = S.tn[S.t_ehs];
  RC(launch_select_rows(tokens, tokens + B * per_tok, prompt_mask, ehs.d, B, per_tok, s));      // :395
  RC(S.forward(xt, t_f32, ehs.d, 1, S.t_text >= 0 ? (const void*)A.pooled : nullptr, 1, time_ids, eps_s, s));
  if (two_stream) HIPCHK(hipStreamWaitEvent(s, ev_join, 0));
  return loss_and_backward(S, &Tt, eps_s, eps_t, noise, zh, prompt_mask, per_tok, per_tok, nullptr, grad_scale, grads, accumulate,
                           losses_out, s);
}

// fused KD loss + gradient seeds (:399-441), data-gradient pass of S, adapter backward.  S: the tape the student rows ran on
// (the student's own, or a merged-pass context whose first B samples they are); Tt: the teacher's tape, or null when the
// teacher rows are the samples behind the student's in S.  per_stok: tokens x width the adapter emits per sample, per_tok: the
// per-sample stride of S's encoder_hidden_states (longer when a shorter student context is zero padded).
int Trainer::loss_and_backward(Tape& S, const Tape* Tt, const float* eps_student, const float* eps_teacher, const float* noise,
                               const long long* zh, const unsigned char* prompt_mask, long long per_stok, long long per_tok,
                               const int* tmap, float grad_scale, float* grads, int accumulate, float* losses_out, hipStream_t s) {
  Adapter& A = *ad;
  const int B = student->B;
  KdLossP kp;
  memset(&kp, 0, sizeof(kp));
  kp.kd_samples_hint = kd_samples_hint;
  kp.ntaps = (int)tap_pairs.size();
  S.begin_backward();
  for (int k = 0; k < kp.ntaps; ++k) {
    Tn& tp = S.tn[S.taps[tap_pairs[k].first]];
    kp.per[k] = tp.rows / S.B * tp.cols;
    kp.fs[k] = tp.d; kp.dfs[k] = tp.g;
    kp.ft[k] = Tt ? Tt->tn[Tt->taps[tap_pairs[k].second]].d : tp.d + kp.per[k] * B;   // the B student samples come first
    tp.gw = true;
  }
  kp.eps_s = eps_student; kp.eps = noise; kp.eps_t = eps_teacher; kp.deps_s = deps;
  kp.per_eps = (long long)S.cfg.in_channels * S.H * S.W; kp.zh = zh; kp.B = B;
  kp.feat_weight = feat_weight; kp.nan_guard = nan_guard; kp.grad_scale = grad_scale; kp.losses = losses;
  kp.partial = (float*)kd_ws;
  kp.tmap = tmap;
  RC(launch_kd_loss(kp, s));
  if (losses_out) HIPCHK(hipMemcpyAsync(losses_out, losses, 16, hipMemcpyDeviceToDevice, s));
  RC(S.backward(deps, s));
  Tn& ehs = S.tn[S.t_ehs];
  SHAPECHK(ehs.gw, "trainer: no gradient reached encoder_hidden_states");
  // route d(ehs) to the cond / uncond adapter rows; pooled gradient only to the cond half (:384,390)
  bf16* dtokens = A.out1 ? A.dtok : A.dz2;
  RC(launch_select_rows_bwd(ehs.g, prompt_mask, dtokens, dtokens + B * per_stok, B, per_stok, s, per_tok));
  if (A.out1) {
    HIPCHK(hipMemsetAsync(A.dpool, 0, (size_t)A.B2 * A.out_dim * 2, s));
    if (S.t_text >= 0 && S.tn[S.t_text].gw)
      HIPCHK(hipMemcpyAsync(A.dpool, S.tn[S.t_text].g, (size_t)B * A.out_dim * 2, hipMemcpyDeviceToDevice, s));
  }
  return A.backward(grads, accumulate, s);
}

// A merged-pass context: `rows` samples (the B student rows first, teacher rows behind them) on the student's weights, of
// which the backward differentiates the first B.  The context is Tt.L tokens long; with a shorter student context the student
// rows carry S.L tokens + zero padding and a per-sample key count masks the padding in the cross-attention kernels.
int Trainer::new_context(int rows, Tape** out) {
  Tape& S = *student;
  Tape& Tt = *teacher;
  std::unique_ptr<Tape> m(new Tape());
  m->cfg = S.cfg;
  m->time_cond_dim = S.time_cond_dim;     // (never set on a merged context: it contributes nothing)
  m->B = rows; m->H = S.H; m->W = S.W; m->L = Tt.L;
  m->needs_grad = true; m->owns_weights = false; m->bwd_batch = S.B;
  RC(m->build());
  RC(m->share_weights_from(S));
  RC(m->alloc());
  if (S.L != Tt.L) {
    std::vector<int> kl(rows, Tt.L);
    for (int i = 0; i < S.B; ++i) kl[i] = S.L;
    HIPCHK(hipMalloc((void**)&m->cross_kvlen, sizeof(int) * rows));
    HIPCHK(hipMemcpy(m->cross_kvlen, kl.data(), sizeof(int) * rows, hipMemcpyHostToDevice));
    m->tn[m->t_ehs].zero_init = true;     // the padding rows of the student samples stay zero
  }
  *out = m.release();
  return PEA_OK;
}

// merged-pass context for B student rows + nt live teacher rows (nt < B); see Trainer::live_teacher_mask
int Trainer::context_for(int nt, Tape** out) {
  const int B = student->B;
  if (nt >= B) { *out = merged; return PEA_OK; }
  auto it = merged_n.find(nt);
  if (it != merged_n.end()) { *out = it->second; return PEA_OK; }
  Tape* m = nullptr;
  RC(new_context(B + nt, &m));
  m->arena_donor = merged;
  merged_n[nt] = m;
  *out = m;
  return PEA_OK;
}

// The same step with the two UNet forwards merged into one pass over 2B samples (rows [0, B): student conditioning,
// rows [B, 2B): teacher conditioning, same noisy latents and timesteps), possible when the teacher context shares the
// student's weights.  Every GEMM / conv / attention launch then works on twice the rows -- at B = 4 that is the
// difference between one and two 128-row tiles per CU in most launches -- and the backward pass walks the tape on
// the leading B samples only (Tape::bwd_batch).  The teacher half runs without `no_grad` bookkeeping differences:
// nothing in the forward depends on whether a gradient will be taken.
int Trainer::step_merged(const float* latents, const float* noise, const long long* timesteps, const float* enc,
                         const float* enc_uncond, const unsigned char* prompt_mask, const long long* zh,
                         const float* teacher_ehs, const float* teacher_neg, const float* teacher_pooled,
                         const float* time_ids, float grad_scale, float* grads, int accumulate, float* losses_out,
                         hipStream_t s) {
  const int B = student->B;
  // live teacher rows (dead-row elimination, model.h): idx[j] = the sample whose teacher row is merged row B + j
  // (both tables are sized from B: a merged pass may run at any batch, merge_passes = 2 with the SD1.5 micro-batch of 40,
  // train_sd_zh.sh:18; the elimination itself needs the mask's bits, hence B <= 30)
  int nt = 0;
  std::vector<int> idx((size_t)B);
  tmap_h.assign((size_t)B, 0);
  const bool dre = live_teacher_mask >= 0 && B <= 30 && (live_teacher_mask & ((1 << B) - 1)) != ((1 << B) - 1);
  for (int i = 0; i < B; ++i) {
    const bool live = !dre || ((live_teacher_mask >> i) & 1);
    tmap_h[i] = live ? nt : -1;
    if (live) idx[nt++] = i;
  }
  Tape* Mp = merged;
  if (dre) RC(context_for(nt, &Mp));
  Tape& M = *Mp;
  SHAPECHK(M.t_text < 0 || (teacher_pooled != nullptr && time_ids != nullptr),
           "trainer: teacher_pooled / time_ids are required for a text_time UNet (added_cond_kwargs, train_sdxl_zh.py:386-396)");
  RC(M.ensure_acts());
  if (last_ctx != Mp && (dre || last_ctx != nullptr)) {
    // the contexts share one pair of arenas with different layouts: whatever must read as zero is cleared again
    for (Tn& t : M.tn)
      if (t.zero_init) HIPCHK(hipMemsetAsync(t.d, 0, (size_t)t.rows * t.cols * 2, s));
    for (int e : M.ext_res) HIPCHK(hipMemsetAsync(M.tn[e].d, 0, (size_t)M.tn[e].rows * M.tn[e].cols * 2, s));
  }
  last_ctx = Mp;
  Adapter& A = *ad;
  const long long per_img = (long long)M.cfg.in_channels * M.H * M.W;
  RC(launch_add_noise(latents, noise, timesteps, ac, xt2, B, per_img, s));
  RC(launch_cast_i64_f32(timesteps, t2, B, s));
  if (!dre) {
    HIPCHK(hipMemcpyAsync(xt2 + B * per_img, xt2, (size_t)B * per_img * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(t2 + B, t2, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  } else {
    for (int j = 0; j < nt; ++j) {
      HIPCHK(hipMemcpyAsync(xt2 + (B + j) * per_img, xt2 + idx[j] * per_img, (size_t)per_img * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(t2 + B + j, t2 + idx[j], 4, hipMemcpyDeviceToDevice, s));
    }
  }
  if (time_ids) {
    HIPCHK(hipMemcpyAsync(tid2, time_ids, (size_t)B * 6 * 4, hipMemcpyDeviceToDevice, s));
    if (!dre) HIPCHK(hipMemcpyAsync(tid2 + B * 6, time_ids, (size_t)B * 6 * 4, hipMemcpyDeviceToDevice, s));
    else
      for (int j = 0; j < nt; ++j)
        HIPCHK(hipMemcpyAsync(tid2 + (B + j) * 6, time_ids + idx[j] * 6, 6 * 4, hipMemcpyDeviceToDevice, s));
  }
  const long long per_tok = (long long)M.L * M.cfg.cross_dim;               // merged context: the teacher's length
  const long long per_stok = (long long)student->L * M.cfg.cross_dim;       // tokens the adapter emits per sample
  Tn& ehs = M.tn[M.t_ehs];
  // teacher rows: where(prompt_mask, negative, prompt) (:413)
  RC(launch_cast_f32_bf16(teacher_ehs, tehs_c, B * per_tok, s));
  RC(launch_cast_f32_bf16(teacher_neg, tehs_n, B * per_tok, s));
  if (!dre) RC(launch_select_rows(tehs_c, tehs_n, prompt_mask, ehs.d + B * per_tok, B, per_tok, s));
  else {
    // every live row is selected straight into its compacted place behind the student rows (the kernel's pointers are
    // __restrict__: no in-place select)
    for (int j = 0; j < nt; ++j)
      RC(launch_select_rows(tehs_c + idx[j] * per_tok, tehs_n + idx[j] * per_tok, prompt_mask + idx[j], ehs.d + (B + j) * per_tok, 1,
                            per_tok, s));
  }
  // student rows: adapter on (cond | uncond), CFG-dropout select (:383-395); a shorter student context leaves the
  // sample's tail rows at their zero padding (masked by Tape::cross_kvlen)
  RC(A.forward(enc, enc_uncond, 0, s));
  const bf16* tokens = A.out1 ? A.tok : A.z2;
  RC(launch_select_rows(tokens, tokens + B * per_stok, prompt_mask, ehs.d, B, per_stok, s, per_tok));
  const void* text = nullptr;
  if (M.t_text >= 0) {
    Tn& q = M.tn[M.t_text];
    HIPCHK(hipMemcpyAsync(q.d, A.pooled, (size_t)B * q.cols * 2, hipMemcpyDeviceToDevice, s));
    if (!dre) RC(launch_cast_f32_bf16(teacher_pooled, q.d + (long long)B * q.cols, (long long)B * q.cols, s));
    else {
      if (!tpool_c) HIPCHK(hipMalloc((void**)&tpool_c, (size_t)B * q.cols * 2));
      RC(launch_cast_f32_bf16(teacher_pooled, tpool_c, (long long)B * q.cols, s));
      for (int j = 0; j < nt; ++j)
        HIPCHK(hipMemcpyAsync(q.d + (long long)(B + j) * q.cols, tpool_c + (long long)idx[j] * q.cols, (size_t)q.cols * 2,
                              hipMemcpyDeviceToDevice, s));
    }
    text = q.d;
  }
  if (dre) {
    if (!tmap_d) HIPCHK(hipMalloc((void**)&tmap_d, sizeof(int) * 32));
    HIPCHK(hipMemcpyAsync(tmap_d, tmap_h.data(), sizeof(int) * B, hipMemcpyHostToDevice, s));
  }
  RC(M.forward(xt2, t2, ehs.d, 1, text, 1, tid2, eps2, s));
  return loss_and_backward(M, nullptr, eps2, eps2 + B * per_img, noise, zh, prompt_mask, per_stok, per_tok, dre ? tmap_d : nullptr,
                           grad_scale, grads, accumulate, losses_out, s);
}
