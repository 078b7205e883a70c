// C-ABI, model level (include/pea_hip.h): UNet contexts, the PEA adapter, the KD trainer.
#include <string.h>

#include <algorithm>
#include <memory>

#include "../../include/pea_hip.h"
#include "model.h"

#define RCX(x)                        \
  do {                                \
    int rc__ = (x);                   \
    if (rc__ != PEA_OK) return rc__;  \
  } while (0)
#define NOTNULL(p, what)                         \
  do {                                           \
    if (!(p)) {                                  \
      pea_set_error("%s: null handle", what);    \
      return PEA_E_INVALID;                      \
    }                                            \
  } while (0)

static_assert(sizeof(pea_unet_config) == sizeof(PeaUnetCfg), "config struct mismatch");

// shared tail of every pea_*_create: build the graph, plan and allocate the weights
static int finish_create(Tape* u, void** out) {
  int rc = u->build();
  if (rc == PEA_OK) rc = u->alloc();
  if (rc != PEA_OK) {
    delete u;
    return rc;
  }
  *out = u;
  return PEA_OK;
}
static int require_device(const char* what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    pea_set_error("%s: no HIP device (there is no CPU fallback)", what);
    return PEA_E_HIP;
  }
  return PEA_OK;
}

// PEA_UNET_GRAD | PEA_UNET_RESIDUAL_INPUTS | PEA_UNET_INPAINT_INPUTS (Tape::build refuses the combinations it cannot serve)
static void set_flags(Tape& u, int flags) {
  u.needs_grad = (flags & PEA_UNET_GRAD) != 0;
  u.residual_inputs = (flags & PEA_UNET_RESIDUAL_INPUTS) != 0;
  u.inpaint_inputs = (flags & PEA_UNET_INPAINT_INPUTS) != 0;
}

extern "C" {

static int check_cond_dim(const char* what, int time_cond_proj_dim) {
  if (time_cond_proj_dim < 0) {
    pea_set_error("%s: time_cond_proj_dim=%d (0: none)", what, time_cond_proj_dim);
    return PEA_E_INVALID;
  }
  return PEA_OK;
}
int pea_unet_create_cond(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim,
                         int own_weights, void** out) {
  NOTNULL(cfg, "pea_unet_create");
  NOTNULL(out, "pea_unet_create");
  RCX(check_cond_dim("pea_unet_create_cond", time_cond_proj_dim));
  RCX(require_device("pea_unet_create"));
  Tape* u = new Tape();
  memcpy(&u->cfg, cfg, sizeof(PeaUnetCfg));
  u->B = B; u->H = H; u->W = W; u->L = L; set_flags(*u, flags);
  u->time_cond_dim = time_cond_proj_dim;
  u->owns_weights = own_weights != 0;
  return finish_create(u, out);
}
int pea_unet_create(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int own_weights,
                    void** out) {
  return pea_unet_create_cond(cfg, B, H, W, L, flags, 0, own_weights, out);
}
int pea_unet_set_timestep_cond(void* h, const float* cond, void* stream) {
  NOTNULL(h, "pea_unet_set_timestep_cond");
  return ((Tape*)h)->set_timestep_cond(cond, (hipStream_t)stream);
}
int pea_unet_plan(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int* n_ops, int* n_weights,
                  long long* n_params, long long* weight_bytes, long long* act_bytes, long long* grad_bytes) {
  return pea_unet_plan_cond(cfg, B, H, W, L, flags, 0, n_ops, n_weights, n_params, weight_bytes, act_bytes, grad_bytes, nullptr,
                            nullptr);
}
int pea_unet_plan_weight(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim,
                         const char* name, long long* numel, int* kind, int* d0, int* d1) {
  NOTNULL(cfg, "pea_unet_plan_weight");
  NOTNULL(name, "pea_unet_plan_weight");
  RCX(check_cond_dim("pea_unet_plan_weight", time_cond_proj_dim));
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  u.B = B; u.H = H; u.W = W; u.L = L; set_flags(u, flags);
  u.time_cond_dim = time_cond_proj_dim;
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  auto it = u.slot_by_name.find(name);
  if (it == u.slot_by_name.end()) {
    pea_set_error("pea_unet_plan_weight: the graph has no weight '%s'", name);
    return PEA_E_NOTFOUND;
  }
  const WSlot& s = u.slots[it->second];
  if (numel) *numel = s.numel;
  if (kind) *kind = s.kind;
  if (d0) *d0 = s.d0;
  if (d1) *d1 = s.d1;
  return PEA_OK;
}
int pea_unet_plan_cond(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int time_cond_proj_dim, int* n_ops,
                       int* n_weights, long long* n_params, long long* weight_bytes, long long* act_bytes,
                       long long* grad_bytes, int* n_attn, int* n_prescaled) {
  NOTNULL(cfg, "pea_unet_plan");
  RCX(check_cond_dim("pea_unet_plan_cond", time_cond_proj_dim));
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  u.B = B; u.H = H; u.W = W; u.L = L; set_flags(u, flags);
  u.time_cond_dim = time_cond_proj_dim;
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  long long np = 0;
  for (const WSlot& s : u.slots) np += s.numel;
  if (n_ops) *n_ops = (int)u.ops.size();
  if (n_weights) *n_weights = (int)u.slots.size();
  if (n_params) *n_params = np;
  if (weight_bytes) *weight_bytes = (long long)u.wbytes;
  if (act_bytes) *act_bytes = (long long)u.abytes;
  if (grad_bytes) *grad_bytes = (long long)u.gbytes;
  if (n_attn) *n_attn = u.n_attn;
  if (n_prescaled) *n_prescaled = u.n_attn_pre;
  return PEA_OK;
}
/* scratch buffers the same context allocates beside its arenas on first use (host only).  bwd_batch > 0: a merged-pass context
 * that differentiates only its leading bwd_batch samples (Tape::bwd_batch) */
int pea_unet_plan_scratch(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int bwd_batch, long long* scratch_bytes) {
  NOTNULL(cfg, "pea_unet_plan_scratch");
  NOTNULL(scratch_bytes, "pea_unet_plan_scratch");
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  u.B = B; u.H = H; u.W = W; u.L = L; set_flags(u, flags);
  u.bwd_batch = bwd_batch;
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  size_t need[8];
  u.scratch_needs(need);
  long long t = 0;
  for (int i = 0; i < 8; ++i) t += (long long)need[i];
  *scratch_bytes = t;
  return PEA_OK;
}
/* attention ops of a graph and how many of them receive a Q already multiplied by scale * log2(e) by the producing
 * projection's epilogue (Tape::tag_q_prescale); every graph the product builds is expected to have the two equal */
int pea_tape_attention_census(void* h, int* n_attn, int* n_prescaled) {
  NOTNULL(h, "pea_tape_attention_census");
  const Tape* u = (const Tape*)h;
  if (n_attn) *n_attn = u->n_attn;
  if (n_prescaled) *n_prescaled = u->n_attn_pre;
  return PEA_OK;
}
int pea_unet_plan_attention(const pea_unet_config* cfg, int B, int H, int W, int L, int flags, int* n_attn, int* n_prescaled) {
  NOTNULL(cfg, "pea_unet_plan_attention");
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  u.B = B; u.H = H; u.W = W; u.L = L; set_flags(u, flags);
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  if (n_attn) *n_attn = u.n_attn;
  if (n_prescaled) *n_prescaled = u.n_attn_pre;
  return PEA_OK;
}
static int plan_census(Tape& u, int* n_attn, int* n_prescaled) {
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  if (n_attn) *n_attn = u.n_attn;
  if (n_prescaled) *n_prescaled = u.n_attn_pre;
  return PEA_OK;
}
/* graph: 1 VAE encoder, 2 ControlNet, 3 VAE decoder (the values of Tape::graph) */
int pea_graph_plan_attention(int graph, const pea_unet_config* cfg, int B, int H, int W, int L, int* n_attn, int* n_prescaled) {
  NOTNULL(cfg, "pea_graph_plan_attention");
  if (graph < 1 || graph > 3) { pea_set_error("pea_graph_plan_attention: graph %d (1 VAE encoder, 2 ControlNet, 3 VAE decoder)", graph); return PEA_E_INVALID; }
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  u.graph = graph;
  u.B = B; u.H = H; u.W = W; u.L = graph == 2 ? L : 0; u.needs_grad = false; u.owns_weights = true;
  return plan_census(u, n_attn, n_prescaled);
}
int pea_text_plan_attention(const pea_text_config* cfg, int B, int L, int* n_attn, int* n_prescaled) {
  NOTNULL(cfg, "pea_text_plan_attention");
  Tape u;
  memset(&u.cfg, 0, sizeof(PeaUnetCfg));
  memcpy(&u.tcfg, cfg, sizeof(PeaTextCfg));
  u.graph = 4;
  u.B = B; u.H = 1; u.W = L; u.L = L; u.needs_grad = false; u.owns_weights = true;
  return plan_census(u, n_attn, n_prescaled);
}
int pea_controlnet_create(const pea_unet_config* cfg, int B, int H, int W, int L, void** out) {
  NOTNULL(cfg, "pea_controlnet_create");
  NOTNULL(out, "pea_controlnet_create");
  RCX(require_device("pea_controlnet_create"));
  Tape* u = new Tape();
  memcpy(&u->cfg, cfg, sizeof(PeaUnetCfg));
  u->graph = 2;
  u->B = B; u->H = H; u->W = W; u->L = L; u->needs_grad = false; u->owns_weights = true;
  return finish_create(u, out);
}
#define CN_HANDLE(h, what)                                                        \
  NOTNULL(h, what);                                                               \
  Tape* u = (Tape*)h;                                                             \
  if (u->graph != 2) { pea_set_error("%s: not a ControlNet handle", what); return PEA_E_INVALID; }
int pea_controlnet_set_cond(void* h, const float* image, void* stream) {
  CN_HANDLE(h, "pea_controlnet_set_cond");
  NOTNULL(image, "pea_controlnet_set_cond");
  std::string miss;
  if (!u->all_loaded(&miss)) {
    pea_set_error("controlnet: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  u->cond_in = image;
  u->ce_valid = false;
  int rc = u->exec_ops(u->ce_begin, u->ce_end, false, (hipStream_t)stream);
  if (rc != PEA_OK) return rc;
  u->ce_valid = true;
  u->cond_in = nullptr;            // the image is consumed here; the embedding stays valid until the next set_cond
  return PEA_OK;
}
int pea_controlnet_forward(void* h, const float* x, const float* t, const void* ehs, int ehs_dtype, const void* text,
                           int text_dtype, const float* time_ids, void* stream) {
  CN_HANDLE(h, "pea_controlnet_forward");
  if (!u->ce_valid) { pea_set_error("pea_controlnet_forward: call pea_controlnet_set_cond first"); return PEA_E_STATE; }
  return u->forward(x, t, ehs, ehs_dtype, text, text_dtype, time_ids, nullptr, (hipStream_t)stream);
}
int pea_controlnet_num_outputs(void* h) { return h ? (int)((Tape*)h)->cn_out.size() : 0; }
int pea_controlnet_output(void* h, int i, void** ptr, int* C, int* H, int* W) {
  CN_HANDLE(h, "pea_controlnet_output");
  if (i < 0 || i >= (int)u->cn_out.size()) {
    pea_set_error("pea_controlnet_output: index %d out of range (%d outputs)", i, (int)u->cn_out.size());
    return PEA_E_INVALID;
  }
  { int rc = u->ensure_acts(); if (rc != PEA_OK) return rc; }
  const Tn& t = u->tn[u->cn_out[i]];
  if (ptr) *ptr = t.d;
  if (C) *C = t.cols;
  if (H) *H = t.H;
  if (W) *W = t.W;
  return PEA_OK;
}
int pea_controlnet_export_nchw(void* h, int i, float* dst, void* stream) {
  CN_HANDLE(h, "pea_controlnet_export_nchw");
  NOTNULL(dst, "pea_controlnet_export_nchw");
  if (i < 0 || i >= (int)u->cn_out.size()) {
    pea_set_error("pea_controlnet_export_nchw: index %d out of range", i);
    return PEA_E_INVALID;
  }
  const Tn& t = u->tn[u->cn_out[i]];
  return launch_nhwc_to_nchw_f32(t.d, dst, u->B, t.H * t.W, t.cols, (hipStream_t)stream);
}
int pea_vae_encoder_create(const pea_unet_config* cfg, int B, int H, int W, void** out) {
  NOTNULL(cfg, "pea_vae_encoder_create");
  NOTNULL(out, "pea_vae_encoder_create");
  RCX(require_device("pea_vae_encoder_create"));
  Tape* u = new Tape();
  memcpy(&u->cfg, cfg, sizeof(PeaUnetCfg));
  u->graph = 1;
  u->B = B; u->H = H; u->W = W; u->L = 0; u->needs_grad = false; u->owns_weights = true;
  return finish_create(u, out);
}
int pea_vae_latent_shape(void* h, int* C, int* H, int* W) {
  NOTNULL(h, "pea_vae_latent_shape");
  Tape* u = (Tape*)h;
  if (u->graph != 1) { pea_set_error("pea_vae_latent_shape: not a VAE encoder handle"); return PEA_E_INVALID; }
  const Tn& t = u->tn[u->t_out_in];
  if (C) *C = u->cfg.out_channels / 2;
  if (H) *H = t.H;
  if (W) *W = t.W;
  return PEA_OK;
}
int pea_vae_encode(void* h, const float* pixels, const float* noise, float scaling, float* moments, float* latents,
                   void* stream) {
  NOTNULL(h, "pea_vae_encode");
  NOTNULL(pixels, "pea_vae_encode");
  Tape* u = (Tape*)h;
  if (u->graph != 1) { pea_set_error("pea_vae_encode: not a VAE encoder handle"); return PEA_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  { int rc0 = u->ensure_acts(); if (rc0 != PEA_OK) return rc0; }
  int rc = u->forward(pixels, nullptr, nullptr, 0, nullptr, 0, nullptr, u->vae_h, s);
  if (rc != PEA_OK) return rc;
  const Tn& t = u->tn[u->t_out_in];
  return launch_vae_posterior(u->vae_h, u->slots[u->w_quant].f32, u->slots[u->b_quant].f32, noise, moments, latents, u->B,
                              u->cfg.out_channels, (long long)t.H * t.W, scaling, s);
}
int pea_vae_decoder_create(const pea_unet_config* cfg, int B, int H, int W, void** out) {
  NOTNULL(cfg, "pea_vae_decoder_create");
  NOTNULL(out, "pea_vae_decoder_create");
  RCX(require_device("pea_vae_decoder_create"));
  Tape* u = new Tape();
  memcpy(&u->cfg, cfg, sizeof(PeaUnetCfg));
  u->graph = 3;
  u->B = B; u->H = H; u->W = W; u->L = 0; u->needs_grad = false; u->owns_weights = true;
  return finish_create(u, out);
}
int pea_vae_decode(void* h, const float* latents, float inv_scaling, float* image, void* stream) {
  NOTNULL(h, "pea_vae_decode");
  NOTNULL(latents, "pea_vae_decode");
  NOTNULL(image, "pea_vae_decode");
  Tape* u = (Tape*)h;
  if (u->graph != 3) { pea_set_error("pea_vae_decode: not a VAE decoder handle"); return PEA_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  std::string miss;
  if (!u->all_loaded(&miss)) {
    pea_set_error("vae decoder: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  { int rc0 = u->ensure_acts(); if (rc0 != PEA_OK) return rc0; }
  int rc = launch_vae_post_quant(latents, u->slots[u->w_quant].f32, u->slots[u->b_quant].f32, u->vae_h, u->B,
                                 u->cfg.in_channels, (long long)u->H * u->W, inv_scaling, s);
  if (rc != PEA_OK) return rc;
  return u->forward(u->vae_h, nullptr, nullptr, 0, nullptr, 0, nullptr, image, s);
}
static_assert(sizeof(pea_text_config) == sizeof(PeaTextCfg), "text config struct mismatch");
int pea_text_create(const pea_text_config* cfg, int B, int L, void** out) {
  NOTNULL(cfg, "pea_text_create");
  NOTNULL(out, "pea_text_create");
  RCX(require_device("pea_text_create"));
  Tape* u = new Tape();
  memset(&u->cfg, 0, sizeof(PeaUnetCfg));
  memcpy(&u->tcfg, cfg, sizeof(PeaTextCfg));
  u->graph = 4;
  u->B = B; u->H = 1; u->W = L; u->L = L; u->needs_grad = false; u->owns_weights = true;
  return finish_create(u, out);
}
int pea_text_forward(void* h, const long long* ids, int hidden_index, float* hidden_out, float* pooled_out, void* stream) {
  NOTNULL(h, "pea_text_forward");
  NOTNULL(ids, "pea_text_forward");
  Tape* u = (Tape*)h;
  if (u->graph != 4) { pea_set_error("pea_text_forward: not a text-encoder handle"); return PEA_E_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  std::string miss;
  if (!u->all_loaded(&miss)) {
    pea_set_error("text encoder: weight '%s' was never loaded", miss.c_str());
    return PEA_E_STATE;
  }
  { int rc0 = u->ensure_acts(); if (rc0 != PEA_OK) return rc0; }
  u->ids_in = ids;
  if (u->tcfg.flavor >= 1) {
    int rc = launch_kv_len(ids, u->kvlen, u->B, u->L, u->tcfg.eos_id, s);
    if (rc != PEA_OK) return rc;
  }
  if (u->tcfg.flavor == 2) {          // block 0's bucket table -> [heads][L][pitch] additive score bias (cheap; weights may have changed)
    int rc = launch_t5_rel_bias(u->slots[u->w_rel].f32, u->rel_bucket, u->rel_bias, u->tcfg.heads, u->L, ((u->L + 63) >> 6) << 6,
                                u->tcfg.rel_buckets / 2, s);
    if (rc != PEA_OK) return rc;
  }
  int rc = u->exec_ops(0, u->ops.size(), false, s);
  if (rc != PEA_OK) return rc;
  if (hidden_out) {
    const int nh = (int)u->hidden.size();
    int t = u->t_final;
    if (hidden_index != -1) {
      const int k = hidden_index < 0 ? nh + hidden_index : hidden_index;
      if (k < 0 || k >= nh) { pea_set_error("pea_text_forward: hidden_index %d out of range (%d states)", hidden_index, nh); return PEA_E_INVALID; }
      t = u->hidden[k];
    }
    rc = launch_cast_bf16_f32(u->tn[t].d, hidden_out, u->tn[t].rows * u->tn[t].cols, s);
    if (rc != PEA_OK) return rc;
  }
  if (pooled_out) {
    if (u->t_pooled < 0) { pea_set_error("pea_text_forward: this encoder has no pooled output"); return PEA_E_INVALID; }
    const Tn& t = u->tn[u->t_pooled];
    rc = launch_cast_bf16_f32(t.d, pooled_out, t.rows * t.cols, s);
    if (rc != PEA_OK) return rc;
  }
  return PEA_OK;
}
int pea_text_rel_bias(void* h, float* bias_out, void* stream) {
  NOTNULL(h, "pea_text_rel_bias");
  NOTNULL(bias_out, "pea_text_rel_bias");
  Tape* u = (Tape*)h;
  if (u->graph != 4 || u->tcfg.flavor != 2) { pea_set_error("pea_text_rel_bias: not a T5 encoder handle"); return PEA_E_INVALID; }
  if (!u->slots[u->w_rel].loaded) { pea_set_error("pea_text_rel_bias: the bias table was never loaded"); return PEA_E_STATE; }
  hipStream_t s = (hipStream_t)stream;
  { int rc0 = u->ensure_acts(); if (rc0 != PEA_OK) return rc0; }
  const int L = u->L, pitch = ((L + 63) >> 6) << 6;
  int rc = launch_t5_rel_bias(u->slots[u->w_rel].f32, u->rel_bucket, u->rel_bias, u->tcfg.heads, L, pitch, u->tcfg.rel_buckets / 2, s);
  if (rc != PEA_OK) return rc;
  HIPCHK(hipMemcpy2DAsync(bias_out, sizeof(float) * L, u->rel_bias, sizeof(float) * pitch, sizeof(float) * L,
                          (size_t)u->tcfg.heads * L, hipMemcpyDeviceToDevice, s));
  return PEA_OK;
}
int pea_unet_destroy(void* h) {
  delete (Tape*)h;
  return PEA_OK;
}
int pea_unet_num_residuals(void* h) { return h ? (int)((Tape*)h)->ext_res.size() : 0; }
int pea_unet_residual_info(void* h, int i, int* C, int* H, int* W) {
  NOTNULL(h, "pea_unet_residual_info");
  Tape* u = (Tape*)h;
  if (i < 0 || i >= (int)u->ext_res.size()) {
    pea_set_error("pea_unet_residual_info: index %d out of range (%d residual inputs)", i, (int)u->ext_res.size());
    return PEA_E_INVALID;
  }
  const Tn& t = u->tn[u->ext_res[i]];
  if (C) *C = t.cols;
  if (H) *H = t.H;
  if (W) *W = t.W;
  return PEA_OK;
}
int pea_unet_set_residuals(void* h, int n, const void* const* ptrs, int dtype, float scale, void* stream) {
  NOTNULL(h, "pea_unet_set_residuals");
  Tape* u = (Tape*)h;
  if (!u->residual_inputs) {
    pea_set_error("pea_unet_set_residuals: context created without PEA_UNET_RESIDUAL_INPUTS");
    return PEA_E_STATE;
  }
  if (n != (int)u->ext_res.size() || !ptrs) {
    pea_set_error("pea_unet_set_residuals: %d pointers given, the graph has %d residual inputs (mid last)", n,
                  (int)u->ext_res.size());
    return PEA_E_SHAPE;
  }
  { int rc = u->ensure_acts(); if (rc != PEA_OK) return rc; }
  for (int i = 0; i < n; ++i) {
    Tn& t = u->tn[u->ext_res[i]];
    if (!ptrs[i]) {
      HIPCHK(hipMemsetAsync(t.d, 0, (size_t)t.rows * t.cols * 2, (hipStream_t)stream));
      continue;
    }
    int rc = launch_residual_import(ptrs[i], dtype, t.d, u->B, t.cols, (long long)t.H * t.W, scale, (hipStream_t)stream);
    if (rc != PEA_OK) return rc;
  }
  return PEA_OK;
}
int pea_unet_set_inpaint_cond(void* h, const float* mask, const float* masked_latents, int cond_batch, int latent_batch,
                              void* stream) {
  NOTNULL(h, "pea_unet_set_inpaint_cond");
  return ((Tape*)h)->set_inpaint_cond(mask, masked_latents, cond_batch, latent_batch, (hipStream_t)stream);
}
int pea_unet_clear_inpaint_cond(void* h) {
  NOTNULL(h, "pea_unet_clear_inpaint_cond");
  Tape* u = (Tape*)h;
  u->inp_set = false;
  u->inp_cond_b = u->inp_lat_b = 0;
  return PEA_OK;
}
int pea_unet_set_freeu(void* h, float s1, float s2, float b1, float b2, void* stream) {
  NOTNULL(h, "pea_unet_set_freeu");
  return ((Tape*)h)->set_freeu(s1, s2, b1, b2, (hipStream_t)stream);
}
int pea_unet_clear_freeu(void* h) {
  NOTNULL(h, "pea_unet_clear_freeu");
  ((Tape*)h)->fu_on = false;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ image prompt (IP-Adapter)
// what a graph must be to take one; on success *kv_op is the stacked text K|V projection
static int ip_check(const Tape& u, int n_tokens, const Op** kv_op) {
  if (u.graph != 0 || u.t_kvall < 0) { pea_set_error("pea_unet_ip: not a UNet handle (ControlNet graphs get no image prompt)"); return PEA_E_INVALID; }
  if (u.needs_grad) {
    pea_set_error("pea_unet_ip: this context was created with PEA_UNET_GRAD; there is no backward through the image branch");
    return PEA_E_STATE;
  }
  SHAPECHK(n_tokens >= 1 && n_tokens <= 32, "pea_unet_ip: n_tokens=%d (1..32 image tokens)", n_tokens);
  SHAPECHK(u.L <= 128, "pea_unet_ip: context length %d (the decoupled attention takes at most 128 text keys)", u.L);
  *kv_op = nullptr;
  for (const Op& o : u.ops)
    if (o.out == u.t_kvall && o.fused >= 0) *kv_op = &o;
  if (!*kv_op) { pea_set_error("pea_unet_ip: stacked K|V projection not found"); return PEA_E_STATE; }
  for (const WSlot& s : u.slots)
    if (s.fused_parent == (*kv_op)->fused && s.pad_mode) {
      pea_set_error("pea_unet_ip: '%s' has padded heads (head_dim %d); the decoupled attention is built for head_dim 64", s.name.c_str(), s.pad_d);
      return PEA_E_SHAPE;
    }
  return PEA_OK;
}
// K column of every cross-attention layer in the stacked K|V projection `fused` -> the layer's index in the order of
// ip_adapter.layer_keys: every down block, then every up block, then the mid block; inside a group the order of the modules,
// which is the order of the slots
static void xattn_layer_order(const Tape& u, int fused, std::map<int, int>& layer_of_col) {
  for (int group = 0; group < 3; ++group)
    for (const WSlot& s : u.slots) {
      const std::string& n = s.name;
      if (s.fused_parent != fused || s.kind != W_LINEAR || n.size() < 12 || n.compare(n.size() - 12, 12, ".to_k.weight")) continue;
      if ((n.rfind("down_blocks.", 0) == 0 ? 0 : n.rfind("up_blocks.", 0) == 0 ? 1 : 2) != group) continue;
      const int idx = (int)layer_of_col.size();
      layer_of_col[s.row_off] = idx;
    }
}
#define IP_HANDLE(h, what)                                                                     \
  NOTNULL(h, what);                                                                            \
  Tape* u = (Tape*)h;                                                                          \
  if (!u->ip) { pea_set_error("%s: call pea_unet_ip_create first", what); return PEA_E_STATE; }
int pea_unet_ip_plan(const pea_unet_config* cfg, int n_tokens, int* n_layers, int* cols, long long* n_params) {
  NOTNULL(cfg, "pea_unet_ip_plan");
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  // layers, stack width and parameters depend on the config alone: any batch / size / context length plans them.  The context
  // length is therefore NOT validated here (ip_check's L <= 128 cannot fire); pea_unet_ip_create checks the real context
  u.B = 1; u.H = 64; u.W = 64; u.L = 77; u.needs_grad = false;
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  const Op* kv = nullptr;
  RCX(ip_check(u, n_tokens, &kv));
  int members = 0;
  for (const WSlot& s : u.slots) members += s.fused_parent == kv->fused && s.kind == W_LINEAR;
  if (n_layers) *n_layers = members / 2;
  if (cols) *cols = u.kvall_total;
  if (n_params) *n_params = (long long)u.kvall_total * u.cfg.cross_dim;
  return PEA_OK;
}
#define IP_SET(h, set, what)                                                                   \
  IP_HANDLE(h, what);                                                                          \
  SHAPECHK(set >= 0 && set < u->ip->nsets, "%s: set %d of %d", what, set, u->ip->nsets);      \
  Tape::IpSet& e = u->ip->set[set];
int pea_unet_ip_create_sets(void* h, int n_sets, const int* n_tokens) {
  NOTNULL(h, "pea_unet_ip_create_sets");
  NOTNULL(n_tokens, "pea_unet_ip_create_sets");
  Tape* u = (Tape*)h;
  SHAPECHK(n_sets >= 1 && n_sets <= 4, "pea_unet_ip_create_sets: %d adapters (1..4)", n_sets);
  const Op* kv = nullptr;
  int total = 0;
  for (int j = 0; j < n_sets; ++j) {
    RCX(ip_check(*u, n_tokens[j], &kv));
    total += n_tokens[j];
  }
  SHAPECHK(total <= 32, "pea_unet_ip_create_sets: %d image tokens over all adapters (one launch takes at most 32)", total);
  RCX(pea_unet_ip_destroy(h));                       // adapters already loaded: replaced, behind whatever still reads them
  Tape::IpState* ip = new Tape::IpState();
  ip->nsets = n_sets; ip->total = total; ip->cols = u->kvall_total; ip->fused = kv->fused;
  // the file's layer order (ip_adapter.layer_keys): every down block, then every up block, then the mid block; inside a group
  // the order of the modules, which is the order of the slots
  xattn_layer_order(*u, kv->fused, ip->layer_of_col);
  const size_t B = (size_t)u->B, K = (size_t)u->cfg.cross_dim;
  bool ok = hipMalloc((void**)&ip->kv, B * total * ip->cols * 2) == hipSuccess &&
            hipMemset(ip->kv, 0, B * total * ip->cols * 2) == hipSuccess;
  for (int j = 0, off = 0; j < n_sets && ok; off += n_tokens[j++]) {
    Tape::IpSet& e = ip->set[j];
    e.n = n_tokens[j]; e.off = off;
    for (const WSlot& s : u->slots) e.loaded.push_back(!(s.fused_parent == kv->fused && s.kind == W_LINEAR));
    ok = hipMalloc((void**)&e.w, (size_t)ip->cols * K * 2) == hipSuccess && hipMalloc((void**)&e.tok, B * e.n * K * 2) == hipSuccess;
  }
  if (!ok) {
    pea_set_error("pea_unet_ip_create: out of device memory (%zu bytes of weights per adapter)", (size_t)ip->cols * K * 2);
    delete ip;
    return PEA_E_HIP;
  }
  u->ip = ip;
  return PEA_OK;
}
int pea_unet_ip_create(void* h, int n_tokens) { return pea_unet_ip_create_sets(h, 1, &n_tokens); }
int pea_unet_ip_load_weight_set(void* h, int set, const char* key, const float* src, long long numel, void* stream) {
  IP_SET(h, set, "pea_unet_ip_load_weight");
  NOTNULL(key, "pea_unet_ip_load_weight");
  NOTNULL(src, "pea_unet_ip_load_weight");
  std::string name(key);
  const size_t at = name.rfind("_ip.weight");
  int slot = -1;
  if (at != std::string::npos && at + 10 == name.size()) {
    auto it = u->slot_by_name.find(name.substr(0, at) + ".weight");      // to_k_ip -> the text stack's to_k of the same layer
    if (it != u->slot_by_name.end() && u->slots[it->second].fused_parent == u->ip->fused) slot = it->second;
  }
  if (slot < 0) { pea_set_error("pea_unet_ip_load_weight: '%s' is no to_k_ip / to_v_ip weight of this UNet", key); return PEA_E_NOTFOUND; }
  const WSlot& w = u->slots[slot];
  SHAPECHK(numel == w.numel, "pea_unet_ip_load_weight: '%s' has %lld elements, expected %lld ([%d][%d])", key, numel, w.numel, w.d0, w.d1);
  RCX(launch_cast_f32_bf16(src, e.w + (size_t)w.row_off * w.d1, numel, (hipStream_t)stream));
  e.loaded[slot] = 1;
  return PEA_OK;
}
int pea_unet_ip_load_weight(void* h, const char* key, const float* src, long long numel, void* stream) {
  return pea_unet_ip_load_weight_set(h, 0, key, src, numel, stream);
}
int pea_unet_ip_set_tokens_set(void* h, int set, const float* tokens, void* stream) {
  IP_SET(h, set, "pea_unet_ip_set_tokens");
  NOTNULL(tokens, "pea_unet_ip_set_tokens");
  Tape::IpState& ip = *u->ip;
  for (size_t i = 0; i < e.loaded.size(); ++i)
    if (!e.loaded[i]) {
      const std::string& n = u->slots[i].name;
      pea_set_error("pea_unet_ip_set_tokens: '%s_ip.weight' was never loaded", n.substr(0, n.size() - 7).c_str());
      return PEA_E_STATE;
    }
  hipStream_t s = (hipStream_t)stream;
  const int rows = u->B * e.n, K = u->cfg.cross_dim;
  RCX(launch_cast_f32_bf16(tokens, e.tok, (long long)rows * K, s));
  // one adapter: ONE GEMM over all samples.  Several: the set's rows of a sample are not adjacent to those of the next, so one
  // GEMM per sample straight into its rows of the packed buffer (once per image, B is the CFG batch)
  const int launches = ip.nsets == 1 ? 1 : u->B, m = rows / launches;
  for (int b = 0; b < launches; ++b) {
    GemmP p; fill_gemm(p);
    p.A = e.tok + (size_t)b * m * K; p.lda = K; p.M = m; p.K = K; p.N = ip.cols; p.W = e.w; p.ldw = K;
    p.C = ip.kv + ((size_t)b * ip.total + e.off) * ip.cols; p.ldc = ip.cols;
    RCX(launch_gemm(p, s));
  }
  e.live = true;
  return PEA_OK;
}
int pea_unet_ip_set_tokens(void* h, const float* tokens, void* stream) { return pea_unet_ip_set_tokens_set(h, 0, tokens, stream); }
int pea_unet_ip_set_scale_set(void* h, int set, float scale) {
  IP_SET(h, set, "pea_unet_ip_set_scale");
  e.scale = scale;
  return PEA_OK;
}
int pea_unet_ip_set_scale(void* h, float scale) { return pea_unet_ip_set_scale_set(h, 0, scale); }
int pea_unet_ip_set_layer_scales(void* h, int set, const float* scales, int n_layers) {
  IP_SET(h, set, "pea_unet_ip_set_layer_scales");
  if (!scales) {                                     // back to 1 in every layer
    e.layer_scale.clear();
    return PEA_OK;
  }
  const int want = (int)u->ip->layer_of_col.size();
  SHAPECHK(n_layers == want, "pea_unet_ip_set_layer_scales: %d scales, this UNet has %d cross-attention layers", n_layers, want);
  e.layer_scale.assign(scales, scales + n_layers);
  return PEA_OK;
}
static void ip_query_counts(const Tape& u, std::vector<int>& out) {
  for (const Op& o : u.ops)
    if (o.kind == OP_ATTN && o.b == u.t_kvall && std::find(out.begin(), out.end(), o.p1) == out.end()) out.push_back(o.p1);
}
int pea_unet_ip_query_counts(void* h, int* counts, int cap, int* n) {
  NOTNULL(h, "pea_unet_ip_query_counts");
  std::vector<int> c;
  ip_query_counts(*(Tape*)h, c);
  if (n) *n = (int)c.size();
  for (int i = 0; counts && i < cap && i < (int)c.size(); ++i) counts[i] = c[i];
  return PEA_OK;
}
int pea_unet_ip_set_mask(void* h, int set, int Sq, const float* mask, int Bm, void* stream) {
  IP_SET(h, set, "pea_unet_ip_set_mask");
  if (!mask) {                                       // drop the mask of that count, or (Sq == 0) all of them
    HIPCHK(hipDeviceSynchronize());                  // a queued forward may still read them
    for (auto it = e.mask.begin(); it != e.mask.end();)
      if (Sq == 0 || it->first == Sq) { (void)hipFree(it->second.first); it = e.mask.erase(it); } else ++it;
    return PEA_OK;
  }
  std::vector<int> c;
  ip_query_counts(*u, c);
  if (std::find(c.begin(), c.end(), Sq) == c.end()) {
    pea_set_error("pea_unet_ip_set_mask: no cross-attention layer of this context has %d queries (pea_unet_ip_query_counts)", Sq);
    return PEA_E_SHAPE;
  }
  SHAPECHK(Bm == 1 || Bm == u->B, "pea_unet_ip_set_mask: Bm=%d (1, or the context's batch %d)", Bm, u->B);
  auto it = e.mask.find(Sq);
  if (it != e.mask.end() && it->second.second != Bm) {
    HIPCHK(hipDeviceSynchronize());
    (void)hipFree(it->second.first);
    e.mask.erase(it);
    it = e.mask.end();
  }
  if (it == e.mask.end()) {
    float* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, (size_t)Bm * Sq * sizeof(float)));
    it = e.mask.emplace(Sq, std::make_pair(buf, Bm)).first;
  }
  HIPCHK(hipMemcpyAsync(it->second.first, mask, (size_t)Bm * Sq * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PEA_OK;
}
// ------------------------------------------------------------------------------ regional text prompts
int pea_unet_set_prompt_regions(void* h, int R, int Sq, const float* w, int Bw, void* stream) {
  NOTNULL(h, "pea_unet_set_prompt_regions");
  Tape* u = (Tape*)h;
  if (u->graph != 0 || u->t_kvall < 0) { pea_set_error("pea_unet_set_prompt_regions: not a UNet handle (ControlNet graphs keep one prompt)"); return PEA_E_INVALID; }
  if (!w) { pea_set_error("pea_unet_set_prompt_regions: null weights"); return PEA_E_INVALID; }
  RCX(u->regions_check(R, false));
  SHAPECHK(!u->regions || u->regions->R == R, "pea_unet_set_prompt_regions: R=%d, but weights for %d regions are set (pea_unet_clear_prompt_regions)",
           R, u->regions ? u->regions->R : 0);
  std::vector<int> c;
  ip_query_counts(*u, c);
  if (std::find(c.begin(), c.end(), Sq) == c.end()) {
    pea_set_error("pea_unet_set_prompt_regions: no cross-attention layer of this context has %d queries (pea_unet_ip_query_counts)", Sq);
    return PEA_E_SHAPE;
  }
  SHAPECHK(Bw == 1 || Bw == u->B, "pea_unet_set_prompt_regions: Bw=%d (1, or the context's batch %d)", Bw, u->B);
  if (!u->regions) { u->regions = new Tape::RegionState(); u->regions->R = R; }
  auto& tab = u->regions->w;
  auto it = tab.find(Sq);
  if (it != tab.end() && it->second.second != Bw) {
    HIPCHK(hipDeviceSynchronize());                  // a queued forward may still read it
    (void)hipFree(it->second.first);
    tab.erase(it);
    it = tab.end();
  }
  const size_t bytes = (size_t)Bw * R * Sq * sizeof(float);
  if (it == tab.end()) {
    float* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, bytes));
    it = tab.emplace(Sq, std::make_pair(buf, Bw)).first;
  }
  HIPCHK(hipMemcpyAsync(it->second.first, w, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PEA_OK;
}
int pea_unet_clear_prompt_regions(void* h) {
  NOTNULL(h, "pea_unet_clear_prompt_regions");
  Tape* u = (Tape*)h;
  if (u->regions) HIPCHK(hipDeviceSynchronize());    // a queued forward may still read the weights
  delete u->regions;
  u->regions = nullptr;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ prompt-to-prompt editing
int pea_unet_set_prompt_edit(void* h, const int* src, const void* Mt, const float* cd, int T, int self_until, int self_max_tokens,
                             void* stream) {
  NOTNULL(h, "pea_unet_set_prompt_edit");
  Tape* u = (Tape*)h;
  if (u->graph != 0 || u->t_kvall < 0) { pea_set_error("pea_unet_set_prompt_edit: not a UNet handle (graph %d has no text cross-attention to edit)", u->graph); return PEA_E_INVALID; }
  if (!src || !Mt || !cd) { pea_set_error("pea_unet_set_prompt_edit: null src, Mt or cd"); return PEA_E_INVALID; }
  RCX(u->edit_check(false));
  const int B = u->B, L = u->L;
  SHAPECHK(T >= 1 && T <= (1 << 20), "pea_unet_set_prompt_edit: T=%d steps", T);
  SHAPECHK(self_until >= 0 && self_max_tokens >= 0, "pea_unet_set_prompt_edit: self_until=%d, self_max_tokens=%d (>= 0)", self_until, self_max_tokens);
  int n_edited = 0;
  for (int b = 0; b < B; ++b) {
    if (src[b] < 0 || src[b] == b) continue;                       // (its own source: not edited)
    SHAPECHK(src[b] < B, "pea_unet_set_prompt_edit: src[%d]=%d is out of range (batch %d)", b, src[b], B);
    SHAPECHK(src[src[b]] < 0 || src[src[b]] == src[b], "pea_unet_set_prompt_edit: src[%d]=%d names a source that is itself edited", b, src[b]);
    ++n_edited;
  }
  RCX(pea_unet_clear_prompt_edit(h));
  Tape::EditState* e = new Tape::EditState();
  for (int b = 0; b < 32; ++b) e->src[b] = b < B && src[b] != b ? src[b] : -1;
  e->n_edited = n_edited; e->T = T; e->self_until = self_until; e->self_max_tokens = self_max_tokens; e->ldm = (L + 7) / 8 * 8;
  const size_t cd_elems = (size_t)T * 2 * B * L;
  std::vector<float> host(cd_elems);
  hipError_t err = hipMalloc((void**)&e->Mt, (size_t)B * L * e->ldm * sizeof(bf16));
  if (err == hipSuccess) err = hipMalloc((void**)&e->cd, cd_elems * sizeof(float));
  if (err == hipSuccess) err = hipMemsetAsync(e->Mt, 0, (size_t)B * L * e->ldm * sizeof(bf16), (hipStream_t)stream);
  if (err == hipSuccess) err = hipMemcpy2DAsync(e->Mt, (size_t)e->ldm * sizeof(bf16), Mt, (size_t)L * sizeof(bf16), (size_t)L * sizeof(bf16),
                                                (size_t)B * L, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (err == hipSuccess) err = hipMemcpyAsync(e->cd, cd, cd_elems * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (err == hipSuccess) err = hipMemcpyAsync(host.data(), cd, cd_elems * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
  if (err != hipSuccess) {
    pea_set_error("pea_unet_set_prompt_edit: %s", hipGetErrorString(err));
    delete e;
    return PEA_E_HIP;
  }
  e->cd_live.assign(T, 0);
  for (int t = 0; t < T; ++t)
    for (int b = 0; b < B && !e->cd_live[t]; ++b) {
      if (e->src[b] < 0) continue;
      const float* c = host.data() + ((size_t)t * 2 * B + b) * L;
      const float* d = c + (size_t)B * L;
      for (int j = 0; j < L; ++j)
        if (c[j] != 0.f || d[j] != 1.f) { e->cd_live[t] = 1; break; }
    }
  u->edit = e;
  return PEA_OK;
}
int pea_unet_set_prompt_edit_step(void* h, int step) {
  NOTNULL(h, "pea_unet_set_prompt_edit_step");
  Tape* u = (Tape*)h;
  if (!u->edit) { pea_set_error("pea_unet_set_prompt_edit_step: call pea_unet_set_prompt_edit first"); return PEA_E_STATE; }
  u->edit->step = step;                               // (a step outside 0..T-1 is refused by the forward that would use it)
  return PEA_OK;
}
int pea_unet_clear_prompt_edit(void* h) {
  NOTNULL(h, "pea_unet_clear_prompt_edit");
  Tape* u = (Tape*)h;
  if (u->edit) HIPCHK(hipDeviceSynchronize());        // a queued forward may still read the tables
  delete u->edit;
  u->edit = nullptr;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ StyleAligned generation
static int self_attn_layers(const Tape& u, std::map<int, int>* layer_of_op) {
  int n = 0;
  for (size_t i = 0; i < u.ops.size(); ++i)
    if (u.is_self_attn(u.ops[i])) {
      if (layer_of_op) (*layer_of_op)[(int)i] = n;
      ++n;
    }
  return n;
}
int pea_unet_num_self_attention_layers(void* h) {
  NOTNULL(h, "pea_unet_num_self_attention_layers");
  return self_attn_layers(*(Tape*)h, nullptr);
}
int pea_unet_set_style_aligned(void* h, const int* ref, const float* layer_on, int n_layers, int adain_queries, int adain_keys,
                               float shared_score_scale, float shared_score_shift, void* stream) {
  NOTNULL(h, "pea_unet_set_style_aligned");
  Tape* u = (Tape*)h;
  if (u->graph != 0) { pea_set_error("pea_unet_set_style_aligned: not a UNet handle (graph %d)", u->graph); return PEA_E_INVALID; }
  if (!ref) { pea_set_error("pea_unet_set_style_aligned: null ref (a host int[B]; negative entries for plain samples)"); return PEA_E_INVALID; }
  RCX(u->style_check(false));
  const int B = u->B;
  SHAPECHK(shared_score_scale == shared_score_scale && shared_score_shift == shared_score_shift && fabsf(shared_score_scale) <= 3.0e38f &&
               fabsf(shared_score_shift) <= 1.0e30f,
           "pea_unet_set_style_aligned: finite shared_score_scale / shared_score_shift (%g %g)", (double)shared_score_scale, (double)shared_score_shift);
  Tape::StyleState* st = new Tape::StyleState();
  std::unique_ptr<Tape::StyleState> guard(st);
  for (int b = 0; b < 32; ++b) st->ref[b] = -1;
  for (int b = 0; b < B; ++b) {
    if (ref[b] < 0 || ref[b] == b) continue;                       // (its own reference: plain)
    SHAPECHK(ref[b] < B, "pea_unet_set_style_aligned: ref[%d]=%d is out of range (batch %d)", b, ref[b], B);
    SHAPECHK(ref[ref[b]] < 0 || ref[ref[b]] == ref[b], "pea_unet_set_style_aligned: ref[%d]=%d names a reference that is itself a target", b, ref[b]);
    st->ref[b] = ref[b];
    ++st->n_targets;
  }
  const int want = self_attn_layers(*u, &st->layer_of_op);
  if (layer_on && n_layers != want) {
    pea_set_error("pea_unet_set_style_aligned: %d layer switches, this UNet has %d self-attention layers", n_layers, want);
    return PEA_E_SHAPE;
  }
  st->on.assign(want, 1);
  for (int i = 0; layer_on && i < want; ++i) st->on[i] = layer_on[i] != 0.f;
  st->adain_q = adain_queries != 0; st->adain_k = adain_keys != 0;
  st->share_scale = shared_score_scale; st->share_shift = shared_score_shift;
  size_t coef_bytes = 0, scratch_bytes = 0;
  for (const Op& o : u->ops) {
    if (!u->is_self_attn(o)) continue;
    coef_bytes = std::max(coef_bytes, sizeof(float) * (size_t)B * 4 * 64 * o.p0);
    scratch_bytes = std::max(scratch_bytes, attn_adain_scratch_bytes(B, o.p0, o.p1));
  }
  RCX(pea_unet_clear_style_aligned(h));
  if (st->n_targets && coef_bytes) {
    hipError_t err = hipMalloc((void**)&st->coef, coef_bytes);
    if (err == hipSuccess) err = hipMalloc((void**)&st->scratch, std::max(scratch_bytes, (size_t)16));
    if (err != hipSuccess) { pea_set_error("pea_unet_set_style_aligned: %s", hipGetErrorString(err)); return PEA_E_HIP; }
  }
  (void)stream;                                                     // nothing is transferred: ref is a host table
  u->style = guard.release();
  return PEA_OK;
}
int pea_unet_clear_style_aligned(void* h) {
  NOTNULL(h, "pea_unet_clear_style_aligned");
  Tape* u = (Tape*)h;
  if (u->style && u->style->coef) HIPCHK(hipDeviceSynchronize());   // a queued forward may still use the buffers
  delete u->style;
  u->style = nullptr;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ self-attention guidance
int pea_unet_enable_sag(void* h, int layer, int first_sample, int n_samples) {
  NOTNULL(h, "pea_unet_enable_sag");
  Tape* u = (Tape*)h;
  if (u->graph != 0) { pea_set_error("pea_unet_enable_sag: not a UNet handle (graph %d)", u->graph); return PEA_E_INVALID; }
  std::map<int, int> layer_of_op;
  const int want = self_attn_layers(*u, &layer_of_op);
  SHAPECHK(layer >= 0 && layer < want, "pea_unet_enable_sag: layer %d, this UNet has %d self-attention layers", layer, want);
  SHAPECHK(first_sample >= 0 && n_samples >= 1 && first_sample + n_samples <= u->B,
           "pea_unet_enable_sag: samples %d .. %d of a batch of %d", first_sample, first_sample + n_samples - 1, u->B);
  Tape::SagState* st = new Tape::SagState();
  std::unique_ptr<Tape::SagState> guard(st);
  for (const auto& lo : layer_of_op)
    if (lo.second == layer) st->op = lo.first;
  const Op& o = u->ops[st->op];
  const int head_dim = (int)lroundf(1.f / (o.f0 * o.f0));           // (the softmax scale is head_dim^-1/2; padded heads keep their own)
  SHAPECHK(o.p3 == 1 && head_dim == 64, "pea_unet_enable_sag: self-attention layer %d has head_dim %d (stored as %d); the column-sum "
           "kernel is built for 64", layer, head_dim, 64 * o.p3);
  st->layer = layer; st->first = first_sample; st->n = n_samples; st->H = o.p0; st->S = o.p1;
  st->G = attention_colsum_groups(n_samples, o.p0, o.p1, o.p2);
  if (st->G < 1) return PEA_E_SHAPE;
  RCX(pea_unet_disable_sag(h));
  u->sag = st;                                                      // (the checks read the state they judge)
  const int rc = u->sag_check(false);
  u->sag = nullptr;
  if (rc) return rc;
  hipError_t err = hipMalloc((void**)&st->lse, sizeof(float) * (size_t)u->B * o.p0 * o.p1);
  if (err == hipSuccess) err = hipMalloc((void**)&st->part, sizeof(float) * (size_t)n_samples * st->G * o.p2);
  if (err == hipSuccess) err = hipMemset(st->part, 0, sizeof(float) * (size_t)n_samples * st->G * o.p2);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) { pea_set_error("pea_unet_enable_sag: %s", hipGetErrorString(err)); return PEA_E_HIP; }
  u->sag = guard.release();
  return PEA_OK;
}
int pea_unet_disable_sag(void* h) {
  NOTNULL(h, "pea_unet_disable_sag");
  Tape* u = (Tape*)h;
  if (u->sag) HIPCHK(hipDeviceSynchronize());        // a queued forward may still write the buffers
  delete u->sag;
  u->sag = nullptr;
  return PEA_OK;
}
int pea_unet_sag_colsum(void* h, float** part, int* G, int* S) {
  NOTNULL(h, "pea_unet_sag_colsum");
  Tape* u = (Tape*)h;
  if (!u->sag) { pea_set_error("pea_unet_sag_colsum: call pea_unet_enable_sag first"); return PEA_E_STATE; }
  if (part) *part = u->sag->part;
  if (G) *G = u->sag->G;
  if (S) *S = u->sag->S;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ cross-attention heat maps
int pea_unet_enable_attention_maps(void* h, const float* layer_on, int n_layers) {
  NOTNULL(h, "pea_unet_enable_attention_maps");
  Tape* u = (Tape*)h;
  if (u->graph != 0 || u->t_kvall < 0) {
    pea_set_error("pea_unet_enable_attention_maps: not a UNet handle (graph %d has no text cross-attention to map)", u->graph);
    return PEA_E_INVALID;
  }
  if (u->needs_grad) {
    pea_set_error("pea_unet_enable_attention_maps: heat maps are an inference feature; this context was created with PEA_UNET_GRAD");
    return PEA_E_STATE;
  }
  SHAPECHK(u->L >= 1 && u->L <= 128, "pea_unet_enable_attention_maps: context length %d (the maps kernel takes 1..128 keys)", u->L);
  const Op* kv = nullptr;
  for (const Op& o : u->ops)
    if (o.out == u->t_kvall && o.fused >= 0) kv = &o;
  if (!kv) { pea_set_error("pea_unet_enable_attention_maps: stacked K|V projection not found"); return PEA_E_STATE; }
  for (const WSlot& s : u->slots)
    SHAPECHK(!(s.fused_parent == kv->fused && s.pad_mode), "pea_unet_enable_attention_maps: '%s' has padded heads (head_dim %d); the maps "
             "kernel is built for head_dim 64", s.name.c_str(), s.pad_d);
  for (const Op& o : u->ops)
    if (o.kind == OP_ATTN && o.b == u->t_kvall)
      SHAPECHK(o.p3 == 1 && o.p2 == u->L, "pea_unet_enable_attention_maps: head_dim 64 cross-attention over the whole context (nd=%d, %d keys)", o.p3, o.p2);
  Tape::MapState* m = new Tape::MapState();
  xattn_layer_order(*u, kv->fused, m->layer_of_col);
  const int want = (int)m->layer_of_col.size();
  if (layer_on && n_layers != want) {
    delete m;
    pea_set_error("pea_unet_enable_attention_maps: %d layer switches, this UNet has %d cross-attention layers", n_layers, want);
    return PEA_E_SHAPE;
  }
  m->on.assign(want, 1);
  for (int i = 0; layer_on && i < want; ++i) m->on[i] = layer_on[i] != 0.f;
  int rc = pea_unet_disable_attention_maps(h);        // accumulators already there: replaced, behind whatever still adds to them
  std::vector<int> c;
  ip_query_counts(*u, c);
  for (size_t i = 0; i < c.size() && rc == PEA_OK; ++i) {
    const size_t bytes = (size_t)u->B * u->L * c[i] * sizeof(float);
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, bytes) != hipSuccess || (m->acc[c[i]] = buf, hipMemset(buf, 0, bytes)) != hipSuccess) {
      pea_set_error("pea_unet_enable_attention_maps: out of device memory (%zu bytes for the %d-query level)", bytes, c[i]);
      rc = PEA_E_HIP;
    }
    m->count[c[i]] = 0;
  }
  if (rc == PEA_OK && hipDeviceSynchronize() != hipSuccess) {  // the zeros are there before a forward on any stream adds to them
    pea_set_error("pea_unet_enable_attention_maps: device synchronisation failed");
    rc = PEA_E_HIP;
  }
  if (rc != PEA_OK) { delete m; return rc; }
  u->maps = m;
  return PEA_OK;
}
int pea_unet_reset_attention_maps(void* h, void* stream) {
  NOTNULL(h, "pea_unet_reset_attention_maps");
  Tape* u = (Tape*)h;
  if (!u->maps) { pea_set_error("pea_unet_reset_attention_maps: call pea_unet_enable_attention_maps first"); return PEA_E_STATE; }
  for (auto& a : u->maps->acc) {
    HIPCHK(hipMemsetAsync(a.second, 0, (size_t)u->B * u->L * a.first * sizeof(float), (hipStream_t)stream));
    u->maps->count[a.first] = 0;
  }
  return PEA_OK;
}
int pea_unet_disable_attention_maps(void* h) {
  NOTNULL(h, "pea_unet_disable_attention_maps");
  Tape* u = (Tape*)h;
  if (u->maps) HIPCHK(hipDeviceSynchronize());       // a queued forward may still add to the accumulators
  delete u->maps;
  u->maps = nullptr;
  return PEA_OK;
}
int pea_unet_attention_maps(void* h, int Sq, float** maps, long long* n_accumulated) {
  NOTNULL(h, "pea_unet_attention_maps");
  Tape* u = (Tape*)h;
  if (!u->maps) { pea_set_error("pea_unet_attention_maps: call pea_unet_enable_attention_maps first"); return PEA_E_STATE; }
  const auto it = u->maps->acc.find(Sq);
  if (it == u->maps->acc.end()) {
    pea_set_error("pea_unet_attention_maps: no cross-attention layer of this context has %d queries (pea_unet_ip_query_counts)", Sq);
    return PEA_E_SHAPE;
  }
  if (maps) *maps = it->second;
  if (n_accumulated) *n_accumulated = u->maps->count[Sq];
  return PEA_OK;
}
int pea_unet_ip_clear_set(void* h, int set) {
  IP_SET(h, set, "pea_unet_ip_clear");
  e.live = false;
  return PEA_OK;
}
int pea_unet_ip_clear(void* h) {
  NOTNULL(h, "pea_unet_ip_clear");
  if (((Tape*)h)->ip)
    for (Tape::IpSet& e : ((Tape*)h)->ip->set) e.live = false;
  return PEA_OK;
}
int pea_unet_ip_destroy(void* h) {
  NOTNULL(h, "pea_unet_ip_destroy");
  Tape* u = (Tape*)h;
  if (u->ip) HIPCHK(hipDeviceSynchronize());       // a queued forward may still read the buffers
  delete u->ip;
  u->ip = nullptr;
  return PEA_OK;
}
int pea_unet_ip_export_kv(void* h, float* out, long long* rows, int* cols, void* stream) {
  IP_HANDLE(h, "pea_unet_ip_export_kv");
  const long long r = (long long)u->B * u->ip->total;
  if (rows) *rows = r;
  if (cols) *cols = u->ip->cols;
  if (!out) return PEA_OK;
  bool live = false;
  for (const Tape::IpSet& e : u->ip->set) live = live || e.live;
  if (!live) { pea_set_error("pea_unet_ip_export_kv: no tokens set"); return PEA_E_STATE; }
  return launch_cast_bf16_f32(u->ip->kv, out, r * u->ip->cols, (hipStream_t)stream);
}
int pea_unet_num_weights(void* h) { return h ? (int)((Tape*)h)->slots.size() : 0; }
int pea_unet_weight_info(void* h, int i, char* name, int name_len, long long* numel, int* kind, int* d0, int* d1) {
  NOTNULL(h, "pea_unet_weight_info");
  Tape* u = (Tape*)h;
  if (i < 0 || i >= (int)u->slots.size()) {
    pea_set_error("pea_unet_weight_info: index %d out of range", i);
    return PEA_E_INVALID;
  }
  const WSlot& s = u->slots[i];
  if (name && name_len > 0) {
    strncpy(name, s.name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (numel) *numel = s.numel;
  if (kind) *kind = s.kind;
  if (d0) *d0 = s.d0;
  if (d1) *d1 = s.d1;
  return PEA_OK;
}
int pea_unet_load_weight(void* h, const char* name, const float* src, long long numel, void* stream) {
  NOTNULL(h, "pea_unet_load_weight");
  Tape* u = (Tape*)h;
  if (!u->owns_weights) {
    pea_set_error("pea_unet_load_weight: context borrows its weights");
    return PEA_E_STATE;
  }
  return u->load_weight(name, src, numel, (hipStream_t)stream);
}
int pea_unet_load_weight_lora(void* h, const char* name, const float* base, long long numel, int n_adapters,
                              const float* const* downs, const float* const* ups, const int* ranks, const float* scales,
                              void* stream) {
  /* argument errors first: they need neither a context nor a device */
  if (n_adapters < 1 || !downs || !ups || !ranks || !scales || !name || !base) {
    pea_set_error("pea_unet_load_weight_lora: n_adapters=%d, null name / base / factor arrays", n_adapters);
    return PEA_E_INVALID;
  }
  for (int i = 0; i < n_adapters; ++i) {
    if (ranks[i] < 1 || ranks[i] > 256) {
      pea_set_error("pea_unet_load_weight_lora: adapter %d has rank=%d (1..256)", i, ranks[i]);
      return PEA_E_SHAPE;
    }
    if (!downs[i] || !ups[i]) {
      pea_set_error("pea_unet_load_weight_lora: adapter %d has a null factor", i);
      return PEA_E_INVALID;
    }
  }
  NOTNULL(h, "pea_unet_load_weight_lora");
  return ((Tape*)h)->load_weight_lora(name, base, numel, n_adapters, downs, ups, ranks, scales, (hipStream_t)stream);
}
int pea_unet_init_random(void* h, unsigned long long seed, void* stream) {
  NOTNULL(h, "pea_unet_init_random");
  return ((Tape*)h)->init_random(seed, (hipStream_t)stream);
}
int pea_unet_share_weights(void* dst, void* src) {
  NOTNULL(dst, "pea_unet_share_weights");
  NOTNULL(src, "pea_unet_share_weights");
  return ((Tape*)dst)->share_weights_from(*(Tape*)src);
}
int pea_unet_forward(void* h, const float* x, const float* t, const void* ehs, int ehs_dtype, const void* text,
                     int text_dtype, const float* time_ids, float* eps_out, void* stream) {
  NOTNULL(h, "pea_unet_forward");
  return ((Tape*)h)->forward(x, t, ehs, ehs_dtype, text, text_dtype, time_ids, eps_out, (hipStream_t)stream);
}
int pea_unet_num_taps(void* h) { return h ? (int)((Tape*)h)->taps.size() : 0; }
int pea_unet_tap_name(void* h, int k, char* name, int name_len) {
  NOTNULL(h, "pea_unet_tap_name");
  NOTNULL(name, "pea_unet_tap_name");
  Tape* u = (Tape*)h;
  if (k < 0 || k >= (int)u->taps.size() || name_len < 2) {
    pea_set_error("pea_unet_tap_name: tap %d out of range", k);
    return PEA_E_INVALID;
  }
  snprintf(name, name_len, "%s", k < (int)u->tap_names.size() ? u->tap_names[k].c_str() : "");
  return PEA_OK;
}
int pea_unet_tap_info(void* h, int k, void** data, void** grad, int* B, int* H, int* W, int* C) {
  NOTNULL(h, "pea_unet_tap_info");
  Tape* u = (Tape*)h;
  if (k < 0 || k >= (int)u->taps.size()) {
    pea_set_error("pea_unet_tap_info: tap %d out of range", k);
    return PEA_E_INVALID;
  }
  { int rc = u->ensure_acts(); if (rc != PEA_OK) return rc; }
  const Tn& t = u->tn[u->taps[k]];
  // raw pointers of a depth-to-space tap: B / H / W / C do not reveal the storage order, so a caller that has never asked
  // for the layout would read (and seed) permuted pixels without any error -- refuse until it has
  if ((data || grad) && t.d2s && !u->tap_layout_queried) {
    pea_set_error("pea_unet_tap_info: tap %d is stored depth-to-space ([B][H/2][W/2][(y&1)*2+(x&1)][C]); call "
                  "pea_unet_tap_layout first (or use pea_unet_tap_export_nchw / pea_unet_tap_import_grad_nchw)", k);
    return PEA_E_STATE;
  }
  if (data) *data = t.d;
  if (grad) *grad = t.g;
  if (B) *B = t.B;
  if (H) *H = t.H;
  if (W) *W = t.W;
  if (C) *C = t.cols;
  return PEA_OK;
}
int pea_unet_tap_export_nchw(void* h, int k, int grad, float* out, void* stream) {
  NOTNULL(h, "pea_unet_tap_export_nchw");
  Tape* u = (Tape*)h;
  if (k < 0 || k >= (int)u->taps.size()) {
    pea_set_error("pea_unet_tap_export_nchw: tap %d out of range", k);
    return PEA_E_INVALID;
  }
  { int rc = u->ensure_acts(); if (rc != PEA_OK) return rc; }
  const Tn& t = u->tn[u->taps[k]];
  const bf16* src = grad ? t.g : t.d;
  NOTNULL(src, "pea_unet_tap_export_nchw(grad)");
  const int nb = (grad && u->bwd_batch > 0) ? u->bwd_batch : t.B;    // gradients exist for the differentiated samples only
  return launch_nhwc_to_nchw_f32(src, out, nb, t.H * t.W, t.cols, (hipStream_t)stream, t.d2s ? t.H : 0, t.d2s ? t.W : 0);
}
int pea_unet_tap_layout(void* h, int k) {
  Tape* u = (Tape*)h;
  if (!u || k < 0 || k >= (int)u->taps.size()) return -1;
  u->tap_layout_queried = true;
  return u->tn[u->taps[k]].d2s ? 1 : 0;
}
int pea_unet_tap_import_grad_nchw(void* h, int k, const float* src, void* stream) {
  NOTNULL(h, "pea_unet_tap_import_grad_nchw");
  NOTNULL(src, "pea_unet_tap_import_grad_nchw");
  Tape* u = (Tape*)h;
  if (k < 0 || k >= (int)u->taps.size()) {
    pea_set_error("pea_unet_tap_import_grad_nchw: tap %d out of range", k);
    return PEA_E_INVALID;
  }
  { int rc = u->ensure_acts(); if (rc != PEA_OK) return rc; }
  const Tn& t = u->tn[u->taps[k]];
  NOTNULL(t.g, "pea_unet_tap_import_grad_nchw(no gradient buffer)");
  const int nb = u->bwd_batch > 0 ? u->bwd_batch : t.B;
  return launch_nchw_f32_to_nhwc(src, t.g, nb, t.H * t.W, t.cols, (hipStream_t)stream, t.d2s ? t.H : 0, t.d2s ? t.W : 0);
}
int pea_unet_backward(void* h, const float* deps, unsigned tap_seed_mask, void* stream) {
  NOTNULL(h, "pea_unet_backward");
  Tape* u = (Tape*)h;
  u->begin_backward();
  for (size_t k = 0; k < u->taps.size(); ++k)
    if (tap_seed_mask & (1u << k)) u->tn[u->taps[k]].gw = true;
  return u->backward(deps, (hipStream_t)stream);
}
int pea_unet_input_grads(void* h, void** d_ehs, void** d_text) {
  NOTNULL(h, "pea_unet_input_grads");
  Tape* u = (Tape*)h;
  if (d_ehs) *d_ehs = u->tn[u->t_ehs].gw ? u->tn[u->t_ehs].g : nullptr;
  if (d_text) *d_text = (u->t_text >= 0 && u->tn[u->t_text].gw) ? u->tn[u->t_text].g : nullptr;
  return PEA_OK;
}
/* Parity instrumentation: the gradients of the two STACKED projections after the last backward pass, per layer.
 * which 0: every cross-attention K|V projection (ONE GEMM over encoder_hidden_states): d(K|V) as fp32 [rows][cols], rows =
 * differentiated samples x context length; which 1: every ResnetBlock2D.time_emb_proj (ONE GEMM over silu(emb)): the fp32
 * per-sample column sums [differentiated samples][cols].  out may be NULL (sizes only).  pea_unet_stacked_layout names the
 * column block of member i (diffusers weight key, e.g. `...attn2.to_k.weight`), PEA_E_NOTFOUND behind the last member. */
static int stacked_op(Tape* u, int which, const Op** op) {
  const int t = which == 0 ? u->t_kvall : u->t_tproj;
  if (t < 0) { pea_set_error("pea_unet_stacked_*: this graph has no such projection"); return PEA_E_INVALID; }
  for (const Op& o : u->ops)
    if (o.out == t && o.fused >= 0) { *op = &o; return PEA_OK; }
  pea_set_error("pea_unet_stacked_*: producer not found");
  return PEA_E_STATE;
}
int pea_unet_stacked_grad(void* h, int which, float* out, long long* rows, int* cols, void* stream) {
  NOTNULL(h, "pea_unet_stacked_grad");
  Tape* u = (Tape*)h;
  if (which != 0 && which != 1) { pea_set_error("pea_unet_stacked_grad: which=%d", which); return PEA_E_INVALID; }
  const Op* op = nullptr;
  { int rc = stacked_op(u, which, &op); if (rc != PEA_OK) return rc; }
  const Tn& t = u->tn[op->out];
  const int Bb = u->bwd_batch > 0 ? u->bwd_batch : u->B;
  const long long r = t.rows / u->B * Bb;
  if (rows) *rows = r;
  if (cols) *cols = t.cols;
  if (!out) return PEA_OK;
  if (which == 1 && !t.rg) {           /* e.g. SD1.5: no text_time conditioning, the adapter's outputs never reach the time embedding */
    pea_set_error("pea_unet_stacked_grad: the time embedding receives no gradient on this graph");
    return PEA_E_NOTFOUND;
  }
  if (!u->needs_grad || !t.g || !u->tproj_grad) { pea_set_error("pea_unet_stacked_grad: no backward pass has run on this context"); return PEA_E_STATE; }
  if (which == 0) return launch_cast_bf16_f32(t.g, out, r * t.cols, (hipStream_t)stream);
  HIPCHK(hipMemcpyAsync(out, u->tproj_grad, sizeof(float) * (size_t)r * t.cols, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PEA_OK;
}
int pea_unet_stacked_layout(void* h, int which, int i, char* name, int name_len, int* col_off, int* cols) {
  NOTNULL(h, "pea_unet_stacked_layout");
  Tape* u = (Tape*)h;
  const Op* op = nullptr;
  { int rc = stacked_op(u, which, &op); if (rc != PEA_OK) return rc; }
  int k = 0;
  for (const WSlot& s : u->slots) {
    if (s.fused_parent != op->fused || s.kind != W_LINEAR) continue;
    if (k++ != i) continue;
    if (name && name_len > 1) snprintf(name, name_len, "%s", s.name.c_str());
    if (col_off) *col_off = s.row_off;
    if (cols) *cols = s.st_n ? s.st_n : s.d0;
    return PEA_OK;
  }
  return PEA_E_NOTFOUND;
}
int pea_unet_memory(void* h, long long* weight_bytes, long long* act_bytes, long long* grad_bytes, int* n_ops) {
  NOTNULL(h, "pea_unet_memory");
  Tape* u = (Tape*)h;
  if (weight_bytes) *weight_bytes = (long long)u->wbytes;
  /* activations / gradients are allocated on first use: report what is resident */
  if (act_bytes) *act_bytes = u->aarena ? (long long)u->abytes : 0;
  if (grad_bytes) *grad_bytes = u->garena ? (long long)u->gbytes : 0;
  if (n_ops) *n_ops = (int)u->ops.size();
  return PEA_OK;
}

int pea_unet_release_activations(void* h) {
  NOTNULL(h, "pea_unet_release_activations");
  return ((Tape*)h)->release_acts();
}

// ------------------------------------------------------------------------------ adapter
int pea_adapter_create(int in_dim, int out_dim, int hidden_dim, int out_dim1, int use_residual, void** out) {
  NOTNULL(out, "pea_adapter_create");
  Adapter* a = new Adapter();
  a->in_dim = in_dim; a->out_dim = out_dim; a->hidden = hidden_dim; a->out1 = out_dim1; a->use_residual = use_residual;
  a->nparam = 2LL * in_dim + (long long)hidden_dim * in_dim + (long long)hidden_dim * hidden_dim +
              (long long)out_dim * hidden_dim + (long long)out_dim1 * out_dim + out_dim1;
  *out = a;
  return PEA_OK;
}
int pea_adapter_destroy(void* h) {
  delete (Adapter*)h;
  return PEA_OK;
}
long long pea_adapter_num_params(void* h) { return h ? ((Adapter*)h)->nparam : 0; }
int pea_adapter_bind(void* h, float* flat_params) {
  NOTNULL(h, "pea_adapter_bind");
  ((Adapter*)h)->params = flat_params;
  return PEA_OK;
}
int pea_adapter_prepare(void* h, int batch, int L) {
  NOTNULL(h, "pea_adapter_prepare");
  RCX(require_device("pea_adapter_prepare"));
  return ((Adapter*)h)->prepare(batch, L);
}
int pea_adapter_sync(void* h, void* stream) {
  NOTNULL(h, "pea_adapter_sync");
  return ((Adapter*)h)->sync_weights((hipStream_t)stream);
}
int pea_adapter_forward(void* h, const void* enc, int dtype, float* pooled, float* tokens, void* stream) {
  NOTNULL(h, "pea_adapter_forward");
  Adapter* a = (Adapter*)h;
  hipStream_t s = (hipStream_t)stream;
  RCX(a->forward(enc, nullptr, dtype, s));
  if (a->out1) {
    if (pooled) RCX(launch_cast_bf16_f32(a->pooled, pooled, (long long)a->B2 * a->out_dim, s));
    if (tokens) RCX(launch_cast_bf16_f32(a->tok, tokens, (long long)a->R * a->out1, s));
  } else if (tokens) {
    RCX(launch_cast_bf16_f32(a->z2, tokens, (long long)a->R * a->out_dim, s));
  }
  return PEA_OK;
}
int pea_adapter_backward(void* h, const float* d_pooled, const float* d_tokens, float* grads, int accumulate,
                         void* stream) {
  NOTNULL(h, "pea_adapter_backward");
  Adapter* a = (Adapter*)h;
  hipStream_t s = (hipStream_t)stream;
  if (a->out1) {
    if (d_tokens) RCX(launch_cast_f32_bf16(d_tokens, a->dtok, (long long)a->R * a->out1, s));
    else HIPCHK(hipMemsetAsync(a->dtok, 0, (size_t)a->R * a->out1 * 2, s));
    if (d_pooled) RCX(launch_cast_f32_bf16(d_pooled, a->dpool, (long long)a->B2 * a->out_dim, s));
    else HIPCHK(hipMemsetAsync(a->dpool, 0, (size_t)a->B2 * a->out_dim * 2, s));
  } else {
    NOTNULL(d_tokens, "pea_adapter_backward(d_tokens)");
    RCX(launch_cast_f32_bf16(d_tokens, a->dz2, (long long)a->R * a->out_dim, s));
  }
  return a->backward(grads, accumulate, s);
}

// ------------------------------------------------------------------------------ trainer
int pea_trainer_create(void* adapter, void* student, void* teacher, float feat_weight, int nan_guard,
                       const float* alphas_cumprod, void** out) {
  NOTNULL(adapter, "pea_trainer_create");
  NOTNULL(student, "pea_trainer_create");
  NOTNULL(teacher, "pea_trainer_create");
  Trainer* t = new Trainer();
  t->ad = (Adapter*)adapter; t->student = (Tape*)student; t->teacher = (Tape*)teacher;
  t->feat_weight = feat_weight; t->nan_guard = nan_guard;
  int rc = t->prepare();
  if (rc == PEA_OK && alphas_cumprod)
    if (hipMemcpy(t->ac, alphas_cumprod, 4000, hipMemcpyDeviceToDevice) != hipSuccess) rc = PEA_E_HIP;
  if (rc != PEA_OK) {
    delete t;
    return rc;
  }
  *out = t;
  return PEA_OK;
}
int pea_trainer_destroy(void* h) {
  delete (Trainer*)h;
  return PEA_OK;
}
int pea_train_step(void* h, const float* latents, const float* noise, const long long* timesteps, const float* enc,
                   const float* enc_uncond, const unsigned char* prompt_mask, const long long* zh_or_not,
                   const float* teacher_ehs, const float* teacher_neg, const float* teacher_pooled,
                   const float* time_ids, float grad_scale, float* grads, int accumulate, float* losses,
                   void* stream) {
  NOTNULL(h, "pea_train_step");
  return ((Trainer*)h)->step(latents, noise, timesteps, enc, enc_uncond, prompt_mask, zh_or_not, teacher_ehs,
                             teacher_neg, teacher_pooled, time_ids, grad_scale, grads, accumulate, losses,
                             (hipStream_t)stream);
}
int pea_trainer_set_option(void* h, const char* name, int value) {
  NOTNULL(h, "pea_trainer_set_option");
  Trainer* t = (Trainer*)h;
  if (!strcmp(name, "two_stream")) t->two_stream = value;
  else if (!strcmp(name, "merge_passes")) t->merge_passes = value;
  else if (!strcmp(name, "nan_guard")) t->nan_guard = value;
  else if (!strcmp(name, "live_teacher_mask")) t->live_teacher_mask = value;   /* dead-row elimination: bit i = compute sample i's teacher row; -1 = all */
  else if (!strcmp(name, "kd_samples_hint")) t->kd_samples_hint = value;    /* profiling only: samples with zh_or_not == 0 */
  else {
    pea_set_error("pea_trainer_set_option: unknown option '%s'", name);
    return PEA_E_INVALID;
  }
  return PEA_OK;
}
int pea_trainer_release_activations(void* h) {
  NOTNULL(h, "pea_trainer_release_activations");
  Trainer* t = (Trainer*)h;
  RCX(t->student->release_acts());
  RCX(t->teacher->release_acts());
  for (auto& kv : t->merged_n) RCX(kv.second->release_acts());     /* borrowers first */
  if (t->merged) RCX(t->merged->release_acts());
  t->last_ctx = nullptr;
  return PEA_OK;
}
int pea_trainer_get_option(void* h, const char* name) {
  if (!h || !name) return PEA_E_INVALID;
  Trainer* t = (Trainer*)h;
  if (!strcmp(name, "two_stream")) return t->two_stream;
  if (!strcmp(name, "merge_passes")) return t->merge_passes;
  if (!strcmp(name, "merge_state")) return t->merge_state;     /* 0 undecided, 1 merged, -1 not eligible */
  if (!strcmp(name, "nan_guard")) return t->nan_guard;
  if (!strcmp(name, "kd_samples_hint")) return t->kd_samples_hint;
  if (!strcmp(name, "live_teacher_mask")) return t->live_teacher_mask;
  if (!strcmp(name, "merged_rows")) return t->last_ctx ? t->last_ctx->B : (t->merged ? t->merged->B : 0);   /* samples in the last merged pass */
  if (!strcmp(name, "merged_mib"))                                /* activations + gradients of the merged-pass context */
  {
    if (!t->merged || !t->merged->aarena) return 0;
    size_t by = t->merged->abytes + t->merged->gbytes + t->merged->scratch_own_bytes();
    for (auto& kv : t->merged_n)                                  /* dead-row contexts: arenas and most scratch are borrowed */
      if (kv.second->aarena) by += kv.second->scratch_own_bytes();
    return (int)(by >> 20);
  }
  return PEA_E_INVALID;
}
/* the UNet context whose backward pass ran in the last step: the merged-pass context (teacher == student checkpoint), else the
 * student's own (parity instrumentation: pea_unet_stacked_grad) */
int pea_trainer_backward_context(void* h, void** unet) {
  NOTNULL(h, "pea_trainer_backward_context");
  NOTNULL(unet, "pea_trainer_backward_context");
  Trainer* t = (Trainer*)h;
  const bool mg = t->merge_passes && t->merge_state == 1;
  *unet = mg ? (void*)(t->last_ctx ? t->last_ctx : t->merged) : (void*)t->student;
  return PEA_OK;
}
int pea_trainer_export(void* h, int which, float* out, void* stream) {
  NOTNULL(h, "pea_trainer_export");
  Trainer* t = (Trainer*)h;
  const size_t n = (size_t)t->student->B * t->student->cfg.in_channels * t->student->H * t->student->W;
  const bool mg = t->merge_passes && t->merge_state == 1;
  const float* src = mg ? (which == 0 ? t->xt2 : which == 1 ? t->eps2 : t->eps2 + n)
                        : (which == 0 ? t->xt : which == 1 ? t->eps_s : t->eps_t);
  const int B = t->student->B;
  if (mg && which == 2 && t->last_ctx && t->last_ctx->B != 2 * B) {
    /* dead-row elimination: the teacher rows are compacted; rows that were not computed come back as NaN */
    const size_t per = n / B;
    HIPCHK(hipMemsetAsync(out, 0xff, n * 4, (hipStream_t)stream));
    for (int i = 0; i < B; ++i)
      if (i < (int)t->tmap_h.size() && t->tmap_h[i] >= 0)
        HIPCHK(hipMemcpyAsync(out + i * per, src + (size_t)t->tmap_h[i] * per, per * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PEA_OK;
  }
  HIPCHK(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PEA_OK;
}

}  // extern "C"
