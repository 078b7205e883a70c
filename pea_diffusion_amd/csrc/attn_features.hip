// The inference features that hang off the UNet's attention ops -- image prompts (IP-Adapter), regional prompts, cross-attention
// heat maps, prompt-to-prompt editing, StyleAligned sharing, self-attention guidance, perturbed-attention / smoothed-energy
// guidance -- on the host: a feature is its state struct
// (model.h), its rules (Tape::attn_rules, below), its setters (the C ABI at the end of this file; include/pea_hip.h) and its place
// among the launches of an attention op (Tape::attn_forward).  No device code here: the kernels and their launchers are
// attention.hip's.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "../../include/pea_hip.h"
#include "model.h"

#define REFUSE(rc, ...)         \
  do {                          \
    pea_set_error(__VA_ARGS__); \
    return rc;                  \
  } while (0)

// ============================================================================ the rules
// the stacked text K|V projection of a UNet graph, or null
static const Op* kv_stack_op(const Tape& u) {
  const Op* kv = nullptr;
  for (const Op& o : u.ops)
    if (o.out == u.t_kvall && o.fused >= 0) kv = &o;
  return kv;
}
// the first live image-prompt set (tokens set and not cleared), or -1
int Tape::ip_live_set() const {
  for (int j = 0; ip && j < ip->nsets; ++j)
    if (ip->set[j].live) return j;
  return -1;
}

// What a context must be for the features of `which` (AF_* bits), every (feature, condition) rule once.  forward false: at set
// time, one feature, `who` its setter, arg the setter's own count (AF_IP: image tokens, AF_REGIONS: R); the state a rule reads may
// not exist yet.  forward true: before the first launch of a forward, every feature that is set, in this order -- features,
// per-sample context lengths or image tokens may have arrived since the setter looked.  A rule fires where it always did: at
// both times unless its line says otherwise.  Welcome everywhere, since none of them sees the launches in question: FreeU,
// ControlNet residuals, and for the self-attention features (StyleAligned, both guidances) image prompts, regions and heat maps.
int Tape::attn_rules(unsigned which, bool forward, int arg) const {
  const int live = ip_live_set();
  // the text cross-attention the regions, edit and maps kernels are built for: head_dim 64 over the whole context
  auto xattn_whole_context = [&](const char* fmt, const char* who) -> int {
    for (const Op& o : ops)
      if (o.kind == OP_ATTN && o.b == t_kvall) SHAPECHK(o.p3 == 1 && o.p2 == L, fmt, who, o.p3, o.p2);
    return PEA_OK;
  };
  // ... and the stacked K|V projection behind it, heads of 64 unpadded (set time only: image prompts, heat maps)
  auto kv_stack_is_64 = [&](const char* who, const char* built) -> int {
    const Op* const kv = kv_stack_op(*this);
    if (!kv) REFUSE(PEA_E_STATE, "%s: stacked K|V projection not found", who);
    for (const WSlot& s : slots)
      SHAPECHK(!(s.fused_parent == kv->fused && s.pad_mode), "%s: '%s' has padded heads (head_dim %d); the %s is built for head_dim 64", who,
               s.name.c_str(), s.pad_d, built);
    return PEA_OK;
  };
  if (which & AF_IP) {
    if (!forward) {                                                  // (pea_unet_ip_create / _create_sets / _plan; arg: n_tokens)
      const char* const who = "pea_unet_ip";
      if (needs_grad) REFUSE(PEA_E_STATE, "%s: this context was created with PEA_UNET_GRAD; there is no backward through the image branch", who);
      SHAPECHK(arg >= 1 && arg <= 32, "%s: n_tokens=%d (1..32 image tokens)", who, arg);
      SHAPECHK(L <= 128, "%s: context length %d (the decoupled attention takes at most 128 text keys)", who, L);
      RC(kv_stack_is_64(who, "decoupled attention"));
    }
    // forward only: a live set with a mask for some of the context's cross-attention query counts needs one for each: a layer
    // without would silently run with a mask of 1
    for (int j = 0; forward && ip && j < ip->nsets; ++j) {
      const IpSet& e = ip->set[j];
      if (!e.live || e.mask.empty()) continue;
      for (const Op& o : ops)
        if (o.kind == OP_ATTN && o.b == t_kvall && !e.mask.count(o.p1))
          REFUSE(PEA_E_STATE, "pea_unet_forward: image prompt %d has a mask for %d queries but none for the layers with %d queries; "
                 "pea_unet_ip_set_mask needs every count of pea_unet_ip_query_counts", j, e.mask.begin()->first, o.p1);
    }
  }
  if (which & AF_REGIONS) {                                          // (arg at set time: R)
    const char* const who = forward ? "pea_unet_forward" : "pea_unet_set_prompt_regions";
    const int R = forward ? regions->R : arg;
    if (needs_grad)
      REFUSE(PEA_E_STATE, "%s: regional prompts are an inference feature (no backward through them); this context was created with PEA_UNET_GRAD", who);
    if (cross_kvlen) REFUSE(PEA_E_STATE, "%s: regional prompts cannot be combined with per-sample context lengths", who);
    if (live >= 0) REFUSE(PEA_E_STATE, "%s: regional prompts cannot be combined with live image prompts (set %d; pea_unet_ip_clear)", who, live);
    SHAPECHK(R >= 1 && R <= 4, "%s: 1..4 regions (R=%d)", who, R);
    SHAPECHK(L % R == 0 && L / R <= 96, "%s: a context of %d rows is no %d prompts of at most 96 rows", who, L, R);
    for (const Op& o : ops) {
      if (o.kind != OP_ATTN || o.b != t_kvall) continue;
      SHAPECHK(o.p3 == 1 && o.p2 == L, "%s: regional prompts need head_dim 64 cross-attention over the whole context (nd=%d, %d keys)", who, o.p3, o.p2);
      if (forward && !regions->w.count(o.p1))                        // forward only: a count without weights would run on another layer's table
        REFUSE(PEA_E_STATE, "%s: regional prompts have no weights for the layers with %d queries; pea_unet_set_prompt_regions needs every "
               "count of pea_unet_ip_query_counts", who, o.p1);
    }
  }
  if (which & AF_MAPS) {
    if (!forward) {                                                  // set time only
      const char* const who = "pea_unet_enable_attention_maps";
      if (needs_grad) REFUSE(PEA_E_STATE, "%s: heat maps are an inference feature; this context was created with PEA_UNET_GRAD", who);
      SHAPECHK(L >= 1 && L <= 128, "%s: context length %d (the maps kernel takes 1..128 keys)", who, L);
      RC(kv_stack_is_64(who, "maps kernel"));
      RC(xattn_whole_context("%s: head_dim 64 cross-attention over the whole context (nd=%d, %d keys)", who));
    }
    if (forward && regions)                                          // forward only
      REFUSE(PEA_E_STATE, "pea_unet_forward: cross-attention heat maps cannot be combined with regional prompts (a context of several prompts has "
             "a softmax per region; pea_unet_disable_attention_maps or pea_unet_clear_prompt_regions)");
  }
  if (which & AF_EDIT) {
    const char* const who = forward ? "pea_unet_forward" : "pea_unet_set_prompt_edit";
    if (needs_grad)
      REFUSE(PEA_E_STATE, "%s: prompt editing is an inference feature (no backward through it); this context was created with PEA_UNET_GRAD", who);
    if (cross_kvlen) REFUSE(PEA_E_STATE, "%s: prompt editing cannot be combined with per-sample context lengths", who);
    if (live >= 0) REFUSE(PEA_E_STATE, "%s: prompt editing cannot be combined with live image prompts (set %d; pea_unet_ip_clear)", who, live);
    if (regions) REFUSE(PEA_E_STATE, "%s: prompt editing cannot be combined with prompt regions (pea_unet_clear_prompt_regions)", who);
    if (maps) REFUSE(PEA_E_STATE, "%s: prompt editing cannot be combined with attention-map capture (pea_unet_disable_attention_maps)", who);
    SHAPECHK(L >= 1 && L <= 96, "%s: prompt editing takes a context of 1..96 rows (L=%d)", who, L);
    SHAPECHK(B <= 32, "%s: prompt editing takes a batch of at most 32 (B=%d)", who, B);
    RC(xattn_whole_context("%s: prompt editing needs head_dim 64 cross-attention over the whole context (nd=%d, %d keys)", who));
    if (forward && (edit->step < 0 || edit->step >= edit->T))        // forward only
      REFUSE(PEA_E_STATE, "%s: prompt-edit step %d is outside 0..%d (pea_unet_set_prompt_edit_step)", who, edit->step, edit->T - 1);
    if (perturb)
      REFUSE(PEA_E_STATE, "%s: prompt editing cannot be combined with perturbed-attention guidance: its self-attention rule rewrites the "
             "outputs of the perturbed samples (pea_unet_clear_attn_perturb)", who);
  }
  if (which & AF_STYLE) {
    const char* const who = forward ? "pea_unet_forward" : "pea_unet_set_style_aligned";
    if (needs_grad)
      REFUSE(PEA_E_STATE, "%s: StyleAligned sharing is an inference feature (no backward through it); this context was created with PEA_UNET_GRAD", who);
    if (edit)
      REFUSE(PEA_E_STATE, "%s: StyleAligned sharing cannot be combined with prompt editing, whose self-attention rule rewrites the same outputs "
             "(pea_unet_clear_prompt_edit or pea_unet_clear_style_aligned)", who);
    SHAPECHK(B <= 32, "%s: StyleAligned sharing takes a batch of at most 32 (B=%d)", who, B);
    for (const Op& o : ops) {
      if (!is_self_attn(o)) continue;
      SHAPECHK(o.p3 == 1 && o.p1 >= 2, "%s: StyleAligned sharing needs head_dim 64 self-attention over at least 2 tokens (nd=%d, %d tokens)", who, o.p3, o.p1);
    }
  }
  if (which & AF_SAG) {                                              // (at set time the setter has hung the state it wants judged)
    const char* const who = forward ? "pea_unet_forward" : "pea_unet_enable_sag";
    if (needs_grad) REFUSE(PEA_E_STATE, "%s: self-attention guidance is an inference feature; this context was created with PEA_UNET_GRAD", who);
    if (edit)
      REFUSE(PEA_E_STATE, "%s: self-attention guidance cannot be combined with prompt editing, whose self-attention rule rewrites the captured "
             "launch (pea_unet_clear_prompt_edit or pea_unet_disable_sag)", who);
    if (sag && style && style->n_targets) {                          // both rewrite or replace the chosen launch
      const auto it = style->layer_of_op.find(sag->op);
      if (it != style->layer_of_op.end() && style->on[it->second])
        REFUSE(PEA_E_STATE, "%s: self-attention layer %d is shared by StyleAligned, which replaces the launch self-attention guidance captures "
               "(switch that layer off in pea_unet_set_style_aligned, or pea_unet_disable_sag)", who, sag->layer);
    }
  }
  if (which & AF_PERTURB) {                                          // (at set time the setter has hung the state it wants judged)
    const char* const who = forward ? "pea_unet_forward" : "pea_unet_set_attn_perturb";
    const PerturbState& pt = *perturb;
    if (needs_grad)
      REFUSE(PEA_E_STATE, "%s: perturbed-attention guidance is an inference feature (the query blur overwrites Q, which a backward "
             "would read); this context was created with PEA_UNET_GRAD", who);
    SHAPECHK(pt.first >= 1 && pt.first < B, "%s: perturbed samples %d .. %d of a batch of %d (a non-empty suffix that leaves plain "
             "samples in front)", who, pt.first, B - 1, B);
    if (edit)
      REFUSE(PEA_E_STATE, "%s: perturbed-attention guidance cannot be combined with prompt editing, whose self-attention rule rewrites "
             "the same outputs (pea_unet_clear_prompt_edit or pea_unet_clear_attn_perturb)", who);
    for (size_t i = 0; i < ops.size(); ++i) {
      const Op& o = ops[i];
      if (!is_self_attn(o)) continue;
      const int layer = pt.layer_of_op.find((int)i)->second;
      if (!pt.on[layer]) continue;
      const int head_dim = (int)lroundf(1.f / (o.f0 * o.f0));       // (the softmax scale is head_dim^-1/2; padded heads keep their own)
      SHAPECHK(o.p3 == 1 && head_dim == 64, "%s: self-attention layer %d has head_dim %d (stored as %d); the perturbed launches are "
               "built for 64", who, layer, head_dim, 64 * o.p3);
      if (style && style->n_targets && style->on[layer])            // both replace or rewrite that layer's launch
        REFUSE(PEA_E_STATE, "%s: self-attention layer %d is shared by StyleAligned and perturbed at once (switch it off in "
               "pea_unet_set_style_aligned or in pea_unet_set_attn_perturb)", who, layer);
      if (sag && sag->op == (int)i)
        REFUSE(PEA_E_STATE, "%s: self-attention layer %d is perturbed, and self-attention guidance captures its launch "
               "(pea_unet_disable_sag, or switch the layer off in pea_unet_set_attn_perturb)", who, layer);
      if (forward && pt.mode == PerturbState::BLUR && !pt.grid.count(o.p1))   // forward only, as the regions' weights
        REFUSE(PEA_E_STATE, "%s: the query blur has no tables for the layers with %d queries; pea_unet_set_attn_perturb needs the "
               "grid of every switched-on layer", who, o.p1);
    }
  }
  return PEA_OK;
}

// ============================================================================ the launches of an attention op
// Image prompts of cross-attention op o.  The weight of set j in this layer is scale_j * layer_scale_j[layer], read here, at
// launch.  A set that is not live or weighs 0 here is dropped: the launch takes the run of rows from the first to the last
// remaining set (AttnP::k2_brows keeps the packed buffer's batch stride), so one remaining set without a mask is the one-set
// launch of a context that holds that adapter alone, bit for bit, and none is the plain attention.  A dropped set BETWEEN two
// remaining ones stays in the run with weight 0 -- exact zeros in P; its rows are zero or an earlier image's, finite either way.
int Tape::ip_attach(const Op& o, AttnP& p) {
  IpState& st = *ip;
  const auto lay = st.layer_of_col.find(o.bcol);
  float w[4] = {0.f, 0.f, 0.f, 0.f};
  int first = -1, last = -1;
  for (int j = 0; j < st.nsets; ++j) {
    const IpSet& e = st.set[j];
    if (!e.live) continue;
    w[j] = e.scale * (e.layer_scale.empty() || lay == st.layer_of_col.end() ? 1.f : e.layer_scale[lay->second]);
    if (w[j] == 0.f) continue;
    if (first < 0) first = j;
    last = j;
  }
  if (first < 0) return PEA_OK;
  const int row0 = st.set[first].off;
  p.K2 = st.kv + (size_t)row0 * st.cols + o.bcol; p.V2 = st.kv + (size_t)row0 * st.cols + o.ccol; p.ldk2 = p.ldv2 = st.cols;
  p.Skv2 = st.set[last].off + st.set[last].n - row0; p.k2_brows = st.total;
  if (first == last && st.set[first].mask.empty()) {
    p.scale2 = w[first];
    return PEA_OK;
  }
  p.nset = last - first + 1;
  for (int j = first; j <= last; ++j) {
    const IpSet& e = st.set[j];
    const int i = j - first;
    p.set_end[i] = e.off + e.n - row0; p.set_w[i] = w[j];
    if (w[j] == 0.f || e.mask.empty()) continue;
    const auto m = e.mask.find(o.p1);
    if (m == e.mask.end()) {                                       // attn_rules has passed: not reached from forward()
      pea_set_error("unet: image prompt %d has masks, but none for the %d queries of this layer (pea_unet_ip_set_mask)", j, o.p1);
      return PEA_E_STATE;
    }
    p.set_mask[i] = m->second.first; p.set_mstride[i] = m->second.second == 1 ? 0 : o.p1;
  }
  return PEA_OK;
}

// What each feature adds to the plain operands p of its op (pea_kernels.h: attn_feature_p carries the rest over).  attn_rules has
// passed: the tables of the op's query count are there.
static AttnRegionsP regions_p(const Tape::RegionState& st, const AttnP& p) {      // R softmaxes over the R runs of context rows
  AttnRegionsP r = attn_feature_p<AttnRegionsP>(p);
  const auto& wt = st.w.find(p.Sq)->second;
  r.R = st.R; r.Lr = p.Skv / st.R; r.w = wt.first; r.Bw = wt.second;
  return r;
}
static AttnEditP edit_p(const Tape::EditState& st, const AttnP& p, int L) {       // the source's softmax mixed into the edited samples'
  AttnEditP e = attn_feature_p<AttnEditP>(p);
  e.Mt = st.Mt; e.ldm = st.ldm;
  e.c = st.cd + (size_t)st.step * 2 * p.B * L; e.d = e.c + (size_t)p.B * L;
  memcpy(e.src, st.src, sizeof(e.src));
  return e;
}
static AttnSharedP shared_p(const Tape::StyleState& st, const AttnP& p) {         // the targets attend to their reference's keys and values as well
  AttnSharedP e = attn_feature_p<AttnSharedP>(p);
  e.coef = st.coef; e.share_scale = st.share_scale; e.share_shift = st.share_shift;
  memcpy(e.ref, st.ref, sizeof(e.ref));
  return e;
}
static AttnColsumP colsum_p(const Tape::SagState& st, const AttnP& p) {           // the captured samples of Q, K and the lse just stored
  AttnColsumP c = attn_feature_p<AttnColsumP>(p);
  c.Q = p.Q + (size_t)st.first * p.Sq * p.ldq; c.K = p.K + (size_t)st.first * p.Skv * p.ldk; c.B = st.n;
  c.lse = st.lse + (size_t)st.first * p.H * p.Sq; c.part = st.part;
  return c;
}
static AttnMapsP maps_p(float* acc, const int* kv_len, const AttnP& p) {          // the text softmax's head mean, added to the level's sum
  AttnMapsP m = attn_feature_p<AttnMapsP>(p);
  m.maps = acc; m.kv_len = kv_len; m.accumulate = 1;
  return m;
}

// Forward of attention op oi (OP_ATTN).  Top to bottom, the precedence of the features: regions replace the launch; else a live
// edit step replaces it; else image prompts attach to it; else StyleAligned replaces it; else the plain launch, with guidance's
// lse pointer in it and the column sums behind it -- on a perturbed layer behind the blur of the perturbed samples' queries, or over
// the plain samples alone with the V -> O copy behind it; then the edit's per-sample self-attention launches; then the heat maps'.
int Tape::attn_forward(size_t oi, hipStream_t s) {
  const Op& o = ops[oi];
  const bool text = o.b == t_kvall;                                  // cross-attention over the text context
  AttnP p; memset(&p, 0, sizeof(p));
  p.Q = tn[o.a].d + o.acol; p.ldq = tn[o.a].cols; p.K = tn[o.b].d + o.bcol; p.ldk = tn[o.b].cols;
  p.V = tn[o.c].d + o.ccol; p.ldv = tn[o.c].cols; p.O = tn[o.out].d; p.ldo = tn[o.out].cols; p.lse = o.aux;
  p.B = B; p.H = o.p0; p.Sq = o.p1; p.Skv = o.p2; p.scale = o.f0; p.nd = o.p3;
  p.causal = o.mask & 1; p.kv_len = (o.mask & 2) ? kvlen : nullptr;
  p.q_prescaled = o.pre;
  if (o.mask & 4) p.bias = rel_bias;
  if (cross_kvlen && text) p.kv_len = cross_kvlen;
  if (regions && text) return launch_attention_fwd_regions(regions_p(*regions, p), s);
  if (edit && text && edit->cd_live[edit->step])                     // (a step whose tables do nothing runs the plain launch)
    return launch_attention_fwd_edit(edit_p(*edit, p, L), s);
  if (ip && text) RC(ip_attach(o, p));                               // the layer's own columns of the image K|V
  if (style && style->n_targets && is_self_attn(o) && style->on[style->layer_of_op.find((int)oi)->second]) {
    // the targets' AdaIN coefficients from this layer's Q and K columns, then the one launch (plain samples keep their bits)
    RC(launch_attn_adain_coef(p.Q, p.ldq, p.K, p.ldk, B, o.p0, o.p1, style->ref, o.f0, o.pre, style->adain_q, style->adain_k,
                              style->coef, style->scratch, s));
    return launch_attention_fwd_shared(shared_p(*style, p), s);
  }
  // perturbed-attention guidance on this layer: the suffix's queries blurred in place in front of the one launch, or the launch
  // over the plain samples alone and V copied to O for the suffix (attn_rules has passed: head_dim 64, the grid's tables are there)
  const int perturbed = perturb && is_self_attn(o) && perturb->on[perturb->layer_of_op.find((int)oi)->second] ? perturb->mode : 0;
  if (perturbed == PerturbState::BLUR) {
    const PerturbState::Grid& g = perturb->grid.find(o.p1)->second;
    RC(launch_query_blur((bf16*)p.Q + (size_t)perturb->first * p.Sq * p.ldq, p.ldq, B - perturb->first, g.h, g.w, 64 * p.H, g.Mh, g.Mw, s));
  }
  if (perturbed == PerturbState::IDENTITY) p.B = perturb->first;
  const bool sag_here = sag && sag->op == (int)oi;
  if (sag_here) p.lse = sag->lse;
  RC(launch_attention_fwd(p, s));
  if (perturbed == PerturbState::IDENTITY) {
    p.B = B;
    RC(launch_copy2d(p.V + (size_t)perturb->first * p.Skv * p.ldv, p.ldv, p.O + (size_t)perturb->first * p.Sq * p.ldo, p.ldo,
                     (long long)(B - perturb->first) * p.Sq, 64 * p.H, 0, s));
  }
  if (sag_here) RC(launch_attention_colsum(colsum_p(*sag, p), s));
  if (edit && graph == 0 && !text && !o.mask && o.p1 == o.p2 && o.p1 <= edit->self_max_tokens && edit->step < edit->self_until) {
    // prompt editing, self-attention: O[b] = softmax(Q[s] K[s]^T) V[b], one B = 1 launch per edited sample behind the
    // ordinary one (unedited samples keep their bits by construction)
    for (int b = 0; b < B; ++b) {
      const int sb = edit->src[b];
      if (sb < 0) continue;
      AttnP e = p;
      e.B = 1; e.lse = nullptr;
      e.Q = p.Q + (size_t)sb * p.Sq * p.ldq; e.K = p.K + (size_t)sb * p.Skv * p.ldk;
      e.V = p.V + (size_t)b * p.Skv * p.ldv; e.O = p.O + (size_t)b * p.Sq * p.ldo;
      RC(launch_attention_fwd(e, s));
    }
  }
  if (maps && text) {
    const auto lay = maps->layer_of_col.find(o.bcol);
    if (lay != maps->layer_of_col.end() && maps->on[lay->second]) {
      RC(launch_attention_maps(maps_p(maps->acc.find(o.p1)->second, cross_kvlen, p), s));
      ++maps->count[o.p1];
    }
  }
  return PEA_OK;
}

// ============================================================================ what the setters share
// The guard of a feature's entry point: a handle, and a UNet graph (text: with the text cross-attention the feature works on).
// why: the rest of the sentence, which may print the graph number.
static int unet_handle(void* h, const char* who, bool text, const char* why, Tape** out) {
  NOTNULL(h, who);
  Tape* const u = (Tape*)h;
  if (u->graph != 0 || (text && u->t_kvall < 0)) {
    char fmt[160];
    snprintf(fmt, sizeof(fmt), "%%s: not a UNet handle (%s)", why);
    REFUSE(PEA_E_INVALID, fmt, who, u->graph);
  }
  *out = u;
  return PEA_OK;
}
// a handle whose image-prompt state exists, and a set of it
static int ip_handle(void* h, const char* who, Tape** out) {
  NOTNULL(h, who);
  *out = (Tape*)h;
  if (!(*out)->ip) REFUSE(PEA_E_STATE, "%s: call pea_unet_ip_create first", who);
  return PEA_OK;
}
static int ip_set_of(void* h, int set, const char* who, Tape** u, Tape::IpSet** e) {
  RC(ip_handle(h, who, u));
  SHAPECHK(set >= 0 && set < (*u)->ip->nsets, "%s: set %d of %d", who, set, (*u)->ip->nsets);
  *e = &(*u)->ip->set[set];
  return PEA_OK;
}
// a feature's state goes: behind whatever queued forward may still use its device buffers (on_device null: any state has some)
template <class S>
static int drop_state(void* h, const char* who, S* Tape::*slot, bool (*on_device)(const S&) = nullptr) {
  NOTNULL(h, who);
  S*& st = ((Tape*)h)->*slot;
  if (st && (!on_device || on_device(*st))) HIPCHK(hipDeviceSynchronize());
  delete st;
  st = nullptr;
  return PEA_OK;
}
// a chain of device calls that stops at its first failure: hipError_t err = hipSuccess; THEN(err, ...); ...; RC(dev_chain(who, err));
#define THEN(err, call) \
  if ((err) == hipSuccess) (err) = (call)
static int dev_chain(const char* who, hipError_t err) {
  if (err != hipSuccess) REFUSE(PEA_E_HIP, "%s: %s", who, hipGetErrorString(err));
  return PEA_OK;
}
// layer switches: null = every one of the `want` layers on, else exactly `want` of them, non-zero = on
static int parse_layer_on(const char* who, const float* layer_on, int n_layers, int want, const char* kind, std::vector<char>& on) {
  SHAPECHK(!layer_on || n_layers == want, "%s: %d layer switches, this UNet has %d %s layers", who, n_layers, want, kind);
  on.assign(want, 1);
  for (int i = 0; layer_on && i < want; ++i) on[i] = layer_on[i] != 0.f;
  return PEA_OK;
}
// the distinct query counts of the context's text cross-attention layers, in tape order; and Sq is one of them
static void ip_query_counts(const Tape& u, std::vector<int>& out) {
  for (const Op& o : u.ops)
    if (o.kind == OP_ATTN && o.b == u.t_kvall && std::find(out.begin(), out.end(), o.p1) == out.end()) out.push_back(o.p1);
}
static int check_query_count(const Tape& u, const char* who, int Sq) {
  std::vector<int> c;
  ip_query_counts(u, c);
  SHAPECHK(std::find(c.begin(), c.end(), Sq) != c.end(), "%s: no cross-attention layer of this context has %d queries (pea_unet_ip_query_counts)", who, Sq);
  return PEA_OK;
}
// a per-query-count device table [Bt][...] of `bytes` bytes (image-prompt masks, region weights): allocated on first use, again
// where its batch Bt changed (behind whatever queued forward may still read the old one), filled from `src` on the stream
static int put_table(std::map<int, std::pair<float*, int>>& tab, int Sq, int Bt, size_t bytes, const float* src, hipStream_t s) {
  auto it = tab.find(Sq);
  if (it != tab.end() && it->second.second != Bt) {
    HIPCHK(hipDeviceSynchronize());
    (void)hipFree(it->second.first);
    tab.erase(it);
    it = tab.end();
  }
  if (it == tab.end()) {
    float* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, bytes));
    it = tab.emplace(Sq, std::make_pair(buf, Bt)).first;
  }
  HIPCHK(hipMemcpyAsync(it->second.first, src, bytes, hipMemcpyDeviceToDevice, s));
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
// the self-attention ops of the tape, in tape order: their number, and (layer_of_op) op index -> layer index
static int self_attn_layers(const Tape& u, std::map<int, int>* layer_of_op) {
  int n = 0;
  for (size_t i = 0; i < u.ops.size(); ++i)
    if (u.is_self_attn(u.ops[i])) {
      if (layer_of_op) (*layer_of_op)[(int)i] = n;
      ++n;
    }
  return n;
}

extern "C" {

// ------------------------------------------------------------------------------ image prompt (IP-Adapter)
int pea_unet_ip_plan(const pea_unet_config* cfg, int n_tokens, int* n_layers, int* cols, long long* n_params) {
  NOTNULL(cfg, "pea_unet_ip_plan");
  Tape u;
  memcpy(&u.cfg, cfg, sizeof(PeaUnetCfg));
  // layers, stack width and parameters depend on the config alone: any batch / size / context length plans them.  The context
  // length is therefore NOT validated here (the rule L <= 128 cannot fire); pea_unet_ip_create checks the real context
  u.B = 1; u.H = 64; u.W = 64; u.L = 77; u.needs_grad = false;
  u.plan_only = true;
  int rc = u.build();
  if (rc == PEA_OK) rc = u.alloc();
  if (rc != PEA_OK) return rc;
  Tape* up = nullptr;
  RC(unet_handle(&u, "pea_unet_ip", true, "ControlNet graphs get no image prompt", &up));
  RC(u.attn_rules(Tape::AF_IP, false, n_tokens));
  const Op* const kv = kv_stack_op(u);
  int members = 0;
  for (const WSlot& s : u.slots) members += s.fused_parent == kv->fused && s.kind == W_LINEAR;
  if (n_layers) *n_layers = members / 2;
  if (cols) *cols = u.kvall_total;
  if (n_params) *n_params = (long long)u.kvall_total * u.cfg.cross_dim;
  return PEA_OK;
}
int pea_unet_ip_create_sets(void* h, int n_sets, const int* n_tokens) {
  NOTNULL(h, "pea_unet_ip_create_sets");
  NOTNULL(n_tokens, "pea_unet_ip_create_sets");
  SHAPECHK(n_sets >= 1 && n_sets <= 4, "pea_unet_ip_create_sets: %d adapters (1..4)", n_sets);
  Tape* u = nullptr;
  RC(unet_handle(h, "pea_unet_ip", true, "ControlNet graphs get no image prompt", &u));
  int total = 0;
  for (int j = 0; j < n_sets; ++j) {
    RC(u->attn_rules(Tape::AF_IP, false, n_tokens[j]));
    total += n_tokens[j];
  }
  const Op* const kv = kv_stack_op(*u);
  SHAPECHK(total <= 32, "pea_unet_ip_create_sets: %d image tokens over all adapters (one launch takes at most 32)", total);
  RC(pea_unet_ip_destroy(h));                        // adapters already loaded: replaced, behind whatever still reads them
  Tape::IpState* ip = new Tape::IpState();
  ip->nsets = n_sets; ip->total = total; ip->cols = u->kvall_total; ip->fused = kv->fused;
  xattn_layer_order(*u, kv->fused, ip->layer_of_col);  // the file's layer order
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
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_load_weight", &u, &e));
  NOTNULL(key, "pea_unet_ip_load_weight");
  NOTNULL(src, "pea_unet_ip_load_weight");
  std::string name(key);
  const size_t at = name.rfind("_ip.weight");
  int slot = -1;
  if (at != std::string::npos && at + 10 == name.size()) {
    auto it = u->slot_by_name.find(name.substr(0, at) + ".weight");      // to_k_ip -> the text stack's to_k of the same layer
    if (it != u->slot_by_name.end() && u->slots[it->second].fused_parent == u->ip->fused) slot = it->second;
  }
  if (slot < 0) REFUSE(PEA_E_NOTFOUND, "pea_unet_ip_load_weight: '%s' is no to_k_ip / to_v_ip weight of this UNet", key);
  const WSlot& w = u->slots[slot];
  SHAPECHK(numel == w.numel, "pea_unet_ip_load_weight: '%s' has %lld elements, expected %lld ([%d][%d])", key, numel, w.numel, w.d0, w.d1);
  RC(launch_cast_f32_bf16(src, e->w + (size_t)w.row_off * w.d1, numel, (hipStream_t)stream));
  e->loaded[slot] = 1;
  return PEA_OK;
}
int pea_unet_ip_load_weight(void* h, const char* key, const float* src, long long numel, void* stream) {
  return pea_unet_ip_load_weight_set(h, 0, key, src, numel, stream);
}
int pea_unet_ip_set_tokens_set(void* h, int set, const float* tokens, void* stream) {
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_set_tokens", &u, &e));
  NOTNULL(tokens, "pea_unet_ip_set_tokens");
  Tape::IpState& ip = *u->ip;
  for (size_t i = 0; i < e->loaded.size(); ++i)
    if (!e->loaded[i]) {
      const std::string& n = u->slots[i].name;
      REFUSE(PEA_E_STATE, "pea_unet_ip_set_tokens: '%s_ip.weight' was never loaded", n.substr(0, n.size() - 7).c_str());
    }
  hipStream_t s = (hipStream_t)stream;
  const int rows = u->B * e->n, K = u->cfg.cross_dim;
  RC(launch_cast_f32_bf16(tokens, e->tok, (long long)rows * K, s));
  // one adapter: ONE GEMM over all samples.  Several: the set's rows of a sample are not adjacent to those of the next, so one
  // GEMM per sample straight into its rows of the packed buffer (once per image, B is the CFG batch)
  const int launches = ip.nsets == 1 ? 1 : u->B, m = rows / launches;
  for (int b = 0; b < launches; ++b) {
    GemmP p; fill_gemm(p);
    p.A = e->tok + (size_t)b * m * K; p.lda = K; p.M = m; p.K = K; p.N = ip.cols; p.W = e->w; p.ldw = K;
    p.C = ip.kv + ((size_t)b * ip.total + e->off) * ip.cols; p.ldc = ip.cols;
    RC(launch_gemm(p, s));
  }
  e->live = true;
  return PEA_OK;
}
int pea_unet_ip_set_tokens(void* h, const float* tokens, void* stream) { return pea_unet_ip_set_tokens_set(h, 0, tokens, stream); }
int pea_unet_ip_set_scale_set(void* h, int set, float scale) {
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_set_scale", &u, &e));
  e->scale = scale;
  return PEA_OK;
}
int pea_unet_ip_set_scale(void* h, float scale) { return pea_unet_ip_set_scale_set(h, 0, scale); }
int pea_unet_ip_set_layer_scales(void* h, int set, const float* scales, int n_layers) {
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_set_layer_scales", &u, &e));
  if (!scales) {                                     // back to 1 in every layer
    e->layer_scale.clear();
    return PEA_OK;
  }
  const int want = (int)u->ip->layer_of_col.size();
  SHAPECHK(n_layers == want, "pea_unet_ip_set_layer_scales: %d scales, this UNet has %d cross-attention layers", n_layers, want);
  e->layer_scale.assign(scales, scales + n_layers);
  return PEA_OK;
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
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_set_mask", &u, &e));
  if (!mask) {                                       // drop the mask of that count, or (Sq == 0) all of them
    HIPCHK(hipDeviceSynchronize());                  // a queued forward may still read them
    for (auto it = e->mask.begin(); it != e->mask.end();)
      if (Sq == 0 || it->first == Sq) { (void)hipFree(it->second.first); it = e->mask.erase(it); } else ++it;
    return PEA_OK;
  }
  RC(check_query_count(*u, "pea_unet_ip_set_mask", Sq));
  SHAPECHK(Bm == 1 || Bm == u->B, "pea_unet_ip_set_mask: Bm=%d (1, or the context's batch %d)", Bm, u->B);
  return put_table(e->mask, Sq, Bm, (size_t)Bm * Sq * sizeof(float), mask, (hipStream_t)stream);
}
int pea_unet_ip_clear_set(void* h, int set) {
  Tape* u; Tape::IpSet* e;
  RC(ip_set_of(h, set, "pea_unet_ip_clear", &u, &e));
  e->live = false;
  return PEA_OK;
}
int pea_unet_ip_clear(void* h) {
  NOTNULL(h, "pea_unet_ip_clear");
  if (((Tape*)h)->ip)
    for (Tape::IpSet& e : ((Tape*)h)->ip->set) e.live = false;
  return PEA_OK;
}
int pea_unet_ip_destroy(void* h) { return drop_state(h, "pea_unet_ip_destroy", &Tape::ip); }
int pea_unet_ip_export_kv(void* h, float* out, long long* rows, int* cols, void* stream) {
  Tape* u;
  RC(ip_handle(h, "pea_unet_ip_export_kv", &u));
  const long long r = (long long)u->B * u->ip->total;
  if (rows) *rows = r;
  if (cols) *cols = u->ip->cols;
  if (!out) return PEA_OK;
  if (u->ip_live_set() < 0) REFUSE(PEA_E_STATE, "pea_unet_ip_export_kv: no tokens set");
  return launch_cast_bf16_f32(u->ip->kv, out, r * u->ip->cols, (hipStream_t)stream);
}
// ------------------------------------------------------------------------------ regional text prompts
int pea_unet_set_prompt_regions(void* h, int R, int Sq, const float* w, int Bw, void* stream) {
  const char* const who = "pea_unet_set_prompt_regions";
  Tape* u = nullptr;
  RC(unet_handle(h, who, true, "ControlNet graphs keep one prompt", &u));
  if (!w) REFUSE(PEA_E_INVALID, "%s: null weights", who);
  RC(u->attn_rules(Tape::AF_REGIONS, false, R));
  SHAPECHK(!u->regions || u->regions->R == R, "%s: R=%d, but weights for %d regions are set (pea_unet_clear_prompt_regions)", who,
           R, u->regions ? u->regions->R : 0);
  RC(check_query_count(*u, who, Sq));
  SHAPECHK(Bw == 1 || Bw == u->B, "%s: Bw=%d (1, or the context's batch %d)", who, Bw, u->B);
  if (!u->regions) { u->regions = new Tape::RegionState(); u->regions->R = R; }
  return put_table(u->regions->w, Sq, Bw, (size_t)Bw * R * Sq * sizeof(float), w, (hipStream_t)stream);
}
int pea_unet_clear_prompt_regions(void* h) { return drop_state(h, "pea_unet_clear_prompt_regions", &Tape::regions); }
// ------------------------------------------------------------------------------ prompt-to-prompt editing
int pea_unet_set_prompt_edit(void* h, const int* src, const void* Mt, const float* cd, int T, int self_until, int self_max_tokens,
                             void* stream) {
  const char* const who = "pea_unet_set_prompt_edit";
  Tape* u = nullptr;
  RC(unet_handle(h, who, true, "graph %d has no text cross-attention to edit", &u));
  if (!src || !Mt || !cd) REFUSE(PEA_E_INVALID, "%s: null src, Mt or cd", who);
  RC(u->attn_rules(Tape::AF_EDIT, false));
  const int B = u->B, L = u->L;
  SHAPECHK(T >= 1 && T <= (1 << 20), "%s: T=%d steps", who, T);
  SHAPECHK(self_until >= 0 && self_max_tokens >= 0, "%s: self_until=%d, self_max_tokens=%d (>= 0)", who, self_until, self_max_tokens);
  int n_edited = 0;
  for (int b = 0; b < B; ++b) {
    if (src[b] < 0 || src[b] == b) continue;                       // (its own source: not edited)
    SHAPECHK(src[b] < B, "%s: src[%d]=%d is out of range (batch %d)", who, b, src[b], B);
    SHAPECHK(src[src[b]] < 0 || src[src[b]] == src[b], "%s: src[%d]=%d names a source that is itself edited", who, b, src[b]);
    ++n_edited;
  }
  RC(pea_unet_clear_prompt_edit(h));
  std::unique_ptr<Tape::EditState> e(new Tape::EditState());
  for (int b = 0; b < 32; ++b) e->src[b] = b < B && src[b] != b ? src[b] : -1;
  e->n_edited = n_edited; e->T = T; e->self_until = self_until; e->self_max_tokens = self_max_tokens; e->ldm = (L + 7) / 8 * 8;
  const size_t cd_elems = (size_t)T * 2 * B * L, mt_bytes = (size_t)B * L * e->ldm * sizeof(bf16);
  std::vector<float> host(cd_elems);
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMalloc((void**)&e->Mt, mt_bytes);
  THEN(err, hipMalloc((void**)&e->cd, cd_elems * sizeof(float)));
  THEN(err, hipMemsetAsync(e->Mt, 0, mt_bytes, s));
  THEN(err, hipMemcpy2DAsync(e->Mt, (size_t)e->ldm * sizeof(bf16), Mt, (size_t)L * sizeof(bf16), (size_t)L * sizeof(bf16), (size_t)B * L,
                             hipMemcpyDeviceToDevice, s));
  THEN(err, hipMemcpyAsync(e->cd, cd, cd_elems * sizeof(float), hipMemcpyDeviceToDevice, s));
  THEN(err, hipMemcpyAsync(host.data(), cd, cd_elems * sizeof(float), hipMemcpyDeviceToHost, s));
  THEN(err, hipStreamSynchronize(s));
  RC(dev_chain(who, err));
  e->cd_live.assign(T, 0);
  for (int t = 0; t < T; ++t)
    for (int b = 0; b < B && !e->cd_live[t]; ++b) {
      if (e->src[b] < 0) continue;
      const float* c = host.data() + ((size_t)t * 2 * B + b) * L;
      const float* d = c + (size_t)B * L;
      for (int j = 0; j < L; ++j)
        if (c[j] != 0.f || d[j] != 1.f) { e->cd_live[t] = 1; break; }
    }
  u->edit = e.release();
  return PEA_OK;
}
int pea_unet_set_prompt_edit_step(void* h, int step) {
  NOTNULL(h, "pea_unet_set_prompt_edit_step");
  Tape* u = (Tape*)h;
  if (!u->edit) REFUSE(PEA_E_STATE, "pea_unet_set_prompt_edit_step: call pea_unet_set_prompt_edit first");
  u->edit->step = step;                               // (a step outside 0..T-1 is refused by the forward that would use it)
  return PEA_OK;
}
int pea_unet_clear_prompt_edit(void* h) { return drop_state(h, "pea_unet_clear_prompt_edit", &Tape::edit); }
// ------------------------------------------------------------------------------ StyleAligned generation
int pea_unet_num_self_attention_layers(void* h) {
  NOTNULL(h, "pea_unet_num_self_attention_layers");
  return self_attn_layers(*(Tape*)h, nullptr);
}
int pea_unet_set_style_aligned(void* h, const int* ref, const float* layer_on, int n_layers, int adain_queries, int adain_keys,
                               float shared_score_scale, float shared_score_shift, void* stream) {
  const char* const who = "pea_unet_set_style_aligned";
  Tape* u = nullptr;
  RC(unet_handle(h, who, false, "graph %d", &u));
  if (!ref) REFUSE(PEA_E_INVALID, "%s: null ref (a host int[B]; negative entries for plain samples)", who);
  RC(u->attn_rules(Tape::AF_STYLE, false));
  const int B = u->B;
  SHAPECHK(shared_score_scale == shared_score_scale && shared_score_shift == shared_score_shift && fabsf(shared_score_scale) <= 3.0e38f &&
               fabsf(shared_score_shift) <= 1.0e30f,
           "%s: finite shared_score_scale / shared_score_shift (%g %g)", who, (double)shared_score_scale, (double)shared_score_shift);
  std::unique_ptr<Tape::StyleState> st(new Tape::StyleState());
  for (int b = 0; b < 32; ++b) st->ref[b] = -1;
  for (int b = 0; b < B; ++b) {
    if (ref[b] < 0 || ref[b] == b) continue;                       // (its own reference: plain)
    SHAPECHK(ref[b] < B, "%s: ref[%d]=%d is out of range (batch %d)", who, b, ref[b], B);
    SHAPECHK(ref[ref[b]] < 0 || ref[ref[b]] == ref[b], "%s: ref[%d]=%d names a reference that is itself a target", who, b, ref[b]);
    st->ref[b] = ref[b];
    ++st->n_targets;
  }
  RC(parse_layer_on(who, layer_on, n_layers, self_attn_layers(*u, &st->layer_of_op), "self-attention", st->on));
  st->adain_q = adain_queries != 0; st->adain_k = adain_keys != 0;
  st->share_scale = shared_score_scale; st->share_shift = shared_score_shift;
  size_t coef_bytes = 0, scratch_bytes = 0;
  for (const Op& o : u->ops) {
    if (!u->is_self_attn(o)) continue;
    coef_bytes = std::max(coef_bytes, sizeof(float) * (size_t)B * 4 * 64 * o.p0);
    scratch_bytes = std::max(scratch_bytes, attn_adain_scratch_bytes(B, o.p0, o.p1));
  }
  RC(pea_unet_clear_style_aligned(h));
  if (st->n_targets && coef_bytes) {
    hipError_t err = hipMalloc((void**)&st->coef, coef_bytes);
    THEN(err, hipMalloc((void**)&st->scratch, std::max(scratch_bytes, (size_t)16)));
    RC(dev_chain(who, err));
  }
  (void)stream;                                                     // nothing is transferred: ref is a host table
  u->style = st.release();
  return PEA_OK;
}
int pea_unet_clear_style_aligned(void* h) {                         // (a state without targets has no buffers)
  return drop_state<Tape::StyleState>(h, "pea_unet_clear_style_aligned", &Tape::style, [](const Tape::StyleState& st) { return st.coef != nullptr; });
}
// ------------------------------------------------------------------------------ self-attention guidance
int pea_unet_enable_sag(void* h, int layer, int first_sample, int n_samples) {
  const char* const who = "pea_unet_enable_sag";
  Tape* u = nullptr;
  RC(unet_handle(h, who, false, "graph %d", &u));
  std::map<int, int> layer_of_op;
  const int want = self_attn_layers(*u, &layer_of_op);
  SHAPECHK(layer >= 0 && layer < want, "%s: layer %d, this UNet has %d self-attention layers", who, layer, want);
  SHAPECHK(first_sample >= 0 && n_samples >= 1 && first_sample + n_samples <= u->B,
           "%s: samples %d .. %d of a batch of %d", who, first_sample, first_sample + n_samples - 1, u->B);
  std::unique_ptr<Tape::SagState> st(new Tape::SagState());
  for (const auto& lo : layer_of_op)
    if (lo.second == layer) st->op = lo.first;
  const Op& o = u->ops[st->op];
  const int head_dim = (int)lroundf(1.f / (o.f0 * o.f0));           // (the softmax scale is head_dim^-1/2; padded heads keep their own)
  SHAPECHK(o.p3 == 1 && head_dim == 64, "%s: self-attention layer %d has head_dim %d (stored as %d); the column-sum "
           "kernel is built for 64", who, layer, head_dim, 64 * o.p3);
  st->layer = layer; st->first = first_sample; st->n = n_samples; st->H = o.p0; st->S = o.p1;
  st->G = attention_colsum_groups(n_samples, o.p0, o.p1, o.p2);
  if (st->G < 1) return PEA_E_SHAPE;
  RC(pea_unet_disable_sag(h));
  u->sag = st.get();                                                // (the rules read the state they judge)
  const int rc = u->attn_rules(Tape::AF_SAG, false);
  u->sag = nullptr;
  if (rc) return rc;
  const size_t part_bytes = sizeof(float) * (size_t)n_samples * st->G * o.p2;
  hipError_t err = hipMalloc((void**)&st->lse, sizeof(float) * (size_t)u->B * o.p0 * o.p1);
  THEN(err, hipMalloc((void**)&st->part, part_bytes));
  THEN(err, hipMemset(st->part, 0, part_bytes));
  THEN(err, hipDeviceSynchronize());
  RC(dev_chain(who, err));
  u->sag = st.release();
  return PEA_OK;
}
int pea_unet_disable_sag(void* h) { return drop_state(h, "pea_unet_disable_sag", &Tape::sag); }
int pea_unet_sag_colsum(void* h, float** part, int* G, int* S) {
  NOTNULL(h, "pea_unet_sag_colsum");
  Tape* u = (Tape*)h;
  if (!u->sag) REFUSE(PEA_E_STATE, "pea_unet_sag_colsum: call pea_unet_enable_sag first");
  if (part) *part = u->sag->part;
  if (G) *G = u->sag->G;
  if (S) *S = u->sag->S;
  return PEA_OK;
}
// ------------------------------------------------------------------------------ perturbed-attention / smoothed-energy guidance
int pea_unet_set_attn_perturb(void* h, int mode, int first_sample, const float* layer_on, int n_layers, int n_grids, const int* grid_h,
                              const int* grid_w, const float* tables, void* stream) {
  const char* const who = "pea_unet_set_attn_perturb";
  Tape* u = nullptr;
  RC(unet_handle(h, who, false, "graph %d", &u));
  typedef Tape::PerturbState PS;
  SHAPECHK(mode == PS::IDENTITY || mode == PS::BLUR, "%s: mode %d (1: identity, 2: query blur)", who, mode);
  SHAPECHK(n_grids >= 0 && n_grids <= 16 && (n_grids == 0 || (grid_h && grid_w && tables)), "%s: %d grids with their sides and tables", who, n_grids);
  std::unique_ptr<PS> st(new PS());
  st->mode = mode; st->first = first_sample;
  RC(parse_layer_on(who, layer_on, n_layers, self_attn_layers(*u, &st->layer_of_op), "self-attention", st->on));
  // the tables of a grid, host fp32: Mh [h][h], then Mw [w][w]; a grid must be that of some self-attention layer (its query count)
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipSuccess;
  for (int i = 0; i < n_grids && mode == PS::BLUR; ++i) {
    const int gh = grid_h[i], gw = grid_w[i];
    SHAPECHK(gh >= 1 && gw >= 1 && gh <= QUERY_BLUR_MAX_SIDE && gw <= QUERY_BLUR_MAX_SIDE,
             "%s: a %d x %d token grid; the query blur holds a grid in LDS, at most %d x %d (%zu of 163840 bytes)", who, gh, gw,
             QUERY_BLUR_MAX_SIDE, QUERY_BLUR_MAX_SIDE, query_blur_lds_bytes(QUERY_BLUR_MAX_SIDE, QUERY_BLUR_MAX_SIDE));
    bool found = false;
    for (const Op& o : u->ops) found = found || (u->is_self_attn(o) && o.p1 == gh * gw);
    SHAPECHK(found && !st->grid.count(gh * gw), "%s: no self-attention layer of this context has %d queries, or the %d x %d grid is given twice",
             who, gh * gw, gh, gw);
    PS::Grid& g = st->grid[gh * gw];
    g.h = gh; g.w = gw;
    THEN(err, hipMalloc((void**)&g.Mh, sizeof(float) * gh * gh));
    THEN(err, hipMalloc((void**)&g.Mw, sizeof(float) * gw * gw));
    THEN(err, hipMemcpyAsync(g.Mh, tables, sizeof(float) * gh * gh, hipMemcpyHostToDevice, s));
    THEN(err, hipMemcpyAsync(g.Mw, tables + gh * gh, sizeof(float) * gw * gw, hipMemcpyHostToDevice, s));
    tables += gh * gh + gw * gw;
  }
  THEN(err, hipStreamSynchronize(s));                                 // the host tables are the caller's again
  RC(dev_chain(who, err));
  RC(pea_unet_clear_attn_perturb(h));
  u->perturb = st.get();                                             // (the rules read the state they judge)
  const int rc = u->attn_rules(Tape::AF_PERTURB, false);
  u->perturb = nullptr;
  if (rc) return rc;
  u->perturb = st.release();
  return PEA_OK;
}
int pea_unet_clear_attn_perturb(void* h) {                           // (the identity mode has no buffers)
  return drop_state<Tape::PerturbState>(h, "pea_unet_clear_attn_perturb", &Tape::perturb,
                                        [](const Tape::PerturbState& st) { return !st.grid.empty(); });
}
// ------------------------------------------------------------------------------ cross-attention heat maps
int pea_unet_enable_attention_maps(void* h, const float* layer_on, int n_layers) {
  const char* const who = "pea_unet_enable_attention_maps";
  Tape* u = nullptr;
  RC(unet_handle(h, who, true, "graph %d has no text cross-attention to map", &u));
  RC(u->attn_rules(Tape::AF_MAPS, false));
  std::unique_ptr<Tape::MapState> m(new Tape::MapState());
  xattn_layer_order(*u, kv_stack_op(*u)->fused, m->layer_of_col);
  RC(parse_layer_on(who, layer_on, n_layers, (int)m->layer_of_col.size(), "cross-attention", m->on));
  int rc = pea_unet_disable_attention_maps(h);        // accumulators already there: replaced, behind whatever still adds to them
  std::vector<int> c;
  ip_query_counts(*u, c);
  for (size_t i = 0; i < c.size() && rc == PEA_OK; ++i) {
    const size_t bytes = (size_t)u->B * u->L * c[i] * sizeof(float);
    float* buf = nullptr;
    if (hipMalloc((void**)&buf, bytes) != hipSuccess || (m->acc[c[i]] = buf, hipMemset(buf, 0, bytes)) != hipSuccess) {
      pea_set_error("%s: out of device memory (%zu bytes for the %d-query level)", who, bytes, c[i]);
      rc = PEA_E_HIP;
    }
    m->count[c[i]] = 0;
  }
  if (rc == PEA_OK && hipDeviceSynchronize() != hipSuccess) {  // the zeros are there before a forward on any stream adds to them
    pea_set_error("%s: device synchronisation failed", who);
    rc = PEA_E_HIP;
  }
  if (rc != PEA_OK) return rc;
  u->maps = m.release();
  return PEA_OK;
}
int pea_unet_reset_attention_maps(void* h, void* stream) {
  NOTNULL(h, "pea_unet_reset_attention_maps");
  Tape* u = (Tape*)h;
  if (!u->maps) REFUSE(PEA_E_STATE, "pea_unet_reset_attention_maps: call pea_unet_enable_attention_maps first");
  for (auto& a : u->maps->acc) {
    HIPCHK(hipMemsetAsync(a.second, 0, (size_t)u->B * u->L * a.first * sizeof(float), (hipStream_t)stream));
    u->maps->count[a.first] = 0;
  }
  return PEA_OK;
}
int pea_unet_disable_attention_maps(void* h) { return drop_state(h, "pea_unet_disable_attention_maps", &Tape::maps); }
int pea_unet_attention_maps(void* h, int Sq, float** maps, long long* n_accumulated) {
  NOTNULL(h, "pea_unet_attention_maps");
  Tape* u = (Tape*)h;
  if (!u->maps) REFUSE(PEA_E_STATE, "pea_unet_attention_maps: call pea_unet_enable_attention_maps first");
  RC(check_query_count(*u, "pea_unet_attention_maps", Sq));        // (the accumulators: one per count)
  if (maps) *maps = u->maps->acc.find(Sq)->second;
  if (n_accumulated) *n_accumulated = u->maps->count[Sq];
  return PEA_OK;
}

}  // extern "C"
